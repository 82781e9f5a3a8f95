// CanvasSomaticCaller: the purity / ploidy grid search of ModelOverallCoverageAndPurity (CanvasSomaticCaller/SomaticCaller.cs:1870-2117).
//
//   host    the model points of every (diploid coverage, purity) model: InitializePloidies' (copy number, major count) order, InitializeModelPoints(model), AdjustedMAF /
//           binomP / logCombinations.  exp and log are the host's libm, so the table is filled by host threads and uploaded once.
//   device  k_somatic_fit, one workgroup per model: RefineDiploidMAF, the clustering loop of ModelDeviation, the accuracy deviation, PercentCN / Ploidy / PercentNormal,
//           Deviation, DiploidModelDistance.  Only + - * / sqrt, no contraction (-ffp-contract=off), every sum over segments added in segment order.
//   host    the model selection (:1921-2116) and InterModelDistance, on the rows of a second launch over the top MaximumRelatedModels models, which also yields the best
//           model's per-segment assignment (the reference's final ModelDeviation call, :2100).
// Not built: the cluster term of ModelDeviation (ClusterDeviation, :1309-1313); CANVAS_SOMATIC_INFO_CLUSTER_TERM says when the reference would have added it.
#include "common.hpp"
#include "somatic_points.hpp"
#include <algorithm>
#include <cmath>

#define SOM_T 256                    // threads of a workgroup = segments of a tile (CANVAS_SOMATIC_TILE)
#define SOM_ROW (SOM_T + 2)          // doubles per value row in LDS: the rows of different accumulator lanes start on different banks
#define SOM_MAXP 36                  // model points at MaximumCopyNumber 10
#define SOM_MAXCN 10
#define SOM_OUT (6 + SOM_MAXCN + 1)  // doubles per model: Deviation, PrecisionDeviation, AccuracyDeviation, Ploidy, PercentNormal, DiploidDistance, PercentCN[0..10]
static_assert(SOM_T == CANVAS_SOMATIC_TILE, "the tile the header documents");

// GetModelDistance (:884-892)
__device__ __forceinline__ double som_distance(double coverage, double coverage2, double maf, double maf2, double cwf) {
    double diff = (coverage - coverage2) * cwf;
    double distance = diff * diff;
    if (maf < 0) return 2 * distance;
    diff = maf - maf2;
    distance += diff * diff;
    return distance;
}

struct SomArgs {
    const double* cov; const double* maf; const double* w; const int32_t* len; int S;
    const double* table;          // [model][2][P]: the points' coverages, then their MAFs
    const int32_t* list;          // models of this launch (NULL: block b is model b)
    int P, maxCN; double cwf, genomeLength;
    double* out;                  // [block][SOM_OUT]
    unsigned char* profile;       // [block][S] copy numbers with LOH counted as 1 (model.CNs), or NULL
    int32_t* segPoint; double* segDist;      // block 0's assignment (info.Ploidy.Index, info.Distance), or NULL
};

__global__ __launch_bounds__(SOM_T) void k_somatic_fit(SomArgs a) {
    __shared__ double ptCov[SOM_MAXP], ptMaf[SOM_MAXP];
    __shared__ unsigned char ptCn[SOM_MAXP], ptMajor[SOM_MAXP];
    __shared__ int code[SOM_T];
    __shared__ double val[6 * SOM_ROW];
    __shared__ double accOut[4 * SOM_MAXP + SOM_MAXCN + 1 + 5];
    const int tid = threadIdx.x, P = a.P, maxCN = a.maxCN, S = a.S;
    const long long model = a.list ? a.list[blockIdx.x] : (long long)blockIdx.x;
    if (tid == 0) {
        int p = 0;
        for (int c = 0; c <= maxCN; c++)
            for (int m = c; m * 2 >= c; m--, p++) { ptCn[p] = (unsigned char)c; ptMajor[p] = (unsigned char)m; }
    }
    if (tid < P) { ptCov[tid] = a.table[model * 2 * P + tid]; ptMaf[tid] = a.table[model * 2 * P + P + tid]; }
    __syncthreads();

    // ---- RefineDiploidMAF (:958-1007): accumulator lane 2k is diploidMAF[k], lane 2k + 1 diploidMAFWeight[k]; the point (2k, k) seeds them with the dummy weight
    const int nEven = 1 + maxCN / 2;
    int evenPoint = 0;
    double acc = 0;
    if (tid < 2 * nEven) {
        for (int p = 0; p < P; p++) if (ptCn[p] == 2 * (tid >> 1) && ptMajor[p] == (tid >> 1)) evenPoint = p;
        const double dummyWeight = 10000000;
        acc = (tid & 1) ? dummyWeight : dummyWeight * ptMaf[evenPoint];
    }
    for (int t0 = 0; t0 < S; t0 += SOM_T) {
        const int n = min(SOM_T, S - t0), s = t0 + tid;
        if (tid < n) {
            const double c = a.cov[s], m = a.maf[s], w = a.w[s];
            int slot = -1;
            if (!(m < 0)) {
                double bestDistance = 1.7976931348623157e308; int best = 0;
                for (int p = 0; p < P; p++) {
                    const double d = som_distance(c, ptCov[p], m, ptMaf[p], a.cwf);
                    if (d < bestDistance) { bestDistance = d; best = p; }
                }
                if (ptCn[best] % 2 == 0 && ptMajor[best] * 2 == ptCn[best] && !(m < 0.4)) slot = ptCn[best] / 2;
            }
            code[tid] = slot; val[tid] = w * m; val[SOM_ROW + tid] = w;
        }
        __syncthreads();
        if (tid < 2 * nEven) {
            const int slot = tid >> 1; const double* v = val + (tid & 1) * SOM_ROW;
            for (int i = 0; i < n; i++) if (code[i] == slot) acc += v[i];
        }
        __syncthreads();
    }
    if (tid < 2 * nEven) accOut[tid] = acc;
    __syncthreads();
    if (tid < nEven) {
        for (int p = 0; p < P; p++) if (ptCn[p] == 2 * tid && ptMajor[p] == tid) ptMaf[p] = accOut[2 * tid] / accOut[2 * tid + 1];
    }
    __syncthreads();

    // ---- the clustering loop of ModelDeviation (:1222-1262).  code = point | copy number << 8 | has a MAF << 16; an accumulator lane adds row `sel` of the segments whose
    // code matches `want` under `mask`: 4 per point (Weight, EmpiricalCoverage, EmpiricalMaf, MafWeight), PercentCN[0..maxCN], precision, total weight, normal bases, and
    // the events of DiploidModelDistance against baseline 2 and against baseline 4 (which starts at 1)
    const int nPoint = 4 * P, nAcc = nPoint + maxCN + 1 + 5;
    int sel = 0, mask = 0, want = 0;
    acc = 0;
    if (tid < nPoint) {
        const int p = tid >> 2, k = tid & 3;
        sel = k == 1 ? 1 : k == 2 ? 2 : 0;
        mask = k >= 2 ? 0x100FF : 0xFF; want = k >= 2 ? (p | 0x10000) : p;
    } else if (tid < nPoint + maxCN + 1) {
        mask = 0xFF00; want = (tid - nPoint) << 8;
    } else if (tid < nAcc) {
        const int k = tid - (nPoint + maxCN + 1);
        sel = k == 0 ? 3 : k == 3 ? 4 : k == 4 ? 5 : 0;
        if (k == 2) { mask = 0xFF; want = P; for (int p = 0; p < P; p++) if (ptCn[p] == 2 && ptMajor[p] == 1) want = p; }      // maxCN >= 2: the point exists
        if (k == 4) acc = 1;
    }
    for (int t0 = 0; t0 < S; t0 += SOM_T) {
        const int n = min(SOM_T, S - t0), s = t0 + tid;
        if (tid < n) {
            const double c = a.cov[s], m = a.maf[s], w = a.w[s];
            double bestDistance = 1.7976931348623157e308; int best = 0;
            for (int p = 0; p < P; p++) {
                const double d = som_distance(c, ptCov[p], m, ptMaf[p], a.cwf);
                if (d < bestDistance) { bestDistance = d; best = p; }
            }
            bestDistance = sqrt(bestDistance);
            const int bestCN = ptCn[best];
            const int cn = (bestCN == 2 && ptMajor[best] == 2) ? 1 : bestCN;       // LOH counts as one event
            const int len = a.len[s];
            code[tid] = best | bestCN << 8 | (m >= 0 ? 0x10000 : 0);
            val[tid] = w; val[SOM_ROW + tid] = w * c; val[2 * SOM_ROW + tid] = w * m; val[3 * SOM_ROW + tid] = bestDistance * w;
            val[4 * SOM_ROW + tid] = abs(cn - 2) * len / a.genomeLength; val[5 * SOM_ROW + tid] = abs(cn - 4) * len / a.genomeLength;
            if (a.profile) a.profile[(size_t)blockIdx.x * S + s] = (unsigned char)cn;
            if (a.segPoint && blockIdx.x == 0) { a.segPoint[s] = best; a.segDist[s] = bestDistance; }
        }
        __syncthreads();
        if (tid < nAcc) {
            const double* v = val + sel * SOM_ROW;
            for (int i = 0; i < n; i++) if ((code[i] & mask) == want) acc += v[i];
        }
        __syncthreads();
    }
    if (tid < nAcc) accOut[tid] = acc;
    __syncthreads();
    if (tid != 0) return;

    // ---- :1263-1326 and DiploidModelDistance (:842-860)
    const double* g = accOut + nPoint + maxCN + 1;
    const double totalWeight = g[1];
    const double precisionDeviation = g[0] / totalWeight;
    double accuracyDeviation = 0;
    for (int p = 0; p < P; p++) {
        const double weight = accOut[4 * p];
        if (weight == 0) continue;
        const double empiricalCoverage = accOut[4 * p + 1] / weight;
        double empiricalMaf = accOut[4 * p + 2];
        if (accOut[4 * p + 3] > 0) empiricalMaf /= accOut[4 * p + 3];
        const double distance = sqrt(som_distance(ptCov[p], empiricalCoverage, ptMaf[p], empiricalMaf, a.cwf));
        accuracyDeviation += distance * weight;
    }
    accuracyDeviation /= totalWeight;
    double* o = a.out + (size_t)blockIdx.x * SOM_OUT;
    double ploidy = 0, amplification = 0;
    for (int c = 0; c <= SOM_MAXCN; c++) o[6 + c] = c <= maxCN ? accOut[nPoint + c] / totalWeight : 0.0;
    for (int c = 0; c <= maxCN; c++) ploidy += c * o[6 + c];
    for (int c = 3; c < maxCN; c++) amplification += o[6 + c];
    const double totalCNevents = amplification > 0.8 ? g[4] : g[3];
    o[0] = precisionDeviation * 0.5f + 0.5f * accuracyDeviation;
    o[1] = precisionDeviation; o[2] = accuracyDeviation; o[3] = ploidy;
    o[4] = g[2] / totalWeight;
    o[5] = 1.0 / (totalCNevents > 0.001 ? totalCNevents : 0.001);
}

// InitializeModelPoints(model) (:754-777) for models m0, m0 + step, ...
static void som_fill_table(const int32_t* mcov, const int32_t* mpur, long long M, long long m0, long long step, int P, const unsigned char* cn, const unsigned char* major,
                           const double* logFactorial, double* table) {
    for (long long m = m0; m < M; m += step) {
        const double diploidCoverage = mcov[m], purity = (double)(mpur[m] / 100.0f);      // model.Purity = percentPurity / 100f
        const double tumorHaploid = diploidCoverage * purity / 2.0, normalHaploid = diploidCoverage * (1.0 - purity) / 2.0;
        for (int p = 0; p < P; p++) {
            const double coverage = cn[p] * tumorHaploid + 2 * normalHaploid;
            const double theoreticalMAcvg = (cn[p] - major[p]) * tumorHaploid + normalHaploid;
            table[m * 2 * P + p] = coverage;
            table[m * 2 * P + P + p] = som_adjusted_maf(theoreticalMAcvg, coverage, logFactorial);
        }
    }
}

static double som_ms(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

extern "C" int32_t canvas_somatic_model_fit(canvas_ctx* ctx, int64_t nseg, const double* coverage, const double* maf, const double* weight, const int32_t* length,
                                            int32_t inputs_on_device, const canvas_somatic_grid* grid, const canvas_somatic_params* params, canvas_somatic_result* h_result,
                                            int32_t* h_seg_point, double* h_seg_distance, const canvas_somatic_models* h_models) {
    auto fail = [&](int32_t code, const std::string& msg) { if (ctx) ctx->err = "canvas_somatic_model_fit: " + msg; return code; };
    if (!grid || !params || !h_result || !coverage || !maf || !weight || !length) return fail(CANVAS_ERR_INVALID, "bad arguments");
    const canvas_somatic_params& pr = *params; const canvas_somatic_grid& gr = *grid;
    if (pr.maximum_copy_number < 2 || pr.maximum_copy_number > SOM_MAXCN) return fail(CANVAS_ERR_INVALID, "MaximumCopyNumber must be 2 .. 10");
    if (pr.maximum_related_models < 1 || pr.maximum_related_models > 64 || pr.deviation_index_cutoff < 0) return fail(CANVAS_ERR_INVALID, "MaximumRelatedModels must be 1 .. 64 and DeviationIndexCutoff >= 0");
    if (nseg < 3) return fail(CANVAS_ERR_INVALID, "fewer than 3 usable segments");
    if (nseg > 0x7FFFFFFFll / 64) return fail(CANVAS_ERR_INVALID, "too many segments");
    if (gr.genome_length <= 0 || !std::isfinite(gr.coverage_weighting_factor) || !std::isfinite(gr.min_minor_allele_coverage)) return fail(CANVAS_ERR_INVALID, "genome_length must be positive, the weighting factor and the minor allele coverage finite");
    if (gr.minimum_purity_hard_limit < 0 || gr.minimum_purity_hard_limit > 99 || gr.fixed_percent_purity > 100) return fail(CANVAS_ERR_INVALID, "minimum_purity_hard_limit must be 0 .. 99 and a fixed purity at most 100");
    const int covLo = gr.fixed_coverage >= 0 ? gr.fixed_coverage : gr.min_coverage, covHi = gr.fixed_coverage >= 0 ? gr.fixed_coverage : gr.max_coverage;
    if (covLo < 1 || covHi > 100000) return fail(CANVAS_ERR_INVALID, "diploid coverages must be 1 .. 100000");
    // the grid (:1899-1914)
    std::vector<int32_t> mcov, mpur;
    for (int cov = covLo; cov <= covHi; cov++) {
        int minPercentPurity = (int)std::max((double)gr.minimum_purity_hard_limit, 100 * (1 - 2 * gr.min_minor_allele_coverage / cov) - 10), maxPercentPurity = 100;
        if (gr.fixed_percent_purity >= 0) minPercentPurity = maxPercentPurity = gr.fixed_percent_purity;
        for (int pp = minPercentPurity; pp <= maxPercentPurity; pp++) { mcov.push_back(cov); mpur.push_back(pp); }
    }
    const long long M = (long long)mcov.size(), S = nseg;
    if (M == 0) return fail(CANVAS_ERR_INVALID, "the grid is empty");
    if (M > 0x7FFFFFFFll / (2 * SOM_MAXP)) return fail(CANVAS_ERR_INVALID, "too many models");
    if (h_models && h_models->capacity < M) return fail(CANVAS_ERR_CAPACITY, "the per-model arrays hold fewer models than the grid has (" + std::to_string(M) + ")");
    const int maxCN = pr.maximum_copy_number;
    unsigned char ptCn[SOM_MAXP], ptMajor[SOM_MAXP];
    const int P = som_points(maxCN, ptCn, ptMajor);

    std::vector<double> hCov, hMaf, hW; std::vector<int32_t> hLen;
    int nMaf = 0;
    auto check_segments = [&](const double* c, const double* m, const double* w, const int32_t* l) -> int32_t {
        double totalWeight = 0;
        for (long long s = 0; s < S; s++) {
            if (!std::isfinite(c[s]) || !std::isfinite(w[s]) || std::isnan(m[s])) return fail(CANVAS_ERR_INVALID, "segment " + std::to_string(s) + ": coverage and weight must be finite and the MAF a number");
            if (l[s] < 0 || (long long)l[s] * maxCN > 0x7FFFFFFFll) return fail(CANVAS_ERR_INVALID, "segment " + std::to_string(s) + ": length times MaximumCopyNumber leaves int32");
            totalWeight += w[s]; nMaf += m[s] >= 0;
        }
        if (totalWeight == 0) return fail(CANVAS_ERR_INVALID, "the total weight is 0");
        return CANVAS_OK;
    };
    if (!inputs_on_device) { int32_t rc = check_segments(coverage, maf, weight, length); if (rc) return rc; }
    *h_result = canvas_somatic_result{};
    h_result->nmodels = (int32_t)M; h_result->best_model = -1;
    if (!ctx) return CANVAS_ERR_INVALID;
    CANVAS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (inputs_on_device) {
        hCov.resize(S); hMaf.resize(S); hW.resize(S); hLen.resize(S);
        CANVAS_HIP_TRY(ctx, hipMemcpyAsync(hCov.data(), coverage, S * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        CANVAS_HIP_TRY(ctx, hipMemcpyAsync(hMaf.data(), maf, S * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        CANVAS_HIP_TRY(ctx, hipMemcpyAsync(hW.data(), weight, S * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        CANVAS_HIP_TRY(ctx, hipMemcpyAsync(hLen.data(), length, S * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        CANVAS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        int32_t rc = check_segments(hCov.data(), hMaf.data(), hW.data(), hLen.data()); if (rc) return rc;
    }
    const int32_t* hLength = inputs_on_device ? hLen.data() : length;
    if (!gr.is_enrichment && S > 100 && nMaf > 100) h_result->info |= CANVAS_SOMATIC_INFO_CLUSTER_TERM;

    // ---- the host table
    auto t0 = std::chrono::steady_clock::now();
    std::vector<double> table((size_t)M * 2 * P);
    {
        const long long nmax = (long long)covHi * maxCN / 2 + 2;          // (int)coverage of the largest point: coverage * purity * CN / 2 + coverage * (1 - purity)
        std::vector<double> logFactorial((size_t)nmax + 1, 0.0);
        for (long long i = 2; i <= nmax; i++) logFactorial[i] = log((double)i) + logFactorial[i - 1];
        const unsigned hw = std::thread::hardware_concurrency();
        const long long nthreads = std::max(1ll, std::min<long long>(std::min<long long>(16, hw ? hw : 1), M));
        std::vector<std::thread> pool;
        for (long long t = 1; t < nthreads; t++) pool.emplace_back(som_fill_table, mcov.data(), mpur.data(), M, t, nthreads, P, ptCn, ptMajor, logFactorial.data(), table.data());
        som_fill_table(mcov.data(), mpur.data(), M, 0, nthreads, P, ptCn, ptMajor, logFactorial.data(), table.data());
        for (auto& th : pool) th.join();
    }
    h_result->host_table_ms = som_ms(t0);

    // ---- upload
    t0 = std::chrono::steady_clock::now();
    const int K = pr.maximum_related_models;
    double *dTable, *dOut, *dOutTop, *dSegDist, *dc, *dm, *dw; int32_t *dList, *dSegPoint, *dl; unsigned char* dProfile;
    int32_t rc = cvx_ws_carve(ctx, 256, [&](WsCarver& cv) {
        cv.take(dTable, (size_t)M * 2 * P); cv.take(dOut, (size_t)M * SOM_OUT); cv.take(dList, K); cv.take(dOutTop, (size_t)K * SOM_OUT); cv.take(dProfile, (size_t)K * S);
        cv.take(dSegPoint, S); cv.take(dSegDist, S);
        if (!inputs_on_device) { cv.take(dc, S); cv.take(dm, S); cv.take(dw, S); cv.take(dl, S); }
    });
    if (rc) return rc;
    SomArgs a{};
    a.cov = coverage; a.maf = maf; a.w = weight; a.len = length;
    if (!inputs_on_device) {
        CANVAS_HIP_TRY(ctx, hipMemcpyAsync(dc, coverage, S * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        CANVAS_HIP_TRY(ctx, hipMemcpyAsync(dm, maf, S * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        CANVAS_HIP_TRY(ctx, hipMemcpyAsync(dw, weight, S * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        CANVAS_HIP_TRY(ctx, hipMemcpyAsync(dl, length, S * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
        a.cov = dc; a.maf = dm; a.w = dw; a.len = dl;
    }
    CANVAS_HIP_TRY(ctx, hipMemcpyAsync(dTable, table.data(), table.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    CANVAS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    h_result->upload_ms = som_ms(t0);

    // ---- every model
    t0 = std::chrono::steady_clock::now();
    a.S = (int)S; a.table = dTable; a.P = P; a.maxCN = maxCN; a.cwf = gr.coverage_weighting_factor; a.genomeLength = (double)gr.genome_length; a.out = dOut;
    {
        ProfScope ps(ctx, "somatic_fit", true);
        hipLaunchKernelGGL(k_somatic_fit, dim3((unsigned)M), dim3(SOM_T), 0, ctx->stream, a);
    }
    CANVAS_HIP_TRY(ctx, hipGetLastError());
    std::vector<double> out((size_t)M * SOM_OUT);
    CANVAS_HIP_TRY(ctx, hipMemcpyAsync(out.data(), dOut, out.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    CANVAS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    h_result->device_ms = som_ms(t0);

    // ---- model selection (:1921-2056)
    t0 = std::chrono::steady_clock::now();
    auto O = [&](long long m, int k) { return out[(size_t)m * SOM_OUT + k]; };
    std::vector<long long> all;                       // allModels
    double bestDeviation = 1.7976931348623157e308;
    for (long long m = 0; m < M; m++) {
        const bool ok = O(m, 3) < pr.max_allowed_ploidy && O(m, 3) > pr.min_allowed_ploidy;
        if (O(m, 0) < bestDeviation && ok) bestDeviation = O(m, 0);
        if (ok) all.push_back(m);
    }
    std::vector<double> score((size_t)M, 0.0); std::vector<int32_t> flags((size_t)M, 0);
    for (long long m : all) flags[m] = CANVAS_SOMATIC_MODEL_VALID;
    auto export_models = [&]() {
        if (!h_models) return;
        const canvas_somatic_models& hm = *h_models;
        for (long long m = 0; m < M; m++) {
            if (hm.coverage) hm.coverage[m] = mcov[m];
            if (hm.percent_purity) hm.percent_purity[m] = mpur[m];
            if (hm.deviation) hm.deviation[m] = O(m, 0);
            if (hm.precision_deviation) hm.precision_deviation[m] = O(m, 1);
            if (hm.accuracy_deviation) hm.accuracy_deviation[m] = O(m, 2);
            if (hm.ploidy) hm.ploidy[m] = O(m, 3);
            if (hm.percent_normal) hm.percent_normal[m] = O(m, 4);
            if (hm.diploid_distance) hm.diploid_distance[m] = O(m, 5);
            if (hm.percent_cn) for (int c = 0; c <= SOM_MAXCN; c++) hm.percent_cn[m * (SOM_MAXCN + 1) + c] = O(m, 6 + c);
            if (hm.flags) hm.flags[m] = flags[m];
            if (hm.score) hm.score[m] = score[m];
        }
    };
    h_result->nvalid = (int32_t)all.size();
    if (all.empty()) { export_models(); return fail(CANVAS_ERR_SOMATIC_NO_MODEL, "no model passes the ploidy filter"); }
    double worstAllowedDeviation = bestDeviation * pr.deviation_factor;
    {
        int counter = 0;
        std::vector<double> deviations;
        for (long long m : all) { if (O(m, 0) < worstAllowedDeviation) counter++; deviations.push_back(O(m, 0)); }
        std::sort(deviations.begin(), deviations.end());
        if (counter < pr.deviation_index_cutoff) {
            worstAllowedDeviation = deviations[std::min<size_t>((size_t)pr.deviation_index_cutoff, deviations.size() - 1)];
            h_result->info |= CANVAS_SOMATIC_INFO_INDEX_CUTOFF;
        }
    }
    double bestCN2 = 0, bestDiploidDistance = 0;
    for (long long m : all) {
        if (O(m, 0) > worstAllowedDeviation) continue;
        if (O(m, 6 + 2) > bestCN2) bestCN2 = O(m, 6 + 2);
        if (O(m, 5) > bestDiploidDistance) bestDiploidDistance = O(m, 5);
    }
    std::vector<long long> bestModels; std::vector<double> scores;
    long long best = -1; double bestScore = 0;
    const double hardLimit = gr.minimum_purity_hard_limit / 100.0;
    for (long long m : all) {
        if (O(m, 0) > worstAllowedDeviation) continue;
        const double purity = (double)(mpur[m] / 100.0f);
        const double lowPurityWeightingFactor = 1.5 / ((1.5 - 0.5) / (1.0 - hardLimit) * (purity - hardLimit) + 1.0);
        const double percentCN2SubScore = lowPurityWeightingFactor * pr.cn2_weighting_factor * (O(m, 6 + 2) / std::max(0.01, bestCN2) - 1);
        double deviationSubScore = 0.0;
        if (worstAllowedDeviation > bestDeviation)
            deviationSubScore = pr.deviation_score_weighting_factor * (worstAllowedDeviation - O(m, 0)) / (worstAllowedDeviation - bestDeviation);
        const double diploidDistanceSubScore = pr.diploid_distance_score_weighting_factor * O(m, 5) / std::max(0.01, bestDiploidDistance);
        const double heterogeneityIndex = 0;             // the cluster term is not built: model.HeterogeneityIndex stays 0
        const double heterogeneitySubScore = pr.heterogeneity_score_weighting_factor * heterogeneityIndex;
        const double sc = percentCN2SubScore + deviationSubScore + diploidDistanceSubScore + heterogeneitySubScore;
        scores.push_back(sc); bestModels.push_back(m);
        score[m] = sc; flags[m] |= CANVAS_SOMATIC_MODEL_SCORED;
        if (sc > bestScore) { best = m; bestScore = sc; }
    }
    export_models();
    h_result->nscored = (int32_t)bestModels.size();
    h_result->best_deviation = bestDeviation; h_result->worst_allowed_deviation = worstAllowedDeviation;
    if (best < 0) return fail(CANVAS_ERR_SOMATIC_NO_SCORE, "no model scores above 0");

    // ---- the stable order by -score (:2083-2084), as far as InterModelDistance looks
    const int ntop = (int)std::min<size_t>(scores.size(), (size_t)K);
    std::vector<int32_t> top; std::vector<char> taken(scores.size(), 0);
    for (int r = 0; r < ntop; r++) {
        long long pick = -1;
        for (size_t i = 0; i < scores.size(); i++) if (!taken[i] && (pick < 0 || -scores[i] < -scores[pick])) pick = (long long)i;
        taken[pick] = 1; top.push_back((int32_t)bestModels[pick]);
    }
    if (top[0] != best) return fail(CANVAS_ERR_INVALID, "the best model is not the first of the score order");       // both are the first model with the highest score
    h_result->selection_ms = som_ms(t0);

    // ---- the top models once more: their copy-number profiles and the best model's assignment (:2088-2100)
    t0 = std::chrono::steady_clock::now();
    rc = canvas_h2d_small(ctx, dList, top.data(), top.size() * sizeof(int32_t)); if (rc) return rc;
    a.list = dList; a.out = dOutTop; a.profile = dProfile; a.segPoint = dSegPoint; a.segDist = dSegDist;
    {
        ProfScope ps(ctx, "somatic_fit_top");
        hipLaunchKernelGGL(k_somatic_fit, dim3((unsigned)ntop), dim3(SOM_T), 0, ctx->stream, a);
    }
    CANVAS_HIP_TRY(ctx, hipGetLastError());
    std::vector<unsigned char> prof((size_t)ntop * S); std::vector<int32_t> segPoint(S); std::vector<double> segDist(S);
    CANVAS_HIP_TRY(ctx, hipMemcpyAsync(prof.data(), dProfile, prof.size(), hipMemcpyDeviceToHost, ctx->stream));
    CANVAS_HIP_TRY(ctx, hipMemcpyAsync(segPoint.data(), dSegPoint, S * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    CANVAS_HIP_TRY(ctx, hipMemcpyAsync(segDist.data(), dSegDist, S * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    CANVAS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    h_result->device_ms += som_ms(t0);
    t0 = std::chrono::steady_clock::now();
    double interModelDistance = 0;
    for (int i = 1; i < ntop; i++) {                      // CalculateModelDistance (:865-879)
        double genomeDistance = 0;
        for (long long s = 0; s < S; s++) genomeDistance += abs((int)prof[s] - (int)prof[(size_t)i * S + s]) * hLength[s] / (double)gr.genome_length;
        interModelDistance += genomeDistance;
    }
    interModelDistance /= (double)K;
    if (h_seg_point) memcpy(h_seg_point, segPoint.data(), S * sizeof(int32_t));
    if (h_seg_distance) memcpy(h_seg_distance, segDist.data(), S * sizeof(double));
    canvas_somatic_result& r = *h_result;
    r.best_model = (int32_t)best; r.best_coverage = mcov[best]; r.best_percent_purity = mpur[best];
    r.diploid_coverage = mcov[best]; r.purity = (double)(mpur[best] / 100.0f);
    r.deviation = O(best, 0); r.precision_deviation = O(best, 1); r.accuracy_deviation = O(best, 2); r.ploidy = O(best, 3); r.percent_normal = O(best, 4); r.diploid_distance = O(best, 5);
    for (int c = 0; c <= SOM_MAXCN; c++) r.percent_cn[c] = O(best, 6 + c);
    r.score = bestScore; r.inter_model_distance = interModelDistance;
    r.selection_ms += som_ms(t0);
    return CANVAS_OK;
}
