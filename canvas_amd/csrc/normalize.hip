// CanvasNormalize, ratio path: weighted-average reference over the control samples, ratio of a sample to the reference
// (LSNorm / Raw), ratios back to counts.  reference: CanvasNormalize/WeightedAverageReferenceGenerator.cs:28-70, BinCounts.cs:36-60,
// LSNormRatioCalculator.cs:20-48, RawRatioCalculator.cs:21-46, CanvasNormalizeUtilities.cs:23-33.
// Element-wise work plus two medians: the medians are exact order statistics from the radix select of CanvasClean (select.hpp), the
// dropped bins are removed with a block-count / scan / scatter compaction.  Which bins are "on target" comes from the caller (the
// manifest parser stays on the host side of the boundary).
// The two other reference generators (BestLR2, PCA) follow at the end of the file.
#include "common.hpp"
#include "select.hpp"
#include "quantize.hpp"
#include <cmath>
#include <vector>

__global__ void __launch_bounds__(256) k_norm_keys_f64(const double* __restrict__ v, const int32_t* __restrict__ idx, int64_t n, unsigned long long* __restrict__ keys) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) keys[i] = key_of_double(v[idx ? idx[i] : i]);
}
__global__ void __launch_bounds__(256) k_norm_keys_f32(const float* __restrict__ v, const int32_t* __restrict__ idx, int64_t n, unsigned long long* __restrict__ keys) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) keys[i] = key_of_double((double)v[idx ? idx[i] : i]);
}
#define NORM_MAX_SAMPLES 64
struct NormPtrs { const double* c[NORM_MAX_SAMPLES]; double w[NORM_MAX_SAMPLES]; };
__global__ void __launch_bounds__(256) k_norm_weighted(NormPtrs P, int nsamples, int64_t n, double* __restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    double w = 0;
    for (int s = 0; s < nsamples; s++) w += P.w[s] * P.c[s][j];      // left to right, product rounded before the add (-ffp-contract=off)
    out[j] = w;
}
__device__ __forceinline__ bool norm_keep(float r, int mode, double minRef, double maxRef) {
    return mode == 0 ? !(r < 1.0f) : !((double)r < minRef) && !((double)r > maxRef);
}
__global__ void __launch_bounds__(256) k_norm_count(const float* __restrict__ ref, int64_t n, int mode, double minRef, double maxRef, uint32_t* __restrict__ blockCnt) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool keep = i < n && norm_keep(ref[i], mode, minRef, maxRef);
    const unsigned long long b = __ballot(keep);
    __shared__ uint32_t s[4];
    if (lane_id() == 0) s[threadIdx.x >> 6] = (uint32_t)__popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) blockCnt[blockIdx.x] = s[0] + s[1] + s[2] + s[3];
}
__global__ void __launch_bounds__(1024) k_norm_scan(uint32_t* __restrict__ blockCnt, int64_t nblocks, long long* __restrict__ total) {
    __shared__ uint32_t sw[16];
    __shared__ uint32_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int64_t base = 0; base < nblocks; base += 1024) {
        const int64_t i = base + threadIdx.x;
        const uint32_t v = i < nblocks ? blockCnt[i] : 0u;
        const uint32_t inc = wave_inclusive_scan_u32(v);
        if (lane_id() == 63) sw[threadIdx.x >> 6] = inc;
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (int w = 0; w < 16; w++) { if (w < (int)(threadIdx.x >> 6)) before += sw[w]; all += sw[w]; }
        const uint32_t c = carry;
        if (i < nblocks) blockCnt[i] = c + before + inc - v;
        __syncthreads();
        if (threadIdx.x == 0) carry = c + all;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}
__global__ void __launch_bounds__(256) k_norm_ratio(const float* __restrict__ sample, const float* __restrict__ ref, const int32_t* __restrict__ ploidy, int64_t n, int mode,
                                                    double minRef, double maxRef, double lsf, const uint32_t* __restrict__ blockOff, int32_t* __restrict__ keepIdx,
                                                    float* __restrict__ ratio, float* __restrict__ count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool keep = i < n && norm_keep(ref[i], mode, minRef, maxRef);
    const unsigned long long b = __ballot(keep);
    __shared__ uint32_t s[4];
    if (lane_id() == 0) s[threadIdx.x >> 6] = (uint32_t)__popcll(b);
    __syncthreads();
    if (!keep) return;
    uint32_t off = blockOff[blockIdx.x];
    for (int w = 0; w < (int)(threadIdx.x >> 6); w++) off += s[w];
    off += (uint32_t)__popcll(b & ((1ull << lane_id()) - 1ull));
    const float q = sample[i] / ref[i];                                   // float / float, as in the C#
    const double rt = mode == 0 ? (double)q * lsf : (double)q;
    const float rf = (float)rt;
    const double factor = 40.0 * (double)(ploidy ? ploidy[i] : 2) / 2.0;  // CanvasDiploidBinRatioFactor * ploidy / 2.0
    keepIdx[off] = (int32_t)i; ratio[off] = rf; count[off] = (float)((double)rf * factor);
}

// SortedList<double>.Median() of the n keys (two order statistics)
static int32_t norm_median(canvas_ctx* ctx, const unsigned long long* dKeys, int64_t n, double& med) {
    if (n <= 0) { med = 0; return CANVAS_OK; }
    std::vector<SelQuery> qs; std::vector<unsigned long long> res;
    if (n & 1) qs.push_back({0, 0, n / 2}); else { qs.push_back({0, 0, n / 2 - 1}); qs.push_back({0, 0, n / 2}); }
    int32_t rc = radix_select<unsigned long long>(ctx, dKeys, 1, std::vector<int64_t>{0, n}, qs, res); if (rc) return rc;
    med = (n & 1) ? host_double_of_key(res[0]) : (host_double_of_key(res[0]) + host_double_of_key(res[1])) / 2;
    return CANVAS_OK;
}

extern "C" {

int32_t canvas_normalize_reference(canvas_ctx* ctx, int32_t nsamples, const double* const* h_d_counts, int64_t n, const int32_t* d_on_target_idx, int64_t n_on_target,
                                   double* d_weighted, double* h_weights) {
    if (!ctx) return CANVAS_ERR_INVALID;
    if (nsamples <= 0 || nsamples > NORM_MAX_SAMPLES || !h_d_counts || n <= 0 || !d_weighted || (d_on_target_idx && n_on_target <= 0)) CANVAS_FAIL(ctx, CANVAS_ERR_INVALID, "canvas_normalize_reference: bad arguments");
    CANVAS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int64_t nk = d_on_target_idx ? n_on_target : n;
    int32_t rc = canvas_ws_reserve(ctx, (size_t)nk * 8 + 4096); if (rc) return rc;
    unsigned long long* dKeys = (unsigned long long*)ctx->ws;
    NormPtrs P;
    double weightSum = 0;
    for (int s = 0; s < nsamples; s++) {
        hipLaunchKernelGGL(k_norm_keys_f64, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, ctx->stream, h_d_counts[s], d_on_target_idx, nk, dKeys);
        double median; rc = norm_median(ctx, dKeys, nk, median); if (rc) return rc;
        P.c[s] = h_d_counts[s]; P.w[s] = median > 0 ? 1.0 / median : 0;
        weightSum += P.w[s];
    }
    for (int s = 0; s < nsamples; s++) { P.w[s] /= weightSum; if (h_weights) h_weights[s] = P.w[s]; }
    hipLaunchKernelGGL(k_norm_weighted, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, P, nsamples, n, d_weighted);
    CANVAS_HIP_TRY(ctx, hipGetLastError());
    return CANVAS_OK;
}

int32_t canvas_normalize_ratio(canvas_ctx* ctx, int64_t n, const float* d_sample, const float* d_reference, const int32_t* d_on_target_idx, int64_t n_on_target,
                               int32_t mode, double min_ref, double max_ref, const int32_t* d_ploidy, int32_t* d_keep_idx, float* d_ratio, float* d_count,
                               int64_t* h_n_out, double* h_library_size_factor) {
    if (!ctx) return CANVAS_ERR_INVALID;
    if (n <= 0 || !d_sample || !d_reference || !d_keep_idx || !d_ratio || !d_count || !h_n_out || (mode != 0 && mode != 1) || (d_on_target_idx && n_on_target <= 0))
        CANVAS_FAIL(ctx, CANVAS_ERR_INVALID, "canvas_normalize_ratio: bad arguments");
    CANVAS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int64_t nk = d_on_target_idx ? n_on_target : n, nblocks = (n + 255) / 256;
    unsigned long long* dKeys; uint32_t* dBlock; long long* dTotal;
    int32_t rc = cvx_ws_carve(ctx, 4096, [&](WsCarver& ws) { ws.take(dKeys, (size_t)nk); ws.take(dBlock, (size_t)nblocks); ws.take(dTotal, 1); }); if (rc) return rc;
    double lsf = 1;
    if (mode == 0) {                                  // LSNormRatioCalculator.cs:29-31
        double sm, rm;
        hipLaunchKernelGGL(k_norm_keys_f32, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, ctx->stream, d_sample, d_on_target_idx, nk, dKeys);
        rc = norm_median(ctx, dKeys, nk, sm); if (rc) return rc;
        hipLaunchKernelGGL(k_norm_keys_f32, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, ctx->stream, d_reference, d_on_target_idx, nk, dKeys);
        rc = norm_median(ctx, dKeys, nk, rm); if (rc) return rc;
        lsf = (sm > 0 && rm > 0) ? rm / sm : 1;
    }
    if (h_library_size_factor) *h_library_size_factor = lsf;
    hipLaunchKernelGGL(k_norm_count, dim3((unsigned)nblocks), dim3(256), 0, ctx->stream, d_reference, n, mode, min_ref, max_ref, dBlock);
    hipLaunchKernelGGL(k_norm_scan, dim3(1), dim3(1024), 0, ctx->stream, dBlock, nblocks, dTotal);
    hipLaunchKernelGGL(k_norm_ratio, dim3((unsigned)nblocks), dim3(256), 0, ctx->stream, d_sample, d_reference, d_ploidy, n, mode, min_ref, max_ref, lsf, dBlock, d_keep_idx, d_ratio, d_count);
    long long total = 0;
    CANVAS_HIP_TRY(ctx, hipMemcpyAsync(&total, dTotal, sizeof total, hipMemcpyDeviceToHost, ctx->stream));
    CANVAS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    CANVAS_HIP_TRY(ctx, hipGetLastError());
    *h_n_out = total;
    return CANVAS_OK;
}

}

// ================================================================================================================================================
// BestLR2ReferenceGenerator.Run (BestLR2ReferenceGenerator.cs:31-80, 83-124) and PCAReferenceGenerator.Run (PCAReferenceGenerator.cs:32-69, 92-148).
// Only WHICH normal BestLR2 picks leaves the module, so its sums of squared log ratios are taken in parallel with an error bound and replayed in the
// reference's order on the host (libm log) only for the normals the bounds cannot separate.  PCA writes its reference counts: the 2-norms of the axes and
// the projection sizes are sequential FP64 chains in the reference's order (one wave per chain, operands staged through LDS, one lane adding); the
// orthogonality test takes a parallel dot with an error bound and a chain only for a pair whose dot lies within the bound of the tolerance.
// ================================================================================================================================================

// deterministic sum of one double per thread over a 256-thread block (tree order fixed by the thread index); the result is valid in thread 0
__device__ __forceinline__ double blk_sum256(double v, double* sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) { if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s]; __syncthreads(); }
    const double r = sh[0];
    __syncthreads();
    return r;
}
#define BLR2_BLOCKS 256
// one term of GetMeanSquaredLogRatios per (bin, normal): partial sums of the kept terms, how many were kept and how many ignored, per block and normal
__global__ void __launch_bounds__(256) k_blr2_partial(const double* __restrict__ tumor, double wt, NormPtrs P, const int32_t* __restrict__ idx, int64_t nk,
                                                      double* __restrict__ psum, double* __restrict__ pkept, double* __restrict__ pign) {
    __shared__ double sh[256];
    const int s = blockIdx.y;
    const gptr<const double> nc = as_global(P.c[s]);
    const double wn = P.w[s];
    double sum = 0, kept = 0, ign = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nk; i += (int64_t)gridDim.x * 256) {
        const int64_t j = idx ? idx[i] : i;
        const double tb = tumor[j] * wt, nb = nc[j] * wn;
        if (nb <= 0) { ign += 1; continue; }
        const double l = log(tb / nb);
        const double sq = l * l;
        if (isinf(sq) || isnan(sq)) { ign += 1; continue; }
        sum += sq; kept += 1;
    }
    sum = blk_sum256(sum, sh); kept = blk_sum256(kept, sh); ign = blk_sum256(ign, sh);
    if (threadIdx.x == 0) { const int64_t o = (int64_t)s * gridDim.x + blockIdx.x; psum[o] = sum; pkept[o] = kept; pign[o] = ign; }
}

// GetMeanSquaredLogRatios (BestLR2ReferenceGenerator.cs:83-124) in the reference's order, libm log: the exact value for one normal
static double blr2_replay(const std::vector<double>& t, double wt, const std::vector<double>& c, double wn, const std::vector<int32_t>& idx) {
    double sum = 0; int nBins = 0;
    const int64_t nk = idx.empty() ? (int64_t)t.size() : (int64_t)idx.size();
    for (int64_t i = 0; i < nk; i++) {
        const int64_t j = idx.empty() ? i : idx[i];
        const double tb = t[j] * wt, nb = c[j] * wn;
        if (nb <= 0) continue;
        const double l = std::log(tb / nb);
        const double sq = l * l;
        if (std::isinf(sq) || std::isnan(sq)) continue;
        sum += sq; nBins++;
    }
    return nBins > 0 ? sum / nBins : sum;
}

// ---- PCA: a table in device memory with the axes (raw, as double.Parse read them), their 2-norms and the projection sizes
#define PCA_MAX_AXES 64
struct PcaTab { const double* a[PCA_MAX_AXES]; double norm[PCA_MAX_AXES]; double size[PCA_MAX_AXES]; };
// NormalizeBy2Norm (Utilities.cs:652-670): a[i] / size, an all-zero axis is kept as it is
__device__ __forceinline__ double pca_unit(gptr<const double> a, double norm, int64_t i) { return norm == 0 ? a[i] : a[i] / norm; }
// the centred sample of PCAReferenceGenerator.cs:38-42: Math.Max(1, count) in float, then (double)count - (double)mu
__device__ __forceinline__ double pca_centred(float c, float mu) { const float cc = 1.0f > c ? 1.0f : c; return (double)cc - (double)mu; }

// One sequential FP64 chain per workgroup of ONE wave: the 64 lanes load the operands of the next chunk while lane 0 adds the products of the current one
// (staged through LDS) one after another in index order, the way the reference's foreach / for loops do (product rounded, then the add; -ffp-contract=off).
//   OP 0  TwoNorm's sum of squares of axis c (Utilities.cs:601-610)
//   OP 1  DotProduct(centred sample, unit axis c) = the projection size (Utilities.cs:672-685, 705-720)
//   OP 2  DotProduct(unit axis i, unit axis j) of pair c (AreOrthogonal, Utilities.cs:687-694)
#define PCA_CHUNK 1024
#define PCA_PER_LANE (PCA_CHUNK / 64)
template <int OP>
__global__ void __launch_bounds__(64) k_pca_chain(const PcaTab* __restrict__ tab, const int2* __restrict__ pairs, const float* __restrict__ cnt, const float* __restrict__ mu,
                                                  int64_t n, double* __restrict__ out) {
    __shared__ double buf[PCA_CHUNK];
    const int c = blockIdx.x, lane = threadIdx.x;
    int ia = c, ib = c;
    if (OP == 2) { const int2 p = pairs[c]; ia = p.x; ib = p.y; }
    const gptr<const double> A = as_global(tab->a[ia]), B = as_global(tab->a[ib]);
    const double nA = tab->norm[ia], nB = tab->norm[ib];
    double ra[PCA_PER_LANE], rb[PCA_PER_LANE]; float rc[PCA_PER_LANE], rm[PCA_PER_LANE];
    auto load = [&](int64_t base) {
#pragma unroll
        for (int t = 0; t < PCA_PER_LANE; t++) {
            const int64_t i = base + t * 64 + lane;
            if (i < n) { ra[t] = A[i]; if (OP == 2) rb[t] = B[i]; if (OP == 1) { rc[t] = cnt[i]; rm[t] = mu[i]; } }
        }
    };
    double acc = 0.0;
    const int64_t nchunks = (n + PCA_CHUNK - 1) / PCA_CHUNK;
    load(0);
    for (int64_t ch = 0; ch < nchunks; ch++) {
        const int64_t base = ch * PCA_CHUNK;
        const int len = (int)min((int64_t)PCA_CHUNK, n - base);
#pragma unroll
        for (int t = 0; t < PCA_PER_LANE; t++) {
            const int k = t * 64 + lane;
            if (k < len) {
                double p;
                if (OP == 0) p = ra[t] * ra[t];
                else if (OP == 1) p = pca_centred(rc[t], rm[t]) * (nA == 0 ? ra[t] : ra[t] / nA);
                else p = (nA == 0 ? ra[t] : ra[t] / nA) * (nB == 0 ? rb[t] : rb[t] / nB);
                buf[k] = p;
            }
        }
        if (ch + 1 < nchunks) load(base + PCA_CHUNK);
        __syncthreads();
        if (lane == 0) {
            int i = 0;
            for (; i + 8 <= len; i += 8) { const double v0 = buf[i], v1 = buf[i + 1], v2 = buf[i + 2], v3 = buf[i + 3], v4 = buf[i + 4], v5 = buf[i + 5], v6 = buf[i + 6], v7 = buf[i + 7];
                acc += v0; acc += v1; acc += v2; acc += v3; acc += v4; acc += v5; acc += v6; acc += v7; }
            for (; i < len; i++) acc += buf[i];
        }
        __syncthreads();
    }
    if (lane == 0) out[c] = acc;
}
// parallel dot of the unit axes of every pair, with the sum of |products| for the error bound: per block and pair
__global__ void __launch_bounds__(256) k_pca_pair_partial(const PcaTab* __restrict__ tab, const int2* __restrict__ pairs, int64_t n, double* __restrict__ pdot, double* __restrict__ pabs) {
    __shared__ double sh[256];
    const int2 p = pairs[blockIdx.y];
    const gptr<const double> A = as_global(tab->a[p.x]), B = as_global(tab->a[p.y]);
    const double nA = tab->norm[p.x], nB = tab->norm[p.y];
    double d = 0, a = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double pr = pca_unit(A, nA, i) * pca_unit(B, nB, i);
        d += pr; a += fabs(pr);
    }
    d = blk_sum256(d, sh); a = blk_sum256(a, sh);
    if (threadIdx.x == 0) { const int64_t o = (int64_t)blockIdx.y * gridDim.x + blockIdx.x; pdot[o] = d; pabs[o] = a; }
}
// Project (Utilities.cs:722-750) + the reference vector (PCAReferenceGenerator.cs:47-48) + its trip through the temporary file: "{F2}" of (float)ref, float.Parse
__global__ void __launch_bounds__(256) k_pca_ref(const PcaTab* __restrict__ tab, int naxes, const float* __restrict__ mu, int64_t n, double* __restrict__ ref, float* __restrict__ refq) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double proj = 0;
    for (int k = 0; k < naxes; k++) {
        const double t = tab->size[k] * pca_unit(as_global(tab->a[k]), tab->norm[k], i);
        proj = k == 0 ? t : proj + t;
    }
    const double x = (double)mu[i] + proj;
    const double r = 1.0 > x ? 1.0 : x;                                   // Math.Max(1, x): NaN stays NaN
    ref[i] = r;
    refq[i] = (float)quantize_f2_one((float)r);
}
__global__ void __launch_bounds__(256) k_pca_out(const double* __restrict__ ref, int64_t n, double medianRatio, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (float)(ref[i] * medianRatio);
}

extern "C" {

int32_t canvas_normalize_best_normal(canvas_ctx* ctx, const double* d_tumor, int32_t nnormals, const double* const* h_d_normals, int64_t n, const int32_t* d_on_target_idx,
                                     int64_t n_on_target, int32_t* h_best, double* h_mean_sq_log_ratio, int64_t* h_ignored, int32_t* h_replayed) {
    if (!ctx) return CANVAS_ERR_INVALID;
    if (!d_tumor || nnormals <= 0 || nnormals > NORM_MAX_SAMPLES || !h_d_normals || n <= 0 || !h_best || (d_on_target_idx && n_on_target <= 0))
        CANVAS_FAIL(ctx, CANVAS_ERR_INVALID, "canvas_normalize_best_normal: bad arguments");
    for (int s = 0; s < nnormals; s++) if (!h_d_normals[s]) CANVAS_FAIL(ctx, CANVAS_ERR_INVALID, "canvas_normalize_best_normal: bad arguments");
    CANVAS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int64_t nk = d_on_target_idx ? n_on_target : n;
    const int nb = (int)std::min<int64_t>(BLR2_BLOCKS, (nk + 255) / 256);
    unsigned long long* dKeys; double *dSum, *dKept, *dIgn; const size_t nPart = (size_t)nb * nnormals;
    int32_t rc = cvx_ws_carve(ctx, 4096, [&](WsCarver& ws) { ws.take(dKeys, (size_t)nk); ws.take(dSum, nPart); ws.take(dKept, nPart); ws.take(dIgn, nPart); }); if (rc) return rc;
    // weight = 1 / OnTargetMedianBinCount, 0 when the median is not positive (BestLR2ReferenceGenerator.cs:41-58)
    auto weight_of = [&](const double* d, double& w) -> int32_t {
        hipLaunchKernelGGL(k_norm_keys_f64, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, ctx->stream, d, d_on_target_idx, nk, dKeys);
        double median; int32_t r = norm_median(ctx, dKeys, nk, median); if (r) return r;
        w = median > 0 ? 1.0 / median : 0; return CANVAS_OK;
    };
    NormPtrs P;
    for (int s = 0; s < nnormals; s++) { P.c[s] = h_d_normals[s]; rc = weight_of(h_d_normals[s], P.w[s]); if (rc) return rc; }
    double wt; rc = weight_of(d_tumor, wt); if (rc) return rc;
    hipLaunchKernelGGL(k_blr2_partial, dim3((unsigned)nb, (unsigned)nnormals), dim3(256), 0, ctx->stream, d_tumor, wt, P, d_on_target_idx, nk, dSum, dKept, dIgn);
    std::vector<double> hs((size_t)nb * nnormals), hk((size_t)nb * nnormals), hi((size_t)nb * nnormals);
    CANVAS_HIP_TRY(ctx, hipMemcpyAsync(hs.data(), dSum, hs.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    CANVAS_HIP_TRY(ctx, hipMemcpyAsync(hk.data(), dKept, hk.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    CANVAS_HIP_TRY(ctx, hipMemcpyAsync(hi.data(), dIgn, hi.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    CANVAS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    CANVAS_HIP_TRY(ctx, hipGetLastError());
    // mean of every normal from the parallel sum, and a bound on its distance to the reference's sequential value:
    //   both sums are within gamma_(m-1) * sum|terms| of the exact sum of their own terms (any summation order), the device's log and glibc's are within
    //   a few ulps of each other (squared: 16 ulps of the term allowed), and the division by m adds an ulp on each side
    std::vector<double> mean(nnormals), err(nnormals);
    const double u = std::ldexp(1.0, -53), ulp = std::ldexp(1.0, -52);
    for (int s = 0; s < nnormals; s++) {
        double T = 0, m = 0, ig = 0;
        for (int b = 0; b < nb; b++) { T += hs[(size_t)s * nb + b]; m += hk[(size_t)s * nb + b]; ig += hi[(size_t)s * nb + b]; }
        mean[s] = m > 0 ? T / m : T;
        err[s] = (m > 0 ? T / m : T) * (2.5 * m * u + 48 * ulp);
        if (h_ignored) h_ignored[s] = (int64_t)ig;
    }
    int best = -1; double minMean = HUGE_VAL;
    for (int s = 0; s < nnormals; s++) if (mean[s] < minMean) { minMean = mean[s]; best = s; }
    if (best < 0) best = 0;
    const double hiBest = mean[best] + err[best];
    std::vector<int> contenders;
    for (int s = 0; s < nnormals; s++) if (s == best || mean[s] - err[s] <= hiBest) contenders.push_back(s);
    int replayed = 0;
    if (contenders.size() > 1) {
        // a normal outside the set is above the best one's upper bound: it can neither win nor tie.  The contenders are replayed exactly, in index order
        std::vector<double> ht((size_t)n), hc((size_t)n); std::vector<int32_t> hidx;
        CANVAS_HIP_TRY(ctx, hipMemcpyAsync(ht.data(), d_tumor, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
        if (d_on_target_idx) { hidx.resize((size_t)nk); CANVAS_HIP_TRY(ctx, hipMemcpyAsync(hidx.data(), d_on_target_idx, (size_t)nk * 4, hipMemcpyDeviceToHost, ctx->stream)); }
        CANVAS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        for (int64_t i = 0; i < (int64_t)hidx.size(); i++) if (hidx[i] < 0 || hidx[i] >= n) CANVAS_FAIL(ctx, CANVAS_ERR_INVALID, "canvas_normalize_best_normal: on-target index out of range");
        double exMin = HUGE_VAL; int exBest = -1;
        for (int s : contenders) {
            CANVAS_HIP_TRY(ctx, hipMemcpyAsync(hc.data(), h_d_normals[s], (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
            CANVAS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            mean[s] = blr2_replay(ht, wt, hc, P.w[s], hidx);
            replayed++;
            if (mean[s] < exMin) { exMin = mean[s]; exBest = s; }       // strict <: the first normal wins a tie (BestLR2ReferenceGenerator.cs:71)
        }
        if (exBest >= 0) best = exBest;
    }
    *h_best = best;
    if (h_mean_sq_log_ratio) for (int s = 0; s < nnormals; s++) h_mean_sq_log_ratio[s] = mean[s];
    if (h_replayed) *h_replayed = replayed;
    return CANVAS_OK;
}

int32_t canvas_normalize_pca_reference(canvas_ctx* ctx, int64_t n, const float* d_sample, const float* d_mu, int32_t naxes, const double* const* h_d_axes,
                                       double min_ref, double max_ref, float* d_reference, double* h_median_ratio, double* h_sizes, int32_t* h_orthogonal) {
    if (!ctx) return CANVAS_ERR_INVALID;
    if (n <= 0 || n > 0x7FFFFFFFll || !d_sample || !d_mu || naxes <= 0 || naxes > PCA_MAX_AXES || !h_d_axes || !d_reference || !h_orthogonal)
        CANVAS_FAIL(ctx, CANVAS_ERR_INVALID, "canvas_normalize_pca_reference: bad arguments");
    for (int k = 0; k < naxes; k++) if (!h_d_axes[k]) CANVAS_FAIL(ctx, CANVAS_ERR_INVALID, "canvas_normalize_pca_reference: bad arguments");
    CANVAS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int npairs = naxes * (naxes - 1) / 2;
    const int64_t nblocks = (n + 255) / 256;
    const int nb = (int)std::min<int64_t>(256, nblocks);
    PcaTab* dTab; double *dChain, *dPairChain, *dDot, *dAbs, *dRef; int2* dPairs; float *dRefQ, *dRatio, *dCount; int32_t* dKeep; unsigned long long* dKeys; uint32_t* dBlock; long long* dTotal;
    int32_t rc = cvx_ws_carve(ctx, 4096, [&](WsCarver& ws) {
        ws.take(dTab, 1); ws.take(dChain, PCA_MAX_AXES); ws.take(dPairs, (size_t)npairs + 1); ws.take(dPairChain, (size_t)npairs + 1);
        ws.take(dDot, (size_t)nb * npairs + 1); ws.take(dAbs, (size_t)nb * npairs + 1);
        ws.take(dRef, (size_t)n); ws.take(dRefQ, (size_t)n); ws.take(dKeep, (size_t)n); ws.take(dRatio, (size_t)n); ws.take(dCount, (size_t)n);
        ws.take(dKeys, (size_t)n); ws.take(dBlock, (size_t)nblocks); ws.take(dTotal, 1);
    });
    if (rc) return rc;

    PcaTab T; memset(&T, 0, sizeof T);
    for (int k = 0; k < naxes; k++) T.a[k] = h_d_axes[k];
    // 1. TwoNorm of every axis: naxes chains side by side; the square root on the host (correctly rounded, as Math.Sqrt)
    CANVAS_HIP_TRY(ctx, hipMemcpyAsync(dTab, &T, sizeof T, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_pca_chain<0>, dim3((unsigned)naxes), dim3(64), 0, ctx->stream, dTab, (const int2*)nullptr, (const float*)nullptr, (const float*)nullptr, n, dChain);
    double sq[PCA_MAX_AXES];
    CANVAS_HIP_TRY(ctx, hipMemcpyAsync(sq, dChain, (size_t)naxes * 8, hipMemcpyDeviceToHost, ctx->stream));
    CANVAS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < naxes; k++) T.norm[k] = std::sqrt(sq[k]);
    CANVAS_HIP_TRY(ctx, hipMemcpyAsync(dTab, &T, sizeof T, hipMemcpyHostToDevice, ctx->stream));
    // 2. AreOrthogonal over every pair (PCAReferenceGenerator.cs:129-140): |DotProduct| > 1e-4 fails.  The parallel dot and the reference's sequential one are
    //    both within gamma_(n-1) * sum|products| of the exact sum of the same rounded products; only a pair whose parallel dot lies within twice that of the
    //    tolerance is summed again by a chain
    int orth = 1;
    if (npairs > 0) {
        std::vector<int2> pr; for (int i = 0; i < naxes; i++) for (int j = i + 1; j < naxes; j++) pr.push_back(make_int2(i, j));
        CANVAS_HIP_TRY(ctx, hipMemcpyAsync(dPairs, pr.data(), pr.size() * sizeof(int2), hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(k_pca_pair_partial, dim3((unsigned)nb, (unsigned)npairs), dim3(256), 0, ctx->stream, dTab, dPairs, n, dDot, dAbs);
        std::vector<double> hd((size_t)nb * npairs), ha((size_t)nb * npairs);
        CANVAS_HIP_TRY(ctx, hipMemcpyAsync(hd.data(), dDot, hd.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
        CANVAS_HIP_TRY(ctx, hipMemcpyAsync(ha.data(), dAbs, ha.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
        CANVAS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        CANVAS_HIP_TRY(ctx, hipGetLastError());
        const double u = std::ldexp(1.0, -53), tol = 1e-4;
        std::vector<int2> undecided;
        for (int p = 0; p < npairs && orth; p++) {
            double d = 0, a = 0;
            for (int b = 0; b < nb; b++) { d += hd[(size_t)p * nb + b]; a += ha[(size_t)p * nb + b]; }
            const double B = a * (2.5 * (double)n * u) + 1e-300;
            if (std::isnan(d) || std::fabs(d) - B > tol) orth = 0;
            else if (std::fabs(d) + B >= tol) undecided.push_back(pr[(size_t)p]);
        }
        if (orth && !undecided.empty()) {
            CANVAS_HIP_TRY(ctx, hipMemcpyAsync(dPairs, undecided.data(), undecided.size() * sizeof(int2), hipMemcpyHostToDevice, ctx->stream));
            hipLaunchKernelGGL(k_pca_chain<2>, dim3((unsigned)undecided.size()), dim3(64), 0, ctx->stream, dTab, (const int2*)dPairs, (const float*)nullptr, (const float*)nullptr, n, dPairChain);
            std::vector<double> ex(undecided.size());
            CANVAS_HIP_TRY(ctx, hipMemcpyAsync(ex.data(), dPairChain, ex.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
            CANVAS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            for (double v : ex) if (std::fabs(v) > tol || std::isnan(v)) orth = 0;
        }
    }
    *h_orthogonal = orth;
    if (!orth) return CANVAS_OK;         // the reference throws while loading the model: nothing is written
    // 3. the projection sizes: naxes chains, written straight into the table
    hipLaunchKernelGGL(k_pca_chain<1>, dim3((unsigned)naxes), dim3(64), 0, ctx->stream, dTab, (const int2*)nullptr, d_sample, d_mu, n, dTab->size);
    // 4. reference vector and its F2 round trip; 5. RawRatioCalculator over the unclamped sample with [min_ref, max_ref] (mode 1 of canvas_normalize_ratio)
    hipLaunchKernelGGL(k_pca_ref, dim3((unsigned)nblocks), dim3(256), 0, ctx->stream, dTab, naxes, d_mu, n, dRef, dRefQ);
    hipLaunchKernelGGL(k_norm_count, dim3((unsigned)nblocks), dim3(256), 0, ctx->stream, dRefQ, n, 1, min_ref, max_ref, dBlock);
    hipLaunchKernelGGL(k_norm_scan, dim3(1), dim3(1024), 0, ctx->stream, dBlock, nblocks, dTotal);
    hipLaunchKernelGGL(k_norm_ratio, dim3((unsigned)nblocks), dim3(256), 0, ctx->stream, d_sample, dRefQ, (const int32_t*)nullptr, n, 1, min_ref, max_ref, 1.0, dBlock, dKeep, dRatio, dCount);
    long long kept = 0; double sizes[PCA_MAX_AXES];
    CANVAS_HIP_TRY(ctx, hipMemcpyAsync(&kept, dTotal, sizeof kept, hipMemcpyDeviceToHost, ctx->stream));
    CANVAS_HIP_TRY(ctx, hipMemcpyAsync(sizes, dTab->size, (size_t)naxes * 8, hipMemcpyDeviceToHost, ctx->stream));
    CANVAS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    CANVAS_HIP_TRY(ctx, hipGetLastError());
    if (h_sizes) for (int k = 0; k < naxes; k++) h_sizes[k] = sizes[k];
    // 6. medianRatio = BinCounts(ratios).OnTargetMedianBinCount: the median of the kept ratios, floats widened to double (PCAReferenceGenerator.cs:56-57)
    double medianRatio = 0;
    if (kept > 0) {
        hipLaunchKernelGGL(k_norm_keys_f32, dim3((unsigned)((kept + 255) / 256)), dim3(256), 0, ctx->stream, dRatio, (const int32_t*)nullptr, (int64_t)kept, dKeys);
        rc = norm_median(ctx, dKeys, kept, medianRatio); if (rc) return rc;
    }
    if (h_median_ratio) *h_median_ratio = medianRatio;
    // 7. (float)(ref * medianRatio) with ref the double of step 4 (PCAReferenceGenerator.cs:62-64)
    hipLaunchKernelGGL(k_pca_out, dim3((unsigned)nblocks), dim3(256), 0, ctx->stream, dRef, n, medianRatio, d_reference);
    CANVAS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    CANVAS_HIP_TRY(ctx, hipGetLastError());
    return CANVAS_OK;
}

}
