// (canvas_call_somatic, CanvasSomaticCaller's calls around the model fit, is the last section of this file: it shares the site kernels and the selects below.)
// CanvasDiploidCaller, first layer: exact order statistics of MANY segments of a float32 array in one fixed sequence of launches (canvas_segment_select).
// The caller's per-segment numbers are all of this kind: medianCoverage = Utilities.Median(float[]) of a segment's counts (CanvasDiploidCaller.cs, AssignPloidyCallsDistance),
// medianMaf = the median of its folded allele frequencies widened to double, MedianCount of a merged run (CanvasSegment.cs, doubles converted from floats), and the
// "upper median" a[n/2] of the 100 kb points of WriteCoveragePlotData (CanvasSegment.cs:696-697).  Segments run from one bin to a chromosome arm (a few 10^5 bins) and there
// are up to ~10^5 of them, so neither one launch nor one workgroup per segment will do (k_wv_segment_median, wavelets.hip, is that form: right for a few hundred stretches).
//
// The keys are the order-preserving 32-bit images of the floats (select.hpp: key_of_float), so the selected key IS the order statistic bit for bit; only the final average of
// an even-length median is arithmetic, in float ((a + b) / 2f) or in double (((double)a + (double)b) / 2), which is why one kernel family serves every mode.
//
// The host has the offsets, so it sorts the segments into three classes and uploads the lists of the classes as one pinned blob (one asynchronous copy); a class that has no segment is not launched:
//   WAVE   n <= 64            k_call_wave: one wave per segment, four segments per workgroup at a time (grid-stride).  Lane i holds key i; its rank is
//                             #{key_j < key_i} + #{j < i : key_j == key_i}, counted with 64 lane broadcasts — a permutation of 0 .. n-1, ties included.  Empty segments
//                             are written here (0).  Bytes: 4 n read, 8 written.
//   LDS    64 < n <= 8192     k_call_lds: one workgroup of 256 per segment stages the keys ONCE (32 KiB) and runs the four 8-bit MSB radix passes over LDS for both ranks of
//                             an even-length median.  32 KiB keys + 2 KiB histograms = 34 KiB per workgroup: four workgroups (16 waves) fit the 160 KiB of a CU, which is the
//                             occupancy the global load of the staging wants; a larger tile would leave two.  Counts of one segment share their exponent byte, so a wave
//                             aggregates equal digits with ballots before it touches LDS (as select_hist_body does).  Bytes: 4 n read, 8 written.
//   TILED  n > 8192           the multi-pass form of select.hpp over tiles of SEL_TILE keys: select_hist_body (with a map from value to key, so there is no key array) and
//                             k_select_pick, four times, then k_call_tiled_out.  Bytes: 4 passes x 4 n read; histograms 16 KiB per rank (SEL_REP replicas).
// At most 1 + 1 + 9 launches, whatever S is.  Every class reads every one of its keys in a first sweep and reports the first non-finite one (CANVAS_ERR_INVALID, as canvas_smooth).
// CANVAS_CALL_CLASS=wave|lds|tiled (a test hook) sends every non-empty segment the named class can hold to it: the classes are compared bit for bit in the tests.
#include "select.hpp"
#include <algorithm>

#define CL_WAVE_MAX 64
#define CL_LDS_MAX 8192                                  // keys per LDS tile (see above)
#define CL_BLOCK 256
#define CL_MODE_MEDIAN_F32 0                               // a[n/2] (odd n), (a[n/2-1] + a[n/2]) / 2 in float (even n): Utilities.Median(IEnumerable<float>)
#define CL_MODE_MEDIAN_F64 1                               // ... the average in double: SortedList<double>.Median() over floats widened to double
#define CL_MODE_UPPER 2                                    // a[n/2]

struct ClItem { long long off; int n; int seg; };       // WAVE / LDS classes: keys [off, off + n) -> out[seg]
struct ClBig { int seg; int q0; int q1; };              // TILED class: ranks q0 (and q1, or -1) of the select -> out[seg]

__device__ __forceinline__ bool cl_finite(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }
// the two ranks of a segment of n >= 1 keys (equal unless the mode is a median and n is even)
__host__ __device__ static inline void cl_ranks(long long n, int mode, long long& r0, long long& r1) { r1 = n >> 1; r0 = (mode == CL_MODE_UPPER || (n & 1)) ? r1 : r1 - 1; }
__device__ __forceinline__ double cl_value(uint32_t k0, uint32_t k1, bool two, int mode) {
    const float a = float_of_key(k0), b = float_of_key(k1);
    if (!two) return (double)b;
    return mode == CL_MODE_MEDIAN_F32 ? (double)((a + b) / 2.0f) : ((double)a + (double)b) / 2.0;
}

__global__ void __launch_bounds__(CL_BLOCK) k_call_wave(const float* __restrict__ vals, const ClItem* __restrict__ items, long long nitems, int mode, double* __restrict__ out,
                                                        unsigned long long* __restrict__ firstBad) {
    const int lane = threadIdx.x & 63;
    const long long stride = (long long)gridDim.x * (CL_BLOCK / 64);
    for (long long it = (long long)blockIdx.x * (CL_BLOCK / 64) + (threadIdx.x >> 6); it < nitems; it += stride) {       // (wave-uniform)
        const ClItem I = items[it];
        const int n = __builtin_amdgcn_readfirstlane(I.n);                                                             // n <= 64 (host); the same in every lane
        if (n == 0) { if (lane == 0) out[I.seg] = 0.0; continue; }
        const bool in = lane < n;
        const float v = in ? vals[I.off + lane] : 0.0f;
        if (in && !cl_finite(v)) atomicMin(firstBad, (unsigned long long)(I.off + lane));
        const uint32_t key = key_of_float(v);
        int cnt = 0;
        for (int j = 0; j < n; j++) { const uint32_t kj = (uint32_t)__builtin_amdgcn_readlane((int)key, j); cnt += (kj < key || (kj == key && j < lane)) ? 1 : 0; }
        long long r0, r1; cl_ranks(n, mode, r0, r1);
        const unsigned long long m0 = __ballot(in && cnt == (int)r0), m1 = __ballot(in && cnt == (int)r1);             // one lane each: the ranks are a permutation
        const uint32_t k0 = (uint32_t)__builtin_amdgcn_readlane((int)key, __builtin_ctzll(m0 | (1ull << 63)));
        const uint32_t k1 = (uint32_t)__builtin_amdgcn_readlane((int)key, __builtin_ctzll(m1 | (1ull << 63)));
        if (lane == 0) out[I.seg] = cl_value(k0, k1, r0 != r1, mode);
    }
}

// one histogram increment per lane with m set, equal (row, digit) cells of a wave folded into one LDS atomic; every lane of the wave calls this
__device__ __forceinline__ void cl_hist_add(uint32_t* h, bool m, uint32_t cell, int lane) {
    unsigned long long todo = __ballot(m);
    for (int it = 0; it < 4 && todo; it++) {
        const int leader = __builtin_ctzll(todo);
        const uint32_t cl = (uint32_t)__builtin_amdgcn_readlane((int)cell, leader);
        const unsigned long long same = __ballot(m && cell == cl) & todo;
        if (lane == leader) atomicAdd(&h[cl], (uint32_t)__builtin_popcountll(same));
        todo &= ~same;
    }
    if ((todo >> lane) & 1ull) atomicAdd(&h[cell], 1u);
}

__global__ void __launch_bounds__(CL_BLOCK) k_call_lds(const float* __restrict__ vals, const ClItem* __restrict__ items, int mode, double* __restrict__ out,
                                                       unsigned long long* __restrict__ firstBad) {
    __shared__ uint32_t sm[CL_LDS_MAX + 512 + 4];            // one array: keys | two histogram rows | prefix[2] | rank[2]
    uint32_t* sKey = sm; uint32_t* sH = sm + CL_LDS_MAX; uint32_t* sPre = sH + 512; uint32_t* sK = sPre + 2;
    const ClItem I = items[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, n = I.n;   // 1 <= n <= CL_LDS_MAX (host)
    for (int i = tid; i < n; i += CL_BLOCK) {
        const float v = vals[I.off + i];
        if (!cl_finite(v)) atomicMin(firstBad, (unsigned long long)(I.off + i));
        sKey[i] = key_of_float(v);
    }
    long long r0, r1; cl_ranks(n, mode, r0, r1);
    if (tid == 0) { sPre[0] = 0; sPre[1] = 0; sK[0] = (uint32_t)r0; sK[1] = (uint32_t)r1; }
    const int nround = (n + 63) & ~63;                       // whole waves go through the key loop (ballots inside)
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int i = tid; i < 512; i += CL_BLOCK) sH[i] = 0;
        __syncthreads();
        const uint32_t p0 = sPre[0], p1 = sPre[1];
        const bool same = p0 == p1;
        for (int i = tid; i < nround; i += CL_BLOCK) {
            const bool in = i < n;
            const uint32_t key = in ? sKey[i] : 0u;
            const uint32_t hi = shift == 24 ? 0u : key >> (shift + 8);
            const int row = hi == p0 ? 0 : ((!same && hi == p1) ? 1 : -1);       // the two prefixes differ when !same: a key matches at most one
            cl_hist_add(sH, in && row >= 0, (uint32_t)(row < 0 ? 0 : row) * 256u + ((key >> shift) & 255u), lane);
        }
        __syncthreads();
        const int w = tid >> 6;
        if (w < 2) {
            const uint32_t* h = sH + (same ? 0 : w) * 256;
            const uint32_t c0 = h[4 * lane], c1 = h[4 * lane + 1], c2 = h[4 * lane + 2], c3 = h[4 * lane + 3];
            const uint32_t sum = c0 + c1 + c2 + c3, inc = wave_inclusive_scan_u32(sum), ex = inc - sum;
            const uint32_t k = sK[w];
            if (k >= ex && k < inc) {
                uint32_t r = k - ex, d;
                if (r < c0) { d = 0; } else if (r < c0 + c1) { d = 1; r -= c0; } else if (r < c0 + c1 + c2) { d = 2; r -= c0 + c1; } else { d = 3; r -= c0 + c1 + c2; }
                sPre[w] = (sPre[w] << 8) | (uint32_t)(4 * lane + d);
                sK[w] = r;
            }
        }
        __syncthreads();
    }
    if (tid == 0) out[I.seg] = cl_value(sPre[0], sPre[1], r0 != r1, mode);
}

// TILED class: the values are mapped to their keys as select_hist_body loads them; the first pass (which sees every key) reports the non-finite ones
struct ClFloatKey {
    unsigned long long* firstBad;                            // null after the first pass
    __device__ __forceinline__ uint32_t operator()(float v, int64_t i) const {
        if (firstBad && !cl_finite(v)) atomicMin(firstBad, (unsigned long long)i);
        return key_of_float(v);
    }
};
__global__ void __launch_bounds__(256) k_call_tiled_hist(const float* __restrict__ vals, const SelTile* __restrict__ tiles, const SelSegQ* __restrict__ segq,
                                                         const unsigned long long* __restrict__ qprefix, int shift, int firstPass, uint32_t* __restrict__ hist, int nq,
                                                         unsigned long long* __restrict__ firstBad) {
    select_hist_body<uint32_t, float, ClFloatKey>(vals, tiles, segq, qprefix, shift, firstPass, hist, nq, nullptr, ClFloatKey{firstBad});
}
__global__ void __launch_bounds__(CL_BLOCK) k_call_tiled_out(const ClBig* __restrict__ big, int nbig, const unsigned long long* __restrict__ qprefix, int mode, double* __restrict__ out) {
    const int b = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (b >= nbig) return;
    const ClBig B = big[b];
    const uint32_t k0 = (uint32_t)qprefix[B.q0], k1 = (uint32_t)qprefix[B.q1 < 0 ? B.q0 : B.q1];
    out[B.seg] = cl_value(k0, k1, B.q1 >= 0, mode);
}

// 0 no forcing, else the class every non-empty segment that fits is sent to
static int cl_forced_class() {
    const char* e = cvx_hook("CANVAS_CALL_CLASS");
    if (!e || !*e) return 0;
    return !strcmp(e, "wave") ? 1 : !strcmp(e, "lds") ? 2 : !strcmp(e, "tiled") ? 3 : 0;
}
static int cl_class_of(long long n, int forced) {
    if (n == 0) return 1;
    if (forced == 3) return 3;
    if (forced == 2 && n <= CL_LDS_MAX) return 2;
    return n <= CL_WAVE_MAX ? 1 : n <= CL_LDS_MAX ? 2 : 3;   // (forced == 1 is the default rule: the wave class holds nothing larger)
}

static int32_t cl_check_offsets(int64_t nseg, const int64_t* h_seg_offset, int32_t mode, std::string& why) {
    if (nseg < 0 || nseg > 0x7FFFFFFFll || !h_seg_offset) { why = "canvas_segment_select: bad arguments (0 .. 2^31-1 segments, offsets of nseg + 1 entries)"; return CANVAS_ERR_INVALID; }
    if (mode < 0 || mode > 2) { why = "canvas_segment_select: mode is 0 (median, float average), 1 (median, double average) or 2 (upper median)"; return CANVAS_ERR_INVALID; }
    if (h_seg_offset[0] < 0) { why = "canvas_segment_select: the offsets must not be negative"; return CANVAS_ERR_INVALID; }
    for (int64_t s = 0; s < nseg; s++) if (h_seg_offset[s + 1] < h_seg_offset[s]) { why = "canvas_segment_select: the segment offsets must be non-decreasing"; return CANVAS_ERR_INVALID; }
    return CANVAS_OK;
}

extern "C" int32_t canvas_segment_select_plan(int64_t* h_out6) {
    if (!h_out6) return CANVAS_ERR_INVALID;
    h_out6[0] = CL_WAVE_MAX; h_out6[1] = CL_LDS_MAX; h_out6[2] = SEL_TILE; h_out6[3] = 1 + 1 + 2 * 4 + 1; h_out6[4] = cl_forced_class(); h_out6[5] = 0;
    return CANVAS_OK;
}

// everything of canvas_segment_select up to its last kernel and the copy of its flag: no synchronisation; *h_bad (pinned) holds the first non-finite index or ~0 once the stream
// has run.  The lists live in ctx->ws and are dead when the kernels have run: a second select may be enqueued behind this one (canvas_call_diploid)
static int32_t cl_segment_select_enqueue(canvas_ctx* ctx, const float* d_values, int64_t nseg, const int64_t* off, int32_t mode, double* d_out, unsigned long long* h_bad) {
    const int forced = cl_forced_class();
    std::vector<ClItem> wave, lds; std::vector<ClBig> big; std::vector<SelTile> tiles; std::vector<SelSegQ> segq; std::vector<unsigned long long> ranks;
    for (int64_t s = 0; s < nseg; s++) {
        const long long o = off[s], n = off[s + 1] - o;
        const int c = cl_class_of(n, forced);
        if (c == 1) wave.push_back({o, (int)n, (int)s});
        else if (c == 2) lds.push_back({o, (int)n, (int)s});
        else {
            long long r0, r1; cl_ranks(n, mode, r0, r1);
            SelSegQ Q; memset(&Q, 0, sizeof(Q));
            ClBig B{(int)s, (int)ranks.size(), -1};
            Q.q[Q.nq++] = (int)ranks.size(); ranks.push_back((unsigned long long)r0);
            if (r1 != r0) { B.q1 = (int)ranks.size(); Q.q[Q.nq++] = (int)ranks.size(); ranks.push_back((unsigned long long)r1); }
            for (long long b = o; b < o + n; b += SEL_TILE) tiles.push_back({(int32_t)segq.size(), b, std::min<long long>(b + SEL_TILE, o + n)});
            segq.push_back(Q); big.push_back(B);
            if (tiles.size() > 0x7FFFFFFFull || ranks.size() > 0x3FFFFFFFull) CANVAS_FAIL(ctx, CANVAS_ERR_INVALID, "canvas_segment_select: too many tiles in one call");
        }
    }
    const size_t nq = ranks.size(), histWords = nq * 256 * SEL_REP;
    // the flag and every list travel as ONE pinned blob with the layout of the device workspace (one asynchronous copy, no wait, whatever S is); the blob is reused by the
    // next select, which first waits for the event behind this copy — the copy only, not the kernels
    unsigned long long *dBad, *dK, *dPrefix, *hBad, *hK; ClItem *dWave, *dLds, *hWave, *hLds; ClBig *dBig, *hBig; SelTile *dTiles, *hTiles; SelSegQ *dSegq, *hSegq; uint32_t* dHist;
    auto blob = [&](WsCarver& c, unsigned long long*& bad, ClItem*& w, ClItem*& l, ClBig*& b, SelTile*& t, SelSegQ*& q, unsigned long long*& k) {
        c.take(bad, 1); c.take(w, wave.size()); c.take(l, lds.size()); c.take(b, big.size()); c.take(t, tiles.size()); c.take(q, segq.size()); c.take(k, nq);
    };
    int32_t rc = cvx_ws_carve(ctx, 256, [&](WsCarver& cv) { blob(cv, dBad, dWave, dLds, dBig, dTiles, dSegq, dK); cv.take(dPrefix, nq); cv.take(dHist, histWords); }); if (rc) return rc;
    size_t blobBytes = 0;
    rc = ws_layout_carve("canvas_segment_select: staging layout", 256, CANVAS_ERR_HIP, &ctx->err, [&](size_t need, void** base) -> int32_t {
        if (!ctx->call_pin_ev) CANVAS_HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->call_pin_ev, hipEventDisableTiming));
        else CANVAS_HIP_TRY(ctx, hipEventSynchronize(ctx->call_pin_ev));
        const size_t b = need - 256;
        const int32_t rcg = cvx_grow_pinned(ctx, &ctx->call_pin, &ctx->call_pin_bytes, need, b + b / 4 + (64u << 10)); *base = ctx->call_pin; return rcg;
    }, [&](WsCarver& hv) { blob(hv, hBad, hWave, hLds, hBig, hTiles, hSegq, hK); }, &blobBytes);
    if (rc) return rc;
    *hBad = ~0ull;
    if (!wave.empty()) memcpy(hWave, wave.data(), wave.size() * sizeof(ClItem));
    if (!lds.empty()) memcpy(hLds, lds.data(), lds.size() * sizeof(ClItem));
    if (!big.empty()) memcpy(hBig, big.data(), big.size() * sizeof(ClBig));
    if (!tiles.empty()) memcpy(hTiles, tiles.data(), tiles.size() * sizeof(SelTile));
    if (!segq.empty()) memcpy(hSegq, segq.data(), segq.size() * sizeof(SelSegQ));
    if (nq) memcpy(hK, ranks.data(), nq * sizeof(unsigned long long));
    CANVAS_HIP_TRY(ctx, hipMemcpyAsync(ctx->ws, ctx->call_pin, blobBytes, hipMemcpyHostToDevice, ctx->stream));
    CANVAS_HIP_TRY(ctx, hipEventRecord(ctx->call_pin_ev, ctx->stream));
    if (!wave.empty()) {
        const unsigned grid = (unsigned)std::min<size_t>((wave.size() + CL_BLOCK / 64 - 1) / (CL_BLOCK / 64), 8192);
        ProfScope ps(ctx, "call_select_wave");
        hipLaunchKernelGGL(k_call_wave, dim3(grid), dim3(CL_BLOCK), 0, ctx->stream, d_values, dWave, (long long)wave.size(), (int)mode, d_out, dBad);
    }
    if (!lds.empty()) {
        ProfScope ps(ctx, "call_select_lds");
        hipLaunchKernelGGL(k_call_lds, dim3((unsigned)lds.size()), dim3(CL_BLOCK), 0, ctx->stream, d_values, dLds, (int)mode, d_out, dBad);
    }
    if (!big.empty()) {
        CANVAS_HIP_TRY(ctx, hipMemsetAsync(dHist, 0, histWords * sizeof(uint32_t), ctx->stream));          // (k_select_pick leaves the rows it read cleared; the workspace is shared with other calls)
        ProfScope ps(ctx, "call_select_tiled");
        for (int shift = 24; shift >= 0; shift -= 8) {
            const int first = shift == 24 ? 1 : 0;
            hipLaunchKernelGGL(k_call_tiled_hist, dim3((unsigned)tiles.size()), dim3(256), 0, ctx->stream, d_values, dTiles, dSegq, dPrefix, shift, first, dHist, (int)nq, first ? dBad : nullptr);
            hipLaunchKernelGGL(k_select_pick, dim3((unsigned)nq), dim3(64), 0, ctx->stream, dHist, dPrefix, dK, (int)nq, first, (const uint32_t*)nullptr);
        }
        hipLaunchKernelGGL(k_call_tiled_out, dim3((unsigned)((big.size() + CL_BLOCK - 1) / CL_BLOCK)), dim3(CL_BLOCK), 0, ctx->stream, dBig, (int)big.size(), dPrefix, (int)mode, d_out);
    }
    CANVAS_HIP_TRY(ctx, hipGetLastError());
    CANVAS_HIP_TRY(ctx, hipMemcpyAsync(h_bad, dBad, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    return CANVAS_OK;
}

// cvx_ws_carve for ctx->call_ws: what a caller keeps across the selects it enqueues (they carve ctx->ws); grow-only, by a quarter and 1 MB
template <class Layout> static int32_t cl_call_ws_carve(canvas_ctx* ctx, Layout&& layout, const char* site = __builtin_FUNCTION()) {
    return ws_layout_carve(site, 256, CANVAS_ERR_HIP, &ctx->err, [&](size_t need, void** base) {
        const size_t b = need - 256;
        const int32_t rc = cvx_grow_device(ctx, &ctx->call_ws, &ctx->call_ws_bytes, need, b + b / 4 + (1u << 20), ctx->stream); *base = ctx->call_ws; return rc;
    }, layout);
}

extern "C" int32_t canvas_segment_select(canvas_ctx* ctx, const float* d_values, int64_t nseg, const int64_t* h_seg_offset, int32_t mode, double* d_out, int64_t* h_nempty) {
    // the offsets and the mode are checked first and without the context (no message then): *h_nempty is written only when they have passed
    std::string why;
    if (cl_check_offsets(nseg, h_seg_offset, mode, why)) { if (ctx) ctx->err = why; return CANVAS_ERR_INVALID; }
    int64_t empty = 0;
    for (int64_t s = 0; s < nseg; s++) empty += h_seg_offset[s + 1] == h_seg_offset[s] ? 1 : 0;
    if (h_nempty) *h_nempty = empty;
    if (!ctx) return CANVAS_ERR_INVALID;
    if (nseg == 0) return CANVAS_OK;
    if (!d_out || (h_seg_offset[nseg] > h_seg_offset[0] && !d_values)) CANVAS_FAIL(ctx, CANVAS_ERR_INVALID, "canvas_segment_select: bad arguments (null device array)");
    CANVAS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    int32_t rc = canvas_pin_reserve(ctx, 64); if (rc) return rc;
    unsigned long long* hBad = (unsigned long long*)ctx->pin;
    rc = cl_segment_select_enqueue(ctx, d_values, nseg, h_seg_offset, mode, d_out, hBad); if (rc) return rc;
    CANVAS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (*hBad != ~0ull) CANVAS_FAIL(ctx, CANVAS_ERR_INVALID, "canvas_segment_select: values must be finite (first non-finite value at index " + std::to_string(*hBad) + ")");
    return CANVAS_OK;
}

// ================================================================ canvas_call_diploid: CallVariants between "files parsed" and "files written" ================================
// Device: k_call_sites (every site to its segment: IO.cs:156-176 as a batched search — with positions and segment ends in order the forward-only pointer of the reference stands
// on the FIRST segment whose End > position, which is a binary search), an order-keeping compaction of the kept sites (block counts, one scan block, scatter) into folded
// frequencies, k_call_segoff (where each segment's sites start), k_call_bin_sum (the sum of the counts as an integer, see below), the select of the segments' counts.
// ONE round trip brings {kept sites, their coverage sum, the bin sum and its flag, the site offsets} to the host: the selects build their classes from host offsets, and the model
// points need Math.Pow (host libm).  Then the select of the folded frequencies and k_call_assign (nearest model point) are enqueued back to back — no host step between
// the selects and the assignment — and a second wait brings the per-segment results.  Q-scores (exp / log10: host), the merge (a scan over <= 10^5 segments) and the filters run
// on the host; a third select gives the merged runs' medians.
//
// diploidCoverage = Utilities.Mean(float[]) is a SERIAL double sum in bin order.  When every count is a non-negative multiple of 2^-24 below 2^29 and the total is below 2^29,
// every partial sum of that loop is exact (29 + 24 = 53 bits), so any order gives its bits: k_call_bin_sum adds the counts as integers of 2^-24 and raises a flag at a
// count that is not of that form (or is so large that nbins of them could wrap the 64-bit sum).  With the flag up (or a total of 2^29 and more) the counts are copied to the host and summed there in the reference's order.
#define CL_POINTS 36
struct ClModel { double cov[CL_POINTS], maf[CL_POINTS]; int cn[CL_POINTS], mcc[CL_POINTS]; double factor; };
struct ClSiteStat { unsigned long long kept, covSum, binUnits, binInexact, unsorted; };      // unsorted: first site that goes backwards (or has a negative count), ~0 none

__global__ void __launch_bounds__(CL_BLOCK) k_call_sites(const int* __restrict__ pos, const int* __restrict__ ref, const int* __restrict__ alt, long long nsites, const long long* __restrict__ chrSite,
                                                         const long long* __restrict__ chrSeg, int nchr, const int* __restrict__ segBegin, const int* __restrict__ segEnd,
                                                         int* __restrict__ siteSeg, unsigned* __restrict__ blockCnt, ClSiteStat* __restrict__ st) {
    const long long i = (long long)blockIdx.x * CL_BLOCK + threadIdx.x;
    int seg = -1; unsigned long long tot = 0;
    if (i < nsites) {
        int lo = 0, hi = nchr;                                  // the last chromosome with chrSite[c] <= i (those without sites in front of it share its offset)
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (chrSite[mid] <= i) lo = mid; else hi = mid; }
        const long long s0 = chrSeg[lo], s1 = chrSeg[lo + 1];
        if (s1 > s0) {                                          // (a site whose chromosome has no segments is ignored)
            const int p = pos[i], r = ref[i], a = alt[i];
            if (r < 0 || a < 0 || (i > chrSite[lo] && pos[i - 1] > p)) atomicMin(&st->unsorted, (unsigned long long)i);
            else if ((long long)r + a >= 10) {
                long long l = s0, h = s1;                       // first segment of the chromosome with End > position (one-based position against zero-based End: kept as it is)
                while (l < h) { const long long mid = (l + h) >> 1; if (segEnd[mid] > p) h = mid; else l = mid + 1; }
                if (l < s1 && segBegin[l] <= p) { seg = (int)l; tot = (unsigned long long)((long long)r + a); }
            }
        }
        siteSeg[i] = seg;
    }
    const int cnt = __syncthreads_count(seg >= 0);
    if (threadIdx.x == 0) blockCnt[blockIdx.x] = (unsigned)cnt;
    tot = wave_reduce_add_u64(tot);
    if ((threadIdx.x & 63) == 0 && tot) atomicAdd(&st->covSum, tot);
}
// exclusive scan of the block counts by ONE workgroup (nb = sites / 256: a few 10^4): blockOff[nb] = kept sites
__global__ void __launch_bounds__(1024) k_call_scan(const unsigned* __restrict__ blockCnt, long long nb, unsigned long long* __restrict__ blockOff, ClSiteStat* __restrict__ st) {
    __shared__ unsigned long long part[1024];
    const long long per = (nb + 1023) / 1024, b0 = threadIdx.x * per, b1 = b0 + per < nb ? b0 + per : nb;
    unsigned long long s = 0;
    for (long long b = b0; b < b1; b++) s += blockCnt[b];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) { unsigned long long run = 0; for (int t = 0; t < 1024; t++) { const unsigned long long v = part[t]; part[t] = run; run += v; } blockOff[nb] = run; st->kept = run; }
    __syncthreads();
    s = part[threadIdx.x];
    for (long long b = b0; b < b1; b++) { blockOff[b] = s; s += blockCnt[b]; }
}
__global__ void __launch_bounds__(CL_BLOCK) k_call_scatter(const int* __restrict__ ref, const int* __restrict__ alt, long long nsites, const int* __restrict__ siteSeg,
                                                           const unsigned long long* __restrict__ blockOff, float* __restrict__ cmaf, int* __restrict__ cseg) {
    __shared__ unsigned wtot[CL_BLOCK / 64];
    const long long i = (long long)blockIdx.x * CL_BLOCK + threadIdx.x;
    const int seg = i < nsites ? siteSeg[i] : -1;
    const bool keep = seg >= 0;
    const unsigned long long m = __ballot(keep);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) wtot[w] = (unsigned)__builtin_popcountll(m);
    __syncthreads();
    if (!keep) return;
    unsigned long long k = blockOff[blockIdx.x] + (unsigned)__builtin_popcountll(m & ((1ull << lane) - 1ull));
    for (int t = 0; t < w; t++) k += wtot[t];
    const int r = ref[i], a = alt[i];
    const float f = (float)a / (float)(r + a);                 // Ballele.GetFrequency: alleleBCounts / (float)total
    cmaf[k] = f > 0.5f ? 1.0f - f : f;                          // the fold of AssignPloidyCallsDistance, subtraction in float
    cseg[k] = seg;
}
// segOff[s] = kept sites in segments in front of s (the kept sites are in segment order), s = 0 .. nseg
__global__ void __launch_bounds__(CL_BLOCK) k_call_segoff(const int* __restrict__ cseg, const ClSiteStat* __restrict__ st, long long nseg, long long* __restrict__ segOff) {
    const long long s = (long long)blockIdx.x * CL_BLOCK + threadIdx.x;
    if (s > nseg) return;
    long long l = 0, h = (long long)st->kept;
    while (l < h) { const long long mid = (l + h) >> 1; if (cseg[mid] >= s) h = mid; else l = mid + 1; }
    segOff[s] = l;
}
__global__ void __launch_bounds__(CL_BLOCK) k_call_bin_sum(const float* __restrict__ count, long long n, float vmax, ClSiteStat* __restrict__ st) {
    unsigned long long u = 0; bool bad = false;
    for (long long i = (long long)blockIdx.x * CL_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * CL_BLOCK) {
        const float v = count[i];
        const float sc = v * 16777216.0f;                       // exact: a power of two
        if (!(v >= 0.0f && v < vmax) || sc != floorf(sc)) bad = true; else u += (unsigned long long)sc;
    }
    u = wave_reduce_add_u64(u);
    if ((threadIdx.x & 63) == 0 && u) atomicAdd(&st->binUnits, u);
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(&st->binInexact, 1ull);
}
// AssignPloidyCallsDistance: the nearest of the 36 model points in (coverage, MAF), the reference's strict < / else-if < scan in double without contraction
__global__ void __launch_bounds__(CL_BLOCK) k_call_assign(long long nseg, const int* __restrict__ segBegin, const int* __restrict__ segEnd, const long long* __restrict__ segOff,
                                                          const double* __restrict__ medCount, const double* __restrict__ medMafIn, const ClModel* __restrict__ model,
                                                          int* __restrict__ informative, double* __restrict__ medMaf, int* __restrict__ cn, int* __restrict__ mcc,
                                                          double* __restrict__ dist, double* __restrict__ dist2) {
    const long long s = (long long)blockIdx.x * CL_BLOCK + threadIdx.x;
    if (s >= nseg) return;
    const long long nMaf = segOff[s + 1] - segOff[s];
    const int cutoff = (segEnd[s] - segBegin[s]) / 463 / 2;
    const bool inf = nMaf >= (cutoff > 10 ? cutoff : 10);
    const double cov = medCount[s], maf = inf ? medMafIn[s] : -1.0, factor = model->factor;
    double best = 1.7976931348623157e308, second = 1.7976931348623157e308; int bi = -1;
    for (int p = 0; p < CL_POINTS; p++) {
        double d = (model->cov[p] - cov) * factor;
        double distance = d * d;
        if (inf) { d = model->maf[p] - maf; distance += d * d; }
        if (distance < best) { second = best; best = distance; bi = p; }
        else if (distance < second) second = distance;
    }
    informative[s] = inf ? 1 : 0; medMaf[s] = maf;
    cn[s] = bi < 0 ? -1 : model->cn[bi];
    mcc[s] = (bi < 0 || nMaf < 10) ? -1 : model->mcc[bi];
    dist[s] = best; dist2[s] = second;
}

// (int)Math.Round(v): round half to even, then the conversion x86 does — anything that does not fit becomes int.MinValue
static int cl_round_to_int(double v) { const double r = nearbyint(v); return (r >= -2147483648.0 && r <= 2147483647.0) ? (int)r : (-2147483647 - 1); }
// ComputeQScore(LogisticGermline), SegmentScoringModel.cs:26-41 with the predictors of :114-171
static int cl_qscore(const double* b, long long binCount, int cn, double dist, double dist2) {
    double score = b[0];
    score += log10(1 + (double)binCount) * b[1];
    score += (dist / std::max(1.0, cn - 4.0)) * b[2];
    score += (dist2 == 0 ? 0.0 : dist / dist2) * b[3];
    score = exp(score);
    score = score / (score + 1);
    int q = cl_round_to_int(-10 * log10(1 - score));
    q = std::min(40, q);
    return std::max(2, q);
}
// InitializePloidies + InitializeModelPoints: CN ascending, major count descending
static void cl_model(double diploidCoverage, double meanCoverage, ClModel& M) {
    int n = 0;
    for (int cn = 0; cn <= 10; cn++)
        for (int major = cn; major * 2 >= cn; major--) {
            double maf;
            if (cn == 0) maf = 0.01;
            else {
                const float vf = major / (float)cn;
                maf = vf < 0.5 ? vf : 1 - vf;
                if (major * 2 == cn) { const double c1 = meanCoverage / 2.0f, c = cn * c1; maf = 0.5 - 1 / (3.352 * pow(c, 0.4747)); }      // Utilities.EstimateDiploidMAF
            }
            if (maf != maf) maf = 0;
            M.cov[n] = diploidCoverage * cn / 2.0f; M.maf[n] = maf; M.cn[n] = cn; M.mcc[n] = major; n++;
        }
    M.factor = 0.6 / diploidCoverage;
}

// the body of canvas_call_diploid, shared with canvas_call_diploid_ids (which builds the host tables from the bins' segment ids first)
static int32_t cl_call_diploid(canvas_ctx* ctx, int64_t nbins, const float* d_count, int32_t nchr, const int64_t* h_chr_seg_offset, const int32_t* h_seg_begin,
                               const int32_t* h_seg_end, const int64_t* h_seg_bin_offset, const int64_t* h_chr_site_offset, const int32_t* d_site_pos,
                               const int32_t* d_site_ref, const int32_t* d_site_alt, const double* h_logistic4,
                               double* h_seg_median_count, int64_t* h_seg_site_offset, int32_t* h_seg_informative, double* h_seg_median_maf, int32_t* h_seg_cn, int32_t* h_seg_mcc,
                               double* h_seg_dist, double* h_seg_dist2, int32_t* h_seg_qscore,
                               int64_t* h_nruns, int64_t* h_run_first, int64_t* h_run_last, int32_t* h_run_qscore, int32_t* h_run_filter, double* h_run_median_count,
                               double* h_scalars2, int64_t* h_info4) {
    // every check of the host tables comes first and needs no context (no message without one): *h_nruns is set to 0 only when they have passed
#define CL_REFUSE(msg) do { if (ctx) ctx->err = (msg); return CANVAS_ERR_INVALID; } while (0)
    if (nchr < 0 || nbins < 0 || !h_chr_seg_offset || !h_chr_site_offset || !h_logistic4 || !h_nruns || !h_scalars2) CL_REFUSE("canvas_call_diploid: bad arguments");
    if (h_chr_seg_offset[0] != 0 || h_chr_site_offset[0] != 0) CL_REFUSE("canvas_call_diploid: the chromosome offsets start at 0");
    for (int c = 0; c < nchr; c++)
        if (h_chr_seg_offset[c + 1] < h_chr_seg_offset[c] || h_chr_site_offset[c + 1] < h_chr_site_offset[c]) CL_REFUSE("canvas_call_diploid: the chromosome offsets must be non-decreasing");
    const long long nseg = h_chr_seg_offset[nchr], nsites = h_chr_site_offset[nchr];
    if (nseg > 0x7FFFFFFFll || nsites > (1ll << 36)) CL_REFUSE("canvas_call_diploid: too many segments or sites");
    if (nseg == 0) CL_REFUSE("canvas_call_diploid: no segments (the reference writes a header-only VCF before it gets here)");
    if (!h_seg_begin || !h_seg_end || !h_seg_bin_offset || !h_seg_median_count || !h_seg_site_offset || !h_seg_informative || !h_seg_median_maf || !h_seg_cn || !h_seg_mcc || !h_seg_dist ||
        !h_seg_dist2 || !h_seg_qscore || !h_run_first || !h_run_last || !h_run_qscore || !h_run_filter || !h_run_median_count || !d_count || (nsites > 0 && (!d_site_pos || !d_site_ref || !d_site_alt)))
        CL_REFUSE("canvas_call_diploid: bad arguments (null array)");
    if (h_seg_bin_offset[0] != 0 || h_seg_bin_offset[nseg] != nbins) CL_REFUSE("canvas_call_diploid: the segments' bin offsets run from 0 to nbins (AggregateCounts: every bin belongs to a segment)");
    for (long long s = 0; s < nseg; s++) {
        if (h_seg_bin_offset[s + 1] <= h_seg_bin_offset[s]) CL_REFUSE("canvas_call_diploid: segment " + std::to_string(s) + " has no bins (the reference's median of an empty list throws)");
        if (h_seg_end[s] < h_seg_begin[s]) CL_REFUSE("canvas_call_diploid: segment " + std::to_string(s) + " ends before it begins");
    }
    for (int c = 0; c < nchr; c++)
        for (long long s = h_chr_seg_offset[c] + 1; s < h_chr_seg_offset[c + 1]; s++)
            if (h_seg_begin[s] < h_seg_begin[s - 1] || h_seg_end[s] <= h_seg_end[s - 1])
                CL_REFUSE("canvas_call_diploid: within a chromosome the segments' begins must not decrease and their ends must increase (segment " + std::to_string(s) + ")");
#undef CL_REFUSE
    *h_nruns = 0;
    if (!ctx) return CANVAS_ERR_INVALID;
    CANVAS_HIP_TRY(ctx, hipSetDevice(ctx->device));

    // ---- buffers that live across the selects
    const long long nb = (nsites + CL_BLOCK - 1) / CL_BLOCK;
    ClSiteStat* dSt; ClModel* dModel; long long *dChrSite, *dChrSeg, *dSegOff; int *dBegin, *dEnd, *dSiteSeg, *dCseg, *dInf, *dCn, *dMcc; unsigned* dBlockCnt; unsigned long long* dBlockOff; float* dMaf;
    double *dMedCount, *dMedMafIn, *dMedMaf, *dDist, *dDist2;
    int32_t rc = cl_call_ws_carve(ctx, [&](WsCarver& cv) {
        const size_t S = (size_t)nseg;
        cv.take(dSt, 1); cv.take(dModel, 1); cv.take(dChrSite, (size_t)nchr + 1); cv.take(dChrSeg, (size_t)nchr + 1); cv.take(dBegin, S); cv.take(dEnd, S);
        cv.take(dSiteSeg, (size_t)nsites); cv.take(dBlockCnt, (size_t)nb); cv.take(dBlockOff, (size_t)nb + 1); cv.take(dMaf, (size_t)nsites); cv.take(dCseg, (size_t)nsites);
        cv.take(dSegOff, S + 1);
        cv.take(dMedCount, S); cv.take(dMedMafIn, S); cv.take(dMedMaf, S); cv.take(dDist, S); cv.take(dDist2, S); cv.take(dInf, S); cv.take(dCn, S); cv.take(dMcc, S);
    });
    if (rc) return rc;
    rc = canvas_pin_reserve(ctx, 256); if (rc) return rc;
    unsigned long long* hBad = (unsigned long long*)ctx->pin;     // [0..2] the selects' flags, [4..8] ClSiteStat
    ClSiteStat* hSt = (ClSiteStat*)(hBad + 4);
    const unsigned long long none = ~0ull;

    { ClSiteStat z{0, 0, 0, 0, none}; rc = canvas_h2d_small(ctx, dSt, &z, sizeof(z)); if (rc) return rc; }
    { std::vector<long long> t(h_chr_site_offset, h_chr_site_offset + nchr + 1); rc = canvas_h2d_small(ctx, dChrSite, t.data(), t.size() * sizeof(long long)); if (rc) return rc; }
    { std::vector<long long> t(h_chr_seg_offset, h_chr_seg_offset + nchr + 1); rc = canvas_h2d_small(ctx, dChrSeg, t.data(), t.size() * sizeof(long long)); if (rc) return rc; }
    rc = canvas_h2d_small(ctx, dBegin, h_seg_begin, (size_t)nseg * sizeof(int)); if (rc) return rc;
    rc = canvas_h2d_small(ctx, dEnd, h_seg_end, (size_t)nseg * sizeof(int)); if (rc) return rc;
    const unsigned segGrid = (unsigned)((nseg + 1 + CL_BLOCK - 1) / CL_BLOCK);
    if (nsites > 0) {
        ProfScope ps(ctx, "call_sites");
        hipLaunchKernelGGL(k_call_sites, dim3((unsigned)nb), dim3(CL_BLOCK), 0, ctx->stream, d_site_pos, d_site_ref, d_site_alt, nsites, dChrSite, dChrSeg, (int)nchr, dBegin, dEnd, dSiteSeg, dBlockCnt, dSt);
        hipLaunchKernelGGL(k_call_scan, dim3(1), dim3(1024), 0, ctx->stream, dBlockCnt, nb, dBlockOff, dSt);
        hipLaunchKernelGGL(k_call_scatter, dim3((unsigned)nb), dim3(CL_BLOCK), 0, ctx->stream, d_site_ref, d_site_alt, nsites, dSiteSeg, dBlockOff, dMaf, dCseg);
    }
    hipLaunchKernelGGL(k_call_segoff, dim3(segGrid), dim3(CL_BLOCK), 0, ctx->stream, dCseg, dSt, nseg, dSegOff);
    int vbits = 29;                                             // a count of 2^vbits and more raises the flag: nbins x 2^vbits x 2^24 stays below 2^64, so the integer sum cannot wrap
    while (vbits > 0 && (double)nbins * ldexp(1.0, vbits + 24) >= 18446744073709551616.0) vbits--;
    hipLaunchKernelGGL(k_call_bin_sum, dim3((unsigned)std::min<long long>((nbins + CL_BLOCK - 1) / CL_BLOCK, 2048)), dim3(CL_BLOCK), 0, ctx->stream, d_count, (long long)nbins, (float)ldexp(1.0, vbits), dSt);
    CANVAS_HIP_TRY(ctx, hipGetLastError());
    rc = cl_segment_select_enqueue(ctx, d_count, nseg, h_seg_bin_offset, CL_MODE_MEDIAN_F32, dMedCount, hBad + 0); if (rc) return rc;
    CANVAS_HIP_TRY(ctx, hipMemcpyAsync(hSt, dSt, sizeof(ClSiteStat), hipMemcpyDeviceToHost, ctx->stream));
    CANVAS_HIP_TRY(ctx, hipMemcpyAsync(h_seg_site_offset, dSegOff, (size_t)(nseg + 1) * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
    CANVAS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));                                                        // ---- the first wait
    if (hBad[0] != none) CANVAS_FAIL(ctx, CANVAS_ERR_INVALID, "canvas_call_diploid: counts must be finite (first non-finite count at index " + std::to_string(hBad[0]) + ")");
    if (hSt->unsorted != none) CANVAS_FAIL(ctx, CANVAS_ERR_INVALID, "canvas_call_diploid: within a chromosome the sites' positions must not decrease and their counts must not be negative (site " + std::to_string(hSt->unsorted) + ")");
    if (hSt->kept == 0) CANVAS_FAIL(ctx, CANVAS_ERR_INVALID, "canvas_call_diploid: no site with ref + alt >= 10 inside a segment (the reference's Average() of an empty sequence throws)");
    const double meanCoverage = (double)(long long)hSt->covSum / (double)(long long)hSt->kept;
    double diploidCoverage; int integerPath = 1;
    if (!hSt->binInexact && hSt->binUnits < (1ull << 53)) diploidCoverage = ((double)hSt->binUnits / 16777216.0) / (double)nbins;
    else {
        integerPath = 0;
        std::vector<float> h((size_t)nbins);
        CANVAS_HIP_TRY(ctx, hipMemcpyAsync(h.data(), d_count, (size_t)nbins * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        CANVAS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        double sum = 0;
        for (long long i = 0; i < nbins; i++) sum += h[(size_t)i];
        diploidCoverage = sum / (double)nbins;
    }
    ClModel M; cl_model(diploidCoverage, meanCoverage, M);
    rc = canvas_h2d_small(ctx, dModel, &M, sizeof(M)); if (rc) return rc;
    rc = cl_segment_select_enqueue(ctx, dMaf, nseg, h_seg_site_offset, CL_MODE_MEDIAN_F64, dMedMafIn, hBad + 1); if (rc) return rc;
    hipLaunchKernelGGL(k_call_assign, dim3(segGrid), dim3(CL_BLOCK), 0, ctx->stream, nseg, dBegin, dEnd, dSegOff, dMedCount, dMedMafIn, dModel, dInf, dMedMaf, dCn, dMcc, dDist, dDist2);
    CANVAS_HIP_TRY(ctx, hipGetLastError());
    CANVAS_HIP_TRY(ctx, hipMemcpyAsync(h_seg_median_count, dMedCount, (size_t)nseg * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    CANVAS_HIP_TRY(ctx, hipMemcpyAsync(h_seg_median_maf, dMedMaf, (size_t)nseg * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    CANVAS_HIP_TRY(ctx, hipMemcpyAsync(h_seg_dist, dDist, (size_t)nseg * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    CANVAS_HIP_TRY(ctx, hipMemcpyAsync(h_seg_dist2, dDist2, (size_t)nseg * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    CANVAS_HIP_TRY(ctx, hipMemcpyAsync(h_seg_informative, dInf, (size_t)nseg * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    CANVAS_HIP_TRY(ctx, hipMemcpyAsync(h_seg_cn, dCn, (size_t)nseg * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    CANVAS_HIP_TRY(ctx, hipMemcpyAsync(h_seg_mcc, dMcc, (size_t)nseg * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    CANVAS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));                                                        // ---- the second wait
    if (hBad[1] != none) CANVAS_FAIL(ctx, CANVAS_ERR_INVALID, "canvas_call_diploid: a folded frequency is not finite");      // (cannot happen: ref + alt >= 10)

    // ---- host: q-scores, MergeSegments(segments) with its defaults, q-scores of the runs, filters
    for (long long s = 0; s < nseg; s++) h_seg_qscore[s] = cl_qscore(h_logistic4, h_seg_bin_offset[s + 1] - h_seg_bin_offset[s], h_seg_cn[s], h_seg_dist[s], h_seg_dist2[s]);
    std::vector<int> chrOf((size_t)nseg);
    for (int c = 0; c < nchr; c++) for (long long s = h_chr_seg_offset[c]; s < h_chr_seg_offset[c + 1]; s++) chrOf[(size_t)s] = c;
    long long nruns = 0; int runEnd = 0;
    for (long long s = 0; s < nseg; s++) {
        const bool join = nruns > 0 && h_seg_cn[h_run_first[nruns - 1]] == h_seg_cn[s] && chrOf[(size_t)h_run_first[nruns - 1]] == chrOf[(size_t)s] && (long long)h_seg_begin[s] - runEnd < 10000;
        if (join) { h_run_last[nruns - 1] = s; runEnd = h_seg_end[s]; }       // (ends increase within a chromosome: MergeIn always takes s.End)
        else { h_run_first[nruns] = s; h_run_last[nruns] = s; runEnd = h_seg_end[s]; nruns++; }
    }
    std::vector<int64_t> runBinOff((size_t)nruns + 1);
    for (long long r = 0; r < nruns; r++) {
        const long long f = h_run_first[r], l = h_run_last[r];
        runBinOff[(size_t)r] = h_seg_bin_offset[f];
        h_run_qscore[r] = cl_qscore(h_logistic4, h_seg_bin_offset[l + 1] - h_seg_bin_offset[f], h_seg_cn[f], h_seg_dist[f], h_seg_dist2[f]);
        h_run_filter[r] = (h_run_qscore[r] < 10 ? 1 : 0) | (h_seg_end[l] - h_seg_begin[f] < 10000 ? 2 : 0);
    }
    runBinOff[(size_t)nruns] = nbins;
    rc = cl_segment_select_enqueue(ctx, d_count, nruns, runBinOff.data(), CL_MODE_MEDIAN_F64, dMedMafIn, hBad + 2); if (rc) return rc;      // (dMedMafIn is free again: nruns <= nseg)
    CANVAS_HIP_TRY(ctx, hipMemcpyAsync(h_run_median_count, dMedMafIn, (size_t)nruns * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    CANVAS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));                                                        // ---- the third wait
    *h_nruns = nruns; h_scalars2[0] = diploidCoverage; h_scalars2[1] = meanCoverage;
    if (h_info4) { h_info4[0] = (int64_t)hSt->kept; h_info4[1] = integerPath; h_info4[2] = (int64_t)hSt->covSum; h_info4[3] = 0; }
    return CANVAS_OK;
}

extern "C" int32_t canvas_call_diploid(canvas_ctx* ctx, int64_t nbins, const float* d_count, int32_t nchr, const int64_t* h_chr_seg_offset, const int32_t* h_seg_begin,
                                       const int32_t* h_seg_end, const int64_t* h_seg_bin_offset, const int64_t* h_chr_site_offset, const int32_t* d_site_pos,
                                       const int32_t* d_site_ref, const int32_t* d_site_alt, const double* h_logistic4,
                                       double* h_seg_median_count, int64_t* h_seg_site_offset, int32_t* h_seg_informative, double* h_seg_median_maf, int32_t* h_seg_cn, int32_t* h_seg_mcc,
                                       double* h_seg_dist, double* h_seg_dist2, int32_t* h_seg_qscore,
                                       int64_t* h_nruns, int64_t* h_run_first, int64_t* h_run_last, int32_t* h_run_qscore, int32_t* h_run_filter, double* h_run_median_count,
                                       double* h_scalars2, int64_t* h_info4) {
    return cl_call_diploid(ctx, nbins, d_count, nchr, h_chr_seg_offset, h_seg_begin, h_seg_end, h_seg_bin_offset, h_chr_site_offset, d_site_pos, d_site_ref, d_site_alt, h_logistic4,
                           h_seg_median_count, h_seg_site_offset, h_seg_informative, h_seg_median_maf, h_seg_cn, h_seg_mcc, h_seg_dist, h_seg_dist2, h_seg_qscore,
                           h_nruns, h_run_first, h_run_last, h_run_qscore, h_run_filter, h_run_median_count, h_scalars2, h_info4);
}

// canvas_segment_tables (segtab.hip), then the call on the tables and float counts it left: the germline sample from per-bin segment ids to copy-number calls without a
// text hand-off and without a per-bin array leaving the device.  One wait for the tables (the selects build their classes from the host offsets) and the call's three.
extern "C" int32_t canvas_call_diploid_ids(canvas_ctx* ctx, int64_t nbins, int32_t nchr, const int64_t* h_chr_offset, const int32_t* d_start, const int32_t* d_stop, const int32_t* d_segment_id,
                                           const double* d_cov, int64_t cap_seg, const int64_t* h_chr_site_offset, const int32_t* d_site_pos, const int32_t* d_site_ref, const int32_t* d_site_alt,
                                           const double* h_logistic4,
                                           int64_t* h_nseg, int64_t* h_chr_seg_offset, int32_t* h_seg_begin, int32_t* h_seg_end, int64_t* h_seg_bin_offset, int32_t* h_seg_ci4, float* d_count_f32,
                                           double* h_seg_median_count, int64_t* h_seg_site_offset, int32_t* h_seg_informative, double* h_seg_median_maf, int32_t* h_seg_cn, int32_t* h_seg_mcc,
                                           double* h_seg_dist, double* h_seg_dist2, int32_t* h_seg_qscore,
                                           int64_t* h_nruns, int64_t* h_run_first, int64_t* h_run_last, int32_t* h_run_qscore, int32_t* h_run_filter, double* h_run_median_count,
                                           double* h_scalars2, int64_t* h_info4) {
    if (!d_cov || !d_count_f32) { if (ctx) ctx->err = "canvas_call_diploid_ids: bad arguments (the call needs the coverage and room for the float counts)"; return CANVAS_ERR_INVALID; }
    // canvas_segment_tables decides its host arguments before it looks at the context, so a NULL ctx still reports them
    int32_t rc = canvas_segment_tables(ctx, nbins, nchr, h_chr_offset, d_start, d_stop, d_segment_id, d_cov, cap_seg, h_nseg, h_chr_seg_offset, h_seg_begin, h_seg_end, h_seg_bin_offset, h_seg_ci4,
                                       d_count_f32);
    if (rc) return rc;
    return cl_call_diploid(ctx, nbins, d_count_f32, nchr, h_chr_seg_offset, h_seg_begin, h_seg_end, h_seg_bin_offset, h_chr_site_offset, d_site_pos, d_site_ref, d_site_alt, h_logistic4,
                           h_seg_median_count, h_seg_site_offset, h_seg_informative, h_seg_median_maf, h_seg_cn, h_seg_mcc, h_seg_dist, h_seg_dist2, h_seg_qscore,
                           h_nruns, h_run_first, h_run_last, h_run_qscore, h_run_filter, h_run_median_count, h_scalars2, h_info4);
}

// ================================================================ canvas_call_somatic: CanvasSomaticCaller.CallVariants around canvas_somatic_model_fit ======================
// Stage 1 is canvas_call_diploid's (the same reader): k_call_sites / k_call_scan / k_call_scatter / k_call_segoff and the selects.  New here:
//   k_scall_to_float   the per-segment medians as floats (enrichment: the list of Convert.ToSingle(Median(Counts)) that Quartiles sorts)
//   k_scall_usable     info.Coverage / Maf / Weight of every segment, gathered to the usable segments' dense arrays the fit reads
//   k_scall_compact    the bins of the usable segments at reference copy number 2, packed for the select of medianCoverageLevel (one thread per bin, its segment by bisection)
//   k_scall_assign     AssignPloidyCalls' scan over the ploidy table of the best model, one thread per segment, strict < / else-if <, double without contraction
//   k_scall_mean       MeanCount of the segments whose best ploidy is MaximumCopyNumber, one workgroup per segment.  The reference's LINQ Sum adds the floats into a double in
//                      bin order and rounds the total to float.  Counts that are non-negative multiples of 2^e with n * max < 2^(53 + e) make every partial sum of that loop a
//                      multiple of 2^e below 2^(53 + e), hence exact, so any order gives its bits: the workgroup finds e and max, and when the bound holds adds the counts as
//                      integers of 2^e (EXACT).  Otherwise lane 0 adds them in bin order out of LDS tiles (WALK).  CANVAS_SOMATIC_MEAN=walk (test hook) sends every segment there.
#include "somatic_points.hpp"
#define SC_MAXP 36
#define SC_WALK_TILE 1024
struct ScModel { double cov[SC_MAXP], maf[SC_MAXP], hcov[SC_MAXP]; int cn[SC_MAXP], major[SC_MAXP]; double cwf; int P, maxCN; };

__global__ void __launch_bounds__(CL_BLOCK) k_scall_to_float(const double* __restrict__ in, long long n, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * CL_BLOCK + threadIdx.x;
    if (i < n) out[i] = (float)in[i];
}
__global__ void __launch_bounds__(CL_BLOCK) k_scall_usable(long long nseg, const int* __restrict__ segBegin, const int* __restrict__ segEnd, const long long* __restrict__ segOff,
                                                           const double* __restrict__ medCount, const double* __restrict__ mafUpper, const int* __restrict__ dense, int threshold,
                                                           double* __restrict__ cov, double* __restrict__ maf, double* __restrict__ weight,
                                                           double* __restrict__ uCov, double* __restrict__ uMaf, double* __restrict__ uW, int* __restrict__ uLen) {
    const long long s = (long long)blockIdx.x * CL_BLOCK + threadIdx.x;
    if (s >= nseg) return;
    const long long nf = segOff[s + 1] - segOff[s];
    const int len = segEnd[s] - segBegin[s];
    const double c = medCount[s], m = nf < threshold ? -1.0 : mafUpper[s];
    double w = (double)len;
    if (nf < 10) w *= (double)nf / 10;
    cov[s] = c; maf[s] = m; weight[s] = w;
    const int d = dense[s];                                    // position among the usable segments, -1: not usable
    if (d >= 0) { uCov[d] = c; uMaf[d] = m; uW[d] = w; uLen[d] = len; }
}
__global__ void __launch_bounds__(CL_BLOCK) k_scall_compact(const float* __restrict__ count, long long nbins, long long nseg, const long long* __restrict__ binOff,
                                                            const long long* __restrict__ dst, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * CL_BLOCK + threadIdx.x;
    if (i >= nbins) return;
    long long lo = 0, hi = nseg;                               // the segment with binOff[s] <= i < binOff[s + 1] (binOff runs from 0 to nbins, no empty segment)
    while (hi - lo > 1) { const long long mid = (lo + hi) >> 1; if (binOff[mid] <= i) lo = mid; else hi = mid; }
    const long long d = dst[lo];
    if (d >= 0) out[d + (i - binOff[lo])] = count[i];
}
__global__ void __launch_bounds__(CL_BLOCK) k_scall_assign(long long nseg, const long long* __restrict__ segOff, const double* __restrict__ medCount, const double* __restrict__ mafUpper,
                                                           const int* __restrict__ refCn, const ScModel* __restrict__ model, int* __restrict__ cn, int* __restrict__ cn2,
                                                           int* __restrict__ mcc, double* __restrict__ dist, double* __restrict__ dist2) {
    const long long s = (long long)blockIdx.x * CL_BLOCK + threadIdx.x;
    if (s >= nseg) return;
    const bool hasMaf = segOff[s + 1] - segOff[s] >= 10;
    const double coverage = medCount[s], maf = hasMaf ? mafUpper[s] : -1.0, cwf = model->cwf;
    const bool haploid = refCn && refCn[s] == 1;
    double best = 1.7976931348623157e308, second = 1.7976931348623157e308; int bi = -1, si = -1;
    for (int p = 0; p < model->P; p++) {
        const double targetCoverage = haploid ? model->hcov[p] : model->cov[p], targetMaf = haploid ? 0.0 : model->maf[p];
        double diff = (coverage - targetCoverage) * cwf;
        double distance = diff * diff;
        if (!hasMaf || maf < 0) distance = 2 * distance;
        else { diff = maf - targetMaf; distance += diff * diff; }
        if (distance < best) { second = best; si = bi; best = distance; bi = p; }
        else if (distance < second) { second = distance; si = p; }
    }
    cn[s] = bi < 0 ? -1 : model->cn[bi];
    cn2[s] = si < 0 ? -1 : model->cn[si];
    mcc[s] = (bi < 0 || !hasMaf) ? -1 : model->major[bi];
    dist[s] = best; dist2[s] = second;
}
__global__ void __launch_bounds__(CL_BLOCK) k_scall_mean(const float* __restrict__ count, const long long* __restrict__ binOff, const int* __restrict__ cn, int maxCN, int forceWalk,
                                                         double* __restrict__ mean, int* __restrict__ route) {
    __shared__ int sE[CL_BLOCK / 64]; __shared__ float sM[CL_BLOCK / 64]; __shared__ int sBad[CL_BLOCK / 64]; __shared__ unsigned long long sU[CL_BLOCK / 64];
    __shared__ float tile[SC_WALK_TILE]; __shared__ double sSum;
    const long long s = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (cn[s] != maxCN) { if (tid == 0) { mean[s] = 0.0; route[s] = CANVAS_SOMATIC_MEAN_NONE; } return; }      // (block-uniform)
    const long long o = binOff[s], n = binOff[s + 1] - o;
    int emin = 0x7FFFFFFF; float vmax = 0.0f; bool bad = false;
    for (long long i = tid; i < n; i += CL_BLOCK) {
        const float v = count[o + i];
        const uint32_t u = __float_as_uint(v), e = (u >> 23) & 255u, m = u & 0x7FFFFFu;
        if ((u >> 31) || e == 255u) bad = true;                 // negative (-0.0 included) or not finite: no proof
        else if (u) { const int low = e ? (int)e - 150 + __builtin_ctz(m | 0x800000u) : -149 + __builtin_ctz(m); emin = min(emin, low); vmax = fmaxf(vmax, v); }
    }
    for (int d = 32; d; d >>= 1) { emin = min(emin, __shfl_xor(emin, d)); vmax = fmaxf(vmax, __shfl_xor(vmax, d)); }
    const bool anyBad = __ballot(bad) != 0;
    if (lane == 0) { sE[w] = emin; sM[w] = vmax; sBad[w] = anyBad ? 1 : 0; }
    __syncthreads();
    bad = false;
    for (int k = 0; k < CL_BLOCK / 64; k++) { emin = min(emin, sE[k]); vmax = fmaxf(vmax, sM[k]); bad = bad || sBad[k]; }      // (block-uniform from here)
    const bool zero = emin == 0x7FFFFFFF;                       // every count is +0
    const bool proven = !bad && !forceWalk && (zero || (double)n * (double)vmax < ldexp(1.0, 53 + emin));
    double sum = 0.0;
    if (proven) {
        unsigned long long u = 0;
        if (!zero) {
            const double scale = ldexp(1.0, -emin);            // emin >= -149: finite; count * scale is an integer below 2^53
            for (long long i = tid; i < n; i += CL_BLOCK) u += (unsigned long long)((double)count[o + i] * scale);
        }
        u = wave_reduce_add_u64(u);
        if (lane == 0) sU[w] = u;
        __syncthreads();
        if (tid == 0) { unsigned long long t = 0; for (int k = 0; k < CL_BLOCK / 64; k++) t += sU[k]; sum = zero ? 0.0 : (double)t * ldexp(1.0, emin); }
    } else {
        if (tid == 0) sSum = 0.0;
        for (long long t0 = 0; t0 < n; t0 += SC_WALK_TILE) {
            const int m = (int)min((long long)SC_WALK_TILE, n - t0);
            __syncthreads();
            for (int i = tid; i < m; i += CL_BLOCK) tile[i] = count[o + t0 + i];
            __syncthreads();
            if (tid == 0) { double a = sSum; for (int i = 0; i < m; i++) a += (double)tile[i]; sSum = a; }
        }
        if (tid == 0) sum = sSum;
    }
    if (tid == 0) { mean[s] = (double)(float)sum / (double)n; route[s] = proven ? CANVAS_SOMATIC_MEAN_EXACT : CANVAS_SOMATIC_MEAN_WALK; }
}

// ComputeQScore(Logistic), SegmentScoringModel.cs:42-62 with the predictors of :121-125 and :151-160
static int sc_qscore(const canvas_somatic_call_params& p, long long binCount, int cn, double dist, double dist2) {
    const double logBins = log10((double)(1 + binCount));
    double score = p.logistic_intercept;
    score += logBins * p.logistic_log_bin_count;
    score += (dist / std::max(1.0, cn - 4.0)) * p.logistic_model_distance;
    score += (dist2 == 0 ? 0.0 : dist / dist2) * p.logistic_distance_ratio;
    score += cn >= 15 ? logBins : 0.0;
    score = exp(score);
    score = score / (score + 1);
    int q = cl_round_to_int(-10 * log10(1 - score));
    q = std::min(60, q);
    return std::max(2, q);
}
// Convert.ToInt32(float): round half to even; false when the result leaves int32 (OverflowException) or the value is NaN
static bool sc_to_int32(float v, int& out) { const double r = nearbyint((double)v); if (!(r >= -2147483648.0 && r <= 2147483647.0)) return false; out = (int)r; return true; }

// the body of canvas_call_somatic, shared with canvas_call_somatic_ids (which builds the host tables and the reference copy numbers from the bins' segment ids first)
static int32_t sc_call_somatic(canvas_ctx* ctx, int64_t nbins, const float* d_count, int32_t nchr, const int64_t* h_chr_seg_offset, const int32_t* h_seg_begin,
                               const int32_t* h_seg_end, const int64_t* h_seg_bin_offset, const int64_t* h_chr_site_offset, const int32_t* d_site_pos,
                               const int32_t* d_site_ref, const int32_t* d_site_alt, const int32_t* h_seg_ref_cn, const int64_t* h_chr_excl_offset,
                               const int32_t* h_excl_start, const int32_t* h_excl_stop, const canvas_somatic_call_params* params, const canvas_somatic_call_out* out,
                               canvas_somatic_call_scalars* h_scalars, canvas_somatic_result* h_fit) {
#define SC_REFUSE(msg) do { if (ctx) ctx->err = std::string("canvas_call_somatic: ") + (msg); return CANVAS_ERR_INVALID; } while (0)
    if (nchr < 0 || nbins < 0 || !h_chr_seg_offset || !h_chr_site_offset || !params || !out || !h_scalars || !h_fit) SC_REFUSE("bad arguments");
    if (h_chr_seg_offset[0] != 0 || h_chr_site_offset[0] != 0) SC_REFUSE("the chromosome offsets start at 0");
    for (int c = 0; c < nchr; c++)
        if (h_chr_seg_offset[c + 1] < h_chr_seg_offset[c] || h_chr_site_offset[c + 1] < h_chr_site_offset[c]) SC_REFUSE("the chromosome offsets must be non-decreasing");
    const long long nseg = h_chr_seg_offset[nchr], nsites = h_chr_site_offset[nchr];
    if (nseg > 0x7FFFFFFFll || nsites > (1ll << 36)) SC_REFUSE("too many segments or sites");
    if (nseg == 0) SC_REFUSE("no segments");
    const canvas_somatic_call_out& O = *out;
    if (!h_seg_begin || !h_seg_end || !h_seg_bin_offset || !d_count || (nsites > 0 && (!d_site_pos || !d_site_ref || !d_site_alt)) || !O.seg_median_count || !O.seg_site_offset ||
        !O.seg_maf_upper || !O.seg_usable || !O.seg_coverage || !O.seg_maf || !O.seg_weight || !O.seg_cn || !O.seg_cn2 || !O.seg_mcc || !O.seg_dist || !O.seg_dist2 || !O.seg_mean_count ||
        !O.seg_mean_route || !O.seg_qscore || !O.seg_run || !O.run_owner || !O.run_begin || !O.run_end || !O.run_bin_count || !O.run_qscore || !O.run_filter)
        SC_REFUSE("bad arguments (null array)");
    if (h_seg_bin_offset[0] != 0 || h_seg_bin_offset[nseg] != nbins) SC_REFUSE("the segments' bin offsets run from 0 to nbins");
    for (long long s = 0; s < nseg; s++) {
        if (h_seg_bin_offset[s + 1] <= h_seg_bin_offset[s]) SC_REFUSE("segment " + std::to_string(s) + " has no bins (the reference's median of an empty list throws)");
        if (h_seg_end[s] < h_seg_begin[s]) SC_REFUSE("segment " + std::to_string(s) + " ends before it begins");
    }
    for (int c = 0; c < nchr; c++)
        for (long long s = h_chr_seg_offset[c] + 1; s < h_chr_seg_offset[c + 1]; s++)
            if (h_seg_begin[s] < h_seg_begin[s - 1] || h_seg_end[s] <= h_seg_end[s - 1])
                SC_REFUSE("within a chromosome the segments' begins must not decrease and their ends must increase (segment " + std::to_string(s) + ")");
    if (h_chr_excl_offset) {
        if (h_chr_excl_offset[0] != 0) SC_REFUSE("the excluded intervals' offsets start at 0");
        for (int c = 0; c < nchr; c++) {
            if (h_chr_excl_offset[c + 1] < h_chr_excl_offset[c]) SC_REFUSE("the excluded intervals' offsets must be non-decreasing");
            if (h_chr_excl_offset[c + 1] > h_chr_excl_offset[c] && (!h_excl_start || !h_excl_stop)) SC_REFUSE("bad arguments (null excluded intervals)");
            for (long long k = h_chr_excl_offset[c] + 1; k < h_chr_excl_offset[c + 1]; k++)
                if (h_excl_start[k] < h_excl_start[k - 1]) SC_REFUSE("the excluded intervals of a chromosome must be sorted by start");
        }
    }
    const canvas_somatic_call_params& P = *params;
    const int maxCN = P.fit.maximum_copy_number;
    if (maxCN < 2 || maxCN > CANVAS_SOMATIC_MAX_CN) SC_REFUSE("MaximumCopyNumber must be 2 .. 10");
    if (!(P.lower_coverage_level_weighting_factor > 0) || !(P.upper_coverage_level_weighting_factor > 0) || !std::isfinite(P.lower_coverage_level_weighting_factor) ||
        !std::isfinite(P.upper_coverage_level_weighting_factor)) SC_REFUSE("the coverage level weighting factors must be positive and finite");
    if (!std::isfinite(P.coverage_weighting) || !std::isfinite(P.coverage_weighting_with_maf_segmentation) || !std::isfinite(P.evenness_score_threshold) || !std::isfinite(P.min_evenness_score) ||
        !std::isfinite(P.logistic_intercept) || !std::isfinite(P.logistic_log_bin_count) || !std::isfinite(P.logistic_model_distance) || !std::isfinite(P.logistic_distance_ratio))
        SC_REFUSE("the coverage weightings, evenness numbers and Logistic parameters must be finite");
    if (P.user_ploidy == 0 || std::isnan(P.user_ploidy) || std::isnan(P.user_purity) || P.user_purity > 1) SC_REFUSE("a user ploidy must not be 0 and a user purity at most 1");
    if (P.genome_length <= 0) SC_REFUSE("genome_length must be positive");
#undef SC_REFUSE
    *h_scalars = canvas_somatic_call_scalars{};
    *h_fit = canvas_somatic_result{}; h_fit->best_model = -1;
    if (!ctx) return CANVAS_ERR_INVALID;
    auto fail = [&](int32_t code, const std::string& msg) { ctx->err = "canvas_call_somatic: " + msg; return code; };
    CANVAS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    canvas_somatic_call_scalars& R = *h_scalars;
    auto clock0 = std::chrono::steady_clock::now();
    auto lap = [&]() { const auto now = std::chrono::steady_clock::now(); const double ms = std::chrono::duration<double, std::milli>(now - clock0).count(); clock0 = now; return ms; };

    // ---- buffers that live across the selects and the fit (which carve ctx->ws)
    const long long nb = (nsites + CL_BLOCK - 1) / CL_BLOCK;
    const size_t S = (size_t)nseg;
    ClSiteStat* dSt; ScModel* dModel; long long *dChrSite, *dChrSeg, *dSegOff, *dBinOff, *dDst; int *dBegin, *dEnd, *dSiteSeg, *dCseg; unsigned* dBlockCnt; unsigned long long* dBlockOff; float *dMaf, *dMedF, *dCompact;
    double *dMedCount, *dMafUp, *dCov, *dMafU, *dW, *dUCov, *dUMaf, *dUW, *dDist, *dDist2, *dMean, *dQ; int *dULen, *dDense, *dRefCn, *dCn, *dCn2, *dMcc, *dRoute;
    int32_t rc = cl_call_ws_carve(ctx, [&](WsCarver& cv) {
        cv.take(dSt, 1); cv.take(dModel, 1); cv.take(dChrSite, (size_t)nchr + 1); cv.take(dChrSeg, (size_t)nchr + 1); cv.take(dBegin, S); cv.take(dEnd, S);
        cv.take(dSiteSeg, (size_t)nsites); cv.take(dBlockCnt, (size_t)nb); cv.take(dBlockOff, (size_t)nb + 1); cv.take(dMaf, (size_t)nsites); cv.take(dCseg, (size_t)nsites);
        cv.take(dSegOff, S + 1); cv.take(dBinOff, S + 1); cv.take(dDst, S);
        cv.take(dMedCount, S); cv.take(dMafUp, S); cv.take(dCov, S); cv.take(dMafU, S); cv.take(dW, S); cv.take(dUCov, S); cv.take(dUMaf, S); cv.take(dUW, S); cv.take(dDist, S); cv.take(dDist2, S); cv.take(dMean, S);
        cv.take(dULen, S); cv.take(dDense, S); cv.take(dRefCn, S); cv.take(dCn, S); cv.take(dCn2, S); cv.take(dMcc, S); cv.take(dRoute, S);
        cv.take(dMedF, S); cv.take(dCompact, (size_t)nbins); cv.take(dQ, 4);
    });
    if (rc) return rc;
    rc = canvas_pin_reserve(ctx, 256); if (rc) return rc;
    unsigned long long* hBad = (unsigned long long*)ctx->pin;     // [0..3] the selects' flags, [4..8] ClSiteStat, [10..11] the two quartile medians
    // (hBad[1] and hBad[3], the flags of the two selects over whole arrays, are not looked at: the per-segment select behind hBad[0] has read every one of those counts)
    ClSiteStat* hSt = (ClSiteStat*)(hBad + 4);
    double* hQ = (double*)(hBad + 10);
    const unsigned long long none = ~0ull;
    const bool enrichment = P.is_enrichment != 0;

    // ---- stage 1 (and the select of stage 2's overallMedianCoverage): the first wait
    { ClSiteStat z{0, 0, 0, 0, none}; rc = canvas_h2d_small(ctx, dSt, &z, sizeof(z)); if (rc) return rc; }
    { std::vector<long long> t(h_chr_site_offset, h_chr_site_offset + nchr + 1); rc = canvas_h2d_small(ctx, dChrSite, t.data(), t.size() * sizeof(long long)); if (rc) return rc; }
    { std::vector<long long> t(h_chr_seg_offset, h_chr_seg_offset + nchr + 1); rc = canvas_h2d_small(ctx, dChrSeg, t.data(), t.size() * sizeof(long long)); if (rc) return rc; }
    { std::vector<long long> t(h_seg_bin_offset, h_seg_bin_offset + nseg + 1); rc = canvas_h2d_small(ctx, dBinOff, t.data(), t.size() * sizeof(long long)); if (rc) return rc; }
    rc = canvas_h2d_small(ctx, dBegin, h_seg_begin, S * sizeof(int)); if (rc) return rc;
    rc = canvas_h2d_small(ctx, dEnd, h_seg_end, S * sizeof(int)); if (rc) return rc;
    if (h_seg_ref_cn) { rc = canvas_h2d_small(ctx, dRefCn, h_seg_ref_cn, S * sizeof(int)); if (rc) return rc; }
    const unsigned segGrid = (unsigned)((nseg + 1 + CL_BLOCK - 1) / CL_BLOCK);
    if (nsites > 0) {
        ProfScope ps(ctx, "scall_sites");
        hipLaunchKernelGGL(k_call_sites, dim3((unsigned)nb), dim3(CL_BLOCK), 0, ctx->stream, d_site_pos, d_site_ref, d_site_alt, nsites, dChrSite, dChrSeg, (int)nchr, dBegin, dEnd, dSiteSeg, dBlockCnt, dSt);
        hipLaunchKernelGGL(k_call_scan, dim3(1), dim3(1024), 0, ctx->stream, dBlockCnt, nb, dBlockOff, dSt);
        hipLaunchKernelGGL(k_call_scatter, dim3((unsigned)nb), dim3(CL_BLOCK), 0, ctx->stream, d_site_ref, d_site_alt, nsites, dSiteSeg, dBlockOff, dMaf, dCseg);
    }
    hipLaunchKernelGGL(k_call_segoff, dim3(segGrid), dim3(CL_BLOCK), 0, ctx->stream, dCseg, dSt, nseg, dSegOff);
    CANVAS_HIP_TRY(ctx, hipGetLastError());
    rc = cl_segment_select_enqueue(ctx, d_count, nseg, h_seg_bin_offset, CL_MODE_MEDIAN_F32, dMedCount, hBad + 0); if (rc) return rc;
    {
        const int64_t all[2] = {0, enrichment ? (int64_t)nseg : nbins};
        if (enrichment) hipLaunchKernelGGL(k_scall_to_float, dim3(segGrid), dim3(CL_BLOCK), 0, ctx->stream, dMedCount, nseg, dMedF);
        rc = cl_segment_select_enqueue(ctx, enrichment ? dMedF : d_count, 1, all, CL_MODE_MEDIAN_F32, dQ, hBad + 1); if (rc) return rc;
    }
    CANVAS_HIP_TRY(ctx, hipMemcpyAsync(hSt, dSt, sizeof(ClSiteStat), hipMemcpyDeviceToHost, ctx->stream));
    CANVAS_HIP_TRY(ctx, hipMemcpyAsync(hQ, dQ, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    CANVAS_HIP_TRY(ctx, hipMemcpyAsync(O.seg_site_offset, dSegOff, (S + 1) * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
    CANVAS_HIP_TRY(ctx, hipMemcpyAsync(O.seg_median_count, dMedCount, S * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    CANVAS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (hBad[0] != none) return fail(CANVAS_ERR_INVALID, "counts must be finite (first non-finite count at index " + std::to_string(hBad[0]) + ")");
    if (hSt->unsorted != none) return fail(CANVAS_ERR_INVALID, "within a chromosome the sites' positions must not decrease and their counts must not be negative (site " + std::to_string(hSt->unsorted) + ")");
    if (hSt->kept == 0) return fail(CANVAS_ERR_INVALID, "no site with ref + alt >= 10 inside a segment (the reference's Average() of an empty sequence throws)");
    R.kept_sites = (int64_t)hSt->kept;
    R.mean_coverage = (double)(long long)hSt->covSum / (double)(long long)hSt->kept;
    const float q2 = (float)hQ[0];
    R.overall_median_coverage = q2;
    // ---- the upper medians of the folded frequencies: the second wait
    rc = cl_segment_select_enqueue(ctx, dMaf, nseg, O.seg_site_offset, CL_MODE_UPPER, dMafUp, hBad + 2); if (rc) return rc;
    CANVAS_HIP_TRY(ctx, hipMemcpyAsync(O.seg_maf_upper, dMafUp, S * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    CANVAS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (hBad[2] != none) return fail(CANVAS_ERR_INVALID, "a folded frequency is not finite");      // (cannot happen: ref + alt >= 10)
    R.stage1_ms = lap();

    // ---- stage 2: the threshold loop is arithmetic on the counts that are back
    int threshold = P.minimum_variant_frequencies;
    std::vector<int> dense(S, -1);
    long long nusable = 0;
    for (long long s = 0; s < nseg; s++) {
        const int len = h_seg_end[s] - h_seg_begin[s];
        const bool ok = !(len < 5000) && !(O.seg_median_count[s] > (double)q2 * 2);
        O.seg_usable[s] = ok ? 1 : 0;
        if (ok) dense[(size_t)s] = (int)nusable++;
    }
    while (true) {
        long long validMafCount = 0;
        for (long long s = 0; s < nseg; s++) if (O.seg_usable[s] && O.seg_site_offset[s + 1] - O.seg_site_offset[s] >= threshold) validMafCount++;
        if (validMafCount > std::min<long long>(20, nseg)) break;
        if (threshold <= 5) break;
        threshold -= 15;
        threshold = std::max(5, threshold);
    }
    R.threshold_used = threshold; R.nusable = nusable;
    // ---- stage 3's compaction plan: the bins of the usable segments at reference copy number 2
    std::vector<long long> dst(S, -1);
    long long total = 0;
    for (long long s = 0; s < nseg; s++)
        if (O.seg_usable[s] && (!h_seg_ref_cn || h_seg_ref_cn[s] == 2)) { dst[(size_t)s] = total; total += h_seg_bin_offset[s + 1] - h_seg_bin_offset[s]; }
    rc = canvas_h2d_small(ctx, dDense, dense.data(), S * sizeof(int)); if (rc) return rc;
    rc = canvas_h2d_small(ctx, dDst, dst.data(), S * sizeof(long long)); if (rc) return rc;
    hipLaunchKernelGGL(k_scall_usable, dim3(segGrid), dim3(CL_BLOCK), 0, ctx->stream, nseg, dBegin, dEnd, dSegOff, dMedCount, dMafUp, dDense, threshold, dCov, dMafU, dW, dUCov, dUMaf, dUW, dULen);
    const bool level = nusable >= 3 && total > 0;
    if (level) {
        ProfScope ps(ctx, "scall_compact");
        hipLaunchKernelGGL(k_scall_compact, dim3((unsigned)((nbins + CL_BLOCK - 1) / CL_BLOCK)), dim3(CL_BLOCK), 0, ctx->stream, d_count, (long long)nbins, nseg, dBinOff, dDst, dCompact);
    }
    CANVAS_HIP_TRY(ctx, hipGetLastError());
    if (level) {
        const int64_t all[2] = {0, total};
        rc = cl_segment_select_enqueue(ctx, dCompact, 1, all, CL_MODE_MEDIAN_F32, dQ + 1, hBad + 3); if (rc) return rc;
        CANVAS_HIP_TRY(ctx, hipMemcpyAsync(hQ + 1, dQ + 1, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    }
    CANVAS_HIP_TRY(ctx, hipMemcpyAsync(O.seg_coverage, dCov, S * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    CANVAS_HIP_TRY(ctx, hipMemcpyAsync(O.seg_maf, dMafU, S * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    CANVAS_HIP_TRY(ctx, hipMemcpyAsync(O.seg_weight, dW, S * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    CANVAS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));                                                        // ---- the third wait
    R.stages = 2; R.stage23_ms = lap();
    if (nusable < 3) return fail(CANVAS_ERR_SOMATIC_FEW_SEGMENTS, "cannot model coverage/purity with less than 3 usable segments (" + std::to_string(nusable) + ")");

    // ---- stage 3: the scalars
    if (total == 0) return fail(CANVAS_ERR_INVALID, "no usable segment at reference copy number 2: the reference's Quartiles of an empty list indexes out of range");
    int medianCoverageLevel = 0;
    if (!sc_to_int32((float)hQ[1], medianCoverageLevel)) return fail(CANVAS_ERR_INVALID, "the median coverage level leaves int32");
    R.median_coverage_level = medianCoverageLevel;
    if (medianCoverageLevel < 1) return fail(CANVAS_ERR_INVALID, "the median coverage level is " + std::to_string(medianCoverageLevel) + ": the reference divides the coverage weighting by it");
    double cwf;
    if (!std::isnan(P.evenness_score) && P.evenness_score < P.evenness_score_threshold) {
        if (P.coverage_weighting <= P.coverage_weighting_with_maf_segmentation) return fail(CANVAS_ERR_INVALID, "CoverageWeighting should be larger than CoverageWeightingWithMafSegmentation");
        const double scaler = std::max(P.evenness_score - P.min_evenness_score, 0.0) / (P.evenness_score_threshold - P.min_evenness_score);
        cwf = P.coverage_weighting_with_maf_segmentation + (P.coverage_weighting - P.coverage_weighting_with_maf_segmentation) * scaler;
        cwf /= medianCoverageLevel;
    } else cwf = P.coverage_weighting / medianCoverageLevel;
    int minCoverage = (int)std::max(10.0f, (float)medianCoverageLevel / P.lower_coverage_level_weighting_factor);
    int maxCoverage = (int)std::max(10.0f, (float)medianCoverageLevel * P.upper_coverage_level_weighting_factor);
    if (P.user_ploidy >= 0) {
        const double fixed = (double)((float)medianCoverageLevel / P.user_ploidy) * 2.0;       // GetDiploidCoverage (:2371)
        if (!(fixed >= 1 && fixed < 100001)) return fail(CANVAS_ERR_INVALID, "the diploid coverage of the user ploidy must be 1 .. 100000");
        minCoverage = maxCoverage = (int)fixed;
    }
    canvas_somatic_params fitParams = P.fit;
    if (nseg < 500) fitParams.deviation_factor = 2.0f;
    R.coverage_weighting_factor = cwf; R.min_coverage = minCoverage; R.max_coverage = maxCoverage; R.deviation_factor = fitParams.deviation_factor;
    R.fixed_percent_purity = P.user_purity >= 0 ? (int)(P.user_purity * 100) : -1;
    R.stages = 3;

    // ---- stage 4: the fit, on the device arrays of stage 2
    canvas_somatic_grid grid{};
    grid.min_coverage = minCoverage; grid.max_coverage = maxCoverage; grid.minimum_purity_hard_limit = P.minimum_purity_hard_limit; grid.fixed_percent_purity = R.fixed_percent_purity;
    grid.fixed_coverage = P.user_ploidy >= 0 ? minCoverage : -1; grid.is_enrichment = enrichment ? 1 : 0; grid.min_minor_allele_coverage = P.min_minor_allele_coverage;
    grid.coverage_weighting_factor = cwf; grid.genome_length = P.genome_length;
    R.stage23_ms += lap();
    rc = canvas_somatic_model_fit(ctx, nusable, dUCov, dUMaf, dUW, dULen, 1, &grid, &fitParams, h_fit, nullptr, nullptr, nullptr);
    R.stage4_ms = lap();
    if (rc) return rc;

    // ---- stage 5: the unrefined ploidy table of the best model (InitializeModelPoints(model), :754-777), the scan and MeanCount: the fourth wait
    ScModel M{};
    {
        unsigned char ptCn[SC_MAXP], ptMajor[SC_MAXP];
        M.P = som_points(maxCN, ptCn, ptMajor); M.maxCN = maxCN; M.cwf = cwf;
        const double diploidCoverage = h_fit->diploid_coverage, purity = h_fit->purity;
        const double tumorHaploid = diploidCoverage * purity / 2.0, normalHaploid = diploidCoverage * (1.0 - purity) / 2.0;
        const long long nmax = (long long)h_fit->best_coverage * maxCN / 2 + 2;
        std::vector<double> logFactorial((size_t)nmax + 1, 0.0);
        for (long long i = 2; i <= nmax; i++) logFactorial[(size_t)i] = log((double)i) + logFactorial[(size_t)i - 1];
        for (int p = 0; p < M.P; p++) {
            const double coverage = ptCn[p] * tumorHaploid + 2 * normalHaploid;
            M.cov[p] = coverage; M.maf[p] = som_adjusted_maf((ptCn[p] - ptMajor[p]) * tumorHaploid + normalHaploid, coverage, logFactorial.data());
            M.hcov[p] = ptCn[p] * tumorHaploid + normalHaploid; M.cn[p] = ptCn[p]; M.major[p] = ptMajor[p];
        }
    }
    rc = canvas_h2d_small(ctx, dModel, &M, sizeof(M)); if (rc) return rc;
    const char* meanHook = cvx_hook("CANVAS_SOMATIC_MEAN");
    const int forceWalk = meanHook && !strcmp(meanHook, "walk") ? 1 : 0;
    {
        ProfScope ps(ctx, "scall_assign");
        hipLaunchKernelGGL(k_scall_assign, dim3(segGrid), dim3(CL_BLOCK), 0, ctx->stream, nseg, dSegOff, dMedCount, dMafUp, h_seg_ref_cn ? dRefCn : (const int*)nullptr, dModel, dCn, dCn2, dMcc, dDist, dDist2);
        hipLaunchKernelGGL(k_scall_mean, dim3((unsigned)nseg), dim3(CL_BLOCK), 0, ctx->stream, d_count, dBinOff, dCn, maxCN, forceWalk, dMean, dRoute);
    }
    CANVAS_HIP_TRY(ctx, hipGetLastError());
    CANVAS_HIP_TRY(ctx, hipMemcpyAsync(O.seg_cn, dCn, S * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    CANVAS_HIP_TRY(ctx, hipMemcpyAsync(O.seg_cn2, dCn2, S * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    CANVAS_HIP_TRY(ctx, hipMemcpyAsync(O.seg_mcc, dMcc, S * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    CANVAS_HIP_TRY(ctx, hipMemcpyAsync(O.seg_dist, dDist, S * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    CANVAS_HIP_TRY(ctx, hipMemcpyAsync(O.seg_dist2, dDist2, S * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    CANVAS_HIP_TRY(ctx, hipMemcpyAsync(O.seg_mean_count, dMean, S * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    CANVAS_HIP_TRY(ctx, hipMemcpyAsync(O.seg_mean_route, dRoute, S * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    CANVAS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    {
        const double diploidCoverage = h_fit->diploid_coverage, purity = h_fit->purity;
        for (long long s = 0; s < nseg; s++) {                   // :2438-2454
            if (O.seg_cn[s] != maxCN) continue;
            const double coverageRatio = O.seg_mean_count[s] / diploidCoverage;
            const int referenceCN = h_seg_ref_cn ? h_seg_ref_cn[s] : 2;
            const double estimateCopyNumber = (2 * coverageRatio - referenceCN * (1 - purity)) / purity;
            const int estimateCN = cl_round_to_int(estimateCopyNumber);
            if (estimateCN > maxCN) {
                O.seg_cn[s] = estimateCN; O.seg_mcc[s] = -1;
                const double coverage = diploidCoverage * ((1 - purity) + purity * estimateCN / 2.0f);
                O.seg_dist[s] = fabs(O.seg_mean_count[s] - coverage) * cwf;
            }
        }
    }

    R.stage5_ms = lap();

    // ---- stage 6: the host tail
    std::vector<int> chrOf(S);
    for (int c = 0; c < nchr; c++) for (long long s = h_chr_seg_offset[c]; s < h_chr_seg_offset[c + 1]; s++) chrOf[(size_t)s] = c;
    for (long long s = 0; s < nseg; s++) O.seg_qscore[s] = sc_qscore(P, h_seg_bin_offset[s + 1] - h_seg_bin_offset[s], O.seg_cn[s], O.seg_dist[s], O.seg_dist2[s]);
    double reportedPurity = h_fit->purity;
    if (!std::isnan(P.snv_purity_estimate)) {                    // SelectPurityEstimate (:2653-2673), on the segments before the merge
        double fractionAbnormal = 0, totalWeight = 0;
        for (long long s = 0; s < nseg; s++) {
            const int len = h_seg_end[s] - h_seg_begin[s];
            totalWeight += len;
            if (O.seg_cn[s] != 2 || O.seg_mcc[s] != 1) fractionAbnormal += len;
        }
        fractionAbnormal /= totalWeight;
        if (fractionAbnormal < 0.07 && reportedPurity < 0.5) reportedPurity = P.snv_purity_estimate;
    }
    struct Seg { int begin, end; long long bins; };
    std::vector<Seg> G(S); std::vector<long long> into(S, -1);
    for (long long s = 0; s < nseg; s++) G[(size_t)s] = Seg{h_seg_begin[s], h_seg_end[s], h_seg_bin_offset[s + 1] - h_seg_bin_offset[s]};
    auto mergeIn = [&](long long a, long long b) {               // G[a].MergeIn(G[b]), CanvasSegment.cs:318-334
        Seg& A = G[(size_t)a]; const Seg B = G[(size_t)b];
        if (B.begin < A.begin) { A.begin = B.begin; A.bins += B.bins; }
        if (B.end > A.end) { A.end = B.end; A.bins += B.bins; }
        into[(size_t)b] = a;
    };
    auto forbidden = [&](int c, int start, int end) {            // IsForbiddenInterval, :752-764
        if (!h_chr_excl_offset) return false;
        for (long long k = h_chr_excl_offset[c]; k < h_chr_excl_offset[c + 1]; k++) {
            if (h_excl_start[k] >= start && h_excl_start[k] <= end) return true;
            if (h_excl_stop[k] >= start && h_excl_stop[k] <= end) return true;
            if (h_excl_start[k] > end) break;
        }
        return false;
    };
    auto size_of = [&](long long i) { return G[(size_t)i].end - G[(size_t)i].begin; };
    const int mcs = P.minimum_call_size, span = P.merge_span;
    std::vector<long long> first, runs;
    for (long long i = 0; i < nseg;) {
        if (size_of(i) >= mcs) { first.push_back(i); i++; continue; }
        long long prev = -1, next = -1; double prevQ = enrichment ? -1 : 0, nextQ = enrichment ? -1 : 0;
        for (long long c = i - 1; enrichment ? c >= 0 : c > 0; c--) {
            if (chrOf[(size_t)c] != chrOf[(size_t)i]) break;
            if (size_of(c) < mcs) continue;
            if (enrichment ? G[(size_t)i].begin - G[(size_t)c].end > span : forbidden(chrOf[(size_t)c], G[(size_t)c].end, G[(size_t)i].begin)) break;
            prev = c; prevQ = O.seg_qscore[c];
            break;
        }
        for (long long c = i + 1; c < nseg; c++) {
            if (chrOf[(size_t)c] != chrOf[(size_t)i]) break;
            if (size_of(c) < mcs) continue;
            if (enrichment ? G[(size_t)c].begin - G[(size_t)i].end > span : forbidden(chrOf[(size_t)c], G[(size_t)i].end, G[(size_t)c].begin)) break;
            next = c; nextQ = O.seg_qscore[c];
            break;
        }
        if ((enrichment ? prevQ >= 0 : prevQ > 0) && prevQ >= nextQ) { mergeIn(prev, i); i++; continue; }
        if (enrichment ? nextQ >= 0 : nextQ > 0) {
            if (enrichment) for (long long t = next - 1; i <= t; t--) mergeIn(next, t);
            else for (long long t = i; t < next; t++) mergeIn(next, t);
            i = next;
            continue;
        }
        first.push_back(i); i++;
    }
    {
        long long last = first[0];
        runs.push_back(last);
        for (size_t k = 1; k < first.size(); k++) {
            const long long s = first[k];
            const bool near = enrichment ? G[(size_t)s].begin - G[(size_t)last].end < span : !forbidden(chrOf[(size_t)last], G[(size_t)last].end, G[(size_t)s].begin);
            if (O.seg_cn[last] == O.seg_cn[s] && chrOf[(size_t)last] == chrOf[(size_t)s] && near) { mergeIn(last, s); continue; }
            last = s; runs.push_back(s);
        }
    }
    const long long nruns = (long long)runs.size();
    std::vector<long long> runOf(S, -1); std::vector<int> passes(S, 1);
    for (long long r = 0; r < nruns; r++) {
        const long long o = runs[(size_t)r]; const Seg& g = G[(size_t)o];
        runOf[(size_t)o] = r;
        O.run_owner[r] = o; O.run_begin[r] = g.begin; O.run_end[r] = g.end; O.run_bin_count[r] = g.bins;
        O.run_qscore[r] = sc_qscore(P, g.bins, O.seg_cn[o], O.seg_dist[o], O.seg_dist2[o]);
        O.run_filter[r] = (O.run_qscore[r] < P.quality_filter_threshold ? 1 : 0) | (g.end - g.begin < 10000 ? 2 : 0);
        passes[(size_t)o] = O.run_filter[r] == 0;
    }
    for (long long s = 0; s < nseg; s++) { long long t = s; while (runOf[(size_t)t] < 0) t = into[(size_t)t]; O.seg_run[s] = runOf[(size_t)t]; }
    // EstimateChromosomeCount (:2613-2646) over the original list: absorbed segments keep their PASS default, absorbers have grown, int32 arithmetic
    double overallCount = 0;
    {
        std::vector<uint32_t> base((size_t)maxCN + 1, 0u);
        auto weighted = [&]() {
            double weightedMean = 0, weight = 0;
            for (int c = 0; c <= maxCN; c++) { weight += (double)(int32_t)base[(size_t)c]; weightedMean += (double)(int32_t)(base[(size_t)c] * (uint32_t)c); }
            return weight == 0 ? 0.0 : weightedMean / weight;
        };
        int current = -1;
        for (long long s = 0; s < nseg; s++) {
            if (chrOf[(size_t)s] != current) {
                if (current >= 0) overallCount += weighted();
                std::fill(base.begin(), base.end(), 0u);
                current = chrOf[(size_t)s];
            }
            if (!passes[(size_t)s]) continue;
            if (O.seg_cn[s] == -1) continue;
            base[(size_t)std::min(O.seg_cn[s], maxCN)] += (uint32_t)(G[(size_t)s].end - G[(size_t)s].begin);
        }
        overallCount += weighted();
    }
    R.nruns = nruns; R.reported_purity = reportedPurity; R.purity_model_fit = h_fit->deviation; R.inter_model_distance = h_fit->inter_model_distance;
    R.estimated_chromosome_count = overallCount; R.heterogeneity_proportion = 0; R.stages = 6; R.stage6_ms = lap();
    return CANVAS_OK;
}

extern "C" int32_t canvas_call_somatic(canvas_ctx* ctx, int64_t nbins, const float* d_count, int32_t nchr, const int64_t* h_chr_seg_offset, const int32_t* h_seg_begin,
                                       const int32_t* h_seg_end, const int64_t* h_seg_bin_offset, const int64_t* h_chr_site_offset, const int32_t* d_site_pos,
                                       const int32_t* d_site_ref, const int32_t* d_site_alt, const int32_t* h_seg_ref_cn, const int64_t* h_chr_excl_offset,
                                       const int32_t* h_excl_start, const int32_t* h_excl_stop, const canvas_somatic_call_params* params, const canvas_somatic_call_out* out,
                                       canvas_somatic_call_scalars* h_scalars, canvas_somatic_result* h_fit) {
    return sc_call_somatic(ctx, nbins, d_count, nchr, h_chr_seg_offset, h_seg_begin, h_seg_end, h_seg_bin_offset, h_chr_site_offset, d_site_pos, d_site_ref, d_site_alt, h_seg_ref_cn,
                           h_chr_excl_offset, h_excl_start, h_excl_stop, params, out, h_scalars, h_fit);
}

// canvas_segment_tables (segtab.hip), canvas_reference_copy_numbers (partstate.hip) on its tables, then the call: the somatic sample from per-bin segment ids to copy-number
// calls without a per-bin array leaving the device.  One wait for the tables and the call's own.
extern "C" int32_t canvas_call_somatic_ids(canvas_ctx* ctx, int64_t nbins, int32_t nchr, const int64_t* h_chr_offset, const int32_t* d_start, const int32_t* d_stop, const int32_t* d_segment_id,
                                           const double* d_cov, int64_t cap_seg, const int64_t* h_chr_site_offset, const int32_t* d_site_pos, const int32_t* d_site_ref, const int32_t* d_site_alt,
                                           const int64_t* h_ploidy_offset, const int32_t* h_ploidy_start, const int32_t* h_ploidy_end, const int32_t* h_ploidy_cn,
                                           const int64_t* h_chr_excl_offset, const int32_t* h_excl_start, const int32_t* h_excl_stop, const canvas_somatic_call_params* params,
                                           int64_t* h_nseg, int64_t* h_chr_seg_offset, int32_t* h_seg_begin, int32_t* h_seg_end, int64_t* h_seg_bin_offset, int32_t* h_seg_ci4, float* d_count_f32,
                                           int32_t* h_seg_ref_cn, const canvas_somatic_call_out* out, canvas_somatic_call_scalars* h_scalars, canvas_somatic_result* h_fit) {
    if (!d_cov || !d_count_f32 || (cap_seg > 0 && !h_seg_ref_cn)) {
        if (ctx) ctx->err = "canvas_call_somatic_ids: bad arguments (the call needs the coverage, room for the float counts and for the reference copy numbers)";
        return CANVAS_ERR_INVALID;
    }
    // canvas_segment_tables decides its host arguments before it looks at the context, so a NULL ctx still reports them
    int32_t rc = canvas_segment_tables(ctx, nbins, nchr, h_chr_offset, d_start, d_stop, d_segment_id, d_cov, cap_seg, h_nseg, h_chr_seg_offset, h_seg_begin, h_seg_end, h_seg_bin_offset, h_seg_ci4,
                                       d_count_f32);
    if (rc) return rc;
    rc = canvas_reference_copy_numbers(nchr, h_chr_seg_offset, h_seg_begin, h_seg_end, h_ploidy_offset, h_ploidy_start, h_ploidy_end, h_ploidy_cn, h_seg_ref_cn);
    if (rc) { ctx->err = "canvas_call_somatic_ids: bad ploidy records (offsets that do not start at 0 or decrease, a missing array, or a copy number outside 0..4)"; return rc; }
    return sc_call_somatic(ctx, nbins, d_count_f32, nchr, h_chr_seg_offset, h_seg_begin, h_seg_end, h_seg_bin_offset, h_chr_site_offset, d_site_pos, d_site_ref, d_site_alt, h_seg_ref_cn,
                           h_chr_excl_offset, h_excl_start, h_excl_stop, params, out, h_scalars, h_fit);
}
