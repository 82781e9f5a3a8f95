// CanvasSmooth: RepeatedMedianSmoother (CanvasSmooth/CanvasSmooth.cs:46-77) = Utilities.MedianFilter (CanvasCommon/Utilities.cs:767-791) with half window
// h = 1 .. W over every chromosome's counts, each pass on the output of the pass before.
//
// One pass over n values emits, in this order, the medians of the index windows
//     k <  n - h :  [max(0, k - h), k + h]                      (the loop over the values: a median once h + 1 values are in the window)
//     k >= n - h :  [k - h, n - 1]            when n >= 2h + 1  (the drain loop: one value leaves per median)
//                   [k - (n - h) + 1, n - 1]  when n <  2h + 1  (the window never filled: the drain starts from index 0)
// for k < f(n, h) = n when n >= 2h + 1, else max(0, n - h) + max(0, n - h - 1).  For n >= 2h + 1 that is the centred window clamped at both ends; a shorter
// chromosome comes out SHORTER than it went in, Enumerable.Zip (CanvasSmooth.cs:61) drops its last bins, and the next pass sees the shorter list.
//
// The median is selected by rank counting: x_i has rank #{x_k < x_i} + #{k < i : x_k == x_i}, a permutation of 0 .. m-1 for any finite window, ties included
// (cleaned counts are two-decimal text: ties are the rule).  Odd m: the element of rank (m-1)/2.  Even m (chromosome ends only): (a + b) / 2 in float of the
// ranks m/2 - 1 and m/2.
//
// FUSED path (k_smooth_fused): the value at j after W passes depends on the inputs within H = W(W+1)/2 of j.  A workgroup loads a tile of T bins plus H bins of halo
// per side (cut at the chromosome's ends) into LDS, runs all W passes there between two buffers — the valid region shrinks by h per side at an interior tile edge and
// not at a chromosome end, where the clamped windows are exact — and stores its T outputs: one read and one write of the counts over HBM for any W.  A chromosome
// that fits one tile is one work item with both ends in it and follows the window list above literally, truncation included; a chromosome that needs several tiles
// is longer than 2W, so it never truncates.  LDS: 2 buffers x SM_CAP floats = 32 KB per workgroup (four workgroups fit the 160 KB of a CU by that measure);
// thread t reads addresses t + const, so the reads of a wave are conflict-free.  The path is taken while the two halos are at most a quarter of the buffer
// (W <= 31): beyond that the recomputed halo outweighs what the saved passes over HBM cost.
// PER-PASS path (k_smooth_pass): one launch per h straight from global memory, between two workspace buffers, the last pass into d_out.  Any W; not built for speed.
#include "common.hpp"

#define SM_BLOCK 256
#define SM_CAP 4096                                        // floats per LDS buffer
#define SM_MAX_HALO (SM_CAP / 8)                           // per side

struct SmItem { long long in0, out0; int L, flags, st0, stN; };      // region [in0, in0 + L) of the counts; flags: 1 = starts at the chromosome's first bin, 2 = ends at its last;
                                                                      // the outputs [st0, st0 + stN) of the region go to out0 ..

// the next length of a chromosome of n bins after the pass with half window h
__host__ __device__ static inline long long sm_next_len(long long n, long long h) {
    if (n >= 2 * h + 1) return n;
    const long long a = n - h, b = n - h - 1;
    return (a > 0 ? a : 0) + (b > 0 ? b : 0);
}
// the window of output k (k < sm_next_len(n, h)) of the pass with half window h over n values
__device__ __forceinline__ void sm_window(long long n, long long h, long long k, long long& lo, long long& hi) {
    if (k < n - h) { lo = k - h > 0 ? k - h : 0; hi = k + h; }
    else { lo = (n >= 2 * h + 1) ? k - h : k - (n - h) + 1; hi = n - 1; }
}
// the length after the passes h = 1 .. W (passes that leave the length alone are skipped: h <= (n-1)/2)
static long long sm_final_len(long long n, long long W) {
    long long h = (n - 1) / 2 + 1; if (h < 1) h = 1;
    for (; h <= W && n > 0; h++) n = sm_next_len(n, h);
    return n;
}

// median of x[lo .. hi] by rank counting (x: LDS or global); a window that holds a NaN selects nothing and gives 0 (the call fails on the non-finite flag)
template <class P, class I>
__device__ __forceinline__ float sm_median(P x, I lo, I hi) {
    const int m = (int)(hi - lo + 1), r1 = (m - 1) >> 1, r2 = m >> 1;
    float v1 = 0.0f, v2 = 0.0f; int found = (r1 == r2) ? 1 : 0;
    for (I i = lo; i <= hi; i++) {
        const float xi = x[i]; int cnt = 0;
        for (I k = lo; k <= hi; k++) { const float xk = x[k]; cnt += (xk < xi || (xk == xi && k < i)) ? 1 : 0; }
        if (cnt == r1) { v1 = xi; found++; }
        if (cnt == r2) { v2 = xi; found++; }
        if (found == 3) break;                              // (odd m: r1 == r2, one hit counts twice)
    }
    return (r1 == r2) ? v1 : (v1 + v2) / 2.0f;
}
__device__ __forceinline__ bool sm_finite(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }

__global__ void __launch_bounds__(SM_BLOCK) k_smooth_fused(const SmItem* __restrict__ items, const float* __restrict__ in, float* __restrict__ out, int W,
                                                           unsigned long long* __restrict__ firstBad) {
    __shared__ float buf[2 * SM_CAP];                     // one array, two halves: every access keeps the LDS address space (ds_read / ds_write, no flat instructions)
    const SmItem it = items[blockIdx.x];
    const int tid = threadIdx.x, L = it.L;                  // L <= SM_CAP (host)
    for (int i = tid; i < L; i += SM_BLOCK) {
        const float v = in[it.in0 + i];
        if (!sm_finite(v)) atomicMin(firstBad, (unsigned long long)(it.in0 + i));
        buf[i] = v;
    }
    __syncthreads();
    int so = 0, dO = SM_CAP;                              // offsets of the source and destination halves
    const bool le = it.flags & 1, re = it.flags & 2, whole = le && re;
    int a = 0, b = L;                                       // the valid region of src; for a whole chromosome [0, b) is its current list
    for (int h = 1; h <= W; h++) {
        if (whole) {
            const int nout = (int)sm_next_len(b, h);
            for (int k = tid; k < nout; k += SM_BLOCK) { long long lo, hi; sm_window(b, h, k, lo, hi); buf[dO + k] = sm_median(buf + so, (int)lo, (int)hi); }
            b = nout;
            if (b == 0) break;                              // uniform over the workgroup
        } else {
            // several tiles: the chromosome is longer than 2W + 1, every window is the centred one clamped at the chromosome's ends (index 0 / L - 1 of the region)
            const int na = le ? a : a + h, nb = re ? b : b - h;
            for (int k = na + tid; k < nb; k += SM_BLOCK) {
                const int lo = k - h > 0 ? k - h : 0, hi = k + h < L - 1 ? k + h : L - 1;
                buf[dO + k] = sm_median(buf + so, lo, hi);
            }
            a = na; b = nb;
        }
        __syncthreads();
        const int t = so; so = dO; dO = t;
    }
    for (int k = tid; k < it.stN; k += SM_BLOCK) out[it.out0 + k] = buf[so + it.st0 + k];       // [st0, st0 + stN) lies inside [a, b) (host)
}

// first non-finite count of in[0, total) (index relative to `base`)
__global__ void __launch_bounds__(SM_BLOCK) k_smooth_check(const float* __restrict__ in, long long total, long long base, unsigned long long* __restrict__ firstBad) {
    const long long g = (long long)blockIdx.x * SM_BLOCK + threadIdx.x;
    if (g < total && !sm_finite(in[g])) atomicMin(firstBad, (unsigned long long)(base + g));
}

// one pass, one thread per bin of the call: src / dst point at the call's first bin, off[] are the caller's offsets (off[0] subtracted here), curN / newN the
// lengths before and after this pass
__global__ void __launch_bounds__(SM_BLOCK) k_smooth_pass(const float* __restrict__ src, float* __restrict__ dst, const long long* __restrict__ off, const long long* __restrict__ curN,
                                                          const long long* __restrict__ newN, int nchr, long long h, long long total) {
    const long long g = (long long)blockIdx.x * SM_BLOCK + threadIdx.x;
    if (g >= total) return;
    const long long idx = off[0] + g;
    int lo = 0, hi = nchr;                                  // the last c with off[c] <= idx (empty chromosomes in front of it share its offset)
    while (hi - lo > 1) { const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1); if (off[mid] <= idx) lo = mid; else hi = mid; }
    const long long c0 = off[lo] - off[0], k = g - c0;
    if (k >= newN[lo]) return;
    long long wl, wh; sm_window(curN[lo], h, k, wl, wh);
    dst[g] = sm_median(src + c0, wl, wh);
}

static bool sm_force_per_pass() { const char* e = cvx_hook("CANVAS_SMOOTH_PER_PASS"); return e && *e && *e != '0'; }
static bool sm_fused(long long W) { return W >= 1 && W * (W + 1) / 2 <= SM_MAX_HALO && !sm_force_per_pass(); }

extern "C" int32_t canvas_smooth_lengths(int32_t nchr, const int64_t* h_n, int32_t max_half_window, int64_t* h_out_n) {
    if (nchr < 0 || max_half_window < 0 || (nchr > 0 && (!h_n || !h_out_n))) return CANVAS_ERR_INVALID;
    for (int c = 0; c < nchr; c++) if (h_n[c] < 0) return CANVAS_ERR_INVALID;
    for (int c = 0; c < nchr; c++) h_out_n[c] = sm_final_len(h_n[c], max_half_window);
    return CANVAS_OK;
}

extern "C" int32_t canvas_smooth_plan(int32_t max_half_window, int64_t* h_out4) {
    if (max_half_window < 0 || !h_out4) return CANVAS_ERR_INVALID;
    const long long W = max_half_window, H = W * (W + 1) / 2;
    if (W == 0) { h_out4[0] = 1; h_out4[1] = SM_CAP; h_out4[2] = 0; h_out4[3] = 0; }                // a copy: no kernel
    else if (sm_fused(W)) { h_out4[0] = 1; h_out4[1] = SM_CAP - 2 * H; h_out4[2] = H; h_out4[3] = 1; }
    else { h_out4[0] = 0; h_out4[1] = 0; h_out4[2] = 0; h_out4[3] = W; }                             // at most: the passes end once every chromosome is empty
    return CANVAS_OK;
}

extern "C" int32_t canvas_smooth(canvas_ctx* ctx, int32_t nchr, const int64_t* h_chr_offset, const float* d_count, int32_t max_half_window, float* d_out, int64_t* h_out_n) {
    if (!ctx) return CANVAS_ERR_INVALID;
    if (nchr < 0 || !h_chr_offset || (nchr > 0 && !h_out_n)) CANVAS_FAIL(ctx, CANVAS_ERR_INVALID, "canvas_smooth: bad arguments");
    if (max_half_window < 0) CANVAS_FAIL(ctx, CANVAS_ERR_INVALID, "canvas_smooth: max_half_window must not be negative");
    if (h_chr_offset[0] < 0) CANVAS_FAIL(ctx, CANVAS_ERR_INVALID, "canvas_smooth: the offsets must not be negative");
    for (int c = 0; c < nchr; c++) {
        if (h_chr_offset[c + 1] < h_chr_offset[c]) CANVAS_FAIL(ctx, CANVAS_ERR_INVALID, "canvas_smooth: the chromosome offsets must be non-decreasing");
        if (h_chr_offset[c + 1] - h_chr_offset[c] >= (1ll << 31)) CANVAS_FAIL(ctx, CANVAS_ERR_INVALID, "canvas_smooth: a chromosome must have fewer than 2^31 bins");
    }
    const long long W = max_half_window, off0 = h_chr_offset[0], total = h_chr_offset[nchr] - off0;
    for (int c = 0; c < nchr; c++) h_out_n[c] = sm_final_len(h_chr_offset[c + 1] - h_chr_offset[c], W);
    if (total == 0) return CANVAS_OK;
    if (!d_count || !d_out) CANVAS_FAIL(ctx, CANVAS_ERR_INVALID, "canvas_smooth: bad arguments");
    {   const uintptr_t a0 = (uintptr_t)(d_count + off0), a1 = (uintptr_t)(d_count + off0 + total), b0 = (uintptr_t)(d_out + off0), b1 = (uintptr_t)(d_out + off0 + total);
        if (a0 < b1 && b0 < a1) CANVAS_FAIL(ctx, CANVAS_ERR_INVALID, "canvas_smooth: d_out must not overlap d_count"); }
    if ((total + SM_BLOCK - 1) / SM_BLOCK > 0x7FFFFFFFll) CANVAS_FAIL(ctx, CANVAS_ERR_INVALID, "canvas_smooth: too many bins in one call");
    CANVAS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    int32_t rc = canvas_pin_reserve(ctx, 64); if (rc) return rc;
    unsigned long long* hBad = (unsigned long long*)ctx->pin;
    const unsigned long long none = ~0ull;
    auto bad_check = [&](unsigned long long* dBad) -> int32_t {                  // waits for everything queued so far
        CANVAS_HIP_TRY(ctx, hipMemcpyAsync(hBad, dBad, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
        CANVAS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (*hBad != none) CANVAS_FAIL(ctx, CANVAS_ERR_INVALID, "canvas_smooth: counts must be finite (first non-finite count at index " + std::to_string(*hBad) + ")");
        return CANVAS_OK;
    };

    if (sm_fused(W)) {
        const long long H = W * (W + 1) / 2, T = SM_CAP - 2 * H;
        std::vector<SmItem> items;
        for (int c = 0; c < nchr; c++) {
            const long long o = h_chr_offset[c], n = h_chr_offset[c + 1] - o;
            if (n == 0) continue;
            if (n <= T) { items.push_back({o, o, (int)n, 3, 0, (int)h_out_n[c]}); continue; }       // (n <= T < SM_CAP)
            for (long long t0 = 0; t0 < n; t0 += T) {
                const long long t1 = std::min(n, t0 + T), r0 = std::max(0ll, t0 - H), r1 = std::min(n, t1 + H);
                items.push_back({o + r0, o + t0, (int)(r1 - r0), (r0 == 0 ? 1 : 0) | (r1 == n ? 2 : 0), (int)(t0 - r0), (int)(t1 - t0)});
            }
        }
        if (items.size() > 0x7FFFFFFFull) CANVAS_FAIL(ctx, CANVAS_ERR_INVALID, "canvas_smooth: too many tiles in one call");
        unsigned long long* dBad; SmItem* dItems;
        rc = cvx_ws_carve(ctx, 256, [&](WsCarver& cv) { cv.take(dBad, 1); cv.take(dItems, items.size()); }); if (rc) return rc;
        CANVAS_HIP_TRY(ctx, hipMemsetAsync(dBad, 0xFF, sizeof(unsigned long long), ctx->stream));
        rc = canvas_h2d_small(ctx, dItems, items.data(), items.size() * sizeof(SmItem)); if (rc) return rc;
        {
            ProfScope ps(ctx, "smooth_fused", true);
            hipLaunchKernelGGL(k_smooth_fused, dim3((unsigned)items.size()), dim3(SM_BLOCK), 0, ctx->stream, dItems, d_count, d_out, (int)W, dBad);
        }
        CANVAS_HIP_TRY(ctx, hipGetLastError());
        return bad_check(dBad);
    }

    // ---- W = 0 (a copy) and the per-pass path
    unsigned long long* dBad; long long *dOff, *dCur, *dNew; float* buf[2] = {nullptr, nullptr};
    rc = cvx_ws_carve(ctx, 256, [&](WsCarver& cv) {
        cv.take(dBad, 1); cv.take(dOff, (size_t)nchr + 1); cv.take(dCur, (size_t)nchr); cv.take(dNew, (size_t)nchr);
        if (W > 1) { cv.take(buf[0], (size_t)total); cv.take(buf[1], (size_t)total); }
    });
    if (rc) return rc;
    const unsigned nblk = (unsigned)((total + SM_BLOCK - 1) / SM_BLOCK);
    CANVAS_HIP_TRY(ctx, hipMemsetAsync(dBad, 0xFF, sizeof(unsigned long long), ctx->stream));
    hipLaunchKernelGGL(k_smooth_check, dim3(nblk), dim3(SM_BLOCK), 0, ctx->stream, d_count + off0, total, off0, dBad);
    CANVAS_HIP_TRY(ctx, hipGetLastError());
    rc = bad_check(dBad); if (rc) return rc;
    if (W == 0) {
        CANVAS_HIP_TRY(ctx, hipMemcpyAsync(d_out + off0, d_count + off0, (size_t)total * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
        CANVAS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return CANVAS_OK;
    }
    { std::vector<long long> o(h_chr_offset, h_chr_offset + nchr + 1); rc = canvas_h2d_small(ctx, dOff, o.data(), o.size() * sizeof(long long)); if (rc) return rc; }
    std::vector<long long> cur((size_t)nchr), nxt((size_t)nchr);
    for (int c = 0; c < nchr; c++) cur[c] = h_chr_offset[c + 1] - h_chr_offset[c];
    const float* src = d_count + off0; int flip = 0;
    for (long long h = 1; h <= W; h++) {
        bool any = false;
        for (int c = 0; c < nchr; c++) { nxt[c] = sm_next_len(cur[c], h); any = any || nxt[c] > 0; }
        if (!any) break;                                    // every chromosome is empty from here on: nothing reaches d_out
        rc = canvas_h2d_small(ctx, dCur, cur.data(), (size_t)nchr * sizeof(long long)); if (rc) return rc;
        rc = canvas_h2d_small(ctx, dNew, nxt.data(), (size_t)nchr * sizeof(long long)); if (rc) return rc;
        float* dst = (h == W) ? d_out + off0 : buf[flip];
        {
            ProfScope ps(ctx, "smooth_pass", true);
            hipLaunchKernelGGL(k_smooth_pass, dim3(nblk), dim3(SM_BLOCK), 0, ctx->stream, src, dst, dOff, dCur, dNew, (int)nchr, h, total);
        }
        CANVAS_HIP_TRY(ctx, hipGetLastError());
        src = dst; flip ^= 1; cur.swap(nxt);
    }
    CANVAS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return CANVAS_OK;
}
