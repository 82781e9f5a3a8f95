// canvas_partition_states_cbs / canvas_partition_states_breakpoints: what CBS and Wavelets leave (segment lengths on the device, breakpoints on the host) turned into the
// per-bin array canvas_segment_ids* takes, on the device.  d_state[i] is the zero-based ordinal, within its chromosome, of the segment that holds bin i; every bin of a
// chromosome for which the method derives no segment gets -1.  k_seg_flags (hmm.hip) opens a segment where state >= 0 && (first bin of the chromosome || state != previous
// state): with ordinals that is exactly "bin i is the first bin of a derived segment", i.e. membership of the bin's start coordinate in the `starts` set that
// SegmentationResultsProcessor.PostProcessSegments looks up — as long as the bins' starts increase strictly within a chromosome (two bins with the same start would both be
// found in the set, but only one of them changes the ordinal).
//
//   CBS          CBSRunner.cs:127-137: segment k of a chromosome starts at the sum of the lengths before it (cs1).  No length (h_nseg[c] == 0): no start, -1 throughout.
//   breakpoints  SegmentationInput.DeriveSegments (Segmentation.cs:83-125): with at least two breakpoints and more than 10 bins the starts are bin 0 and every breakpoint,
//                otherwise the chromosome is one segment.  Only the SET of starts reaches PostProcessSegments, so flags are marked: order and repeats do not matter.
//
// Launches (plain multi-launch scan, the form of k_segtab_flags / k_segtab_scan / k_segtab_scatter; no look-back, no spin-wait):
//   (memset)          the start flags, one byte per bin
//   k_ps_cbs_flags    one workgroup per chromosome: a tiled inclusive scan of its lengths (PS_BLOCK per tile, the running sum carried from tile to tile in 64 bits), one flag
//                     per segment start; the checks go into ONE error word by atomicMin (first chromosome, then kind)
//   k_ps_bp_flags     one thread per uploaded breakpoint, and one per chromosome for bin 0
//   k_ps_count        starts per workgroup of PS_BLOCK bins
//   k_ps_scan         ONE workgroup: exclusive scan of those counts (thread t loops over its share: any number of workgroups), then the number of starts in front of each
//                     chromosome (one wave per chromosome: the scanned count of the workgroup its first bin lies in + the flags between that workgroup's first bin and it)
//   k_ps_apply        one thread per bin: inclusive rank of the bin's last start, minus the starts in front of its chromosome, minus 1
// The kernels behind the flag pass read the error word and write nothing once it is set: a refused call leaves d_state alone.  One wait per call (the error word's copy).
#include "common.hpp"
#include <algorithm>

#define PS_BLOCK 256
#define PS_ERR_NSEG 0      // h_nseg[c] outside 0 .. T_c
#define PS_ERR_LEN 1       // a length < 1
#define PS_ERR_SUM 2       // the lengths do not sum to T_c
#define PS_NONE (~0ull)

// the last chromosome c with chrOff[c] <= i (the empty ones in front of it share its offset)
__device__ __forceinline__ int ps_chr_of(const long long* __restrict__ chrOff, int nchr, long long i) {
    int lo = 0, hi = nchr;
    while (hi - lo > 1) { const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1); if (chrOff[mid] <= i) lo = mid; else hi = mid; }
    return lo;
}

__global__ void __launch_bounds__(PS_BLOCK) k_ps_cbs_flags(const long long* __restrict__ chrOff, const int* __restrict__ nseg, const int* __restrict__ segLen, unsigned char* __restrict__ flags,
                                                          unsigned long long* __restrict__ err) {
    __shared__ long long wsum[PS_BLOCK / 64];
    __shared__ long long carry;
    const int c = blockIdx.x;
    const long long b0 = chrOff[c], T = chrOff[c + 1] - b0;
    const int K = nseg[c];
    if (K < 0 || (long long)K > T) { if (threadIdx.x == 0) atomicMin(err, 4ull * (unsigned)c + PS_ERR_NSEG); return; }       // (uniform: nothing of this chromosome is read)
    if (K == 0) return;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    bool badLen = false;
    for (int base = 0; base < K; base += PS_BLOCK) {
        const int k = base + (int)threadIdx.x;
        const long long len = k < K ? (long long)segLen[b0 + k] : 0;      // k < K <= T: inside the chromosome's slots
        if (k < K && len < 1) badLen = true;
        long long inc = len;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const long long o = __shfl_up(inc, d, 64); if (lane >= d) inc += o; }
        if (lane == 63) wsum[w] = inc;
        __syncthreads();
        long long before = carry;
        for (int t = 0; t < w; t++) before += wsum[t];
        const long long first = before + inc - len;                       // cs1 of segment k
        if (k < K && first >= 0 && first < T) flags[b0 + first] = 1;
        __syncthreads();
        if (threadIdx.x == PS_BLOCK - 1) carry = before + inc;
        __syncthreads();
    }
    if (__syncthreads_or(badLen)) { if (threadIdx.x == 0) atomicMin(err, 4ull * (unsigned)c + PS_ERR_LEN); return; }
    if (threadIdx.x == 0 && carry != T) atomicMin(err, 4ull * (unsigned)c + PS_ERR_SUM);
}

// threads [0, nbp): one uploaded breakpoint each (checked on the host: inside its chromosome); threads [nbp, nbp + nchr): bin 0 of a chromosome that has bins
__global__ void __launch_bounds__(PS_BLOCK) k_ps_bp_flags(const long long* __restrict__ chrOff, int nchr, const int* __restrict__ bp, const long long* __restrict__ bpOff, long long nbp,
                                                         unsigned char* __restrict__ flags) {
    const long long t = (long long)blockIdx.x * PS_BLOCK + threadIdx.x;
    if (t < nbp) {
        const int c = ps_chr_of(bpOff, nchr, t);
        const long long b0 = chrOff[c], T = chrOff[c + 1] - b0;
        if (bpOff[c + 1] - bpOff[c] >= 2 && T > 10) { const long long p = bp[t]; if (p >= 0 && p < T) flags[b0 + p] = 1; }
    } else if (t < nbp + nchr) {
        const int c = (int)(t - nbp);
        if (chrOff[c + 1] > chrOff[c]) flags[chrOff[c]] = 1;
    }
}

__global__ void __launch_bounds__(PS_BLOCK) k_ps_count(const unsigned char* __restrict__ flags, long long n, unsigned* __restrict__ blockCnt, const unsigned long long* __restrict__ err) {
    if (*err != PS_NONE) return;
    const long long i = (long long)blockIdx.x * PS_BLOCK + threadIdx.x;
    const int f = i < n ? flags[i] : 0;
    const int cnt = __syncthreads_count(f);
    if (threadIdx.x == 0) blockCnt[blockIdx.x] = (unsigned)cnt;
}

// exclusive scan of the workgroup counts by ONE workgroup (thread t takes the counts [t * per, (t + 1) * per): correct for any nb; blockOff[nb] = all starts), then
// chrBase[c] = starts in front of chromosome c, one wave per chromosome in turn
__global__ void __launch_bounds__(1024) k_ps_scan(const unsigned* __restrict__ blockCnt, long long nb, unsigned* __restrict__ blockOff, const unsigned char* __restrict__ flags, long long n,
                                                  const long long* __restrict__ chrOff, int nchr, unsigned* __restrict__ chrBase, const unsigned long long* __restrict__ err) {
    __shared__ unsigned part[1024];
    if (*err != PS_NONE) return;
    const long long per = (nb + 1023) / 1024, q0 = threadIdx.x * per, q1 = q0 + per < nb ? q0 + per : nb;
    unsigned s = 0;
    for (long long b = q0; b < q1; b++) s += blockCnt[b];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) { unsigned run = 0; for (int t = 0; t < 1024; t++) { const unsigned v = part[t]; part[t] = run; run += v; } blockOff[nb] = run; }
    __syncthreads();
    s = part[threadIdx.x];
    for (long long b = q0; b < q1; b++) { blockOff[b] = s; s += blockCnt[b]; }
    __threadfence_block();
    __syncthreads();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int c = w; c < nchr; c += 1024 / 64) {
        const long long j = chrOff[c], b = j / PS_BLOCK;                  // j == n: b == nb when n is a multiple of the block, otherwise the last, partial workgroup
        unsigned v = 0;
        for (long long i = b * PS_BLOCK + lane; i < j; i += 64) v += flags[i];
        v = wave_reduce_add_u32(v);
        if (lane == 0) chrBase[c] = blockOff[b] + v;
    }
}

__global__ void __launch_bounds__(PS_BLOCK) k_ps_apply(const unsigned char* __restrict__ flags, long long n, const unsigned* __restrict__ blockOff, const long long* __restrict__ chrOff, int nchr,
                                                      const unsigned* __restrict__ chrBase, int* __restrict__ state, const unsigned long long* __restrict__ err) {
    __shared__ unsigned wtot[PS_BLOCK / 64];
    if (*err != PS_NONE) return;
    const long long i = (long long)blockIdx.x * PS_BLOCK + threadIdx.x;
    const bool f = i < n && flags[i];
    const unsigned long long m = __ballot(f);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) wtot[w] = (unsigned)__builtin_popcountll(m);
    __syncthreads();
    if (i >= n) return;
    unsigned incl = blockOff[blockIdx.x] + (unsigned)__builtin_popcountll(m & (lane == 63 ? ~0ull : ((1ull << (lane + 1)) - 1ull)));
    for (int t = 0; t < w; t++) incl += wtot[t];
    // a chromosome that derives segments has a start at its first bin, so the difference is at least 1 there; without any start it is 0 throughout: -1
    state[i] = (int)(incl - chrBase[ps_chr_of(chrOff, nchr, i)]) - 1;
}

#define PS_REFUSE(msg) do { if (ctx) ctx->err = std::string(what) + ": " + (msg); return CANVAS_ERR_INVALID; } while (0)
// the chromosome offsets, decided without the context (no message without one)
static int32_t ps_check_offsets(canvas_ctx* ctx, const char* what, int32_t nchr, const int64_t* h_chr_offset) {
    if (nchr < 1 || !h_chr_offset) PS_REFUSE("bad arguments (at least one chromosome, offsets of nchr + 1 entries)");
    if (h_chr_offset[0] != 0) PS_REFUSE("the chromosome offsets start at 0");
    for (int c = 0; c < nchr; c++) if (h_chr_offset[c + 1] < h_chr_offset[c]) PS_REFUSE("the chromosome offsets must be non-decreasing");
    if (h_chr_offset[nchr] > 0x7FFFFFFFll) PS_REFUSE("too many bins in one call");
    return CANVAS_OK;
}

struct PsBuffers { unsigned long long* err; long long* chrOff; unsigned char* flags; unsigned* blockCnt; unsigned* blockOff; unsigned* chrBase; long long nb; };

// everything behind the flag pass
static void ps_enqueue_rest(canvas_ctx* ctx, const PsBuffers& B, int32_t nchr, long long n, int32_t* d_state) {
    hipLaunchKernelGGL(k_ps_count, dim3((unsigned)B.nb), dim3(PS_BLOCK), 0, ctx->stream, B.flags, n, B.blockCnt, B.err);
    hipLaunchKernelGGL(k_ps_scan, dim3(1), dim3(1024), 0, ctx->stream, B.blockCnt, B.nb, B.blockOff, B.flags, n, B.chrOff, (int)nchr, B.chrBase, B.err);
    hipLaunchKernelGGL(k_ps_apply, dim3((unsigned)B.nb), dim3(PS_BLOCK), 0, ctx->stream, B.flags, n, B.blockOff, B.chrOff, (int)nchr, B.chrBase, d_state, B.err);
}
// the one wait; *h_err = the error word
static int32_t ps_wait(canvas_ctx* ctx, const PsBuffers& B, unsigned long long* h_err) {
    CANVAS_HIP_TRY(ctx, hipGetLastError());
    int32_t rc = canvas_pin_reserve(ctx, 256); if (rc) return rc;
    unsigned long long* hErr = (unsigned long long*)ctx->pin;
    CANVAS_HIP_TRY(ctx, hipMemcpyAsync(hErr, B.err, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    CANVAS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));                                                        // ---- the one wait
    *h_err = *hErr;
    return CANVAS_OK;
}

// carves the workspace behind `extra` bytes of the caller's own tables, uploads the offsets, clears the flags and the error word
template <class Extra> static int32_t ps_begin(canvas_ctx* ctx, int32_t nchr, const int64_t* h_chr_offset, long long n, PsBuffers& B, Extra&& extra) {
    CANVAS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    B.nb = (n + PS_BLOCK - 1) / PS_BLOCK;
    int32_t rc = cvx_ws_carve(ctx, 256, [&](WsCarver& cv) {
        cv.take(B.err, 1); cv.take(B.chrOff, (size_t)nchr + 1); cv.take(B.flags, (size_t)n); cv.take(B.blockCnt, (size_t)B.nb);
        cv.take(B.blockOff, (size_t)B.nb + 1); cv.take(B.chrBase, (size_t)nchr); extra(cv);
    });
    if (rc) return rc;
    const unsigned long long none = PS_NONE;
    rc = canvas_h2d_small(ctx, B.err, &none, sizeof(none)); if (rc) return rc;
    { std::vector<long long> t(h_chr_offset, h_chr_offset + nchr + 1); rc = canvas_h2d_small(ctx, B.chrOff, t.data(), t.size() * sizeof(long long)); if (rc) return rc; }
    CANVAS_HIP_TRY(ctx, hipMemsetAsync(B.flags, 0, (size_t)n, ctx->stream));
    return CANVAS_OK;
}

extern "C" int32_t canvas_partition_states_cbs(canvas_ctx* ctx, int32_t nchr, const int64_t* h_chr_offset, const int32_t* d_seg_len, const int32_t* h_nseg, int32_t* d_state) {
    const char* what = "canvas_partition_states_cbs";
    int32_t rc = ps_check_offsets(ctx, what, nchr, h_chr_offset); if (rc) return rc;
    if (!h_nseg) PS_REFUSE("bad arguments (null array)");
    if (!ctx) return CANVAS_ERR_INVALID;
    const long long n = h_chr_offset[nchr];
    if (n == 0) {      // no bin: nothing to write, but a chromosome without bins still cannot hold a segment
        for (int c = 0; c < nchr; c++) if (h_nseg[c] != 0) PS_REFUSE("chromosome " + std::to_string(c) + ": h_nseg must be 0 (it has no bins)");
        return CANVAS_OK;
    }
    if (!d_seg_len || !d_state) PS_REFUSE("bad arguments (null array)");
    PsBuffers B; int* dNseg = nullptr;
    rc = ps_begin(ctx, nchr, h_chr_offset, n, B, [&](WsCarver& cv) { cv.take(dNseg, (size_t)nchr); }); if (rc) return rc;
    rc = canvas_h2d_small(ctx, dNseg, h_nseg, (size_t)nchr * sizeof(int)); if (rc) return rc;
    unsigned long long err = PS_NONE;
    {
        ProfScope ps(ctx, "partition_states");
        hipLaunchKernelGGL(k_ps_cbs_flags, dim3((unsigned)nchr), dim3(PS_BLOCK), 0, ctx->stream, B.chrOff, dNseg, d_seg_len, B.flags, B.err);
        ps_enqueue_rest(ctx, B, nchr, n, d_state);
    }
    rc = ps_wait(ctx, B, &err); if (rc) return rc;
    if (err != PS_NONE) {
        const long long c = (long long)(err >> 2); const int kind = (int)(err & 3);
        const long long T = h_chr_offset[c + 1] - h_chr_offset[c];
        if (kind == PS_ERR_NSEG) PS_REFUSE("chromosome " + std::to_string(c) + ": h_nseg must lie in 0 .. " + std::to_string(T) + " (its number of bins)");
        if (kind == PS_ERR_LEN) PS_REFUSE("chromosome " + std::to_string(c) + ": a segment length below 1");
        PS_REFUSE("chromosome " + std::to_string(c) + ": the segment lengths must sum to its " + std::to_string(T) + " bins");
    }
    return CANVAS_OK;
}

extern "C" int32_t canvas_partition_states_breakpoints(canvas_ctx* ctx, int32_t nchr, const int64_t* h_chr_offset, const int32_t* h_breakpoints, const int64_t* h_bp_offset, int32_t* d_state) {
    const char* what = "canvas_partition_states_breakpoints";
    // every host argument is decided before the context is looked at, and before any launch
    int32_t rc = ps_check_offsets(ctx, what, nchr, h_chr_offset); if (rc) return rc;
    if (!h_bp_offset) PS_REFUSE("bad arguments (null array)");
    if (h_bp_offset[0] != 0) PS_REFUSE("the breakpoint offsets start at 0");
    for (int c = 0; c < nchr; c++) if (h_bp_offset[c + 1] < h_bp_offset[c]) PS_REFUSE("the breakpoint offsets must be non-decreasing");
    const long long nbp = h_bp_offset[nchr];
    if (nbp > 0x7FFFFFFFll) PS_REFUSE("too many breakpoints in one call");
    if (nbp > 0 && !h_breakpoints) PS_REFUSE("bad arguments (null array)");
    for (int c = 0; c < nchr; c++) {
        const long long T = h_chr_offset[c + 1] - h_chr_offset[c];
        for (long long k = h_bp_offset[c]; k < h_bp_offset[c + 1]; k++)
            if (h_breakpoints[k] < 0 || (long long)h_breakpoints[k] >= T)
                PS_REFUSE("chromosome " + std::to_string(c) + ": breakpoint " + std::to_string(h_breakpoints[k]) + " outside its bins 0 .. " + std::to_string(T - 1));
    }
    if (!ctx) return CANVAS_ERR_INVALID;
    const long long n = h_chr_offset[nchr];
    if (n == 0) return CANVAS_OK;
    if (!d_state) PS_REFUSE("bad arguments (null array)");
    PsBuffers B; int* dBp = nullptr; long long* dBpOff = nullptr;
    rc = ps_begin(ctx, nchr, h_chr_offset, n, B, [&](WsCarver& cv) { cv.take(dBp, (size_t)nbp + 1); cv.take(dBpOff, (size_t)nchr + 1); }); if (rc) return rc;
    if (nbp > 0) { rc = canvas_h2d_small(ctx, dBp, h_breakpoints, (size_t)nbp * sizeof(int)); if (rc) return rc; }
    { std::vector<long long> t(h_bp_offset, h_bp_offset + nchr + 1); rc = canvas_h2d_small(ctx, dBpOff, t.data(), t.size() * sizeof(long long)); if (rc) return rc; }
    unsigned long long err = PS_NONE;
    {
        ProfScope ps(ctx, "partition_states");
        hipLaunchKernelGGL(k_ps_bp_flags, dim3((unsigned)((nbp + nchr + PS_BLOCK - 1) / PS_BLOCK)), dim3(PS_BLOCK), 0, ctx->stream, B.chrOff, (int)nchr, dBp, dBpOff, nbp, B.flags);
        ps_enqueue_rest(ctx, B, nchr, n, d_state);
    }
    return ps_wait(ctx, B, &err);
}
#undef PS_REFUSE

// PloidyInfo.GetReferenceCopyNumber (PloidyInfo.cs:56-72) over getPloidyCounts (:92-110) per segment: plain host code, no context
extern "C" int32_t canvas_reference_copy_numbers(int32_t nchr, const int64_t* h_chr_seg_offset, const int32_t* h_seg_begin, const int32_t* h_seg_end, const int64_t* h_ploidy_offset,
                                                 const int32_t* h_ploidy_start, const int32_t* h_ploidy_end, const int32_t* h_ploidy_cn, int32_t* h_seg_ref_cn) {
    if (nchr < 0 || !h_chr_seg_offset || h_chr_seg_offset[0] != 0) return CANVAS_ERR_INVALID;
    for (int c = 0; c < nchr; c++) if (h_chr_seg_offset[c + 1] < h_chr_seg_offset[c]) return CANVAS_ERR_INVALID;
    const long long nseg = h_chr_seg_offset[nchr];
    if (nseg > 0 && (!h_seg_begin || !h_seg_end || !h_seg_ref_cn)) return CANVAS_ERR_INVALID;
    if (h_ploidy_offset) {
        if (h_ploidy_offset[0] != 0) return CANVAS_ERR_INVALID;
        for (int c = 0; c < nchr; c++) if (h_ploidy_offset[c + 1] < h_ploidy_offset[c]) return CANVAS_ERR_INVALID;
        const long long npl = h_ploidy_offset[nchr];
        if (npl > 0 && (!h_ploidy_start || !h_ploidy_end || !h_ploidy_cn)) return CANVAS_ERR_INVALID;
        for (long long k = 0; k < npl; k++) if (h_ploidy_cn[k] < 0 || h_ploidy_cn[k] > 4) return CANVAS_ERR_INVALID;      // getPloidyCounts indexes a 5-element array: the reference throws
    }
    for (int c = 0; c < nchr; c++)
        for (long long s = h_chr_seg_offset[c]; s < h_chr_seg_offset[c + 1]; s++) {
            int ref = 2;
            if (h_ploidy_offset && h_ploidy_offset[c + 1] > h_ploidy_offset[c]) {
                // the one-based interval [Begin + 1, End]: Length = End - Begin
                const int qs = h_seg_begin[s] + 1, qe = h_seg_end[s];
                int counts[5] = {0, 0, qe - qs + 1, 0, 0};
                for (long long k = h_ploidy_offset[c]; k < h_ploidy_offset[c + 1]; k++) {
                    const int p = h_ploidy_cn[k];
                    if (p == 2) continue;
                    const int overlapStart = std::max(qs - 1, h_ploidy_start[k] - 1);
                    if (overlapStart > h_ploidy_end[k]) continue;
                    const int overlapBases = std::min(qe, h_ploidy_end[k]) - overlapStart;
                    if (overlapBases <= 0) continue;
                    counts[2] -= overlapBases; counts[p] += overlapBases;
                }
                int best = 0;
                for (int cn = 0; cn < 5; cn++) if (counts[cn] > best) { best = counts[cn]; ref = cn; }
            }
            h_seg_ref_cn[s] = ref;
        }
    return CANVAS_OK;
}
