// canvas_segment_tables: Segments.ReadSegments (CanvasCommon/Segments.cs:52-115) applied to device-resident bins instead of the rows of a *.partitioned file.  Every
// partition entry (canvas_sample_pipeline, canvas_cbs, canvas_wavelets, canvas_hmm_*, canvas_segment_ids*) ends in a per-bin segment id on the device; the callers
// (canvas_call_diploid, canvas_call_somatic) start from host segment tables and a float count array.  This is the join.
//
// GroupByAdjacent by chromosome, then by id (:55, :63): bin i starts a segment when it is the first bin of its chromosome or when id[i] != id[i-1].  Only adjacency counts: an
// id that returns later is a new segment, an id that runs across a chromosome boundary is split there, a negative id is a value like any other.  Everything a boundary
// needs is the bin pair (i-1, i): Begin and the start interval of the segment that opens at i, End and the end interval of the one that closes at i-1.  Integers only, so
// there is no ordering question.
//
// Three launches, the form of k_call_sites / k_call_scan / k_call_scatter (call.hip):
//   k_segtab_flags    one thread per bin: the start flag (kept as a byte: bit 0 segment start, bit 1 first bin of its chromosome), the workgroup's count of starts, the
//                     checks (first offending bin by atomicMin) and count_f32[i] = (float)cov[i].  Reads 12 + 8 B/bin, writes 4 + 1.
//   k_segtab_scan     exclusive scan of the workgroup counts by ONE workgroup that loops over its share: any number of workgroups.
//   k_segtab_scatter  one thread per bin: a start bin i of rank s writes begin[s], bin_offset[s], ci[s].start and, for s > 0, end[s-1] and ci[s-1].end from the bins i-1
//                     and i; the last bin closes the last segment.  A bin that opens a chromosome also writes that chromosome's rank (and that of the empty ones in front of it).
// No look-back, no spin-wait: the scan is a launch of its own.  The tables land in pinned staging and are handed to the caller's arrays after the ONE wait, so a refused
// call leaves them alone.
#include "common.hpp"
#include <algorithm>

#define ST_BLOCK 256

struct StStat { unsigned long long unsorted, badStop, badCov, nseg; };      // first bin whose start goes backwards / that ends before it starts / whose coverage is not finite (~0 none)

// (int)Math.Round(Length / 2.0, MidpointRounding.AwayFromZero) for Length = stop - start >= 0 (GetHalfLength, Segments.cs:95-98)
__device__ __forceinline__ int st_half(int start, int stop) { const long long L = (long long)stop - (long long)start; return (int)((L + 1) >> 1); }
__device__ __forceinline__ bool st_finite(double v) { return ((unsigned long long)__double_as_longlong(v) & 0x7FF0000000000000ull) != 0x7FF0000000000000ull; }
// the last chromosome c with chrOff[c] <= i (the empty ones in front of it share its offset)
__device__ __forceinline__ int st_chr_of(const long long* __restrict__ chrOff, int nchr, long long i) {
    int lo = 0, hi = nchr;
    while (hi - lo > 1) { const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1); if (chrOff[mid] <= i) lo = mid; else hi = mid; }
    return lo;
}

__global__ void __launch_bounds__(ST_BLOCK) k_segtab_flags(long long nbins, const int* __restrict__ start, const int* __restrict__ stop, const int* __restrict__ id, const double* __restrict__ cov,
                                                           const long long* __restrict__ chrOff, int nchr, unsigned char* __restrict__ flags, unsigned* __restrict__ blockCnt,
                                                           float* __restrict__ countF32, StStat* __restrict__ st) {
    const long long i = (long long)blockIdx.x * ST_BLOCK + threadIdx.x;
    int f = 0;
    if (i < nbins) {
        const int a = start[i], b = stop[i];
        const bool chrFirst = chrOff[st_chr_of(chrOff, nchr, i)] == i;
        if (chrFirst) f = 3;
        else {
            if (id[i] != id[i - 1]) f = 1;
            if (a < start[i - 1]) atomicMin(&st->unsorted, (unsigned long long)i);
        }
        if (b < a) atomicMin(&st->badStop, (unsigned long long)i);
        if (cov) {
            const double v = cov[i];
            if (!st_finite(v)) atomicMin(&st->badCov, (unsigned long long)i);
            countF32[i] = (float)v;
        }
        flags[i] = (unsigned char)f;
    }
    const int cnt = __syncthreads_count(f & 1);
    if (threadIdx.x == 0) blockCnt[blockIdx.x] = (unsigned)cnt;
}

// exclusive scan of the workgroup counts by ONE workgroup; thread t takes the counts [t * per, (t + 1) * per): correct for any nb.  blockOff[nb] = segments
__global__ void __launch_bounds__(1024) k_segtab_scan(const unsigned* __restrict__ blockCnt, long long nb, unsigned long long* __restrict__ blockOff, StStat* __restrict__ st) {
    __shared__ unsigned long long part[1024];
    const long long per = (nb + 1023) / 1024, b0 = threadIdx.x * per, b1 = b0 + per < nb ? b0 + per : nb;
    unsigned long long s = 0;
    for (long long b = b0; b < b1; b++) s += blockCnt[b];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) { unsigned long long run = 0; for (int t = 0; t < 1024; t++) { const unsigned long long v = part[t]; part[t] = run; run += v; } blockOff[nb] = run; st->nseg = run; }
    __syncthreads();
    s = part[threadIdx.x];
    for (long long b = b0; b < b1; b++) { blockOff[b] = s; s += blockCnt[b]; }
}

// nothing is written when there are more segments than `cap` (the tables hold cap entries, bin_offset cap + 1)
__global__ void __launch_bounds__(ST_BLOCK) k_segtab_scatter(long long nbins, const int* __restrict__ start, const int* __restrict__ stop, const unsigned char* __restrict__ flags,
                                                             const unsigned long long* __restrict__ blockOff, long long nb, unsigned long long cap, const long long* __restrict__ chrOff, int nchr,
                                                             int* __restrict__ begin, int* __restrict__ end, long long* __restrict__ binOff, int* __restrict__ ci4, long long* __restrict__ chrSeg) {
    __shared__ unsigned wtot[ST_BLOCK / 64];
    const unsigned long long total = blockOff[nb];
    if (total > cap) return;                                  // (uniform over the grid)
    const long long i = (long long)blockIdx.x * ST_BLOCK + threadIdx.x;
    const int f = i < nbins ? flags[i] : 0;
    const bool open = f & 1;
    const unsigned long long m = __ballot(open);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) wtot[w] = (unsigned)__builtin_popcountll(m);
    __syncthreads();
    if (i >= nbins) return;
    const int a = start[i], b = stop[i], h = st_half(a, b);
    if (open) {
        unsigned long long s = blockOff[blockIdx.x] + (unsigned)__builtin_popcountll(m & ((1ull << lane) - 1ull));
        for (int t = 0; t < w; t++) s += wtot[t];
        begin[s] = a; binOff[s] = i;
        int hp = 0; bool abut = false;
        if (i > 0) { const int pa = start[i - 1], pb = stop[i - 1]; hp = st_half(pa, pb); abut = !(f & 2) && pb == a; if (s > 0) end[s - 1] = pb; }
        // GetStartConfidenceInterval (:81-86): the previous bin counts only inside the chromosome and when it abuts
        ci4[4 * s + 0] = abut ? -hp : -h; ci4[4 * s + 1] = h;
        // GetEndConfidenceInterval (:88-93) of the segment that closes at i - 1
        if (s > 0) { ci4[4 * (s - 1) + 2] = -hp; ci4[4 * (s - 1) + 3] = abut ? h : hp; }
        if (f & 2) { int c = st_chr_of(chrOff, nchr, i); for (; c >= 0 && chrOff[c] == i; c--) chrSeg[c] = (long long)s; }
    }
    if (i == nbins - 1) {
        end[total - 1] = b; ci4[4 * (total - 1) + 2] = -h; ci4[4 * (total - 1) + 3] = h;
        binOff[total] = nbins;
        for (int c = nchr; c >= 0 && chrOff[c] == nbins; c--) chrSeg[c] = (long long)total;      // chrSeg[nchr] and the empty chromosomes behind the last bin
    }
}

extern "C" int32_t canvas_segment_tables(canvas_ctx* ctx, int64_t nbins, int32_t nchr, const int64_t* h_chr_offset, const int32_t* d_start, const int32_t* d_stop, const int32_t* d_segment_id,
                                         const double* d_cov, int64_t cap_seg, int64_t* h_nseg, int64_t* h_chr_seg_offset, int32_t* h_seg_begin, int32_t* h_seg_end, int64_t* h_seg_bin_offset,
                                         int32_t* h_seg_ci4, float* d_count_f32) {
    // the host arguments are decided first and without the context (no message without one): *h_nseg is written only by a call that reached the device
#define ST_REFUSE(msg) do { if (ctx) ctx->err = (msg); return CANVAS_ERR_INVALID; } while (0)
    if (nbins < 1) ST_REFUSE("canvas_segment_tables: at least one bin");
    if (cap_seg < 0) ST_REFUSE("canvas_segment_tables: cap_seg must not be negative");
    if (nchr < 1 || !h_chr_offset) ST_REFUSE("canvas_segment_tables: bad arguments (at least one chromosome, offsets of nchr + 1 entries)");
    if (h_chr_offset[0] != 0) ST_REFUSE("canvas_segment_tables: the chromosome offsets start at 0");
    for (int c = 0; c < nchr; c++) if (h_chr_offset[c + 1] < h_chr_offset[c]) ST_REFUSE("canvas_segment_tables: the chromosome offsets must be non-decreasing");
    if (h_chr_offset[nchr] != nbins) ST_REFUSE("canvas_segment_tables: the chromosome offsets end at nbins");
    const long long nb = (nbins + ST_BLOCK - 1) / ST_BLOCK;
    if (nb > 0x7FFFFFFFll) ST_REFUSE("canvas_segment_tables: too many bins in one call");
    if (!ctx) return CANVAS_ERR_INVALID;
    if (!d_start || !d_stop || !d_segment_id || !h_nseg || !h_chr_seg_offset || (cap_seg > 0 && (!h_seg_begin || !h_seg_end || !h_seg_bin_offset || !h_seg_ci4)) || (d_cov && !d_count_f32))
        ST_REFUSE("canvas_segment_tables: bad arguments (null array)");
#undef ST_REFUSE
    CANVAS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    // there are at most nbins segments, and 2^31 and more are refused: the tables never hold more than that
    const size_t cap = (size_t)std::min<long long>(std::min<long long>(cap_seg, nbins), 0x7FFFFFFFll);
    StStat* dSt; long long *dChrOff, *dChrSeg, *dBinOff; unsigned char* dFlags; unsigned* dBlockCnt; unsigned long long* dBlockOff; int *dBegin, *dEnd, *dCi;
    int32_t rc = cvx_ws_carve(ctx, 256, [&](WsCarver& cv) {
        cv.take(dSt, 1); cv.take(dChrOff, (size_t)nchr + 1); cv.take(dFlags, (size_t)nbins); cv.take(dBlockCnt, (size_t)nb); cv.take(dBlockOff, (size_t)nb + 1);
        cv.take(dChrSeg, (size_t)nchr + 1); cv.take(dBegin, cap); cv.take(dEnd, cap); cv.take(dBinOff, cap + 1); cv.take(dCi, 4 * cap);
    });
    if (rc) return rc;
    // the tables lie behind one another in the workspace (dChrSeg first): ONE copy brings them into a pinned image with the same layout, a second the flags
    const size_t outBytes = (size_t)((char*)(dCi + 4 * cap) - (char*)dChrSeg);
    rc = canvas_pin_reserve(ctx, 256 + outBytes); if (rc) return rc;
    StStat* hSt = (StStat*)ctx->pin; char* hOut = (char*)ctx->pin + 256;
    auto image = [&](const void* d) { return (const void*)(hOut + ((const char*)d - (const char*)dChrSeg)); };
    const unsigned long long none = ~0ull;
    { StStat z{none, none, none, 0}; rc = canvas_h2d_small(ctx, dSt, &z, sizeof(z)); if (rc) return rc; }
    { std::vector<long long> t(h_chr_offset, h_chr_offset + nchr + 1); rc = canvas_h2d_small(ctx, dChrOff, t.data(), t.size() * sizeof(long long)); if (rc) return rc; }
    {
        ProfScope ps(ctx, "segment_tables");
        hipLaunchKernelGGL(k_segtab_flags, dim3((unsigned)nb), dim3(ST_BLOCK), 0, ctx->stream, (long long)nbins, d_start, d_stop, d_segment_id, d_cov, dChrOff, (int)nchr, dFlags, dBlockCnt, d_count_f32, dSt);
        hipLaunchKernelGGL(k_segtab_scan, dim3(1), dim3(1024), 0, ctx->stream, dBlockCnt, nb, dBlockOff, dSt);
        hipLaunchKernelGGL(k_segtab_scatter, dim3((unsigned)nb), dim3(ST_BLOCK), 0, ctx->stream, (long long)nbins, d_start, d_stop, dFlags, dBlockOff, nb, (unsigned long long)cap, dChrOff, (int)nchr,
                           dBegin, dEnd, dBinOff, dCi, dChrSeg);
    }
    CANVAS_HIP_TRY(ctx, hipGetLastError());
    CANVAS_HIP_TRY(ctx, hipMemcpyAsync(hSt, dSt, sizeof(StStat), hipMemcpyDeviceToHost, ctx->stream));
    CANVAS_HIP_TRY(ctx, hipMemcpyAsync(hOut, dChrSeg, outBytes, hipMemcpyDeviceToHost, ctx->stream));
    CANVAS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));                                                        // ---- the one wait
    const unsigned long long nseg = hSt->nseg;
    *h_nseg = (int64_t)nseg;
    if (hSt->unsorted != none) CANVAS_FAIL(ctx, CANVAS_ERR_INVALID, "canvas_segment_tables: within a chromosome the bins' starts must not decrease (bin " + std::to_string(hSt->unsorted) + ")");
    if (hSt->badStop != none) CANVAS_FAIL(ctx, CANVAS_ERR_INVALID, "canvas_segment_tables: a bin must not stop before it starts (bin " + std::to_string(hSt->badStop) + ")");
    if (hSt->badCov != none) CANVAS_FAIL(ctx, CANVAS_ERR_INVALID, "canvas_segment_tables: the coverage must be finite (first non-finite value at bin " + std::to_string(hSt->badCov) + ")");
    if (nseg > 0x7FFFFFFFull) CANVAS_FAIL(ctx, CANVAS_ERR_INVALID, "canvas_segment_tables: 2^31 segments and more");
    if (nseg > (unsigned long long)cap_seg) CANVAS_FAIL(ctx, CANVAS_ERR_INVALID, "canvas_segment_tables: " + std::to_string(nseg) + " segments, room for " + std::to_string(cap_seg) + " (cap_seg)");
    memcpy(h_chr_seg_offset, image(dChrSeg), ((size_t)nchr + 1) * sizeof(long long));
    memcpy(h_seg_begin, image(dBegin), (size_t)nseg * sizeof(int)); memcpy(h_seg_end, image(dEnd), (size_t)nseg * sizeof(int));
    memcpy(h_seg_bin_offset, image(dBinOff), ((size_t)nseg + 1) * sizeof(long long)); memcpy(h_seg_ci4, image(dCi), 4 * (size_t)nseg * sizeof(int));
    return CANVAS_OK;
}
