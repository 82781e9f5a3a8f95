// CanvasBin's observed alignments: LoadObservedAlignmentsBAM (CanvasBin/CanvasBin.cs:207-275) over RAW BAM record bytes, in the chunk format of canvas_snv_count (snv.hip):
// the host inflates BGZF blocks and finds where each record starts, nothing of a record is decoded there.
//
// The reference's loop is sequential in two places only: it ENDS at the first record that passes the read filters and belongs to another reference (a prefix rule), and
// the fragment length of a position is the one of the LAST kept read that starts there.  Everything else is a filter per record and a saturating count per position.
//   k_obs_classify  one lane per record: the fixed fields with their shape checks against the record's and the chunk's length (bam_record.hpp: bam_rec_load) and the first
//                   CIGAR word, the filters in the reference's order (:239-262).  8 bytes per record go to the workspace {pos, clamped tlen, class}, 8 bytes per tile of
//                   256 records {lane of the tile's first kept record, its pos}.  The smallest index of a stopping record: bam_block_first, then ONE atomicMax per
//                   workgroup on d_state[6] with the stop key of bam_record.hpp (epoch and index in one word, so that nothing has to reset it between chunks).
//   k_obs_apply     one lane per record below the stop: counters (reduced per workgroup), hits, fragment lengths.
//                   hits, mode 0: a byte store of 1.  Modes 3 / 5: a compare-and-swap on the aligned 32-bit word that holds the byte, adding 1 << shift only while the byte is
//                   below 255 — the sum cannot carry into the neighbour, and a byte that has reached 255 costs a load and no atomic.  Expected contention is low (a fraction
//                   of a kept start per position); a pile-up serialises on its word.  The count does not depend on the order of the records.
//                   frag: with positions non-decreasing, the kept records of one position are neighbours among the kept records; the winner is the one whose NEXT kept
//                   record below the stop has another position or does not exist.  The next kept record is looked up in the wave's ballot, then in the masks of the later
//                   waves of the tile (LDS), then — for the tile's last kept record only — in the tile summaries, 64 tiles per step by wave 0: a stretch of skipped records
//                   costs one 512-byte read per 16 384 of them.  One store per position; across chunks the stream's order makes the later chunk win.
// The record bytes are read once (36 + l_read_name-dependent 4 bytes per record, through the sectors they touch); the 8-byte record summaries are written and read once,
// coalesced; hits / frag are touched only where a kept read starts.
// Byte loads, offsets and their checks are bam_record.hpp's.
#include "bam_record.hpp"

#define OBS_BLOCK 256
#define OBS_WAVES (OBS_BLOCK / WAVE)
enum { OBS_STOPPED = 0, OBS_SEEN = 1, OBS_KEPT = 2, OBS_OOR = 3, OBS_MALFORMED = 4, OBS_LAST_POS = 5, OBS_STOP_KEY = 6, OBS_NSTATE = 8 };
enum { OBS_CLS_SKIPPED = 0, OBS_CLS_KEPT = 1, OBS_CLS_MALFORMED = 2 };

__global__ void __launch_bounds__(OBS_BLOCK) k_obs_classify(const uint8_t* __restrict__ rec, uint64_t nbytes, const uint64_t* __restrict__ offs, int64_t nrec, int32_t refId,
                                                            int32_t pairedEnd, uint32_t epoch, uint2* __restrict__ summary, int2* __restrict__ tiles,
                                                            unsigned long long* __restrict__ state) {
    __shared__ int32_t sStop[OBS_WAVES], sFirst[OBS_WAVES];
    const int tid = threadIdx.x;
    if (bam_stopped_before(state[OBS_STOP_KEY], epoch)) return;          // uniform over the grid: a word of this epoch is only written when no older one stood there
    const int64_t r = (int64_t)blockIdx.x * OBS_BLOCK + tid;
    uint32_t cls = OBS_CLS_SKIPPED; bool stop = false; int32_t pos = 0, frag = 0;
    if (r < nrec) {
        const uint64_t off = offs[r]; BamRec b;
        if (!bam_rec_load(rec, nbytes, off, b)) cls = OBS_CLS_MALFORMED;
        else if (!(b.flag & (0x4u | 0x200u | 0x400u | 0x10u | 0x900u)) && b.n_cigar_op != 0u) {
            const uint32_t c0 = bam_ld32(rec, bam_cigar_at(off, b.l_read_name));            // inside the record: 32 + l_read_name + 4 n_cigar <= block_size
            if ((c0 & 15u) == 0u && (c0 >> 4) >= 35u && !(pairedEnd && !(b.flag & 0x2u))) {
                if (b.refID != refId) stop = true;
                else if (b.refID != -1) {
                    cls = OBS_CLS_KEPT; pos = b.pos;
                    frag = b.tlen < 0 ? 0 : (b.tlen > 32767 ? 32767 : b.tlen);
                }
            }
        }
        summary[r] = make_uint2((uint32_t)pos, (uint32_t)frag | (cls << 16));
    }
    const int s = bam_block_first(stop, sStop), f = bam_block_first(cls == OBS_CLS_KEPT, sFirst);
    if (tid == (f < 0 ? 0 : f)) tiles[blockIdx.x] = make_int2(f, f < 0 ? 0 : pos);          // the tile's first kept record writes its own position
    if (tid == 0 && s >= 0) atomicMax(&state[OBS_STOP_KEY], bam_stop_key(epoch, (int64_t)blockIdx.x * OBS_BLOCK + s));
}

__global__ void __launch_bounds__(OBS_BLOCK) k_obs_apply(const uint2* __restrict__ summary, const int2* __restrict__ tiles, int64_t nrec, int64_t ntiles, uint32_t epoch,
                                                         int32_t mode, int64_t len, uint8_t* __restrict__ hits, int16_t* __restrict__ fragOut,
                                                         unsigned long long* __restrict__ state) {
    __shared__ unsigned long long sMask[OBS_WAVES];
    __shared__ int32_t sPos[OBS_BLOCK];
    __shared__ uint32_t sCnt[3];
    __shared__ int32_t sNext[2];                                         // the first kept record behind this tile: {found, pos}
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // records [0, limit) act; seenAdd of them are seen (the stopping record is seen and does nothing)
    const unsigned long long key = state[OBS_STOP_KEY];                  // (not written by this kernel)
    int64_t limit = nrec, seenAdd = nrec; bool stopHere = false;
    if (bam_stopped_before(key, epoch)) { limit = 0; seenAdd = 0; }
    else if (key != 0ull) { limit = bam_stop_index(key); seenAdd = limit + 1; stopHere = true; }
    if (blockIdx.x == 0 && tid == 0) { state[OBS_SEEN] += (unsigned long long)seenAdd; if (stopHere) state[OBS_STOPPED] = 1ull; }
    const int64_t tile0 = (int64_t)blockIdx.x * OBS_BLOCK;
    if (tile0 >= limit) return;
    if (tid < 3) sCnt[tid] = 0;
    const int64_t r = tile0 + tid;
    const bool act = r < limit;
    uint2 s = make_uint2(0u, 0u);
    if (act) s = summary[r];
    const uint32_t cls = s.y >> 16; const int32_t pos = (int32_t)s.x;
    const bool kept = act && cls == OBS_CLS_KEPT, bad = act && cls == OBS_CLS_MALFORMED, inRange = kept && pos >= 0 && (int64_t)pos < len;
    const unsigned long long mKept = __ballot(kept), mBad = __ballot(bad), mOor = __ballot(kept && !inRange);
    sPos[tid] = pos;
    if (lane == 0) sMask[wave] = mKept;
    __syncthreads();
    if (lane == 0) {
        if (mKept) atomicAdd(&sCnt[0], (uint32_t)__popcll(mKept));
        if (mOor) atomicAdd(&sCnt[1], (uint32_t)__popcll(mOor));
        if (mBad) atomicAdd(&sCnt[2], (uint32_t)__popcll(mBad));
    }
    // ---- hits
    if (inRange) {
        if (mode == CANVAS_MODE_BINARY) hits[pos] = 1;
        else {
            const uintptr_t a = (uintptr_t)(hits + pos);
            uint32_t* w = (uint32_t*)(a & ~(uintptr_t)3); const uint32_t sh = (uint32_t)(a & 3) * 8u;
            uint32_t old = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            while (((old >> sh) & 255u) != 255u) {                       // below 255: adding 1 << sh cannot carry
                const uint32_t prev = atomicCAS(w, old, old + (1u << sh));
                if (prev == old) break;
                old = prev;
            }
        }
    }
    // ---- the next kept record of every kept record
    const bool anyKept = (sMask[0] | sMask[1] | sMask[2] | sMask[3]) != 0ull;      // uniform over the workgroup
    if (anyKept) {
        if (wave == 0) {
            int found = 0, npos = 0;
            for (int64_t base = (int64_t)blockIdx.x + 1; base < ntiles && base * OBS_BLOCK < limit; base += WAVE) {
                const int64_t t = base + lane; bool has = false; int2 ts = make_int2(-1, 0);
                if (t < ntiles && t * OBS_BLOCK < limit) { ts = tiles[t]; has = ts.x >= 0 && t * OBS_BLOCK + ts.x < limit; }
                const unsigned long long m = __ballot(has);
                if (m) { found = 1; npos = __shfl(ts.y, __ffsll((long long)m) - 1, 64); break; }
            }
            if (lane == 0) { sNext[0] = found; sNext[1] = npos; }
        }
        __syncthreads();
        if (kept) {
            bool haveNext = false; int32_t nextPos = 0;
            const unsigned long long above = mKept & ~((2ull << lane) - 1ull);      // (lane 63: 2 << 63 wraps to 0, the mask is empty)
            if (above) { haveNext = true; nextPos = sPos[wave * WAVE + __ffsll((long long)above) - 1]; }
            else {
                for (int w = wave + 1; w < OBS_WAVES && !haveNext; w++) if (sMask[w]) { haveNext = true; nextPos = sPos[w * WAVE + __ffsll((long long)sMask[w]) - 1]; }
                if (!haveNext && sNext[0]) { haveNext = true; nextPos = sNext[1]; }
            }
            if (mode == CANVAS_MODE_GC_CONTENT_WEIGHTED && inRange && (!haveNext || nextPos != pos)) fragOut[pos] = (int16_t)(s.y & 0xFFFFu);
            if (!haveNext) state[OBS_LAST_POS] = (unsigned long long)(long long)pos;      // one lane of the grid
        }
    }
    __syncthreads();
    if (tid < 3 && sCnt[tid]) atomicAdd(&state[OBS_KEPT + tid], (unsigned long long)sCnt[tid]);
}

static std::atomic<uint32_t> g_obs_epoch{0};

extern "C" int32_t canvas_hits_from_bam(canvas_ctx* ctx, const uint8_t* d_records, uint64_t nbytes, const uint64_t* d_record_offsets, int64_t nrecords, int32_t ref_id,
                                        int32_t paired_end, int32_t mode, int64_t len, uint8_t* d_hits, int16_t* d_frag, int64_t* d_state, int64_t* h_info) {
    if (!ctx) return CANVAS_ERR_INVALID;
    if (nrecords < 0 || (nrecords > 0 && (!d_records || !d_record_offsets)) || !d_hits || !d_state) CANVAS_FAIL(ctx, CANVAS_ERR_INVALID, "canvas_hits_from_bam: bad arguments");
    if (mode != CANVAS_MODE_BINARY && mode != CANVAS_MODE_TRUNCATED_DYNAMIC_RANGE && mode != CANVAS_MODE_GC_CONTENT_WEIGHTED)
        CANVAS_FAIL(ctx, CANVAS_ERR_INVALID, "canvas_hits_from_bam: mode must be 0, 3 or 5");
    if (mode == CANVAS_MODE_GC_CONTENT_WEIGHTED && !d_frag) CANVAS_FAIL(ctx, CANVAS_ERR_INVALID, "canvas_hits_from_bam: GCContentWeighted needs d_frag");
    if (len < 0 || len >= ((int64_t)1 << 31)) CANVAS_FAIL(ctx, CANVAS_ERR_INVALID, "canvas_hits_from_bam: len must be in [0, 2^31)");
    if (nrecords >= ((int64_t)1 << 31) - OBS_BLOCK) CANVAS_FAIL(ctx, CANVAS_ERR_INVALID, "canvas_hits_from_bam: too many records in one chunk");
    CANVAS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    unsigned long long* dState = (unsigned long long*)d_state;
    if (nrecords > 0) {
        const int64_t ntiles = (nrecords + OBS_BLOCK - 1) / OBS_BLOCK;
        uint2* summary; int2* tiles;
        int32_t rc = cvx_ws_carve(ctx, 256, [&](WsCarver& cv) { cv.take(summary, (size_t)nrecords); cv.take(tiles, (size_t)ntiles); }); if (rc) return rc;
        uint32_t epoch = ++g_obs_epoch; if (epoch == 0) epoch = ++g_obs_epoch;
        ProfScope ps(ctx, "hits_from_bam", true);
        hipLaunchKernelGGL(k_obs_classify, dim3((unsigned)ntiles), dim3(OBS_BLOCK), 0, ctx->stream, d_records, nbytes, d_record_offsets, nrecords, ref_id, paired_end, epoch,
                           summary, tiles, dState);
        hipLaunchKernelGGL(k_obs_apply, dim3((unsigned)ntiles), dim3(OBS_BLOCK), 0, ctx->stream, (const uint2*)summary, (const int2*)tiles, nrecords, ntiles, epoch, mode, len,
                           d_hits, d_frag, dState);
    }
    CANVAS_HIP_TRY(ctx, hipGetLastError());
    if (!h_info) return CANVAS_OK;                        // asynchronous: arrays and state are complete once the stream has been waited for
    return bam_mail_fetch(ctx, dState, OBS_NSTATE, h_info, "canvas_hits_from_bam");      // the state, through the pinned mailbox
}
