// canvas_bam_frame: the offsets of a chunk's records, the tool's take / skip / stop / refuse decision per record and the start of the carried tail, found on the
// device from the bytes canvas_bgzf_inflate leaves (bam_frame.hpp: the chain rule, the kinds, the shape test — the part a host program runs under AddressSanitizer).
//
// The block_size chain is sequential: where record k + 1 starts stands in record k.  What can be done side by side is walking the chain INSIDE tiles of FRAME_TILE bytes
// from a guessed entry; one wave then stitches the tiles together, and a guess counts only where the chain from the tiles before arrives at exactly that offset.
//   k_frame_tiles     one wave per tile: the tile and 36 bytes of overhang go to LDS, every byte position is put to the shape test (one ballot per 64 positions), and
//                     lane 0 takes as the tile's entry the first candidate from which a walk to the tile's end meets nothing but candidates and at least
//                     one more of them (FRAME_TRIES attempts; failing that the first candidate that leaves the tile at once; none: the tile has no guess).
//                     The tile's record starts (16-bit, relative), their number and the offset the walk left the tile at are kept.  Tile 0 is walked from
//                     `first` by the chain rule alone, and a last tile of at most 3 bytes has its own start as guess: a chain that ends exactly there
//                     arrives at it.  (A last tile that holds nothing but the head of an incomplete record has no candidate and is walked twice: one tile.)
//   k_frame_link      one wave, the only dependent chain: 64 tiles per step.  Lane l holds tile cur + l; its link holds when its exit is the guess of tile cur + l + 1; a
//                     ballot gives the run of links that hold, a wave scan the number of records in front of every tile of the run.  Where the run ends the chain has
//                     jumped over tiles (a record longer than a tile) or arrives beside the guess: the tile it arrives in is staged and walked again from the true
//                     entry, by the chain rule alone, and counted in h_info[6].  On well-formed input that is one step per 64 tiles, not one per record.
//   k_frame_classify  one wave per reached tile: bam_frame_classify per record, into arrays indexed by the record's ordinal on the chain.
//   k_frame_reduce / k_frame_blocks / k_frame_final   the scan over the records in blocks of 256: the running maximum of the positions that reach the sortedness
//                     comparison (seeded with the carried one), the number of taken records in front of every record, the first stopping or malformed record, the first
//                     unsorted one.  Minima travel as per-block values and are reduced by one workgroup: no atomic on a shared word anywhere.
//   k_frame_event     one workgroup: the event is the smaller of the two indices; h_info, and d_state unless the offsets do not fit.
//   k_frame_write     the taken records in front of the event (and a taken stopping record) put their offset at their ordinal.
// The speculation decides which tiles are walked twice and nothing else: every output is a function of the chain from `first`.  CANVAS_FRAME_NO_GUESS=1 (test hook)
// gives no tile a guess, so that every tile goes through the second walk.
// Bytes: the chunk is read once in k_frame_tiles (staging, plus 36 bytes of overhang per tile), 36 bytes per record in k_frame_classify; 2 bytes per record of tile slots, 17
// per record of summaries.  Wave64 throughout; LDS per workgroup 4.7 KiB.
#include "bam_frame.hpp"

#define FRAME_TILE 4096u
#define FRAME_OVERHANG 36u
#define FRAME_SLOTS 128u                 // a tile holds at most FRAME_TILE / 36 + 1 = 114 record starts
#define FRAME_TRIES 8
#define FRAME_BLOCK 256
#define FRAME_END (1ull << 63)           // flag of a tile's exit: the chain ends at this offset
#define FRAME_NO_GUESS (~0ull)
#define FRAME_NO_INDEX 0xFFFFFFFFu
#define FRAME_NO_POS INT64_MIN
enum { FK_N = 0, FK_CHAIN_END, FK_WRONG, FK_HARD, FK_TOTAL_SUM, FK_TOTAL_MAX, FK_HARD_SUM, FK_HARD_MAX, FK_EVENT, FK_FITS, FK_INFO = 16, FK_WORDS = 32 };
enum { CANVAS_FRAME_INFO_WORDS = 8 };

struct FrameArgs {
    const uint8_t* rec; uint64_t nbytes, first, base0; uint32_t ntiles, maxRec; BamFrameRule rule; int32_t noGuess; int64_t capacity;
    unsigned long long* ctl; unsigned long long *tileGuess, *tileExit; uint32_t *tileCount, *tileRecBase, *tileReached; uint16_t* slots;
    unsigned long long* recOff; int32_t* recPos; uint8_t* recPre; uint32_t* takeIdx;
    long long *blkMax, *blkMaxEx, *blkUnsAgainst; unsigned long long *blkSum, *blkSumEx, *blkUnsSum; uint32_t *blkHard, *blkUns;
};

__device__ __forceinline__ unsigned long long frame_shfl(unsigned long long v, int src) {
    return ((unsigned long long)(uint32_t)__shfl((int)(v >> 32), src, 64) << 32) | (uint32_t)__shfl((int)(uint32_t)v, src, 64);
}
__device__ __forceinline__ unsigned long long frame_shfl_up(unsigned long long v, int d) {
    return ((unsigned long long)(uint32_t)__shfl_up((int)(v >> 32), d, 64) << 32) | (uint32_t)__shfl_up((int)(uint32_t)v, d, 64);
}

// the tile's bytes rec[base, base + FRAME_TILE + FRAME_OVERHANG), as far as the chunk has them, into LDS: returns p with p[k] = rec[base + k].  LDS index and address agree
// mod 16, so the body goes in 16-byte words.  One wave; the caller puts a barrier behind it.
struct FrameLds { uint8_t b[FRAME_TILE + FRAME_OVERHANG + 32] __attribute__((aligned(16))); };
__device__ __forceinline__ const uint8_t* frame_stage(FrameLds& S, const uint8_t* __restrict__ rec, uint64_t nbytes, uint64_t base, uint32_t lane) {
    const uint64_t left = nbytes > base ? nbytes - base : 0ull;
    const uint32_t n = (uint32_t)(left < (uint64_t)(FRAME_TILE + FRAME_OVERHANG) ? left : (uint64_t)(FRAME_TILE + FRAME_OVERHANG));
    const uint8_t* from = rec + base;
    const uint32_t skew = (uint32_t)((uintptr_t)from & 15u);
    uint8_t* p = S.b + skew;
    const uint32_t align = (16u - skew) & 15u, head = align < n ? align : n, body = (n - head) & ~15u;
    for (uint32_t k = lane; k < head; k += 64) p[k] = from[k];
    for (uint32_t k = 16 * lane; k < body; k += 16 * 64) *(uint4*)(p + head + k) = *(const uint4*)(from + head + k);
    for (uint32_t k = head + body + lane; k < n; k += 64) p[k] = from[k];
    return p;
}

// The chain inside one tile, from `entry` (base <= entry) to the first offset at or behind base + FRAME_TILE, on the staged bytes.  strict: every whole record has to pass
// the shape test as well (false: it does not — `entry` is no guess to make).  The record starts go to `slots`; `exit` carries FRAME_END where the chain ends.
__device__ __forceinline__ bool frame_walk(const uint8_t* __restrict__ p, uint64_t nbytes, uint64_t base, uint64_t entry, bool strict, uint16_t* __restrict__ slots, uint32_t& count, unsigned long long& exit) {
    uint64_t o = entry; uint32_t n = 0; const uint64_t end = base + FRAME_TILE;
    while (o < end) {
        int32_t bs;
        if (!bam_frame_whole(p, nbytes - base, o - base, bs)) { o |= FRAME_END; break; }       // (the chunk as the tile sees it: nbytes - base bytes from p)
        if (strict && (bs < 32 || !bam_frame_shape(p + (o - base), nbytes - o))) return false;
        if (n < FRAME_SLOTS) slots[n] = (uint16_t)(o - base);
        n++;
        if (bs < 32) { o |= FRAME_END; break; }                                                 // MALFORMED: the chain ends at it
        o += 4ull + (uint64_t)(uint32_t)bs;
    }
    count = n < FRAME_SLOTS ? n : FRAME_SLOTS; exit = o;
    return true;
}

__global__ void __launch_bounds__(64) k_frame_tiles(FrameArgs a) {
    __shared__ FrameLds S; __shared__ unsigned long long sCand[FRAME_TILE / 64];
    const uint32_t lane = threadIdx.x, t = blockIdx.x;
    const uint64_t base = a.base0 + (uint64_t)t * FRAME_TILE;
    if (a.noGuess) { if (lane == 0) { a.tileGuess[t] = FRAME_NO_GUESS; a.tileExit[t] = FRAME_END; a.tileCount[t] = 0; } return; }
    if (t != 0 && a.nbytes - base < 4) { if (lane == 0) { a.tileGuess[t] = base; a.tileExit[t] = base | FRAME_END; a.tileCount[t] = 0; } return; }      // (base <= nbytes: the tile that holds offset nbytes is the last)
    const uint8_t* p = frame_stage(S, a.rec, a.nbytes, base, lane);
    __syncthreads();
    if (t != 0) {
        for (uint32_t i = 0; i < FRAME_TILE / 64; i++) {
            const uint32_t k = i * 64 + lane; const uint64_t at = base + k;
            const bool ok = at < a.nbytes && a.nbytes - at >= 36 && bam_frame_shape(p + k, a.nbytes - at);
            const unsigned long long m = __ballot(ok);
            if (lane == 0) sCand[i] = m;
        }
        __syncthreads();
    }
    if (lane != 0) return;
    uint16_t* slots = a.slots + (size_t)t * FRAME_SLOTS;
    unsigned long long guess = FRAME_NO_GUESS, exit = FRAME_END; uint32_t count = 0;
    if (t == 0) { guess = a.first; frame_walk(p, a.nbytes, base, a.first, false, slots, count, exit); }
    else {
        // confirmed: the walk met a second candidate inside the tile, or the chunk's end.  A candidate whose block_size leaves the tile at once has shown nothing (two
        // quality bytes in front of a block_size word read as a block_size of megabytes); the first such one is kept for a tile that confirms none.
        int tries = 0; unsigned long long lone = FRAME_NO_GUESS;
        for (uint32_t i = 0; i < FRAME_TILE / 64 && guess == FRAME_NO_GUESS && tries < FRAME_TRIES; i++)
            for (unsigned long long m = sCand[i]; m && guess == FRAME_NO_GUESS && tries < FRAME_TRIES; m &= m - 1, tries++) {
                const uint64_t c = base + i * 64 + (uint32_t)(__ffsll((long long)m) - 1);
                if (!frame_walk(p, a.nbytes, base, c, true, slots, count, exit)) continue;
                if (count >= 2 || (exit & FRAME_END)) guess = c;
                else if (lone == FRAME_NO_GUESS) lone = c;
            }
        if (guess == FRAME_NO_GUESS && lone != FRAME_NO_GUESS && frame_walk(p, a.nbytes, base, lone, true, slots, count, exit)) guess = lone;
        if (guess == FRAME_NO_GUESS) { count = 0; exit = FRAME_END; }
    }
    a.tileGuess[t] = guess; a.tileExit[t] = exit; a.tileCount[t] = count;
}

__global__ void __launch_bounds__(64) k_frame_link(FrameArgs a) {
    __shared__ FrameLds S;
    const uint32_t lane = threadIdx.x;
    unsigned long long x = a.first, running = 0, wrong = 0, chainEnd = a.first;
    uint32_t m = 0;
    for (;;) {
        // the chain arrives in tile m at offset x
        bool walked = false; unsigned long long wExit = 0; uint32_t wCount = 0;
        if (a.tileGuess[m] != x) {
            const uint64_t base = a.base0 + (uint64_t)m * FRAME_TILE;
            __syncthreads();
            const uint8_t* p = frame_stage(S, a.rec, a.nbytes, base, lane);
            __syncthreads();
            if (lane == 0) frame_walk(p, a.nbytes, base, x, false, a.slots + (size_t)m * FRAME_SLOTS, wCount, wExit);
            wExit = frame_shfl(wExit, 0); wCount = (uint32_t)__shfl((int)wCount, 0, 64);
            walked = true; wrong++;
        }
        const uint32_t t = m + lane; const bool live = t < a.ntiles;
        unsigned long long ex = live ? a.tileExit[t] : FRAME_END, gs = live ? a.tileGuess[t] : FRAME_NO_GUESS;
        uint32_t cnt = live ? a.tileCount[t] : 0u;
        if (lane == 0 && walked) { ex = wExit; cnt = wCount; }
        const unsigned long long gNext = ((unsigned long long)(uint32_t)__shfl_down((int)(gs >> 32), 1, 64) << 32) | (uint32_t)__shfl_down((int)(uint32_t)gs, 1, 64);
        const bool ok = lane < 63 && t + 1 < a.ntiles && !(ex & FRAME_END) && (ex - a.base0) / FRAME_TILE == (uint64_t)(t + 1) && gNext == ex;
        const unsigned long long mask = __ballot(ok);
        const int run = __ffsll((long long)~mask) - 1;          // lanes 0 .. run hold reached tiles (lane 63 never links on: ~mask is not 0)
        uint32_t incl = cnt;
        for (int d = 1; d < 64; d <<= 1) { const uint32_t o = (uint32_t)__shfl_up((int)incl, d, 64); if ((int)lane >= d) incl += o; }
        if ((int)lane <= run && live) {
            a.tileRecBase[t] = (uint32_t)running + (incl - cnt); a.tileReached[t] = 1u;
            if (lane == 0 && walked) a.tileCount[t] = cnt;
        }
        running += (uint32_t)__shfl((int)incl, run, 64);
        const unsigned long long last = frame_shfl(ex, run);
        if (last & FRAME_END) { chainEnd = last & ~FRAME_END; break; }
        x = last; m = (uint32_t)((x - a.base0) / FRAME_TILE);
    }
    if (lane == 0) { a.ctl[FK_N] = running; a.ctl[FK_CHAIN_END] = chainEnd; a.ctl[FK_WRONG] = wrong; }
}

__global__ void __launch_bounds__(64) k_frame_classify(FrameArgs a) {
    const uint32_t lane = threadIdx.x, t = blockIdx.x;
    if (!a.tileReached[t]) return;
    uint32_t cnt = a.tileCount[t]; if (cnt > FRAME_SLOTS) cnt = FRAME_SLOTS;
    const uint32_t rb = a.tileRecBase[t];
    const uint64_t base = a.base0 + (uint64_t)t * FRAME_TILE;
    for (uint32_t j = lane; j < cnt; j += 64) {
        const uint64_t off = base + a.slots[(size_t)t * FRAME_SLOTS + j];
        int32_t pos; bool cmp;
        const int cls = bam_frame_classify(a.rec, a.nbytes, off, a.rule, &pos, &cmp);
        const uint32_t i = rb + j;
        if (i < a.maxRec) { a.recOff[i] = off; a.recPos[i] = pos; a.recPre[i] = (uint8_t)(cls | (cmp ? 16 : 0)); }
    }
}

// exclusive scans over the workgroup, in thread order: running maximum (FRAME_NO_POS = none) and sum; the totals as well.  Two barriers; the arrays are free again behind it.
template <int WAVES> __device__ __forceinline__ void frame_block_scan(long long mx, unsigned long long sm, long long& mxEx, unsigned long long& smEx, long long& mxAll, unsigned long long& smAll,
                                                                      long long (&sM)[WAVES], unsigned long long (&sS)[WAVES]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int d = 1; d < 64; d <<= 1) {
        const long long om = (long long)frame_shfl_up((unsigned long long)mx, d); const unsigned long long os = frame_shfl_up(sm, d);
        if (lane >= d) { mx = om > mx ? om : mx; sm += os; }
    }
    long long em = (long long)frame_shfl_up((unsigned long long)mx, 1); unsigned long long es = frame_shfl_up(sm, 1);
    if (lane == 0) { em = FRAME_NO_POS; es = 0ull; }
    if (lane == 63) { sM[wave] = mx; sS[wave] = sm; }
    __syncthreads();
    long long pm = FRAME_NO_POS, am = FRAME_NO_POS; unsigned long long ps = 0ull, as = 0ull;
    for (int w = 0; w < WAVES; w++) { if (w < wave) { pm = sM[w] > pm ? sM[w] : pm; ps += sS[w]; } am = sM[w] > am ? sM[w] : am; as += sS[w]; }
    mxEx = em > pm ? em : pm; smEx = ps + es; mxAll = am; smAll = as;
    __syncthreads();
}
// the smallest value of the workgroup, for every thread
template <int WAVES> __device__ __forceinline__ uint32_t frame_block_min(uint32_t v, uint32_t (&sV)[WAVES]) {
    for (int d = 32; d >= 1; d >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)v, d, 64); v = o < v ? o : v; }
    if ((threadIdx.x & 63) == 0) sV[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t r = FRAME_NO_INDEX;
    for (int w = 0; w < WAVES; w++) r = sV[w] < r ? sV[w] : r;
    __syncthreads();
    return r;
}
// the records on the chain (never more than the summaries hold: every record but the last is 36 bytes and more)
__device__ __forceinline__ uint32_t frame_records(const FrameArgs& a) { const unsigned long long n = a.ctl[FK_N]; return n < a.maxRec ? (uint32_t)n : a.maxRec; }
struct FrameRecView { bool live, cmp; int cls; long long mx; unsigned long long sm; };
__device__ __forceinline__ FrameRecView frame_rec_view(const FrameArgs& a, uint32_t i, uint32_t n) {
    FrameRecView v; v.live = i < n;
    const uint32_t pre = v.live ? a.recPre[i] : (uint32_t)BAM_FRAME_SKIP;
    v.cls = (int)(pre & 15u); v.cmp = (pre & 16u) != 0u;
    v.mx = v.cmp ? (long long)a.recPos[i] : FRAME_NO_POS;
    v.sm = ((unsigned long long)(v.cmp ? 1u : 0u) << 32) | (unsigned long long)(v.live && v.cls == BAM_FRAME_TAKE ? 1u : 0u);      // (a taken stopping record is added where it is the event)
    return v;
}

__global__ void __launch_bounds__(FRAME_BLOCK) k_frame_reduce(FrameArgs a) {
    __shared__ long long sM[FRAME_BLOCK / 64]; __shared__ unsigned long long sS[FRAME_BLOCK / 64]; __shared__ uint32_t sV[FRAME_BLOCK / 64];
    const uint32_t n = frame_records(a), b = blockIdx.x;
    if ((uint64_t)b * FRAME_BLOCK >= n) return;
    const uint32_t i = b * FRAME_BLOCK + threadIdx.x;
    const FrameRecView v = frame_rec_view(a, i, n);
    long long mxEx, mxAll; unsigned long long smEx, smAll;
    frame_block_scan(v.mx, v.sm, mxEx, smEx, mxAll, smAll, sM, sS);
    const bool hard = v.live && (v.cls == BAM_FRAME_TAKE_AND_STOP || v.cls == BAM_FRAME_STOP || v.cls == BAM_FRAME_MALFORMED);
    const uint32_t first = frame_block_min(hard ? i : FRAME_NO_INDEX, sV);
    if (threadIdx.x == 0) { a.blkMax[b] = mxAll; a.blkSum[b] = smAll; a.blkHard[b] = first; }
}

// one workgroup: the per-block values in front of every block, seeded with the carried position; the first stopping or malformed record
__global__ void __launch_bounds__(1024) k_frame_blocks(FrameArgs a, const long long* __restrict__ state) {
    __shared__ long long sM[16]; __shared__ unsigned long long sS[16]; __shared__ uint32_t sV[16];
    const uint32_t n = frame_records(a), nb = (n + FRAME_BLOCK - 1) / FRAME_BLOCK;
    long long runMax = state[0] > 0 ? state[1] : FRAME_NO_POS; unsigned long long runSum = 0ull; uint32_t hard = FRAME_NO_INDEX;
    for (uint32_t at = 0; at < nb; at += 1024) {
        const uint32_t b = at + threadIdx.x; const bool live = b < nb;
        long long mxEx, mxAll; unsigned long long smEx, smAll;
        frame_block_scan(live ? a.blkMax[b] : FRAME_NO_POS, live ? a.blkSum[b] : 0ull, mxEx, smEx, mxAll, smAll, sM, sS);
        if (live) { a.blkMaxEx[b] = mxEx > runMax ? mxEx : runMax; a.blkSumEx[b] = runSum + smEx; const uint32_t h = a.blkHard[b]; hard = h < hard ? h : hard; }
        runMax = mxAll > runMax ? mxAll : runMax; runSum += smAll;
    }
    hard = frame_block_min(hard, sV);
    if (threadIdx.x == 0) { a.ctl[FK_HARD] = hard; a.ctl[FK_TOTAL_SUM] = runSum; a.ctl[FK_TOTAL_MAX] = (unsigned long long)runMax; }
}

__global__ void __launch_bounds__(FRAME_BLOCK) k_frame_final(FrameArgs a) {
    __shared__ long long sM[FRAME_BLOCK / 64]; __shared__ unsigned long long sS[FRAME_BLOCK / 64]; __shared__ uint32_t sV[FRAME_BLOCK / 64];
    const uint32_t n = frame_records(a), b = blockIdx.x;
    if ((uint64_t)b * FRAME_BLOCK >= n) return;
    const uint32_t i = b * FRAME_BLOCK + threadIdx.x;
    const FrameRecView v = frame_rec_view(a, i, n);
    long long mxEx, mxAll; unsigned long long smEx, smAll;
    frame_block_scan(v.mx, v.sm, mxEx, smEx, mxAll, smAll, sM, sS);
    const long long before = a.blkMaxEx[b] > mxEx ? a.blkMaxEx[b] : mxEx;      // the running maximum in front of record i, the carried position included
    const unsigned long long sumBefore = a.blkSumEx[b] + smEx;
    if (v.live) a.takeIdx[i] = (uint32_t)sumBefore;
    const bool uns = v.cmp && before != FRAME_NO_POS && v.mx < before;
    const uint32_t first = frame_block_min(uns ? i : FRAME_NO_INDEX, sV);
    if (threadIdx.x == 0) a.blkUns[b] = first;
    if (uns && i == first) { a.blkUnsAgainst[b] = before; a.blkUnsSum[b] = sumBefore; }
    if (v.live && (unsigned long long)i == a.ctl[FK_HARD]) { a.ctl[FK_HARD_SUM] = sumBefore; a.ctl[FK_HARD_MAX] = (unsigned long long)before; }
}

// one workgroup: the first unsorted record, the event, h_info (ctl[FK_INFO ..]) and, if the offsets fit, d_state
__global__ void __launch_bounds__(1024) k_frame_event(FrameArgs a, long long* __restrict__ state) {
    __shared__ uint32_t sV[16];
    const uint32_t n = frame_records(a), nb = (n + FRAME_BLOCK - 1) / FRAME_BLOCK;
    uint32_t uns = FRAME_NO_INDEX;
    for (uint32_t b = threadIdx.x; b < nb; b += 1024) { const uint32_t u = a.blkUns[b]; uns = u < uns ? u : uns; }
    uns = frame_block_min(uns, sV);
    if (threadIdx.x != 0) return;
    const uint32_t hard = (uint32_t)a.ctl[FK_HARD];
    long long event = 0, evOff = -1, against = 0, taken, used, classified, last; unsigned long long sum; uint32_t evIndex = FRAME_NO_INDEX;
    if (uns < hard) {
        const uint32_t b = uns / FRAME_BLOCK;
        event = 3; evIndex = uns; sum = a.blkUnsSum[b]; against = last = a.blkUnsAgainst[b]; taken = (long long)(uint32_t)sum; evOff = used = (long long)a.recOff[uns]; classified = (long long)uns + 1;
    } else if (hard != FRAME_NO_INDEX) {
        const int cls = a.recPre[hard] & 15;
        evIndex = hard; sum = a.ctl[FK_HARD_SUM]; last = (long long)a.ctl[FK_HARD_MAX]; evOff = (long long)a.recOff[hard]; classified = (long long)hard + 1;
        event = cls == BAM_FRAME_MALFORMED ? 2 : 1;
        taken = (long long)(uint32_t)sum + (cls == BAM_FRAME_TAKE_AND_STOP ? 1 : 0);
        used = cls == BAM_FRAME_TAKE_AND_STOP ? evOff + 4 + (long long)bam_ld32(a.rec, (uint64_t)evOff) : evOff;      // (a whole record of block_size >= 32)
    } else {
        sum = a.ctl[FK_TOTAL_SUM]; last = (long long)a.ctl[FK_TOTAL_MAX]; taken = (long long)(uint32_t)sum; used = (long long)a.ctl[FK_CHAIN_END]; classified = (long long)n;
    }
    const bool fits = taken <= a.capacity;
    unsigned long long* info = a.ctl + FK_INFO;
    info[0] = (unsigned long long)classified; info[1] = (unsigned long long)taken; info[2] = (unsigned long long)used; info[3] = (unsigned long long)(fits ? event : 4);
    info[4] = (unsigned long long)evOff; info[5] = (unsigned long long)against; info[6] = a.ctl[FK_WRONG]; info[7] = FRAME_TILE;
    a.ctl[FK_EVENT] = evIndex; a.ctl[FK_FITS] = fits ? 1ull : 0ull;
    if (fits) {
        const long long passed = (long long)(sum >> 32);
        if (passed > 0) { state[0] += passed; state[1] = last; }
        state[2] += taken; state[3] = event;
    }
}

__global__ void __launch_bounds__(FRAME_BLOCK) k_frame_write(FrameArgs a, unsigned long long* __restrict__ out) {
    const uint32_t n = frame_records(a), i = blockIdx.x * FRAME_BLOCK + threadIdx.x;
    if (i >= n || !a.ctl[FK_FITS]) return;
    const uint32_t ev = (uint32_t)a.ctl[FK_EVENT]; const int cls = a.recPre[i] & 15;
    if ((i < ev && cls == BAM_FRAME_TAKE) || (i == ev && cls == BAM_FRAME_TAKE_AND_STOP)) out[a.takeIdx[i]] = a.recOff[i];
}

extern "C" int32_t canvas_bam_frame(canvas_ctx* ctx, const uint8_t* d_records, uint64_t nbytes, uint64_t first, const canvas_bam_frame_rule* rule, uint64_t* d_record_offsets,
                                    int64_t capacity, int64_t* d_state, int64_t* h_info) {
    if (!ctx) return CANVAS_ERR_INVALID;
    if (!rule || !d_state || !h_info) CANVAS_FAIL(ctx, CANVAS_ERR_INVALID, "canvas_bam_frame: rule, d_state and h_info are required");
    if (first > nbytes || (!d_records && nbytes > 0)) CANVAS_FAIL(ctx, CANVAS_ERR_INVALID, "canvas_bam_frame: `first` lies behind the chunk, or there is no chunk");
    if (rule->kind < 0 || rule->kind >= BAM_FRAME_KINDS) CANVAS_FAIL(ctx, CANVAS_ERR_INVALID, "canvas_bam_frame: unknown kind " + std::to_string(rule->kind));
    if (capacity < 0 || (capacity > 0 && !d_record_offsets)) CANVAS_FAIL(ctx, CANVAS_ERR_INVALID, "canvas_bam_frame: capacity must not be negative, and the offsets need a buffer");
    if (nbytes - first >= ((uint64_t)1 << 32)) CANVAS_FAIL(ctx, CANVAS_ERR_INVALID, "canvas_bam_frame: a chunk of 2^32 bytes and more has to be cut by the caller");
    if (nbytes - first < 4) {
        h_info[0] = h_info[1] = 0; h_info[2] = (int64_t)first; h_info[3] = CANVAS_BAM_FRAME_NONE; h_info[4] = -1; h_info[5] = h_info[6] = 0; h_info[7] = FRAME_TILE;
        return CANVAS_OK;
    }
    const char* hook = cvx_hook("CANVAS_FRAME_NO_GUESS");
    FrameArgs a;
    a.rec = d_records; a.nbytes = nbytes; a.first = first; a.base0 = first / FRAME_TILE * FRAME_TILE;
    a.ntiles = (uint32_t)(nbytes / FRAME_TILE - first / FRAME_TILE + 1);                        // (the tile that holds offset nbytes is one of them: a chain may end exactly there)
    a.maxRec = (uint32_t)((nbytes - first) / 36 + 2);                                           // every record of the chain but its last is whole: 36 bytes and more
    a.rule.kind = rule->kind; a.rule.ref_id = rule->ref_id; a.rule.paired_end = rule->paired_end; a.rule.sorted = rule->sorted;
    a.noGuess = hook && atoi(hook) == 1 ? 1 : 0; a.capacity = capacity;
    const uint32_t nblk = (a.maxRec + FRAME_BLOCK - 1) / FRAME_BLOCK;
    CANVAS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    int32_t rc = cvx_ws_carve(ctx, 256, [&](WsCarver& cv) {
        cv.take(a.ctl, FK_WORDS); cv.take(a.tileReached, a.ntiles); cv.take(a.tileGuess, a.ntiles); cv.take(a.tileExit, a.ntiles); cv.take(a.tileCount, a.ntiles); cv.take(a.tileRecBase, a.ntiles);
        cv.take(a.slots, (size_t)a.ntiles * FRAME_SLOTS);
        cv.take(a.recOff, a.maxRec); cv.take(a.recPos, a.maxRec); cv.take(a.recPre, a.maxRec); cv.take(a.takeIdx, a.maxRec);
        cv.take(a.blkMax, nblk); cv.take(a.blkMaxEx, nblk); cv.take(a.blkUnsAgainst, nblk); cv.take(a.blkSum, nblk); cv.take(a.blkSumEx, nblk); cv.take(a.blkUnsSum, nblk);
        cv.take(a.blkHard, nblk); cv.take(a.blkUns, nblk);
    });
    if (rc) return rc;
    {
        ProfScope ps(ctx, "bam_frame", true);
        // ctl and the reached flags lie next to each other at the front of the layout: one fill
        CANVAS_HIP_TRY(ctx, hipMemsetAsync(a.ctl, 0, (size_t)((uint8_t*)(a.tileReached + a.ntiles) - (uint8_t*)a.ctl), ctx->stream));
        hipLaunchKernelGGL(k_frame_tiles, dim3(a.ntiles), dim3(64), 0, ctx->stream, a);
        hipLaunchKernelGGL(k_frame_link, dim3(1), dim3(64), 0, ctx->stream, a);
        hipLaunchKernelGGL(k_frame_classify, dim3(a.ntiles), dim3(64), 0, ctx->stream, a);
        hipLaunchKernelGGL(k_frame_reduce, dim3(nblk), dim3(FRAME_BLOCK), 0, ctx->stream, a);
        hipLaunchKernelGGL(k_frame_blocks, dim3(1), dim3(1024), 0, ctx->stream, a, (const long long*)d_state);
        hipLaunchKernelGGL(k_frame_final, dim3(nblk), dim3(FRAME_BLOCK), 0, ctx->stream, a);
        hipLaunchKernelGGL(k_frame_event, dim3(1), dim3(1024), 0, ctx->stream, a, (long long*)d_state);
        hipLaunchKernelGGL(k_frame_write, dim3(nblk), dim3(FRAME_BLOCK), 0, ctx->stream, a, (unsigned long long*)d_record_offsets);
    }
    CANVAS_HIP_TRY(ctx, hipGetLastError());
    return bam_mail_fetch(ctx, a.ctl + FK_INFO, CANVAS_FRAME_INFO_WORDS, h_info, "canvas_bam_frame");
}
