// Tools/FlagUniqueKmers (KmerChecker.cs): which positions of a reference start a 35-mer that occurs once in the whole input, both strands counted.
//
// The reference keeps a Dictionary<string, long> of at most 400 M entries and re-reads the genome once per dictionary fill.  Only the COUNT of a key matters for the
// answer (1 or more than 1; KmerChecker.cs:156-199 — the first-occurrence position it stores is bookkeeping for going back to flag it), so here:
//   k_kmer_hist    one sweep that counts the keyed positions of each of 1 024 key classes (LDS histogram per workgroup, flushed once);
//   the host groups the classes into passes so that a pass's keyed positions — an upper bound of its distinct keys — fit the table at load <= 1/2;
//   k_kmer_insert  sweep A of a pass: every key of the pass's classes is put into an open-addressing table in HBM, one 64-bit word per slot = key remainder << 2 | count state
//                  (1: seen once, 3: seen more than once); claimed with a 64-bit compare-and-swap, raised with a 64-bit atomic or;
//   k_kmer_lookup  sweep B: every key is looked up again, the wave's ballot of (state == 1) is one word of the mask (BitArray layout, canvas_hip.h).
// The result does not depend on the order in which threads arrive: a slot's key never changes once claimed and its state only rises.  No kernel waits for another
// workgroup; a table cannot fill (each class has a sub-table of its own, 2 x its keyed positions + 64 slots), so every probe sequence ends at an empty slot or at its key.
//
// Work split: one lane per position, one wave per 64 positions of one contig (a word of its mask).  The wave reads its 64 + 34 bases once; the two bits of every base and
// the "not ACGT" bit are ballotted into three 64 + 34-bit planes, and a lane's 35-mer is a 35-bit window of each plane.  With A=0 C=1 G=2 T=3 the reverse complement's
// planes are the bit-reversed complements of the forward ones, so both strands cost a handful of 64-bit operations per lane.
// The key: KmerChecker.GetKeyForKmer (:30-105) takes the ordinally smaller of the two packed strings.  Any rule that picks the same representative of {35-mer, reverse
// complement} whichever of the two is met gives the same equivalence classes, and the flags depend on nothing else; this file compares the strands as the 70-bit numbers
// (high plane, low plane), which needs no interleaving of the planes.  35 is odd: a 35-mer never equals its own reverse complement.
// 70 bits do not fit a 64-bit atomic: the canonical pair goes through a bijection of the 70-bit numbers (four Feistel rounds over the 35-bit halves: canonical keys of real
// sequence are heavily skewed towards A-rich prefixes, mixed ones are not), its top 10 bits are the key class — the sub-table — and the other 60 are stored in the slot.
// Many contigs: the sweeps run over the words of all contigs at once (a table of word offsets, searched once per wave and then walked); rule "p + 35 >= L" and the
// absence of bases past a contig's end keep every 35-mer inside its contig.
//
// Algorithmic bytes: per sweep 1 B/position of bases (+ 34/64 B re-read at the seams of the words, out of cache), sweep B 1/8 B/position of mask; per keyed position one
// 8-byte slot access per probe in each of the two sweeps (a compare-and-swap or an atomic or in A unless the plain look already shows state 3, a plain load in B), to a
// random address: the table is what the time goes to, not the streams.  Measured figures: DESIGN.md (FlagUniqueKmers).
#include "common.hpp"
#include <algorithm>

#define KMER_K 35
#define KMER_BLOCK 256
#define KMER_CLASS_BITS 10
#define KMER_CLASSES (1 << KMER_CLASS_BITS)
#define KMER_M35 0x7FFFFFFFFull
enum { KMER_ST_KEYED = 0, KMER_ST_UNIQUE = 1, KMER_ST_PROBE = 2, KMER_ST_N = 4 };

struct KmerContigs {                     // device tables, one entry per contig (wordOff has one more)
    const int64_t* wordOff;              // first mask word of the contig in the concatenation of all contigs' words
    const int64_t* len;
    const uint8_t* const* bases;
    uint64_t* const* mask;
    int32_t nchr; int64_t words;
};
struct KmerClassSlot { unsigned long long base, n; };       // sub-table of a class inside the pass's table; n == 0: the class is not part of this pass

__device__ __forceinline__ uint64_t kmer_mix64(uint64_t x) {
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
    return x;
}
// bijection of the 70-bit numbers (a, b), a and b 35 bits each: Feistel rounds (invertible whatever the round function is)
__device__ __forceinline__ void kmer_feistel(uint64_t& a, uint64_t& b) {
    a ^= kmer_mix64(b + 0x9e3779b97f4a7c15ull) & KMER_M35;
    b ^= kmer_mix64(a + 0xbf58476d1ce4e5b9ull) & KMER_M35;
    a ^= kmer_mix64(b + 0x94d049bb133111ebull) & KMER_M35;
    b ^= kmer_mix64(a + 0x2545f4914f6cdd1dull) & KMER_M35;
}

// The 64 positions of mask word `w` of contig c (first position p0): is this lane's position keyed, and if so its class and the 60 stored bits.
// Every lane of the wave must call this (ballots).
__device__ __forceinline__ bool kmer_key_of_lane(gptr<const uint8_t> bases, int64_t L, int64_t p0, int lane, uint32_t& cls, uint64_t& rest) {
    const int64_t p = p0 + lane, q = p0 + 64 + lane;
    const uint32_t b = p < L ? (uint32_t)bases[p] : 0u;
    const uint32_t e = (lane < KMER_K - 1 && q < L) ? (uint32_t)bases[q] : 0u;
    // upper-casing (KmerChecker.cs:124) and the switch of GetKeyForKmer in one: only 'A' 'C' 'G' 'T' and their lower-case forms are bases
    const uint32_t bl = b | 0x20u, el = e | 0x20u;
    const bool bOk = bl == 'a' || bl == 'c' || bl == 'g' || bl == 't', eOk = el == 'a' || el == 'c' || el == 'g' || el == 't';
    const uint32_t bc = ((b >> 1) ^ (b >> 2)) & 3u, ec = ((e >> 1) ^ (e >> 2)) & 3u;        // A=0 C=1 G=2 T=3, either case
    const uint64_t m0 = __ballot(bc & 1u), m1 = __ballot(bc >> 1), mb = __ballot(!bOk);
    const uint64_t x0 = __ballot(ec & 1u), x1 = __ballot(ec >> 1), xb = __ballot(!eOk);      // lanes 34..63 carry "bad": never inside a window that starts in this word
    const int s = lane;
    uint64_t f0, f1, bad;
    if (s == 0) { f0 = m0; f1 = m1; bad = mb; }
    else { f0 = (m0 >> s) | (x0 << (64 - s)); f1 = (m1 >> s) | (x1 << (64 - s)); bad = (mb >> s) | (xb << (64 - s)); }
    f0 &= KMER_M35; f1 &= KMER_M35; bad &= KMER_M35;
    if (p + KMER_K >= L || bad) return false;                      // KmerChecker.cs:136 (>=: the last 35 positions) and :147-154
    const uint64_t r0 = __brevll(~f0 & KMER_M35) >> 29, r1 = __brevll(~f1 & KMER_M35) >> 29;      // reverse complement: 3 - code, order reversed
    uint64_t a, c;
    if (f1 < r1 || (f1 == r1 && f0 < r0)) { a = f1; c = f0; } else { a = r1; c = r0; }
    kmer_feistel(a, c);
    cls = (uint32_t)(a >> (KMER_K - KMER_CLASS_BITS));
    rest = ((a & ((1ull << (KMER_K - KMER_CLASS_BITS)) - 1ull)) << KMER_K) | c;               // 25 + 35 = 60 bits
    return true;
}

// the words [w0, w1) of one wave: contiguous, so the contig index only ever moves forward
struct KmerWalk {
    int64_t w, w1; int32_t c; int64_t cFirst, cNext;
    __device__ __forceinline__ void init(const KmerContigs& G, int64_t wavesTotal, int64_t waveId) {
        const int64_t per = (G.words + wavesTotal - 1) / wavesTotal;
        w = waveId * per; w1 = w + per < G.words ? w + per : G.words;
        c = 0; cFirst = 0; cNext = 0;
        if (w >= w1) return;
        int lo = 0, hi = G.nchr - 1;                                     // the last contig whose first word is <= w: the one that owns w (empty contigs in front share the offset)
        while (lo < hi) { const int mid = (int)(((unsigned)lo + (unsigned)hi + 1u) >> 1); if (G.wordOff[mid] <= w) lo = mid; else hi = mid - 1; }
        c = lo; cFirst = G.wordOff[c]; cNext = G.wordOff[c + 1];
    }
    __device__ __forceinline__ void seek(const KmerContigs& G) {          // w < w1 <= G.words: a contig with wordOff[c + 1] > w exists
        while (w >= cNext) { c++; cFirst = cNext; cNext = G.wordOff[c + 1]; }
    }
};

__global__ void __launch_bounds__(KMER_BLOCK) k_kmer_hist(KmerContigs G, unsigned long long* __restrict__ hist) {
    __shared__ uint32_t sHist[KMER_CLASSES];
    for (int i = threadIdx.x; i < KMER_CLASSES; i += KMER_BLOCK) sHist[i] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    KmerWalk W; W.init(G, (int64_t)gridDim.x * (KMER_BLOCK / 64), (int64_t)blockIdx.x * (KMER_BLOCK / 64) + (threadIdx.x >> 6));
    // (32-bit LDS counters: the host launches enough workgroups that one's share stays below 2^32 positions, see kmer_grid)
    for (; W.w < W.w1; W.w++) {
        W.seek(G);
        uint32_t cls = 0; uint64_t rest = 0;
        if (kmer_key_of_lane(as_global(G.bases[W.c]), G.len[W.c], (W.w - W.cFirst) * 64, lane, cls, rest)) atomicAdd(&sHist[cls], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < KMER_CLASSES; i += KMER_BLOCK) if (sHist[i]) atomicAdd(&hist[i], (unsigned long long)sHist[i]);
}

__device__ __forceinline__ uint64_t kmer_home(uint64_t rest, unsigned long long n) { return __umul64hi(kmer_mix64(rest ^ 0xd6e8feb86659fd93ull), n); }      // [0, n)

__global__ void __launch_bounds__(KMER_BLOCK) k_kmer_insert(KmerContigs G, const KmerClassSlot* __restrict__ classes, unsigned long long* __restrict__ table,
                                                            unsigned long long* __restrict__ stats) {
    __shared__ KmerClassSlot sCls[KMER_CLASSES];
    for (int i = threadIdx.x; i < KMER_CLASSES; i += KMER_BLOCK) sCls[i] = classes[i];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    KmerWalk W; W.init(G, (int64_t)gridDim.x * (KMER_BLOCK / 64), (int64_t)blockIdx.x * (KMER_BLOCK / 64) + (threadIdx.x >> 6));
    unsigned long long longest = 0;
    for (; W.w < W.w1; W.w++) {
        W.seek(G);
        uint32_t cls = 0; uint64_t rest = 0;
        if (!kmer_key_of_lane(as_global(G.bases[W.c]), G.len[W.c], (W.w - W.cFirst) * 64, lane, cls, rest)) continue;
        const KmerClassSlot S = sCls[cls];
        if (S.n == 0) continue;                                     // another pass's class
        unsigned long long* sub = table + S.base;
        uint64_t at = kmer_home(rest, S.n);
        const unsigned long long once = (rest << 2) | 1ull;
        unsigned long long probes = 1;
        // at most n probes: the sub-table holds fewer keys than slots, so an empty slot or the key comes first (the bound only keeps a broken table from spinning)
        for (; probes <= S.n; probes++) {
            // the plain look may be stale (another compute die's copy of the line): a stale 0 fails the compare-and-swap, which returns the slot's true word; a stale
            // "once" repeats an or that is already in; "more than once" and another key never revert.  So it can cost an atomic, never an answer.
            unsigned long long cur = __hip_atomic_load(&sub[at], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cur == 0) { cur = atomicCAS(&sub[at], 0ull, once); if (cur == 0) break; }
            if ((cur >> 2) == rest) { if ((cur & 3ull) == 1ull) atomicOr(&sub[at], 2ull); break; }
            if (++at == S.n) at = 0;
        }
        if (probes > longest) longest = probes;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const unsigned long long o = __shfl_xor(longest, d, 64); if (o > longest) longest = o; }
    if (lane == 0 && longest) atomicMax(&stats[KMER_ST_PROBE], longest);
}

__global__ void __launch_bounds__(KMER_BLOCK) k_kmer_lookup(KmerContigs G, const KmerClassSlot* __restrict__ classes, const unsigned long long* __restrict__ table,
                                                            int32_t firstPass, unsigned long long* __restrict__ stats) {
    __shared__ KmerClassSlot sCls[KMER_CLASSES];
    for (int i = threadIdx.x; i < KMER_CLASSES; i += KMER_BLOCK) sCls[i] = classes[i];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    KmerWalk W; W.init(G, (int64_t)gridDim.x * (KMER_BLOCK / 64), (int64_t)blockIdx.x * (KMER_BLOCK / 64) + (threadIdx.x >> 6));
    unsigned long long nUnique = 0;
    for (; W.w < W.w1; W.w++) {
        W.seek(G);
        uint32_t cls = 0; uint64_t rest = 0;
        bool unique = false;
        if (kmer_key_of_lane(as_global(G.bases[W.c]), G.len[W.c], (W.w - W.cFirst) * 64, lane, cls, rest)) {
            const KmerClassSlot S = sCls[cls];
            if (S.n) {
                const unsigned long long* sub = table + S.base;
                uint64_t at = kmer_home(rest, S.n);
                for (unsigned long long probes = 1; probes <= S.n; probes++) {
                    const unsigned long long cur = sub[at];
                    if (cur == 0) break;                            // (not reached: sweep A put every key of the pass in)
                    if ((cur >> 2) == rest) { unique = (cur & 3ull) == 1ull; break; }
                    if (++at == S.n) at = 0;
                }
            }
        }
        const unsigned long long bits = __ballot(unique);
        nUnique += (unsigned long long)__popcll(bits);
        if (lane == 0) {                                            // this wave is the only writer of the word in this launch; the passes follow one another on the stream
            gptr<uint64_t> mw = as_global(G.mask[W.c]) + (W.w - W.cFirst);
            if (firstPass) *mw = bits; else if (bits) *mw |= bits;
        }
    }
    if (lane == 0 && nUnique) atomicAdd(&stats[KMER_ST_UNIQUE], nUnique);      // (nUnique is wave-uniform: counted from the ballot)
}

// inverse of k_mask_from_fasta: 16 positions per thread
__global__ void __launch_bounds__(256) k_fasta_case_from_mask(uint8_t* __restrict__ bases, int64_t len, const uint64_t* __restrict__ mask) {
    const int64_t p = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 16;
    if (p >= len) return;
    const uint32_t m16 = (uint32_t)((mask[p >> 6] >> (p & 63)) & 0xFFFFull);
    if (p + 16 <= len) {
        uint4 v = *reinterpret_cast<uint4*>(bases + p);
        uint32_t ws[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            uint32_t x = ws[k], out = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                uint32_t b = (x >> (8 * j)) & 0xFFu;
                const uint32_t l = b | 0x20u;
                if (l >= 'a' && l <= 'z' && b < 0x80u) b = ((m16 >> (4 * k + j)) & 1u) ? (b & ~0x20u) : l;
                out |= b << (8 * j);
            }
            ws[k] = out;
        }
        *reinterpret_cast<uint4*>(bases + p) = make_uint4(ws[0], ws[1], ws[2], ws[3]);
    } else {
        for (int i = 0; i < 16 && p + i < len; i++) {
            uint32_t b = bases[p + i]; const uint32_t l = b | 0x20u;
            if (l >= 'a' && l <= 'z' && b < 0x80u) bases[p + i] = (uint8_t)(((m16 >> i) & 1u) ? (b & ~0x20u) : l);
        }
    }
}

static inline unsigned long long kmer_slots_for(unsigned long long keyed) { return keyed ? 2ull * keyed + 64ull : 0ull; }
// workgroups of a sweep: 16 per compute unit, fewer for a short input, more when a workgroup's share would otherwise reach 2^25 words (2^31 positions: k_kmer_hist counts
// a workgroup's positions in 32-bit LDS words)
static inline unsigned kmer_grid(int64_t words, int cus) {
    const int64_t perBlock = KMER_BLOCK / 64, wantBlocks = (words + perBlock - 1) / perBlock;
    return (unsigned)std::min<int64_t>(wantBlocks, std::max<int64_t>((int64_t)cus * 16, (words >> 25) + 1));
}

extern "C" int32_t canvas_flag_unique_kmers(canvas_ctx* ctx, int32_t nchr, const uint8_t* const* d_bases, const int64_t* h_len, uint64_t* const* d_mask, int64_t max_table_bytes,
                                            int64_t* h_stats) {
    if (!ctx) return CANVAS_ERR_INVALID;
    if (nchr < 0 || max_table_bytes < 0 || (nchr > 0 && (!d_bases || !h_len || !d_mask))) CANVAS_FAIL(ctx, CANVAS_ERR_INVALID, "canvas_flag_unique_kmers: bad arguments");
    int64_t words = 0, positions = 0;
    std::vector<int64_t> wordOff((size_t)nchr + 1, 0);
    for (int c = 0; c < nchr; c++) {
        if (h_len[c] < 0 || h_len[c] > 0x7FFFFFFFll) CANVAS_FAIL(ctx, CANVAS_ERR_INVALID, "canvas_flag_unique_kmers: a contig's length must lie in [0, 2^31)");
        if (h_len[c] > 0 && (!d_bases[c] || !d_mask[c])) CANVAS_FAIL(ctx, CANVAS_ERR_INVALID, "canvas_flag_unique_kmers: a contig without bases or mask");
        words += (h_len[c] + 63) / 64; positions += h_len[c]; wordOff[(size_t)c + 1] = words;
    }
    if (h_stats) { for (int i = 0; i < 8; i++) h_stats[i] = 0; h_stats[0] = positions; }
    if (words == 0) return CANVAS_OK;
    CANVAS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    { int32_t rcf = canvas_upload_fence(ctx); if (rcf) return rcf; }

    // ---- device tables: contigs, class histogram, counters, one pass's class table
    int64_t *dWordOff, *dLen; const uint8_t** dBases; uint64_t** dMask; unsigned long long *dHist, *dStats; KmerClassSlot* dClasses;
    int32_t rc = cvx_ws_carve(ctx, 256, [&](WsCarver& cv) {
        cv.take(dWordOff, (size_t)nchr + 1); cv.take(dLen, (size_t)nchr); cv.take(dBases, (size_t)nchr); cv.take(dMask, (size_t)nchr);
        cv.take(dHist, KMER_CLASSES); cv.take(dStats, KMER_ST_N); cv.take(dClasses, KMER_CLASSES);
    });
    if (rc) return rc;
    CANVAS_HIP_TRY(ctx, hipMemcpyAsync(dWordOff, wordOff.data(), ((size_t)nchr + 1) * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    CANVAS_HIP_TRY(ctx, hipMemcpyAsync(dLen, h_len, (size_t)nchr * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    CANVAS_HIP_TRY(ctx, hipMemcpyAsync(dBases, d_bases, (size_t)nchr * sizeof(void*), hipMemcpyHostToDevice, ctx->stream));
    CANVAS_HIP_TRY(ctx, hipMemcpyAsync(dMask, d_mask, (size_t)nchr * sizeof(void*), hipMemcpyHostToDevice, ctx->stream));
    CANVAS_HIP_TRY(ctx, hipMemsetAsync(dHist, 0, KMER_CLASSES * sizeof(unsigned long long), ctx->stream));
    CANVAS_HIP_TRY(ctx, hipMemsetAsync(dStats, 0, KMER_ST_N * sizeof(unsigned long long), ctx->stream));
    CANVAS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));      // the sources of the table copies are the caller's and this frame's pageable arrays

    KmerContigs G; G.wordOff = dWordOff; G.len = dLen; G.bases = dBases; G.mask = dMask; G.nchr = nchr; G.words = words;
    // persistent workgroups, each wave a contiguous run of words: enough of them to fill the device several times over, few enough that the class table in LDS and the
    // histogram flush are paid a few thousand times, not once per word
    int cus = 256; { hipDeviceProp_t prop; if (hipGetDeviceProperties(&prop, ctx->device) == hipSuccess && prop.multiProcessorCount > 0) cus = prop.multiProcessorCount; }
    const unsigned grid = kmer_grid(words, cus);

    std::vector<unsigned long long> hist(KMER_CLASSES);
    {
        ProfScope ps(ctx, "kmer_hist");
        hipLaunchKernelGGL(k_kmer_hist, dim3(grid), dim3(KMER_BLOCK), 0, ctx->stream, G, dHist);
    }
    CANVAS_HIP_TRY(ctx, hipGetLastError());
    CANVAS_HIP_TRY(ctx, hipMemcpyAsync(hist.data(), dHist, KMER_CLASSES * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    CANVAS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));

    // ---- the passes: classes in order, as many as the table holds
    unsigned long long keyed = 0, needOnePass = 0, largest = 0;
    for (int k = 0; k < KMER_CLASSES; k++) { keyed += hist[k]; needOnePass += kmer_slots_for(hist[k]); largest = std::max(largest, kmer_slots_for(hist[k])); }
    if (h_stats) h_stats[1] = (int64_t)keyed;
    if (keyed == 0) {                                              // nothing is keyed (short contigs, no ACGT): every bit is 0
        for (int c = 0; c < nchr; c++) if (h_len[c] > 0) CANVAS_HIP_TRY(ctx, hipMemsetAsync(d_mask[c], 0, (size_t)((h_len[c] + 63) / 64) * 8, ctx->stream));
        CANVAS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return CANVAS_OK;
    }
    unsigned long long budgetSlots;
    if (max_table_bytes > 0) budgetSlots = std::min<unsigned long long>((unsigned long long)max_table_bytes / 8ull, needOnePass);
    else {
        size_t freeB = 0, totalB = 0;
        CANVAS_HIP_TRY(ctx, hipMemGetInfo(&freeB, &totalB));
        budgetSlots = std::min<unsigned long long>((unsigned long long)(freeB / 2) / 8ull, needOnePass);      // a shared card: half of what is free at most, and no more than one pass needs
    }
    if (largest > budgetSlots) {
        char msg[256]; snprintf(msg, sizeof msg, "canvas_flag_unique_kmers: the table budget of %llu bytes does not hold the largest key class (%llu bytes)", budgetSlots * 8ull, largest * 8ull);
        CANVAS_FAIL(ctx, CANVAS_ERR_CAPACITY, msg);
    }
    std::vector<int> passEnd;                                      // class index one past each pass's last class
    unsigned long long passSlotsMax = 0;
    { unsigned long long acc = 0;
      for (int k = 0; k < KMER_CLASSES; k++) {
          const unsigned long long s = kmer_slots_for(hist[k]);
          if (acc + s > budgetSlots) { passEnd.push_back(k); passSlotsMax = std::max(passSlotsMax, acc); acc = 0; }
          acc += s;
      }
      passEnd.push_back(KMER_CLASSES); passSlotsMax = std::max(passSlotsMax, acc); }
    unsigned long long* dTable = nullptr;
    CANVAS_HIP_TRY(ctx, hipMalloc((void**)&dTable, (size_t)passSlotsMax * 8));
    int32_t result = CANVAS_OK;
    std::vector<KmerClassSlot> classes(KMER_CLASSES);
    int k0 = 0, pass = 0;
    for (size_t pi = 0; pi < passEnd.size() && result == CANVAS_OK; pi++) {
        const int k1 = passEnd[pi];
        unsigned long long acc = 0;
        for (int k = 0; k < KMER_CLASSES; k++) {
            classes[(size_t)k].base = 0; classes[(size_t)k].n = 0;
            if (k >= k0 && k < k1) { classes[(size_t)k].base = acc; classes[(size_t)k].n = kmer_slots_for(hist[k]); acc += classes[(size_t)k].n; }
        }
        k0 = k1;
        if (acc == 0 && pass > 0) continue;                        // classes without a keyed position; the first pass always runs: it writes every word of the mask
        hipError_t e = hipSuccess;
        result = canvas_h2d_small(ctx, dClasses, classes.data(), KMER_CLASSES * sizeof(KmerClassSlot));
        if (result == CANVAS_OK && acc) e = hipMemsetAsync(dTable, 0, (size_t)acc * 8, ctx->stream);
        if (result == CANVAS_OK && e == hipSuccess) {
            { ProfScope ps(ctx, "kmer_insert", true); hipLaunchKernelGGL(k_kmer_insert, dim3(grid), dim3(KMER_BLOCK), 0, ctx->stream, G, dClasses, dTable, dStats); }
            { ProfScope ps(ctx, "kmer_lookup", true); hipLaunchKernelGGL(k_kmer_lookup, dim3(grid), dim3(KMER_BLOCK), 0, ctx->stream, G, dClasses, dTable, pass == 0 ? 1 : 0, dStats); }
            e = hipGetLastError();
        }
        if (result == CANVAS_OK && e != hipSuccess) { ctx->err = std::string("canvas_flag_unique_kmers: ") + hipGetErrorString(e); result = CANVAS_ERR_HIP; }
        pass++;
    }
    unsigned long long st[KMER_ST_N] = {0, 0, 0, 0};
    if (result == CANVAS_OK) {
        hipError_t e = hipMemcpyAsync(st, dStats, sizeof st, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) { ctx->err = std::string("canvas_flag_unique_kmers: ") + hipGetErrorString(e); result = CANVAS_ERR_HIP; }
    } else (void)hipStreamSynchronize(ctx->stream);
    (void)hipFree(dTable);
    if (result != CANVAS_OK) return result;
    if (h_stats) { h_stats[2] = (int64_t)st[KMER_ST_UNIQUE]; h_stats[3] = pass; h_stats[4] = (int64_t)passSlotsMax; h_stats[5] = (int64_t)st[KMER_ST_PROBE]; h_stats[6] = (int64_t)(passSlotsMax * 8ull); }
    return CANVAS_OK;
}

extern "C" int32_t canvas_fasta_case_from_mask(canvas_ctx* ctx, uint8_t* d_bases, int64_t len, const uint64_t* d_mask) {
    if (!ctx) return CANVAS_ERR_INVALID;
    if (len < 0 || (len > 0 && (!d_bases || !d_mask))) CANVAS_FAIL(ctx, CANVAS_ERR_INVALID, "canvas_fasta_case_from_mask: bad arguments");
    if (len == 0) return CANVAS_OK;
    CANVAS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    { int32_t rcf = canvas_upload_fence(ctx); if (rcf) return rcf; }
    const int64_t groups = (len + 15) / 16;
    hipLaunchKernelGGL(k_fasta_case_from_mask, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, ctx->stream, d_bases, len, d_mask);
    CANVAS_HIP_TRY(ctx, hipGetLastError());
    return CANVAS_OK;
}
