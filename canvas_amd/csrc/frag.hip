// CanvasBin -m Fragment: FragmentBinner.BinTask (CanvasBin/FragmentBinner.cs:186-369: binFragments, BinOneAlignment, FindBestBin) over RAW BAM record bytes, in the
// chunk format of canvas_snv_count (snv.hip) and canvas_hits_from_bam (obs.hip).
//
// The reference walks the stream with a dictionary (read name -> bin it was counted in), a set (names seen once at pos == mate pos) and a forward pointer into the bins.
// Reads of different names meet in two places only: the integer sums (bin counts, usable fragments), which do not depend on order, and the pointer.  With positions
// non-decreasing (the reference throws otherwise) every bin the pointer has passed has Stop <= an earlier, not larger, start: the pointer a fragment ends on is the
// first bin whose prefix maximum of Stop exceeds the fragment's start, whatever the order of the BED file.  What is left is, per NAME, a two-variable state machine
// (binned into bin b or not, in the same-position set or not) driven by the records of that name in file order.
//   k_frag_prefmax   one workgroup: running maximum of d_bin_stop into the workspace.
//   k_frag_classify  one lane per record: the fixed fields with their shape checks (bam_record.hpp: bam_rec_load), the smallest index of a record of another reference
//                    (bam_block_first, then ONE atomicMax per workgroup on a word of the call's control block, with bam_record.hpp's stop key), the skip filters, a 64-bit hash of the name
//                    bytes.  32 bytes per record go to the workspace {pos, next_pos, tlen, class, hash, offset of the record}.
//   k_frag_insert    one lane per item — the carried entries first ("records in front of index 0"), then the records below the stop: paired / malformed counters
//                    (ballot, one atomic per wave), sortedness against the nearest well-formed record on the left (the summaries; the chunk before through state[5]),
//                    the last position, and for every record that survived the skip filters a push onto the chain of its hash slot (atomicExch on the slot head,
//                    a `next` link per item).  The ORDER of a chain depends on arrival; nothing below does: every walk takes the whole chain and orders by index.
//   k_frag_leader    one lane per chained item: the smallest index in its chain that carries the same name (equal hash first, then the BYTES: the hash finds, it never
//                    decides).  That item leads the group.
//   k_frag_resolve   one lane per group: its members in index order (repeated selection of the next larger index over the chain: a group is almost always two
//                    records; one of thousands is quadratic in its chain — slow, and correct), the state machine, the pointer by binary search in the prefix maximum,
//                    the FindBestBin walk.  Every record gets at most one event (+1 or -1 on one bin), stored in the workspace; a group that ends binned or in the
//                    same-position set takes a slot of the new carry (header and name bytes, in the workspace).
//   k_frag_commit    if the new carry fits: the events go to d_count (integer atomics), the new carry to d_carry, the counters to d_state.  Otherwise nothing is
//                    written and the call reports the bytes needed.
// No float atomics; counts, state words and the SET of carried entries do not depend on arrival order (the order of the entries inside d_carry does, and nothing reads it:
// a name has one entry, and every entry lies in front of every record).
// Bytes per record: 36 fixed + the name (read twice: hash, and the comparison with its mate) from the chunk; 32 written and about three times read as summary; 4 of link,
// 4 of leader, 4 of event, 8 of slot head.
// Byte loads, offsets and their checks are bam_record.hpp's.
#include "bam_record.hpp"

#define FRAG_BLOCK 256
#define FRAG_WAVES (FRAG_BLOCK / WAVE)
enum { FRAG_STOPPED = 0, FRAG_SEEN = 1, FRAG_PAIRED = 2, FRAG_USABLE = 3, FRAG_MALFORMED = 4, FRAG_LAST_POS = 5, FRAG_UNSORTED = 6, FRAG_ENTRIES = 7, FRAG_CARRY_BYTES = 8,
       FRAG_SPLIT_GROUPS = 9, FRAG_LONGEST = 10, FRAG_HAVE_LAST = 11, FRAG_NSTATE = 16 };
// class word of a record summary
enum { FC_MALFORMED = 1u, FC_LIVE = 2u, FC_BAD = 4u, FC_REF_MISMATCH = 8u, FC_PAIRED = 16u, FC_OTHER_REF = 32u, FC_NAME_SHIFT = 8 };
// the call's control block (workspace, zeroed before the kernels)
enum { FK_STOP_KEY = 0, FK_UNSORTED_KEY = 1, FK_LAST_KEY = 2, FK_PAIRED = 3, FK_MALFORMED = 4, FK_USABLE = 5, FK_ENTRIES = 6, FK_NAME_BYTES = 7, FK_SPLIT = 8, FK_LONGEST = 9, FK_WORDS = 16 };
#define FRAG_HDR_BYTES 24
struct FragRec { int32_t pos, nextPos, tlen; uint32_t cls; unsigned long long hash, off; };      // 32 bytes
struct FragHdr { unsigned long long hash; uint32_t nameOff; int32_t bin; uint32_t nameLen, samePos; };      // 24 bytes: d_carry = n headers, then the name bytes
struct FragArgs {
    const uint8_t* rec; uint64_t nbytes; const uint64_t* offs; int64_t nrec; int32_t refId; const int32_t* binStart; const int32_t* binStop; int64_t nbins; int32_t quality;
    const uint8_t* carry; int64_t ncarry; uint64_t carryUsed; const long long* state; unsigned long long hashMask;
    // workspace
    unsigned long long* ctl; int32_t* prefMax; FragRec* summary; int32_t* head; uint32_t slotMask; int32_t* next; int32_t* leader; uint32_t* ev; FragHdr* newHdr; uint8_t* newNames; uint64_t nameCap;
};

__device__ __forceinline__ unsigned long long frag_hash(const uint8_t* __restrict__ p, uint32_t n) {      // FNV-1a with a final mix
    unsigned long long h = 0xcbf29ce484222325ull;
    for (uint32_t i = 0; i < n; i++) h = (h ^ (unsigned long long)p[i]) * 0x100000001b3ull;
    h ^= h >> 33; h *= 0xff51afd7ed558ccdull; h ^= h >> 33;
    return h;
}
// records [0, limit) of this chunk act; the stopping record (index limit, when stopHere) is seen and does nothing
__device__ __forceinline__ int64_t frag_limit(const FragArgs& a, bool* stopHere) {
    const unsigned long long key = a.ctl[FK_STOP_KEY];
    if (stopHere) *stopHere = key != 0ull;
    return key ? bam_stop_index(key) : a.nrec;
}
// item i: a carried entry (i < ncarry) or record i - ncarry.  Name bytes and hash.
__device__ __forceinline__ const uint8_t* frag_item_name(const FragArgs& a, int64_t i, uint32_t* len, unsigned long long* hash) {
    if (i < a.ncarry) {
        const FragHdr h = ((const FragHdr*)a.carry)[i];
        const uint64_t blob = (uint64_t)a.ncarry * FRAG_HDR_BYTES;
        uint32_t n = h.nameLen;
        if (n > 254u || (uint64_t)h.nameOff + n > a.carryUsed - blob) n = 0;      // (a carry nobody but the library wrote never gets here)
        *len = n; *hash = h.hash & a.hashMask;
        return a.carry + blob + h.nameOff;
    }
    const FragRec s = a.summary[i - a.ncarry];
    *len = s.cls >> FC_NAME_SHIFT; *hash = s.hash;
    return a.rec + bam_name_at(s.off);
}
__device__ __forceinline__ bool frag_same_bytes(const uint8_t* __restrict__ x, const uint8_t* __restrict__ y, uint32_t n) {
    for (uint32_t i = 0; i < n; i++) if (x[i] != y[i]) return false;
    return true;
}

// running maximum of the bin stops (one workgroup of 1024: a BED file has tens of thousands of bins per chromosome)
__global__ void __launch_bounds__(1024) k_frag_prefmax(const int32_t* __restrict__ stop, int64_t n, int32_t* __restrict__ out) {
    __shared__ int32_t sW[16]; __shared__ int32_t sRun;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) sRun = INT32_MIN;
    __syncthreads();
    for (int64_t base = 0; base < n; base += 1024) {
        const int64_t i = base + tid;
        int32_t v = i < n ? stop[i] : INT32_MIN;
        for (int d = 1; d < 64; d <<= 1) { const int32_t o = __shfl_up(v, d, 64); if (lane >= d) v = max(v, o); }
        if (lane == 63) sW[wave] = v;
        __syncthreads();
        int32_t pre = sRun;
        for (int w = 0; w < wave; w++) pre = max(pre, sW[w]);
        v = max(v, pre);
        if (i < n) out[i] = v;
        __syncthreads();
        if (tid == 1023) sRun = v;
        __syncthreads();
    }
}

__global__ void __launch_bounds__(FRAG_BLOCK) k_frag_classify(FragArgs a) {
    __shared__ int32_t sStop[FRAG_WAVES];
    const int tid = threadIdx.x;
    const int64_t r = (int64_t)blockIdx.x * FRAG_BLOCK + tid;
    bool stop = false;
    if (r < a.nrec) {
        FragRec s; s.pos = 0; s.nextPos = 0; s.tlen = 0; s.cls = FC_MALFORMED; s.hash = 0ull; s.off = 0ull;
        const uint64_t off = a.offs[r]; BamRec b;
        if (bam_rec_load(a.rec, a.nbytes, off, b)) {
            const uint32_t flag = b.flag, nlen = b.l_read_name ? b.l_read_name - 1u : 0u;       // the name without its NUL: inside the record (32 + l_read_name <= block_size)
            uint32_t cls = nlen << FC_NAME_SHIFT;
            if (b.refID != a.refId) { cls |= FC_OTHER_REF; stop = true; }
            else {
                if (flag & 0x1u) cls |= FC_PAIRED;
                if (!(flag & (0x4u | 0x8u | 0x100u)) && (flag & 0x3u) == 0x3u) {               // IsMapped, IsMateMapped, IsPrimaryAlignment, IsPaired && IsProperPair
                    cls |= FC_LIVE;
                    if ((flag & 0x600u) || b.mapq == 255u || (int32_t)b.mapq < a.quality) cls |= FC_BAD;
                    if (b.refID != b.next_refID) cls |= FC_REF_MISMATCH;
                    s.hash = frag_hash(a.rec + bam_name_at(off), nlen) & a.hashMask;
                }
            }
            s.pos = b.pos; s.nextPos = b.next_pos; s.tlen = b.tlen; s.cls = cls; s.off = off;
        }
        a.summary[r] = s;
    }
    const int first = bam_block_first(stop, sStop);
    if (tid == 0 && first >= 0) atomicMax(&a.ctl[FK_STOP_KEY], bam_stop_key(1u, (int64_t)blockIdx.x * FRAG_BLOCK + first));      // the smallest index wins
}

__global__ void __launch_bounds__(FRAG_BLOCK) k_frag_insert(FragArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * FRAG_BLOCK + threadIdx.x;
    const int64_t limit = frag_limit(a, nullptr);
    bool paired = false, malformed = false, valid = false, live = i < a.ncarry;
    unsigned long long hash = 0ull;
    const int64_t r = i - a.ncarry;
    if (i < a.ncarry) hash = ((const FragHdr*)a.carry)[i].hash & a.hashMask;
    else if (r < limit) {
        const FragRec s = a.summary[r];
        malformed = (s.cls & FC_MALFORMED) != 0u; valid = !malformed; paired = (s.cls & FC_PAIRED) != 0u; live = (s.cls & FC_LIVE) != 0u; hash = s.hash;
        if (valid) {                                                                           // the nearest well-formed record on the left: almost always r - 1
            bool have = a.state[FRAG_HAVE_LAST] != 0; int32_t prev = have ? (int32_t)a.state[FRAG_LAST_POS] : -1;
            for (int64_t q = r - 1; q >= 0; q--) { const FragRec t = a.summary[q]; if (!(t.cls & FC_MALFORMED)) { prev = t.pos; break; } }
            if (s.pos < prev) atomicMax(&a.ctl[FK_UNSORTED_KEY], bam_stop_key(1u, r));
        }
    }
    const unsigned long long mPaired = __ballot(paired), mBad = __ballot(malformed), mValid = __ballot(valid);
    if (lane == 0) {
        if (mPaired) atomicAdd(&a.ctl[FK_PAIRED], (unsigned long long)__popcll(mPaired));
        if (mBad) atomicAdd(&a.ctl[FK_MALFORMED], (unsigned long long)__popcll(mBad));
        if (mValid) atomicMax(&a.ctl[FK_LAST_KEY], (unsigned long long)(r + (63 - __clzll((long long)mValid))) + 1ull);      // 1 + index of the last well-formed record
    }
    if (live) a.next[i] = atomicExch(&a.head[(uint32_t)hash & a.slotMask], (int32_t)i);
}

__global__ void __launch_bounds__(FRAG_BLOCK) k_frag_leader(FragArgs a) {
    const int64_t i = (int64_t)blockIdx.x * FRAG_BLOCK + threadIdx.x;
    const int64_t limit = frag_limit(a, nullptr);
    if (i >= a.ncarry + limit) return;
    if (i >= a.ncarry && !(a.summary[i - a.ncarry].cls & FC_LIVE)) return;
    uint32_t len; unsigned long long hash; const uint8_t* name = frag_item_name(a, i, &len, &hash);
    int64_t lead = i; bool split = false;
    for (int32_t j = a.head[(uint32_t)hash & a.slotMask]; j >= 0; j = a.next[j]) {
        if (j == i) continue;
        uint32_t len2; unsigned long long hash2; const uint8_t* name2 = frag_item_name(a, j, &len2, &hash2);
        if (hash2 != hash) continue;
        if (len2 == len && frag_same_bytes(name, name2, len)) { if (j < lead) lead = j; }
        else split = true;                                                                      // equal hashes, other bytes
    }
    a.leader[i] = (int32_t)lead;
    if (lead == i && split) atomicAdd(&a.ctl[FK_SPLIT], 1ull);
}

__global__ void __launch_bounds__(FRAG_BLOCK) k_frag_resolve(FragArgs a) {
    const int64_t i = (int64_t)blockIdx.x * FRAG_BLOCK + threadIdx.x;
    const int64_t limit = frag_limit(a, nullptr);
    if (i >= a.ncarry + limit) return;
    if (i >= a.ncarry && !(a.summary[i - a.ncarry].cls & FC_LIVE)) return;
    if (a.leader[i] != (int32_t)i) return;
    uint32_t len; unsigned long long hash; const uint8_t* name = frag_item_name(a, i, &len, &hash);
    const int32_t first = a.head[(uint32_t)hash & a.slotMask];
    int32_t binned = -1; bool samePos = false; long long usable = 0; unsigned long long members = 0;
    const int32_t nbins = (int32_t)a.nbins;
    for (int64_t cur = i; cur >= 0;) {
        members++;
        if (cur < a.ncarry) { const FragHdr h = ((const FragHdr*)a.carry)[cur]; binned = h.bin >= 0 && h.bin < nbins ? h.bin : -1; samePos = h.samePos != 0u; }
        else {
            const int64_t r = cur - a.ncarry; const FragRec s = a.summary[r];
            const bool bad = (s.cls & FC_BAD) != 0u;
            if (binned >= 0) {                                                                  // the mate was binned: undo when this read is bad
                if (bad) { usable--; a.ev[r] = ((uint32_t)binned << 1) | 1u; }
                binned = -1;
            } else if (!bad && !(s.cls & FC_REF_MISMATCH) && s.pos <= s.nextPos) {
                bool go = true;
                if (s.pos == s.nextPos) { go = !samePos; samePos = !samePos; }
                if (go && s.tlen != 0) {
                    const int32_t fStart = s.pos, fStop = (int32_t)((uint32_t)s.pos + (uint32_t)s.tlen);      // wraps, as unchecked C# does
                    int32_t lo = 0, hi = nbins;                                                 // the pointer: the first bin whose running maximum of Stop exceeds the start
                    while (lo < hi) { const int32_t mid = lo + ((hi - lo) >> 1); if (a.prefMax[mid] > fStart) hi = mid; else lo = mid + 1; }
                    int32_t best = -1, bestOverlap = 0;
                    for (int32_t b = lo; b < nbins; b++) {                                      // FindBestBin (:349-369)
                        const int32_t overlap = (int32_t)((uint32_t)min(a.binStop[b], fStop) - (uint32_t)max(a.binStart[b], fStart));
                        if (overlap <= 0) break;
                        if (overlap > bestOverlap) { bestOverlap = overlap; best = b; }
                    }
                    if (best >= 0) { usable++; a.ev[r] = (uint32_t)best << 1; binned = best; }
                }
            }
        }
        int64_t nxt = -1;                                                                       // the member with the next larger index
        for (int32_t j = first; j >= 0; j = a.next[j]) if (j > cur && a.leader[j] == (int32_t)i && (nxt < 0 || j < nxt)) nxt = j;
        cur = nxt;
    }
    if (usable) atomicAdd(&a.ctl[FK_USABLE], (unsigned long long)usable);                       // (two's complement: the net sum)
    atomicMax(&a.ctl[FK_LONGEST], members);
    if (binned >= 0 || samePos) {
        const unsigned long long slot = atomicAdd(&a.ctl[FK_ENTRIES], 1ull), at = atomicAdd(&a.ctl[FK_NAME_BYTES], (unsigned long long)len);
        if (at + len > a.nameCap) len = 0;                                                      // (only a carry the library did not write can name more bytes than it holds)
        FragHdr h; h.hash = 0ull; h.nameOff = (uint32_t)at; h.bin = binned; h.nameLen = len; h.samePos = samePos ? 1u : 0u;
        h.hash = frag_hash(name, len);                                                          // the FULL hash: the test hook may differ from chunk to chunk
        a.newHdr[slot] = h;
        for (uint32_t k = 0; k < len; k++) a.newNames[at + k] = name[k];
    }
}

__device__ __forceinline__ unsigned long long frag_need(const unsigned long long* ctl) {
    const unsigned long long n = ctl[FK_ENTRIES];
    return n ? n * FRAG_HDR_BYTES + ((ctl[FK_NAME_BYTES] + 7ull) & ~7ull) : 0ull;
}
// one lane per record (events) and per new entry (header and name); lane 0 of the grid adds the counters.  Nothing is written when the carry does not fit.
__global__ void __launch_bounds__(FRAG_BLOCK) k_frag_commit(FragArgs a, int32_t* __restrict__ count, uint8_t* __restrict__ carryOut, uint64_t capacity, long long* __restrict__ state) {
    const unsigned long long need = frag_need(a.ctl);
    if (need > capacity) return;
    const int64_t i = (int64_t)blockIdx.x * FRAG_BLOCK + threadIdx.x;
    bool stopHere; const int64_t limit = frag_limit(a, &stopHere);
    if (i < limit) { const uint32_t e = a.ev[i]; if (e != 0xFFFFFFFFu) atomicAdd(&count[e >> 1], (e & 1u) ? -1 : 1); }
    const unsigned long long n = a.ctl[FK_ENTRIES];
    if ((unsigned long long)i < n) {
        const FragHdr h = a.newHdr[i];
        ((FragHdr*)carryOut)[i] = h;
        uint8_t* dst = carryOut + n * FRAG_HDR_BYTES + h.nameOff;
        for (uint32_t k = 0; k < h.nameLen; k++) dst[k] = a.newNames[h.nameOff + k];
    }
    if (i == 0) {
        const long long seenBefore = state[FRAG_SEEN];
        state[FRAG_SEEN] += limit + (stopHere ? 1 : 0);
        if (stopHere) state[FRAG_STOPPED] = 1;
        state[FRAG_PAIRED] += (long long)a.ctl[FK_PAIRED];
        state[FRAG_USABLE] += (long long)a.ctl[FK_USABLE];
        state[FRAG_MALFORMED] += (long long)a.ctl[FK_MALFORMED];
        const unsigned long long u = a.ctl[FK_UNSORTED_KEY];
        if (u && state[FRAG_UNSORTED] == 0) state[FRAG_UNSORTED] = seenBefore + bam_stop_index(u) + 1;      // 1 + its ordinal among the records seen
        const unsigned long long lastKey = a.ctl[FK_LAST_KEY];
        if (lastKey) { state[FRAG_LAST_POS] = (long long)a.summary[lastKey - 1ull].pos; state[FRAG_HAVE_LAST] = 1; }
        state[FRAG_ENTRIES] = (long long)n; state[FRAG_CARRY_BYTES] = (long long)need;
        state[FRAG_SPLIT_GROUPS] += (long long)a.ctl[FK_SPLIT];
        if ((long long)a.ctl[FK_LONGEST] > state[FRAG_LONGEST]) state[FRAG_LONGEST] = (long long)a.ctl[FK_LONGEST];
    }
}

// the state travels through the context's pinned mailbox (common.hpp: payload, system fence, sequence word last); words 16 / 17: the bytes the carry needs, and whether it fits
__global__ void k_frag_mail(const long long* __restrict__ state, const unsigned long long* __restrict__ ctl, uint64_t capacity, long long* pin, unsigned* seqWord, unsigned seq) {
    if (threadIdx.x < FRAG_NSTATE) pin[threadIdx.x] = state[threadIdx.x];
    if (threadIdx.x == FRAG_NSTATE) { const unsigned long long need = ctl ? frag_need(ctl) : 0ull; pin[16] = (long long)need; pin[17] = need > capacity ? 0 : 1; }
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) cvx_mail_publish(seqWord, seq);
}

extern "C" int32_t canvas_fragments_from_bam(canvas_ctx* ctx, const uint8_t* d_records, uint64_t nbytes, const uint64_t* d_record_offsets, int64_t nrecords, int32_t ref_id,
                                             const int32_t* d_bin_start, const int32_t* d_bin_stop, int64_t nbins, int32_t quality_threshold, int32_t* d_count,
                                             uint8_t* d_carry, uint64_t carry_capacity, int64_t* d_state, int64_t* h_info) {
    if (!ctx) return CANVAS_ERR_INVALID;
    if (nrecords < 0 || (nrecords > 0 && (!d_records || !d_record_offsets)) || !d_count || !d_carry || !d_state || !h_info) CANVAS_FAIL(ctx, CANVAS_ERR_INVALID, "canvas_fragments_from_bam: bad arguments");
    if (ref_id < 0) CANVAS_FAIL(ctx, CANVAS_ERR_INVALID, "canvas_fragments_from_bam: ref_id must not be negative");
    if (nbins < 0 || nbins >= ((int64_t)1 << 31) || (nbins > 0 && (!d_bin_start || !d_bin_stop))) CANVAS_FAIL(ctx, CANVAS_ERR_INVALID, "canvas_fragments_from_bam: nbins must be in [0, 2^31) and the bins given");
    if (quality_threshold < 0) CANVAS_FAIL(ctx, CANVAS_ERR_INVALID, "canvas_fragments_from_bam: quality_threshold must not be negative");
    if (nrecords >= ((int64_t)1 << 30)) CANVAS_FAIL(ctx, CANVAS_ERR_INVALID, "canvas_fragments_from_bam: too many records in one chunk");
    unsigned long long hashMask = ~0ull;
    if (const char* e = cvx_hook("CANVAS_FRAG_HASH_BITS")) { const int k = atoi(e); if (k >= 0 && k < 64) hashMask = k == 0 ? 0ull : ((1ull << k) - 1ull); }
    CANVAS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    int32_t rc = canvas_pin_reserve(ctx, 256); if (rc) return rc;
    long long* pin = (long long*)ctx->pin; unsigned* seqWord = (unsigned*)(pin + 18);
    // the state as the chunk before left it: whether the chromosome has stopped, and how many entries the carry holds (the grid of the kernels depends on it)
    CANVAS_HIP_TRY(ctx, hipMemcpyAsync(pin, d_state, FRAG_NSTATE * 8, hipMemcpyDeviceToHost, ctx->stream));
    CANVAS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const long long stopped = pin[FRAG_STOPPED], ncarry = pin[FRAG_ENTRIES], carryUsed = pin[FRAG_CARRY_BYTES];
    if (ncarry < 0 || ncarry >= ((long long)1 << 30) || carryUsed < ncarry * FRAG_HDR_BYTES || (uint64_t)carryUsed > carry_capacity)
        CANVAS_FAIL(ctx, CANVAS_ERR_INVALID, "canvas_fragments_from_bam: d_state does not describe d_carry (zero it before the first chunk; keep the carry's contents when it is enlarged)");
    if (stopped || nrecords == 0) { for (int i = 0; i < FRAG_NSTATE; i++) h_info[i] = pin[i]; return CANVAS_OK; }      // nothing behind the stopping record has any effect

    const int64_t nitems = ncarry + nrecords, ntilesRec = (nrecords + FRAG_BLOCK - 1) / FRAG_BLOCK, ntilesItem = (nitems + FRAG_BLOCK - 1) / FRAG_BLOCK;
    uint64_t slots = 1024; while (slots < 2ull * (uint64_t)nitems) slots <<= 1;
    // the new carry: at most one entry per item, its name no longer than the item's — the old carry's name bytes, and 254 per record at the most (bounded by the chunk)
    const uint64_t nameCap = ((uint64_t)carryUsed - (uint64_t)ncarry * FRAG_HDR_BYTES) + std::min<uint64_t>(nbytes, 254ull * (uint64_t)nrecords) + 8;
    FragArgs a;
    a.rec = d_records; a.nbytes = nbytes; a.offs = d_record_offsets; a.nrec = nrecords; a.refId = ref_id; a.binStart = d_bin_start; a.binStop = d_bin_stop; a.nbins = nbins; a.quality = quality_threshold;
    a.carry = d_carry; a.ncarry = ncarry; a.carryUsed = (uint64_t)carryUsed; a.state = (const long long*)d_state; a.hashMask = hashMask;
    a.slotMask = (uint32_t)(slots - 1); a.nameCap = nameCap;
    rc = cvx_ws_carve(ctx, 256, [&](WsCarver& cv) {
        cv.take(a.ctl, FK_WORDS); cv.take(a.prefMax, (size_t)nbins); cv.take(a.summary, (size_t)nrecords); cv.take(a.head, (size_t)slots);
        cv.take(a.next, (size_t)nitems); cv.take(a.leader, (size_t)nitems); cv.take(a.ev, (size_t)nrecords); cv.take(a.newHdr, (size_t)nitems); cv.take(a.newNames, (size_t)nameCap);
    });
    if (rc) return rc;
    {
        ProfScope ps(ctx, "fragments_from_bam", true);
        CANVAS_HIP_TRY(ctx, hipMemsetAsync(a.ctl, 0, FK_WORDS * 8, ctx->stream));
        CANVAS_HIP_TRY(ctx, hipMemsetAsync(a.head, 0xFF, slots * 4, ctx->stream));
        CANVAS_HIP_TRY(ctx, hipMemsetAsync(a.ev, 0xFF, (size_t)nrecords * 4, ctx->stream));
        if (nbins > 0) hipLaunchKernelGGL(k_frag_prefmax, dim3(1), dim3(1024), 0, ctx->stream, d_bin_stop, nbins, a.prefMax);
        hipLaunchKernelGGL(k_frag_classify, dim3((unsigned)ntilesRec), dim3(FRAG_BLOCK), 0, ctx->stream, a);
        hipLaunchKernelGGL(k_frag_insert, dim3((unsigned)ntilesItem), dim3(FRAG_BLOCK), 0, ctx->stream, a);
        hipLaunchKernelGGL(k_frag_leader, dim3((unsigned)ntilesItem), dim3(FRAG_BLOCK), 0, ctx->stream, a);
        hipLaunchKernelGGL(k_frag_resolve, dim3((unsigned)ntilesItem), dim3(FRAG_BLOCK), 0, ctx->stream, a);
        hipLaunchKernelGGL(k_frag_commit, dim3((unsigned)ntilesItem), dim3(FRAG_BLOCK), 0, ctx->stream, a, d_count, d_carry, carry_capacity, (long long*)d_state);
    }
    CANVAS_HIP_TRY(ctx, hipGetLastError());
    const unsigned seq = cvx_mail_arm(ctx, seqWord);
    hipLaunchKernelGGL(k_frag_mail, dim3(1), dim3(64), 0, ctx->stream, (const long long*)d_state, (const unsigned long long*)a.ctl, carry_capacity, pin, seqWord, seq);
    CANVAS_HIP_TRY(ctx, hipGetLastError());
    CANVAS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    rc = cvx_mail_await(ctx, seqWord, seq, "canvas_fragments_from_bam"); if (rc) return rc;
    for (int i = 0; i < FRAG_NSTATE; i++) h_info[i] = pin[i];
    if (!pin[17]) { h_info[FRAG_CARRY_BYTES] = pin[16]; CANVAS_FAIL(ctx, CANVAS_ERR_CAPACITY, "canvas_fragments_from_bam: the carried entries need " + std::to_string(pin[16]) + " bytes of d_carry"); }
    return CANVAS_OK;
}
