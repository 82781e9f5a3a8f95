// The framing rules of a chunk of RAW BAM record bytes, once, for the kernels of frame.hip and for a host program (tests/bam_frame_host.cpp runs them under
// AddressSanitizer on chunks with no byte of padding behind them): where the block_size chain goes on, what a record is to a tool, and what an offset has to look like
// to be GUESSED as a record start.
//
// The chain: a record at `at` is whole when 4 bytes are left and, with block_size >= 32, the record ends inside the chunk; the next one stands at at + 4 + block_size.
// Anything else ends the chunk there (the carry of the next one) and is no event.  A whole record with block_size < 32 (negative values included) is MALFORMED and the
// chain ends at it.
//
// The kinds restate the three `frame` callables of the tools (tools/canvas_snv_main.cpp, tools/canvas_bin_main.cpp: load_bam_device, bin_fragments_device) and the loop
// around them (tools/tool_common.hpp: BamChunkLoop::run), decision by decision in their order.  The first record in chain order whose class is STOP, TAKE_AND_STOP,
// MALFORMED or UNSORTED is the event; nothing behind it is classified, taken or counted.
//
// Sortedness in parallel: bam_frame_classify answers TAKE with *compared set for a record that reaches the tool's comparison with the last taken position.  The
// sequential rule ("pos below the position of the record that reached the comparison last") equals "the first such record whose pos lies below the running MAXIMUM of
// the records that reached the comparison before it, the carried one included": up to the first violation the sequence is non-decreasing, so its last element is its
// maximum.  A running maximum is a scan; frame.hip takes it that way.
//
// Plain C++, <cstdint> only outside __HIPCC__ (bam_record.hpp's rule).
#pragma once
#include "bam_record.hpp"

// canvas_bam_frame_rule.kind (include/canvas_hip.h: CANVAS_BAM_FRAME_ALL / _SNV / _HITS / _FRAGMENTS)
enum { BAM_FRAME_ALL = 0, BAM_FRAME_SNV = 1, BAM_FRAME_HITS = 2, BAM_FRAME_FRAGMENTS = 3, BAM_FRAME_KINDS = 4 };
// what a record is to the tool
enum { BAM_FRAME_TAKE = 0, BAM_FRAME_SKIP = 1, BAM_FRAME_TAKE_AND_STOP = 2, BAM_FRAME_STOP = 3, BAM_FRAME_MALFORMED = 4, BAM_FRAME_UNSORTED = 5 };
struct BamFrameRule { int32_t kind, ref_id, paired_end, sorted; };      // the layout of canvas_bam_frame_rule (16 bytes)

// true: a whole record stands at `at` (at <= nbytes), bs = its block_size — possibly below 32: the chain ends AT it, and it is MALFORMED.
// false: the chunk ends here (fewer than 4 bytes, or a record the next chunk completes)
BAM_FN bool bam_frame_whole(const uint8_t* __restrict__ rec, uint64_t nbytes, uint64_t at, int32_t& bs) {
    if (at > nbytes || nbytes - at < 4) return false;
    bs = (int32_t)bam_ld32(rec, at);
    return !(bs >= 32 && (uint64_t)(uint32_t)bs > nbytes - at - 4);
}

// the read filters of LoadObservedAlignmentsBAM's loop (CanvasBin.cs:239-262; tools/canvas_bin_main.cpp: passes_read_filters), the ones in front of its comparison of
// reference ids.  b passed bam_rec_load: with n_cigar_op > 0 the first CIGAR word lies inside the record.
BAM_FN bool bam_frame_read_filters(const uint8_t* __restrict__ rec, uint64_t off, const BamRec& b, bool pairedEnd) {
    if (b.flag & 0x4u) return false;                        // !IsMapped
    if (b.flag & 0x200u) return false;                      // IsFailedQC
    if (b.flag & 0x400u) return false;                      // IsDuplicate
    if (b.flag & 0x10u) return false;                       // IsReverseStrand
    if (b.flag & 0x900u) return false;                      // !IsMainAlignment
    if (b.n_cigar_op == 0u) return false;
    const uint32_t c0 = bam_ld32(rec, bam_cigar_at(off, b.l_read_name));
    if ((c0 & 0xFu) != 0u || (c0 >> 4) < 35u) return false;   // must start with 35 bases of 'M'
    if (pairedEnd && !(b.flag & 0x2u)) return false;        // IsProperPair
    return true;
}

// The class of the whole record at `at` (bam_frame_whole said true) under `rule`, sortedness left out: a record that reaches the comparison comes back as TAKE with
// *compared = true and is UNSORTED when *pos lies below the running maximum (above).  *pos is the record's pos field (0 for block_size < 32).
BAM_FN int bam_frame_classify(const uint8_t* __restrict__ rec, uint64_t nbytes, uint64_t at, const BamFrameRule& rule, int32_t* pos, bool* compared) {
    *pos = 0; *compared = false;
    BamRec b;
    if ((int32_t)bam_ld32(rec, at) < 32) return BAM_FRAME_MALFORMED;
    const bool fit = bam_rec_load(rec, nbytes, at, b);            // (a whole record of block_size >= 32 leaves 36 bytes: b is filled; false = name and CIGAR do not fit)
    *pos = b.pos;
    switch (rule.kind) {
        case BAM_FRAME_SNV:
            if (!bam_rec_holds_seq(b)) return BAM_FRAME_MALFORMED;
            if (b.refID < 0 || b.pos < 0 || b.refID > rule.ref_id) return BAM_FRAME_STOP;      // past the chromosome of interest
            if (b.refID != rule.ref_id) return BAM_FRAME_SKIP;
            *compared = true; return BAM_FRAME_TAKE;
        case BAM_FRAME_HITS:
            if (!fit) return BAM_FRAME_MALFORMED;
            if (b.refID == rule.ref_id && !rule.sorted) return BAM_FRAME_TAKE;                 // cannot stop, and its position does not matter
            if (!bam_frame_read_filters(rec, at, b, rule.paired_end != 0)) return BAM_FRAME_TAKE;
            if (b.refID != rule.ref_id) return BAM_FRAME_TAKE_AND_STOP;
            *compared = true; return BAM_FRAME_TAKE;
        case BAM_FRAME_FRAGMENTS:
            if (!fit) return BAM_FRAME_MALFORMED;
            return b.refID != rule.ref_id ? BAM_FRAME_TAKE_AND_STOP : BAM_FRAME_TAKE;
        default:
            return BAM_FRAME_TAKE;                                                             // BAM_FRAME_ALL: every whole record
    }
}

// The shape test of a candidate: p points at 36 readable bytes, `room` = the bytes from p to the chunk's end (>= 36).  true: what stands here could be the start of an
// alignment record as aligners write them.  It decides where a tile's walk is STARTED on speculation and nothing else: a record of the chain that fails it is framed
// all the same (its tile is walked again from the true entry), and bytes that pass it without being on the chain are never reported.
BAM_FN bool bam_frame_shape(const uint8_t* __restrict__ p, uint64_t room) {
    const int32_t bs = (int32_t)bam_ld32(p, 0);
    if (bs < 32 || (uint64_t)(uint32_t)bs > room - 4) return false;
    const int32_t refID = (int32_t)bam_ld32(p, 4), pos = (int32_t)bam_ld32(p, 8), l_seq = (int32_t)bam_ld32(p, 20), nref = (int32_t)bam_ld32(p, 24), npos = (int32_t)bam_ld32(p, 28);
    const uint32_t lname = bam_ld8(p, 12), ncig = bam_ld16(p, 16);
    if (refID < -1 || refID >= (1 << 24) || pos < -1 || nref < -1 || nref >= (1 << 24) || npos < -1 || lname == 0u || l_seq < 0) return false;
    return 32ull + lname + 4ull * ncig + ((uint64_t)l_seq + 1) / 2 + (uint64_t)l_seq <= (uint64_t)bs;
}
