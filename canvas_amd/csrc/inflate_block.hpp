// One raw-deflate decoder for canvas_bgzf_inflate (inflate.hip) and for the host (tests/inflate_host.cpp runs it under AddressSanitizer), and the BGZF block walk of
// canvas_bgzf_scan.  Plain C++ under the BAM_FN pattern of bam_record.hpp: everything that reads input and decides a status is here, once; what differs between the two
// builds is the Io the decoder is given:
//   uint32_t word(uint32_t k)                          bytes [4k, 4k + 4) of the stream, little endian, every byte at or behind src_bytes as 0 (the clamp of the bit reader)
//   void put(uint32_t pos, uint32_t byte)              out[pos] = byte
//   void copy(uint32_t pos, uint32_t dist, uint32_t n) out[pos + i] = out[pos - dist + i] for i = 0 .. n - 1 in that order (dist < n repeats the last dist bytes)
//   void stored(uint32_t pos, uint32_t at, uint32_t n) out[pos + i] = stream byte at + i
// The decoder has checked every range before it calls one of the last three: pos + n <= out_bytes, dist <= pos, at + n <= src_bytes.
//
// Acceptance is zlib's (inflateInit2(-15), Z_FINISH, Z_STREAM_END with exactly out_bytes written; inflate_raw of tools/bam_io.hpp), rule by rule:
//   BTYPE 3; stored LEN != ~NLEN; more than 286 literal/length or 30 distance codes                  CANVAS_INFLATE_HEADER
//   repeat 16 first, a repeat past HLIT + HDIST, no end-of-block code, an over-subscribed set, an incomplete set other than zlib's two exceptions (one code of length 1;
//   no distance code at all), an unassigned code, literal/length symbols 286 / 287, distance symbols 30 / 31                                        CANVAS_INFLATE_CODE
//   a distance that reaches before the first output byte of THIS stream (no window is shared; one reaching back across deflate blocks inside it is fine)   _DISTANCE
//   the stream needs a bit behind src_bytes   _INPUT;   a byte behind out_bytes   _OVERRUN;   the final block ends before out_bytes   _SHORT
// Unused input behind the final block is accepted, and nothing checks a CRC, as there.
// Every loop consumes at least one bit or produces at least one byte per turn and stops once the bits or the bytes are used up: it ends on any input.
// No array of the decoder is a dynamically indexed local: the tables are the caller's (LDS on the device), so the device build needs no scratch.
#pragma once
#include "bam_record.hpp"
#if !defined(__HIPCC__)
#include "../../include/canvas_hip.h"
#endif

#define INF_FAST_BITS 9
struct InflateTables {
    uint16_t litFast[1 << INF_FAST_BITS], distFast[1 << INF_FAST_BITS];      // next 9 bits -> (symbol << 4) | length; 0: longer than 9 bits or unassigned
    uint16_t litSym[288], distSym[32], clSym[19];                             // symbols in canonical order
    uint16_t litCount[16], distCount[16], clCount[16], offs[16];              // codes per length
    uint8_t lens[320];                                                        // HLIT + HDIST code lengths (at most 286 + 30)
};

// ---- the bit reader: 32-bit words through io.word, which clamps; the count of bits taken is compared with the stream's 8 * src_bytes
template <class Io> struct InflateBits {
    Io& io; uint64_t bb = 0; uint32_t cnt = 0, next = 0; uint64_t total;
    BAM_FN InflateBits(Io& i, uint32_t srcBytes) : io(i), total(8ull * srcBytes) {}
    BAM_FN void refill() { if (cnt < 32) { bb |= (uint64_t)io.word(next++) << cnt; cnt += 32; } }      // at least 32 bits behind it
    BAM_FN uint32_t peek(uint32_t n) const { return (uint32_t)bb & ((1u << n) - 1u); }                 // n <= 31
    BAM_FN void drop(uint32_t n) { bb >>= n; cnt -= n; }
    BAM_FN uint32_t take(uint32_t n) { const uint32_t v = peek(n); drop(n); return v; }
    BAM_FN uint64_t used() const { return 32ull * next - cnt; }
    BAM_FN bool over() const { return used() > total; }                                                 // a bit behind the stream's last was taken
    BAM_FN void seek_byte(uint32_t at) { next = at >> 2; bb = 0; cnt = 0; refill(); drop(8 * (at & 3)); }
};

BAM_FN uint32_t inflate_rev(uint32_t code, uint32_t len) {      // the low len bits (len <= 15) in reverse order
    code = ((code & 0x5555u) << 1) | ((code >> 1) & 0x5555u); code = ((code & 0x3333u) << 2) | ((code >> 2) & 0x3333u);
    code = ((code & 0x0F0Fu) << 4) | ((code >> 4) & 0x0F0Fu); code = ((code & 0x00FFu) << 8) | ((code >> 8) & 0x00FFu);
    return code >> (16 - len);
}

// canonical code of lens[0 .. n): count, sym and (fast != nullptr) the 9-bit table.  -1 over-subscribed; otherwise the unused code space in units of 2^-15 (0 = complete);
// maxLen = the longest code, 0 when there is none
BAM_FN int32_t inflate_build(const uint8_t* lens, uint32_t n, uint16_t* count, uint16_t* sym, uint16_t* offs, uint16_t* fast, uint32_t& maxLen) {
    for (uint32_t l = 0; l < 16; l++) count[l] = 0;
    for (uint32_t i = 0; i < n; i++) count[lens[i]]++;
    int32_t left = 1; maxLen = 0;
    for (uint32_t l = 1; l < 16; l++) { left = 2 * left - (int32_t)count[l]; if (left < 0) return -1; if (count[l]) maxLen = l; }
    offs[1] = 0;
    for (uint32_t l = 1; l < 15; l++) offs[l + 1] = (uint16_t)(offs[l] + count[l]);
    for (uint32_t i = 0; i < n; i++) if (lens[i]) sym[offs[lens[i]]++] = (uint16_t)i;
    if (fast) {
        for (uint32_t k = 0; k < (1u << INF_FAST_BITS); k++) fast[k] = 0;
        uint32_t code = 0, idx = 0;
        for (uint32_t l = 1; l <= INF_FAST_BITS; l++) {
            for (uint32_t j = 0; j < count[l]; j++, code++, idx++) {
                const uint16_t e = (uint16_t)((sym[idx] << 4) | l);
                for (uint32_t k = inflate_rev(code, l); k < (1u << INF_FAST_BITS); k += 1u << l) fast[k] = e;
            }
            code <<= 1;
        }
    }
    return left;
}
// the symbol of the code that starts at the reader's next bit (at least 15 bits are there), its bits dropped; -1: no code of the set starts like this
template <class Io> BAM_FN int32_t inflate_symbol(InflateBits<Io>& br, const uint16_t* count, const uint16_t* sym, const uint16_t* fast) {
    if (fast) { const uint32_t e = fast[br.peek(INF_FAST_BITS)]; if (e) { br.drop(e & 15u); return (int32_t)(e >> 4); } }
    uint32_t v = br.peek(15);
    int32_t code = 0, first = 0, index = 0;
    for (uint32_t l = 1; l < 16; l++) {
        code |= (int32_t)(v & 1u); v >>= 1;
        const int32_t c = count[l];
        if (code - c < first) { br.drop(l); return sym[index + (code - first)]; }
        index += c; first = (first + c) << 1; code <<= 1;
    }
    return -1;
}

// the deflate stream of src_bytes bytes behind io, which has to give exactly out_bytes (both at most 65536) -> a CANVAS_INFLATE_* status
template <class Io> BAM_FN int32_t inflate_stream(Io& io, uint32_t srcBytes, uint32_t outBytes, InflateTables& T) {
    InflateBits<Io> br(io, srcBytes);
    uint32_t pos = 0;
    for (;;) {
        br.refill();
        const uint32_t last = br.take(1), type = br.take(2);
        if (br.over()) return CANVAS_INFLATE_INPUT;
        if (type == 3) return CANVAS_INFLATE_HEADER;
        if (type == 0) {
            br.drop(br.cnt & 7u);                                   // to the byte boundary (32 * next is one)
            br.refill();
            const uint32_t len = br.take(16), nlen = br.take(16);
            if (br.over()) return CANVAS_INFLATE_INPUT;
            if ((len ^ 0xFFFFu) != nlen) return CANVAS_INFLATE_HEADER;
            const uint32_t at = (uint32_t)(br.used() >> 3);
            if (len > srcBytes - at) return CANVAS_INFLATE_INPUT;
            if (len > outBytes - pos) return CANVAS_INFLATE_OVERRUN;
            if (len) io.stored(pos, at, len);
            pos += len; br.seek_byte(at + len);
        } else {
            uint32_t maxLen;
            if (type == 1) {
                for (uint32_t i = 0; i < 144; i++) T.lens[i] = 8;
                for (uint32_t i = 144; i < 256; i++) T.lens[i] = 9;
                for (uint32_t i = 256; i < 280; i++) T.lens[i] = 7;
                for (uint32_t i = 280; i < 288; i++) T.lens[i] = 8;
                for (uint32_t i = 288; i < 320; i++) T.lens[i] = 5;
                (void)inflate_build(T.lens, 288, T.litCount, T.litSym, T.offs, T.litFast, maxLen);
                (void)inflate_build(T.lens + 288, 32, T.distCount, T.distSym, T.offs, T.distFast, maxLen);
            } else {
                br.refill();
                const uint32_t nlit = br.take(5) + 257, ndist = br.take(5) + 1, ncl = br.take(4) + 4;
                if (br.over()) return CANVAS_INFLATE_INPUT;
                if (nlit > 286 || ndist > 30) return CANVAS_INFLATE_HEADER;
                for (uint32_t i = 0; i < 19; i++) T.lens[i] = 0;
                for (uint32_t i = 0; i < ncl; i++) {
                    br.refill();
                    // the order of the code-length code's lengths, 5 bits each: 16 17 18 0 8 7 9 6 10 5 11 4 | 12 3 13 2 14 1 15
                    const uint64_t order = i < 12 ? 0x22CAA324E804A30ull : 0x3C2E1346Cull;
                    T.lens[(order >> (5 * (i < 12 ? i : i - 12))) & 31u] = (uint8_t)br.take(3);
                }
                if (br.over()) return CANVAS_INFLATE_INPUT;
                if (inflate_build(T.lens, 19, T.clCount, T.clSym, T.offs, nullptr, maxLen) != 0) return CANVAS_INFLATE_CODE;      // (zlib lets an EMPTY set pass and then misses the end-of-block code)
                uint32_t have = 0;
                while (have < nlit + ndist) {
                    br.refill();
                    const int32_t s = inflate_symbol(br, T.clCount, T.clSym, nullptr);
                    if (s < 0) return br.over() ? CANVAS_INFLATE_INPUT : CANVAS_INFLATE_CODE;
                    uint32_t rep = 1, v = (uint32_t)s;
                    if (s == 16) { if (have == 0) return br.over() ? CANVAS_INFLATE_INPUT : CANVAS_INFLATE_CODE; v = T.lens[have - 1]; rep = 3 + br.take(2); }
                    else if (s == 17) { v = 0; rep = 3 + br.take(3); }
                    else if (s == 18) { v = 0; rep = 11 + br.take(7); }
                    if (br.over()) return CANVAS_INFLATE_INPUT;
                    if (rep > nlit + ndist - have) return CANVAS_INFLATE_CODE;
                    for (uint32_t j = 0; j < rep; j++) T.lens[have++] = (uint8_t)v;
                }
                if (T.lens[256] == 0) return CANVAS_INFLATE_CODE;
                int32_t left = inflate_build(T.lens + nlit, ndist, T.distCount, T.distSym, T.offs, T.distFast, maxLen);
                if (left < 0 || (left > 0 && maxLen > 1)) return CANVAS_INFLATE_CODE;
                left = inflate_build(T.lens, nlit, T.litCount, T.litSym, T.offs, T.litFast, maxLen);
                if (left < 0 || (left > 0 && maxLen != 1)) return CANVAS_INFLATE_CODE;
            }
            for (;;) {
                br.refill();
                const int32_t s = inflate_symbol(br, T.litCount, T.litSym, T.litFast);
                if (s < 0) return br.over() ? CANVAS_INFLATE_INPUT : CANVAS_INFLATE_CODE;
                if (s < 256) {
                    if (br.over()) return CANVAS_INFLATE_INPUT;
                    if (pos >= outBytes) return CANVAS_INFLATE_OVERRUN;
                    io.put(pos++, (uint32_t)s);
                    continue;
                }
                if (s == 256) { if (br.over()) return CANVAS_INFLATE_INPUT; break; }
                if (s > 285) return br.over() ? CANVAS_INFLATE_INPUT : CANVAS_INFLATE_CODE;
                uint32_t len;
                if (s < 265) len = (uint32_t)s - 254;
                else if (s == 285) len = 258;
                else { const uint32_t k = (uint32_t)s - 261, e = k >> 2; len = ((4 + (k & 3u)) << e) + 3 + br.take(e); }
                br.refill();
                const int32_t d = inflate_symbol(br, T.distCount, T.distSym, T.distFast);
                if (d < 0 || d > 29) return br.over() ? CANVAS_INFLATE_INPUT : CANVAS_INFLATE_CODE;
                uint32_t dist;
                if (d < 4) dist = (uint32_t)d + 1;
                else { const uint32_t e = ((uint32_t)d >> 1) - 1; dist = ((2 + ((uint32_t)d & 1u)) << e) + 1 + br.take(e); }
                if (br.over()) return CANVAS_INFLATE_INPUT;
                if (dist > pos) return CANVAS_INFLATE_DISTANCE;
                if (len > outBytes - pos) return CANVAS_INFLATE_OVERRUN;
                io.copy(pos, dist, len);
                pos += len;
            }
        }
        if (last) break;
    }
    return pos == outBytes ? CANVAS_INFLATE_OK : CANVAS_INFLATE_SHORT;
}

// a descriptor a block may be run with: both sizes within BGZF's bound, both ranges inside their buffers
BAM_FN bool inflate_descriptor_ok(const canvas_bgzf_block& b, uint64_t srcNbytes, uint64_t dstNbytes) {
    return b.src_bytes <= 65536u && b.out_bytes <= 65536u && b.src_offset <= srcNbytes && b.src_bytes <= srcNbytes - b.src_offset &&
           b.dst_offset <= dstNbytes && b.out_bytes <= dstNbytes - b.dst_offset;
}

// ---- the host's Io: a stream and a destination of exactly their sizes
struct InflateHostIo {
    const uint8_t* src; uint32_t srcBytes; uint8_t* out;
    uint32_t word(uint32_t k) const { uint32_t w = 0; for (uint32_t j = 0; j < 4; j++) { const uint64_t at = 4ull * k + j; if (at < srcBytes) w |= (uint32_t)src[at] << (8 * j); } return w; }
    void put(uint32_t pos, uint32_t byte) { out[pos] = (uint8_t)byte; }
    void copy(uint32_t pos, uint32_t dist, uint32_t n) { for (uint32_t i = 0; i < n; i++) out[pos + i] = out[pos - dist + i]; }
    void stored(uint32_t pos, uint32_t at, uint32_t n) { for (uint32_t i = 0; i < n; i++) out[pos + i] = src[at + i]; }
};
static inline int32_t inflate_block_host(const uint8_t* src, uint64_t srcNbytes, uint8_t* dst, uint64_t dstNbytes, const canvas_bgzf_block& b) {
    if (!inflate_descriptor_ok(b, srcNbytes, dstNbytes)) return CANVAS_INFLATE_DESCRIPTOR;
    InflateHostIo io{src + b.src_offset, b.src_bytes, dst + b.dst_offset};
    InflateTables T;
    return inflate_stream(io, b.src_bytes, b.out_bytes, T);
}

// ---- the BGZF block at h, of which avail bytes are there, by the rules of bgzf_parse (tools/bam_io.hpp): the magic bytes, FEXTRA, a `BC` subfield with SLEN 2, BSIZE
// large enough for header and trailer, the whole block inside avail, ISIZE <= 65536.  The block's size, or 0: these bytes are no block, or not all of one.
static inline uint64_t bgzf_block_at(const uint8_t* h, uint64_t avail, uint64_t& dataAt, uint32_t& dataBytes, uint32_t& isize) {
    if (avail < 12 || h[0] != 31 || h[1] != 139 || h[2] != 8 || !(h[3] & 4)) return 0;
    const uint64_t xlen = bam_ld16(h, 10);
    if (avail < 12 + xlen) return 0;
    int64_t bsize = -1;
    for (uint64_t i = 0; i + 4 <= xlen;) {
        const uint64_t s = 12 + i, slen = bam_ld16(h, s + 2);
        if (h[s] == 'B' && h[s + 1] == 'C' && slen == 2 && i + 6 <= xlen) bsize = (int64_t)bam_ld16(h, s + 4);
        i += 4 + slen;
    }
    if (bsize < 0 || (uint64_t)bsize + 1 < 12 + xlen + 8) return 0;
    const uint64_t size = (uint64_t)bsize + 1;
    if (avail < size) return 0;
    dataAt = 12 + xlen; dataBytes = (uint32_t)(size - dataAt - 8); isize = bam_ld32(h, size - 4);
    return isize <= 65536u ? size : 0;
}
// canvas_bgzf_scan without its argument checks
static inline void bgzf_scan_blocks(const uint8_t* bytes, uint64_t nbytes, uint64_t at, uint64_t maxOut, canvas_bgzf_block* blocks, int64_t capacity, int64_t* info) {
    int64_t n = 0; uint64_t total = 0; int64_t why;
    for (;;) {
        if (n >= capacity || total >= maxOut) { why = CANVAS_BGZF_SCAN_LIMIT; break; }
        if (at >= nbytes) { why = CANVAS_BGZF_SCAN_END; break; }
        uint64_t dataAt = 0; uint32_t dataBytes = 0, isize = 0;
        const uint64_t size = bgzf_block_at(bytes + at, nbytes - at, dataAt, dataBytes, isize);
        if (size == 0) { why = CANVAS_BGZF_SCAN_DAMAGED; break; }
        blocks[n].src_offset = at + dataAt; blocks[n].dst_offset = total; blocks[n].src_bytes = dataBytes; blocks[n].out_bytes = isize;
        n++; total += isize; at += size;
    }
    info[0] = n; info[1] = (int64_t)at; info[2] = (int64_t)total; info[3] = why;
}
