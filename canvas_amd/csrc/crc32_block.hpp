// The CRC32 of RFC 1952 (zlib's crc32: polynomial 0xEDB88320 reflected, register preset to and result inverted with 0xFFFFFFFF) for canvas_bgzf_crc32 (crc.hip) and for
// the host (tests/crc32_host.cpp runs it under AddressSanitizer).  Plain C++ under the BAM_FN pattern of bam_record.hpp; the look-up tables are the caller's (LDS on the
// device), so no array here is a dynamically indexed local.
//
// A register value stands for a polynomial over GF(2) modulo P, bit 31 the coefficient of x^0 and bit 0 that of x^31: one shift to the right multiplies by x.  With
// raw(D) = the register after the bytes D from a register of 0, and n = |D|:
//   crc(D)        = ~( raw(D) ^ 0xFFFFFFFF * x^(8n) )                         the preset is a term of its own, the inversion comes last: both once per block
//   raw(A || B)   = raw(A) * x^(8|B|) ^ raw(B)                                what lets a block be cut into slices that are reduced side by side
//   crc(A || B)   = crc(A) * x^(8|B|) ^ crc(B)                                the same rule on finished values (the presets and inversions cancel): crc32_combine
// x^(8n) for any n up to 65536 (and beyond: n < 2^17) is the product of the entries of CRC32_X8POW its bits select, each product one 32-step multiply-reduce.
#pragma once
#include "bam_record.hpp"
#if !defined(__HIPCC__)
#include "../../include/canvas_hip.h"
#endif

#define CRC32_POLY 0xEDB88320u
#define CRC32_SLICE_BYTES 260u      // what one lane reduces: 65 words, an odd count, so that the 32 lanes of an LDS lane group read 32 different banks at every step; 253 slices in 64 KiB
#define CRC32_TABLE_WORDS 1024      // four tables of 256: table k takes a byte that has k more bytes behind it in its 32-bit word

// a * b mod P: the bits of a from x^0 up select b * x^i
BAM_FN constexpr uint32_t crc32_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 31; i >= 0; i--) {
        p ^= b & (0u - ((a >> i) & 1u));
        b = (b >> 1) ^ (CRC32_POLY & (0u - (b & 1u)));
    }
    return p;
}
// x^(8 * 2^k) mod P, k = 0 .. 16
#define CRC32_X8POW_INIT {0x00800000u, 0x00008000u, 0xEDB88320u, 0xB1E6B092u, 0xA06A2517u, 0xED627DAEu, 0x88D14467u, 0xD7BBFE6Au, 0xEC447F11u, 0x8E7EA170u, 0x6427800Eu, 0x4D47BAE0u, 0x09FE548Fu, 0x83852D0Fu, 0x30362F1Au, 0x7B5A9CC3u, 0x31FEC169u}
#define CRC32_X8POW_COUNT 17
static constexpr uint32_t CRC32_X8POW[CRC32_X8POW_COUNT] = CRC32_X8POW_INIT;
constexpr bool crc32_x8pow_squares() { for (int k = 0; k + 1 < CRC32_X8POW_COUNT; k++) if (crc32_mul(CRC32_X8POW[k], CRC32_X8POW[k]) != CRC32_X8POW[k + 1]) return false; return true; }
static_assert(CRC32_X8POW[0] == 0x80000000u >> 8 && crc32_x8pow_squares(), "CRC32_X8POW: x^8, then every entry the square of the one before");

// c * x^(8 nbytes) mod P, nbytes < 2^17: the register after nbytes more bytes of zeros
BAM_FN uint32_t crc32_shift(uint32_t c, uint32_t nbytes) {
    constexpr uint32_t X[CRC32_X8POW_COUNT] = CRC32_X8POW_INIT;
#if defined(__HIPCC__)
#pragma unroll                      // (every X[k] a constant of the code)
#endif
    for (int k = 0; k < CRC32_X8POW_COUNT; k++) if ((nbytes >> k) & 1u) c = crc32_mul(c, X[k]);
    return c;
}
BAM_FN uint32_t crc32_combine(uint32_t crcA, uint32_t crcB, uint32_t bytesB) { return crc32_shift(crcA, bytesB) ^ crcB; }

// entry i of table k: the byte i, 8 (k + 1) shifts on
BAM_FN uint32_t crc32_table_entry(uint32_t k, uint32_t i) {
    uint32_t c = i;
    for (uint32_t s = 0; s < 8 * (k + 1); s++) c = (c >> 1) ^ (CRC32_POLY & (0u - (c & 1u)));
    return c;
}
// raw(p[0, n)): four bytes a step through the four tables, the last n % 4 one at a time.  p has any alignment; no byte outside [p, p + n) is read
BAM_FN uint32_t crc32_raw(const uint8_t* p, uint32_t n, const uint32_t* T) {
    uint32_t c = 0, at = 0;
    for (; at + 4 <= n; at += 4) {
        c ^= bam_ld32(p, at);
        c = T[768 + (c & 255u)] ^ T[512 + ((c >> 8) & 255u)] ^ T[256 + ((c >> 16) & 255u)] ^ T[c >> 24];
    }
    for (; at < n; at++) c = T[(c ^ p[at]) & 255u] ^ (c >> 8);
    return c;
}
// the share of slice t (bytes [t * slice, (t + 1) * slice) of the block, cut at n) in raw(block): raw(slice) * x^(8 * bytes behind it); 0 for a slice behind n
BAM_FN uint32_t crc32_slice_term(const uint8_t* block, uint32_t n, uint32_t t, uint32_t slice, const uint32_t* T) {
    const uint64_t lo = (uint64_t)t * slice;
    if (lo >= n) return 0;
    const uint32_t hi = lo + slice < n ? (uint32_t)lo + slice : n;
    return crc32_shift(crc32_raw(block + lo, hi - (uint32_t)lo, T), n - hi);
}
// the xor of every slice's term -> the block's CRC32
BAM_FN uint32_t crc32_finish(uint32_t terms, uint32_t n) { return ~(terms ^ crc32_shift(0xFFFFFFFFu, n)); }

// a descriptor canvas_bgzf_crc32 may sum: at most 64 KiB at a range inside the destination, and (when a source is given) the trailer word inside the source
BAM_FN bool crc32_descriptor_ok(const canvas_bgzf_block& b, uint64_t dstNbytes, bool haveSrc, uint64_t srcNbytes) {
    if (b.out_bytes > 65536u || b.dst_offset > dstNbytes || b.out_bytes > dstNbytes - b.dst_offset) return false;
    if (!haveSrc) return true;
    return b.src_offset <= srcNbytes && (uint64_t)b.src_bytes + 4u <= srcNbytes - b.src_offset;
}

// ---- the host's form: the tables filled and every slice in turn
static inline void crc32_fill_tables(uint32_t* T) { for (uint32_t k = 0; k < CRC32_TABLE_WORDS; k++) T[k] = crc32_table_entry(k >> 8, k & 255u); }
static inline uint32_t crc32_sliced(const uint8_t* p, uint32_t n, uint32_t slice, const uint32_t* T) {
    uint32_t terms = 0;
    for (uint32_t t = 0; (uint64_t)t * slice < n; t++) terms ^= crc32_slice_term(p, n, t, slice, T);
    return crc32_finish(terms, n);
}
