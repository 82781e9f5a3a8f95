// Raw inflate and BGZF / BAM / BAI reading, shared by every tool that reads compressed files.  Included by fast_io.hpp, inside the tool's one translation unit.
#pragma once
#include <zlib.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <string>
#include <vector>

static inline uint16_t le16(const uint8_t* p) { return (uint16_t)(p[0] | (p[1] << 8)); }
static inline uint32_t le32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

// a raw deflate stream of clen bytes that has to give exactly isize bytes.  syncFlushEnd: the stream may stop at a sync flush instead of a final block (the chunks of
// fast_io.hpp's write_gz_rows but the last); it then has to be consumed to its last byte
static bool inflate_raw(const void* src, size_t clen, void* dst, size_t isize, bool syncFlushEnd = false) {
    z_stream zs; memset(&zs, 0, sizeof zs);
    if (inflateInit2(&zs, -15) != Z_OK) return false;
    zs.next_in = (Bytef*)src; zs.avail_in = (uInt)clen; zs.next_out = (Bytef*)dst; zs.avail_out = (uInt)isize;
    const int rc = inflate(&zs, Z_FINISH); inflateEnd(&zs);
    if (syncFlushEnd) return (rc == Z_STREAM_END || rc == Z_OK || rc == Z_BUF_ERROR) && zs.avail_in == 0 && zs.avail_out == 0;
    return rc == Z_STREAM_END && zs.avail_out == 0;
}

// ---------------------------------------------------------------- BGZF / BAM / BAI
struct BgzfBlock { size_t in, clen, size; uint32_t isize, crc; };      // deflate data at [in, in + clen) of a block of `size` bytes that inflates to isize bytes whose CRC32 is crc
// CANVAS_TOOL_CHECK_CRC=1 (configuration of the executables, off by default): every place that inflates a BGZF block of a BAM holds the CRC32 of the inflated bytes against
// the word of the block's trailer (RFC 1952), and a block that fails is handled as one that does not inflate to its recorded size.  A block of ISIZE 0 is not inflated.
static inline bool bgzf_check_crc() { static const bool on = [] { const char* e = getenv("CANVAS_TOOL_CHECK_CRC"); return e && atoi(e) == 1; }(); return on; }
static inline bool bgzf_crc_ok(const void* data, size_t n, uint32_t want) { return (uint32_t)crc32(crc32(0L, Z_NULL, 0), (const Bytef*)data, (uInt)n) == want; }
// The BGZF block that starts at h, of which avail bytes are at hand.  0: these bytes are no BGZF block.  More than avail: that many bytes are needed to go on (12, then the
// extra field, then the whole block): get them and call again.  Otherwise b is filled and the value is the block's size.
static size_t bgzf_parse(const uint8_t* h, size_t avail, BgzfBlock& b) {
    if (avail < 12) return 12;
    if (h[0] != 31 || h[1] != 139 || h[2] != 8 || !(h[3] & 4)) return 0;
    const size_t xlen = le16(h + 10);
    if (avail < 12 + xlen) return 12 + xlen;
    long bsize = -1;
    for (size_t i = 0; i + 4 <= xlen;) { const uint8_t* s = h + 12 + i; const size_t slen = le16(s + 2); if (s[0] == 'B' && s[1] == 'C' && slen == 2 && i + 6 <= xlen) bsize = le16(s + 4); i += 4 + slen; }
    if (bsize < 0 || (size_t)bsize + 1 < 12 + xlen + 8) return 0;
    b.size = (size_t)bsize + 1;
    if (avail < b.size) return b.size;
    b.in = 12 + xlen; b.clen = b.size - b.in - 8; b.crc = le32(h + b.size - 8); b.isize = le32(h + b.size - 4);
    return b.isize <= 65536 ? b.size : 0;
}
// a BGZF file read as one stream.  When read() fails, `bad` tells a damaged file (a block that does not parse, does not inflate to its ISIZE or, with CANVAS_TOOL_CHECK_CRC=1,
// fails its CRC32; the file ending inside a block) from its clean end at a block boundary
struct Bgzf {
    FILE* f = nullptr; std::vector<uint8_t> raw = std::vector<uint8_t>(65536 + 16), block; size_t pos = 0; bool bad = false;
    bool open(const std::string& p) { f = fopen(p.c_str(), "rb"); return f != nullptr; }
    ~Bgzf() { if (f) fclose(f); }
    bool next_block() {
        BgzfBlock b; size_t have = 0, need = 12;
        while (need > have) {
            const size_t got = fread(raw.data() + have, 1, need - have, f);
            if (got != need - have) { bad = have + got > 0; return false; }
            have = need; need = bgzf_parse(raw.data(), have, b);
        }
        block.resize(need ? b.isize : 0); pos = 0;
        if (!need || (b.isize && !inflate_raw(raw.data() + b.in, b.clen, block.data(), b.isize))) bad = true;
        else if (b.isize && bgzf_check_crc() && !bgzf_crc_ok(block.data(), b.isize, b.crc)) bad = true;
        return !bad;
    }
    bool read(void* dst, size_t n) {
        uint8_t* d = (uint8_t*)dst;
        while (n) {
            if (pos >= block.size()) { do { if (!next_block()) return false; } while (block.empty()); }
            size_t k = std::min(n, block.size() - pos); memcpy(d, block.data() + pos, k); pos += k; d += k; n -= k;
        }
        return true;
    }
    bool seek_virtual(uint64_t voff) { if (fseeko(f, (off_t)(voff >> 16), SEEK_SET) != 0) return false; if (!next_block()) return false; pos = voff & 0xFFFF; return pos <= block.size(); }
};
// smallest virtual offset of a chunk of reference `ref` in the .bai (BamReader.Jump(ref, 0)); 0 = the reference has no reads
static bool bai_first_offset(const std::string& path, int ref, uint64_t& voff, bool& any) {
    FILE* f = fopen(path.c_str(), "rb"); if (!f) return false;
    auto rd = [&](void* p, size_t n) { return fread(p, 1, n, f) == n; };
    char magic[4]; int32_t nref;
    if (!rd(magic, 4) || memcmp(magic, "BAI\1", 4) != 0 || !rd(&nref, 4)) { fclose(f); return false; }
    any = false; voff = ~0ull;
    for (int r = 0; r < nref; r++) {
        int32_t nbin; if (!rd(&nbin, 4)) break;
        for (int b = 0; b < nbin; b++) {
            uint32_t bin; int32_t nchunk; if (!rd(&bin, 4) || !rd(&nchunk, 4)) { fclose(f); return false; }
            for (int c = 0; c < nchunk; c++) { uint64_t cb, ce; if (!rd(&cb, 8) || !rd(&ce, 8)) { fclose(f); return false; } if (r == ref && bin != 37450) { any = true; voff = std::min(voff, cb); } }
        }
        int32_t nintv; if (!rd(&nintv, 4)) break;
        if (fseeko(f, (off_t)nintv * 8, SEEK_CUR) != 0) break;
        if (r == ref) break;
    }
    fclose(f); return true;
}
struct BamHeader { std::vector<std::string> refNames; };
static bool read_bam_header(Bgzf& z, BamHeader& h) {
    char magic[4]; int32_t ltext, nref;
    if (!z.read(magic, 4) || memcmp(magic, "BAM\1", 4) != 0 || !z.read(&ltext, 4)) return false;
    { std::vector<char> t(ltext); if (ltext && !z.read(t.data(), ltext)) return false; }
    if (!z.read(&nref, 4)) return false;
    for (int r = 0; r < nref; r++) { int32_t ln, lref; if (!z.read(&ln, 4)) return false; std::vector<char> nm(ln); if (!z.read(nm.data(), ln) || !z.read(&lref, 4)) return false; h.refNames.push_back(nm.data()); }
    return true;
}
// A BAM opened at a chromosome: the header read, the chromosome's reference id found by name, the .bai there and read.  The steps run in this order and the first that
// fails is the answer; the tools word it themselves.  Ok: z stands behind the header, and voff is the first virtual offset of the chromosome if `any` of its reads exist.
enum class BamOpen { Ok, NotBam, NoSuchRef, NoIndex, BadIndex };
struct BamAt { Bgzf z; BamHeader h; int ref = -1; uint64_t voff = 0; bool any = false; };
static BamOpen bam_open_at(const std::string& bam, const std::string& chrom, BamAt& o) {
    if (!o.z.open(bam) || !read_bam_header(o.z, o.h)) return BamOpen::NotBam;
    const auto it = std::find(o.h.refNames.begin(), o.h.refNames.end(), chrom);
    if (it == o.h.refNames.end()) return BamOpen::NoSuchRef;
    o.ref = (int)(it - o.h.refNames.begin());
    FILE* f = fopen((bam + ".bai").c_str(), "rb"); if (!f) return BamOpen::NoIndex;
    fclose(f);
    return bai_first_offset(bam + ".bai", o.ref, o.voff, o.any) ? BamOpen::Ok : BamOpen::BadIndex;
}
// the 32 fixed bytes of an alignment record (they follow its block_size word)
struct BamFixed {
    int32_t refID, pos; uint8_t l_read_name, mapq; uint16_t n_cigar, flag; int32_t l_seq, next_refID, next_pos, tlen;
    bool decode(const uint8_t* r, int32_t block_size) {
        if (block_size < 32) return false;
        refID = (int32_t)le32(r); pos = (int32_t)le32(r + 4); l_read_name = r[8]; mapq = r[9]; n_cigar = le16(r + 12); flag = le16(r + 14);
        l_seq = (int32_t)le32(r + 16); next_refID = (int32_t)le32(r + 20); next_pos = (int32_t)le32(r + 24); tlen = (int32_t)le32(r + 28);
        return true;
    }
    // the fixed fields, the name and the CIGAR lie inside block_size
    bool name_and_cigar_fit(int32_t block_size) const { return 32 + (int64_t)l_read_name + 4 * (int64_t)n_cigar <= block_size; }
};
// the next record of the stream into rec, its fixed fields into a.  false: the stream's end, or, with z.bad set, a damaged block or a record whose block_size does not
// hold its fixed fields, name and CIGAR
static bool read_bam_record(Bgzf& z, std::vector<uint8_t>& rec, BamFixed& a) {
    int32_t bs; if (!z.read(&bs, 4)) return false;
    rec.resize((size_t)std::max(bs, 0));
    if (bs >= 32 && !z.read(rec.data(), bs)) return false;
    if (!a.decode(rec.data(), bs) || !a.name_and_cigar_fit(bs)) z.bad = true;
    return !z.bad;
}
