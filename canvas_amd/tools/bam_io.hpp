// BGZF / BAM / BAI reading shared by the drop-in tools that open alignments (CanvasBin, CanvasSNV).  Included behind tool_common.hpp, inside one translation unit.
#pragma once
#include <zlib.h>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <string>
#include <vector>

// ---------------------------------------------------------------- BGZF / BAM / BAI
struct Bgzf {
    FILE* f = nullptr; std::vector<uint8_t> block; size_t pos = 0; int64_t blockAddr = 0; bool eof = false;
    bool open(const std::string& p) { f = fopen(p.c_str(), "rb"); return f != nullptr; }
    ~Bgzf() { if (f) fclose(f); }
    bool next_block() {
        blockAddr = ftello(f);
        uint8_t h[18];
        if (fread(h, 1, 18, f) != 18) { eof = true; return false; }
        if (h[0] != 31 || h[1] != 139 || h[2] != 8 || !(h[3] & 4)) return false;
        const int xlen = h[10] | (h[11] << 8);
        std::vector<uint8_t> extra(xlen);
        memcpy(extra.data(), h + 12, std::min(6, xlen));
        if (xlen > 6 && fread(extra.data() + 6, 1, xlen - 6, f) != (size_t)(xlen - 6)) return false;
        int bsize = -1;
        for (int i = 0; i + 4 <= xlen;) { int slen = extra[i + 2] | (extra[i + 3] << 8); if (extra[i] == 'B' && extra[i + 1] == 'C' && slen == 2) bsize = extra[i + 4] | (extra[i + 5] << 8); i += 4 + slen; }
        if (bsize < 0) return false;
        const int clen = bsize - xlen - 19;
        std::vector<uint8_t> comp(clen + 8);
        if (fread(comp.data(), 1, clen + 8, f) != (size_t)(clen + 8)) return false;
        const uint32_t isize = comp[clen + 4] | (comp[clen + 5] << 8) | (comp[clen + 6] << 16) | ((uint32_t)comp[clen + 7] << 24);
        block.resize(isize); pos = 0;
        if (isize == 0) return true;
        z_stream zs; memset(&zs, 0, sizeof zs);
        if (inflateInit2(&zs, -15) != Z_OK) return false;
        zs.next_in = comp.data(); zs.avail_in = clen; zs.next_out = block.data(); zs.avail_out = isize;
        int rc = inflate(&zs, Z_FINISH); inflateEnd(&zs);
        return rc == Z_STREAM_END;
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
