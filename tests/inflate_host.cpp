// Runs the deflate decoder and the BGZF block walk of canvas_amd/csrc/inflate_block.hpp on the host, for tests/test_inflate_host.py: built with
// -fsanitize=address,undefined, so that a byte read outside a stream or written outside a destination ends the program.
//   inflate_host inflate IN OUT     IN: uint64 ncases, then per case uint32 src_bytes, uint32 out_bytes and the stream.  Every stream goes into a heap buffer of exactly
//                                   src_bytes and is inflated into one of exactly out_bytes.  OUT: per case int32 status, then the out_bytes bytes where it is 0.
//   inflate_host scan FILE AT MAX_OUT CAPACITY     FILE into a heap buffer of exactly its size; prints the four info words, then one line per block.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
#include "../canvas_amd/csrc/inflate_block.hpp"

static bool read_all(const char* path, std::vector<uint8_t>& v) {
    FILE* f = fopen(path, "rb"); if (!f) return false;
    fseek(f, 0, SEEK_END); const long n = ftell(f); fseek(f, 0, SEEK_SET);
    v.resize((size_t)n);
    const bool ok = n == 0 || fread(v.data(), 1, (size_t)n, f) == (size_t)n;
    fclose(f); return ok;
}

int main(int argc, char** argv) {
    static_assert(sizeof(canvas_bgzf_block) == 24, "canvas_bgzf_block is 24 bytes");
    if (argc == 4 && std::string(argv[1]) == "inflate") {
        std::vector<uint8_t> in; if (!read_all(argv[2], in)) { fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
        FILE* out = fopen(argv[3], "wb"); if (!out) { fprintf(stderr, "cannot write %s\n", argv[3]); return 2; }
        size_t at = 8; uint64_t ncases; memcpy(&ncases, in.data(), 8);
        for (uint64_t c = 0; c < ncases; c++) {
            uint32_t head[2]; memcpy(head, in.data() + at, 8); at += 8;
            std::unique_ptr<uint8_t[]> src(new uint8_t[head[0]]), dst(new uint8_t[head[1]]);      // exactly their sizes: the sanitizer's red zones start right behind
            memcpy(src.get(), in.data() + at, head[0]); at += head[0];
            const canvas_bgzf_block b = {0, 0, head[0], head[1]};
            const int32_t st = inflate_block_host(src.get(), head[0], dst.get(), head[1], b);
            fwrite(&st, 4, 1, out);
            if (st == CANVAS_INFLATE_OK) fwrite(dst.get(), 1, head[1], out);
        }
        fclose(out);
        return 0;
    }
    if (argc == 6 && std::string(argv[1]) == "scan") {
        std::vector<uint8_t> file; if (!read_all(argv[2], file)) { fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
        std::unique_ptr<uint8_t[]> bytes(new uint8_t[file.size()]); if (!file.empty()) memcpy(bytes.get(), file.data(), file.size());
        const int64_t capacity = atoll(argv[5]);
        std::unique_ptr<canvas_bgzf_block[]> blocks(new canvas_bgzf_block[(size_t)capacity]);
        int64_t info[4];
        bgzf_scan_blocks(bytes.get(), file.size(), strtoull(argv[3], nullptr, 10), strtoull(argv[4], nullptr, 10), blocks.get(), capacity, info);
        printf("%lld %lld %lld %lld\n", (long long)info[0], (long long)info[1], (long long)info[2], (long long)info[3]);
        for (int64_t i = 0; i < info[0]; i++)
            printf("%llu %llu %u %u\n", (unsigned long long)blocks[i].src_offset, (unsigned long long)blocks[i].dst_offset, blocks[i].src_bytes, blocks[i].out_bytes);
        return 0;
    }
    fprintf(stderr, "usage: inflate_host inflate IN OUT | inflate_host scan FILE AT MAX_OUT CAPACITY\n");
    return 2;
}
