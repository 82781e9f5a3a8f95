// Runs the CRC32 arithmetic of canvas_amd/csrc/crc32_block.hpp on the host, for tests/test_crc32_host.py: built with -fsanitize=address,undefined, so that a byte read
// outside a case ends the program.
// Input file: uint32 ncases, uint32 npairs, npairs x (uint32 value, uint32 nbytes), then per case uint32 n and n bytes.  Every case goes into a heap buffer of exactly n bytes.
// Output: "shift V" per pair (value * x^(8 nbytes) mod P); per case "case N" and one value for every slice size the kernel may use (CRC32_SLICE_BYTES is the only one),
// then the same block as a single slice; "slices" and the sizes, first.
#include <cstdio>
#include <memory>
#include <vector>
#include "../canvas_amd/csrc/crc32_block.hpp"

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: crc32_host CASE_FILE\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    uint32_t head[2];
    if (!f || fread(head, 4, 2, f) != 2) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::vector<uint32_t> T(CRC32_TABLE_WORDS);
    crc32_fill_tables(T.data());
    const uint32_t sizes[] = {CRC32_SLICE_BYTES};
    printf("slices");
    for (uint32_t s : sizes) printf(" %u", s);
    printf("\n");
    for (uint32_t i = 0; i < head[1]; i++) {
        uint32_t pair[2];
        if (fread(pair, 4, 2, f) != 2) { fprintf(stderr, "%s is shorter than its header says\n", argv[1]); return 2; }
        printf("shift %u\n", crc32_shift(pair[0], pair[1]));
    }
    for (uint32_t i = 0; i < head[0]; i++) {
        uint32_t n;
        if (fread(&n, 4, 1, f) != 1) { fprintf(stderr, "%s is shorter than its header says\n", argv[1]); return 2; }
        std::unique_ptr<uint8_t[]> buf(new uint8_t[n]);
        if (fread(buf.get(), 1, n, f) != n) { fprintf(stderr, "%s is shorter than its header says\n", argv[1]); return 2; }
        printf("case %u", n);
        for (uint32_t s : sizes) printf(" %u", crc32_sliced(buf.get(), n, s, T.data()));
        printf(" %u\n", crc32_sliced(buf.get(), n, n ? n : 1u, T.data()));
    }
    fclose(f);
    return 0;
}
