// Runs the framing rules of canvas_amd/csrc/bam_frame.hpp on the host, for tests/test_bam_frame_host.py: built with -fsanitize=address,undefined, so that a byte read
// outside the chunk ends the program.
// Input file: uint64 nbytes, uint64 first, int32 kind, ref_id, paired_end, sorted, int64 passed, last (the carried sortedness state), nbytes of record bytes.  The chunk
// goes into a heap buffer of exactly nbytes.
// Output: "rec OFFSET CLASS" for every record the chain classifies, with the sortedness rule applied through the running maximum as the header states it;
// "end USED PASSED LAST AGAINST" (the offset the chain stopped at, the state, the position an unsorted record was compared with); "shape" and every offset of the chunk
// that passes the shape test.
#include <cstdio>
#include <cstring>
#include <memory>
#include "../canvas_amd/csrc/bam_frame.hpp"

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: bam_frame_host CASE_FILE\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    uint64_t head[2]; int32_t r[4]; int64_t st[2];
    if (!f || fread(head, 8, 2, f) != 2 || fread(r, 4, 4, f) != 4 || fread(st, 8, 2, f) != 2) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    const uint64_t nbytes = head[0], first = head[1];
    std::unique_ptr<uint8_t[]> rec(new uint8_t[nbytes]);
    if (fread(rec.get(), 1, nbytes, f) != nbytes) { fprintf(stderr, "%s is shorter than its header says\n", argv[1]); return 2; }
    fclose(f);
    const BamFrameRule rule{r[0], r[1], r[2], r[3]};
    int64_t passed = st[0], running = st[1], against = 0;
    uint64_t at = first;
    for (int32_t bs; bam_frame_whole(rec.get(), nbytes, at, bs);) {
        int32_t pos; bool compared;
        int cls = bam_frame_classify(rec.get(), nbytes, at, rule, &pos, &compared);
        if (compared) {
            if (passed > 0 && pos < running) { cls = BAM_FRAME_UNSORTED; against = running; }
            else { running = passed > 0 && running > pos ? running : pos; passed++; }
        }
        printf("rec %llu %d\n", (unsigned long long)at, cls);
        if (cls == BAM_FRAME_STOP || cls == BAM_FRAME_MALFORMED || cls == BAM_FRAME_UNSORTED) break;
        at += 4ull + (uint64_t)(uint32_t)bs;
        if (cls == BAM_FRAME_TAKE_AND_STOP) break;
    }
    printf("end %llu %lld %lld %lld\n", (unsigned long long)at, (long long)passed, (long long)running, (long long)against);
    printf("shape");
    for (uint64_t o = 0; o + 36 <= nbytes; o++) if (bam_frame_shape(rec.get() + o, nbytes - o)) printf(" %llu", (unsigned long long)o);
    printf("\n");
    return 0;
}
