// Runs the record decoder of canvas_amd/csrc/bam_record.hpp on the host, for tests/test_bam_record_host.py: built with -fsanitize=address,undefined, so that a byte
// read outside the chunk ends the program.
// Input file: uint64 nbytes, uint64 noffsets, the offsets (uint64 each), nbytes of record bytes.  The chunk goes into a heap buffer of exactly nbytes.
// One line per offset: "malformed", or "ok" and the eleven fields, whether bam_rec_holds_seq holds, and the first and last byte of the name, the CIGAR, the bases and
// the qualities as the accessors find them (-1 -1 for a part that is empty, or, for bases and qualities, not vouched for).
#include <cstdio>
#include <memory>
#include <vector>
#include "../canvas_amd/csrc/bam_record.hpp"

static void ends(const uint8_t* rec, uint64_t at, uint64_t n) {
    if (n == 0) { printf(" -1 -1"); return; }
    printf(" %u %u", bam_ld8(rec, at), bam_ld8(rec, at + n - 1));
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: bam_record_host CHUNK_FILE\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    uint64_t head[2];
    if (!f || fread(head, 8, 2, f) != 2) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    const uint64_t nbytes = head[0], noffs = head[1];
    std::vector<uint64_t> offs(noffs);
    std::unique_ptr<uint8_t[]> rec(new uint8_t[nbytes]);
    if (fread(offs.data(), 8, noffs, f) != noffs || fread(rec.get(), 1, nbytes, f) != nbytes) { fprintf(stderr, "%s is shorter than its header says\n", argv[1]); return 2; }
    fclose(f);
    for (const uint64_t off : offs) {
        BamRec b;
        if (!bam_rec_load(rec.get(), nbytes, off, b)) { printf("malformed\n"); continue; }
        const bool seq = bam_rec_holds_seq(b);
        printf("ok %d %d %d %u %u %u %u %d %d %d %d %d", b.block_size, b.refID, b.pos, b.l_read_name, b.mapq, b.n_cigar_op, b.flag, b.l_seq, b.next_refID, b.next_pos, b.tlen, seq ? 1 : 0);
        ends(rec.get(), bam_name_at(off), b.l_read_name);
        ends(rec.get(), bam_cigar_at(off, b.l_read_name), 4ull * b.n_cigar_op);
        ends(rec.get(), bam_seq_at(off, b.l_read_name, b.n_cigar_op), seq ? ((uint64_t)b.l_seq + 1) / 2 : 0);
        ends(rec.get(), bam_qual_at(off, b.l_read_name, b.n_cigar_op, b.l_seq), seq ? (uint64_t)b.l_seq : 0);
        printf("\n");
    }
    return 0;
}
