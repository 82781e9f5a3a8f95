// Drop-in FlagUniqueKmers executable on top of the C ABI: Tools/FlagUniqueKmers (Program.cs:7-21, KmerChecker.Main :231-298), the tool that makes kmer.fa.
//   FlagUniqueKmers $InputFASTA $OutputFASTA [--table-gb X]
// Fewer than two arguments: the reference's two usage lines on stderr, exit code 0 (Program.cs:13-18), no GPU context.  An unreadable input or an unwritable output: a
// message and exit code 1.  The flags come from canvas_flag_unique_kmers, the letter case from canvas_fasta_case_from_mask; there is no host implementation of either.
// File layout (Isas.SequencingFiles' FastaReader / FastaWriter are not part of the reference tree): an entry's name is what follows '>' up to the first blank
// or tab; '\r' and line folds of the input are dropped; the output is '>' + name, '\n', the whole sequence on ONE line, '\n' — the layout CanvasBin maps without a copy
// (canvas_bin_main.cpp: read_fasta; the scan both share: fast_io.hpp); an empty entry is its header and an empty line.
// --table-gb X bounds the working table of the device (canvas_flag_unique_kmers' max_table_bytes); the output does not depend on it.
#include "tool_common.hpp"
#include <memory>
using namespace tool;

int main(int argc, char** argv) {
    std::vector<std::string> pos; double tableGb = 0; bool badOpt = false;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        if (a == "--table-gb") { if (i + 1 < argc) tableGb = atof(argv[++i]); else badOpt = true; }
        else if (a.rfind("--table-gb=", 0) == 0) tableGb = atof(a.c_str() + 11);
        else pos.push_back(a);
    }
    if (pos.size() < 2) {
        fprintf(stderr, "Usage info:\n");
        fprintf(stderr, "  FlagUniqueKmers $InputFASTA $OutputFASTA\n");
        return 0;
    }
    if (badOpt || tableGb < 0 || pos.size() > 2) { fprintf(stderr, "FlagUniqueKmers: expected $InputFASTA $OutputFASTA [--table-gb X]\n"); return 1; }
    const std::string inFile = pos[0], outFile = pos[1];
    Phases ph("FlagUniqueKmers");
    const double t0 = Phases::now();
    MappedFile mf;
    if (!mf.open(inFile, true)) { fprintf(stderr, "FlagUniqueKmers: cannot read %s\n", inFile.c_str()); return 1; }
    const int fd = ::open(outFile.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (fd < 0) { fprintf(stderr, "FlagUniqueKmers: cannot write %s\n", outFile.c_str()); return 1; }
    AsyncCtx actx;                                              // the context comes up while the file is scanned

    const std::vector<FastaEntry> ents = scan_fasta(mf);
    const int nchr = (int)ents.size();
    // every contig starts at a multiple of 64 bytes of one staging buffer: its mask words then line up with the buffer's own (word i = bytes 64 i .. 64 i + 63), so
    // the case of the whole genome is set by ONE canvas_fasta_case_from_mask call over the buffer; the padding bytes are 0, no letters
    int64_t words = 0; std::vector<int64_t> at((size_t)nchr);                // offset of every entry in the staging buffer
    for (int c = 0; c < nchr; c++) {
        if (ents[(size_t)c].len > 0x7FFFFFFFll) { fprintf(stderr, "FlagUniqueKmers: entry %s is longer than 2^31 - 1 bases\n", ents[(size_t)c].name.c_str()); return 1; }
        at[(size_t)c] = words * 64; words += (ents[(size_t)c].len + 63) / 64;
    }
    std::vector<uint8_t> stage((size_t)words * 64, 0);
    parallel_for(nchr, [&](int64_t k) { unfold(mf.p + ents[(size_t)k].seq, mf.p + ents[(size_t)k].end, (char*)stage.data() + at[(size_t)k]); });
    ph.mark("read");
    const double t1 = Phases::now();

    int64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (auto& e : ents) stats[0] += e.len;
    if (words > 0) {
        canvas_ctx* ctx = actx.require("FlagUniqueKmers"); if (!ctx) return 1;
        Dev dBases(ctx, words * 64), dMask(ctx, words * 8);
        if (!dBases.p || !dMask.p) { fprintf(stderr, "FlagUniqueKmers: cannot allocate %lld bytes of device memory\n", (long long)(words * 72)); return 1; }
        TOOL_TRY(ctx, canvas_memcpy_h2d(ctx, dBases.p, stage.data(), words * 64));
        std::vector<const uint8_t*> pb((size_t)nchr); std::vector<uint64_t*> pm((size_t)nchr); std::vector<int64_t> lens((size_t)nchr);
        for (int c = 0; c < nchr; c++) { pb[(size_t)c] = dBases.as<uint8_t>() + at[(size_t)c]; pm[(size_t)c] = dMask.as<uint64_t>() + at[(size_t)c] / 64; lens[(size_t)c] = ents[(size_t)c].len; }
        TOOL_TRY(ctx, canvas_flag_unique_kmers(ctx, nchr, pb.data(), lens.data(), pm.data(), (int64_t)(tableGb * 1073741824.0), stats));
        TOOL_TRY(ctx, canvas_fasta_case_from_mask(ctx, dBases.as<uint8_t>(), words * 64, dMask.as<uint64_t>()));
        TOOL_TRY(ctx, canvas_memcpy_d2h(ctx, stage.data(), dBases.p, words * 64));
    }
    ph.mark("device");
    const double t2 = Phases::now();

    // '>' name '\n' sequence '\n' per entry, every entry written at its own offset on several threads
    std::vector<int64_t> off((size_t)nchr + 1, 0);
    for (int c = 0; c < nchr; c++) off[(size_t)c + 1] = off[(size_t)c] + 1 + (int64_t)ents[(size_t)c].name.size() + 1 + ents[(size_t)c].len + 1;
    std::atomic<bool> ok(true);
    auto put = [&](const void* src, size_t n, int64_t at) { const char* s = (const char*)src; while (n) { const ssize_t k = pwrite(fd, s, n, (off_t)at); if (k <= 0) { ok = false; return; } s += k; n -= (size_t)k; at += k; } };
    parallel_for(nchr, [&](int64_t k) {
        const FastaEntry& e = ents[(size_t)k];
        const std::string hdr = ">" + e.name + "\n";
        put(hdr.data(), hdr.size(), off[(size_t)k]);
        put(stage.data() + at[(size_t)k], (size_t)e.len, off[(size_t)k] + (int64_t)hdr.size());
        put("\n", 1, off[(size_t)k] + (int64_t)hdr.size() + e.len);
    });
    if (::close(fd) != 0 || !ok) { fprintf(stderr, "FlagUniqueKmers: cannot write %s\n", outFile.c_str()); return 1; }
    ph.mark("write");
    const double t3 = Phases::now();
    printf("FlagUniqueKmers: %d entries, %lld positions, %lld keyed, %lld unique, %lld passes (table %lld bytes, longest probe %lld); read %.3f s, device %.3f s, write %.3f s\n", nchr,
           (long long)stats[0], (long long)stats[1], (long long)stats[2], (long long)stats[3], (long long)stats[6], (long long)stats[5], t1 - t0, t2 - t1, t3 - t2);
    return finish(ph, 0);
}
