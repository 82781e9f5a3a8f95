// Drop-in CanvasSNV executable on top of the C ABI: command line, files and exit codes of CanvasSNV/Program.cs + SNVReviewer.cs.
//   CanvasSNV -c chr1 -v S.vcf[.gz] -b S.bam -o chr1.vaf.gz [-n sample] [-i] [-q minMapQ] [-s]
// LoadVariants (SNVReviewer.cs:86-152) and the two writers (:276-365) are host code as in the reference; ProcessBamFile + ProcessReadBases (:172-271) is
// canvas_snv_count.  The host's part of the pileup is to INFLATE: the BAM file is mapped, the BGZF blocks of a chunk are inflated on the worker threads straight into
// a pinned staging buffer, the block_size chain is walked once for the byte offset of every record (with the shape checks that need only the fixed fields), and the
// chunk travels as raw record bytes.  Two staging buffers: chunk k + 1 is inflated while chunk k is uploaded and counted.  (The loop: tool_common.hpp, BamChunkLoop.)
// Not built: -c histogram / -c regionhistogram (HistogramVF.cs, developer modes): exit code 1 with a message.  Input that is not sorted by position (VCF records of the
// chromosome, BAM records) is refused with exit code 1: the reference's answer for it depends on its scan pointer, and this library has no host pileup to reproduce it.
// The reference's VcfReader (Isas.SequencingFiles) is not part of the reference tree: records are parsed by the VCF specification.
#include "tool_common.hpp"
#include <memory>
using namespace tool;

struct Site { int32_t pos; std::string ref, alt; };

// the sample columns of the #CHROM line; false: the file cannot be read
static bool vcf_samples(const std::string& path, std::vector<std::string>& samples) {
    GzReader rd(path); if (!rd.ok()) return false;
    std::string row;
    while (rd.line(row)) { if (row.empty()) continue; if (row[0] != '#') break; if (row.rfind("#CHROM", 0) == 0) { auto h = split_tab(row); for (size_t i = 9; i < h.size(); i++) samples.push_back(h[i]); break; } }
    return true;
}
static bool het(const std::string& g) { return g == "0/1" || g == "1/0" || g == "0|1" || g == "1|0"; }
// decimal.Parse(GQX) < cutoff; what decimal.Parse refuses is the reference's FormatException
static bool parse_decimal(const std::string& s, double& v) { if (s.empty()) return false; char* e = nullptr; v = strtod(s.c_str(), &e); return e && *e == 0; }

// LoadVariants; 0 ok, otherwise the exit code (message printed)
static int load_variants(const std::string& path, const std::string& chrom, int sampleIndex, bool isSomatic, std::vector<Site>& sites, long& countThis) {
    std::string data; if (!read_gz_all(path, data)) { fprintf(stderr, "CanvasSNV: cannot read %s\n", path.c_str()); return 1; }
    countThis = 0;
    const char* p = data.data(); const char* end = p + data.size();
    while (p < end) {
        const char* e = (const char*)memchr(p, '\n', (size_t)(end - p)); if (!e) e = end;
        const char* le = e; while (le > p && le[-1] == '\r') le--;
        const char* next = e < end ? e + 1 : end;
        if (le == p || *p == '#') { p = next; continue; }
        const char* t = (const char*)memchr(p, '\t', (size_t)(le - p));
        const size_t nameLen = t ? (size_t)(t - p) : (size_t)(le - p);
        if (nameLen != chrom.size() || memcmp(p, chrom.data(), nameLen) != 0) { if (countThis > 0) break; p = next; continue; }
        countThis++;
        auto c = split_tab(std::string(p, (size_t)(le - p)));
        p = next;
        if (c.size() < 5) continue;
        if (c[3].size() != 1 || c[4].size() != 1) continue;                    // single-allele SNVs only (a second ALT brings a comma: length > 1)
        if (c.size() > 9) {
            if ((size_t)(9 + sampleIndex) >= c.size()) { fprintf(stderr, "CanvasSNV: VCF record at %s:%s has no column for the sample\n", c[0].c_str(), c[1].c_str()); return 255; }
            const VcfFormat fmt(c[8], c[9 + sampleIndex]);
            const std::string* ft = fmt.find("FT");
            if (c[6] != "PASS" || (ft && *ft != "PASS")) continue;
            const std::string* gt = fmt.find("GT"); if (!gt) continue;
            if (isSomatic) {
                if (!het(*gt)) continue;
                if (const std::string* gqx = fmt.find("GQX")) {
                    if (*gqx == ".") continue;
                    double v; if (!parse_decimal(*gqx, v)) { fprintf(stderr, "System.FormatException: GQX '%s' at %s:%s is not a number\n", gqx->c_str(), c[0].c_str(), c[1].c_str()); return 255; }
                    if (v < 30) continue;
                }
            } else if (!(het(*gt) || *gt == "1/1" || *gt == "1|1")) continue;
        }
        Site s; s.pos = atoi(c[1].c_str()); s.ref = c[3]; s.alt = c[4];
        if (!sites.empty() && s.pos < sites.back().pos) { fprintf(stderr, "CanvasSNV (MI355X): %s is not sorted by position: %s:%d follows %s:%d (unsorted input is refused)\n", path.c_str(), chrom.c_str(), s.pos, chrom.c_str(), sites.back().pos); return 1; }
        sites.push_back(s);
    }
    return 0;
}

static inline uint8_t allele_code(char ch) { const char* t = "=ACMGRSVTWYHKDBN"; const char* f = ch ? strchr(t, ch) : nullptr; return f ? (uint8_t)(f - t) : (uint8_t)0xFF; }
static int b_allele_preference(const std::string& a) { if (a.size() == 1) switch (tolower((unsigned char)a[0])) { case 'a': return 0; case 't': return 1; case 'g': return 2; case 'c': return 3; } return -1; }

// double.ToString() of .NET Core 2.x; format_g keeps fixed notation down to 1E-05 where .NET already switches (scale < -3): that one decade is written here
static std::string format_double(double v) {
    std::string d; int scale; sig_digits(v, 15, d, scale);
    if (d.empty() || scale != -4) return format_g(v, 15);
    std::string out = std::signbit(v) ? "-" : ""; out.push_back(d[0]); if (d.size() > 1) { out.push_back('.'); out += d.substr(1); }
    return out + "E-05";
}

int main(int argc, char** argv) {
    printf(">>>Command-line arguments:\n"); for (int i = 1; i < argc; i++) printf("%s ", argv[i]); printf("\n");   // Utilities.LogCommandLine
    Phases ph("CanvasSNV");
    std::vector<Opt> opts = {{"c", "chromosome", true}, {"v", "vcfPath", true}, {"b", "bamPath", true}, {"o", "outputPath", true}, {"n", "sampleName", true},
                             {"i", "isDbSnpVcf", false}, {"q", "minMapQ", true}, {"s", "isSomatic", false}, {"h", "help", false}};
    Parsed a = parse(argc, argv, opts);
    auto help = []() { printf("Usage: CanvasSNV.exe [OPTIONS]+\nParses bam file to derive allele counts.\n\nOptions:\n  -c, --chromosome=VALUE  -v, --vcfPath=VALUE  -b, --bamPath=VALUE  -o, --outputPath=VALUE\n"
                              "  -n, --sampleName=VALUE  -i, --isDbSnpVcf  -q, --minMapQ=VALUE  -s, --isSomatic  -h, --help\n"); };
    if (!a.extra.empty()) { printf("* Error: I don't understand the argument '%s'\n", a.extra[0].c_str()); help(); return 0; }
    if (a.has("help") || a.get("chromosome").empty() || a.get("outputPath").empty()) { help(); return 0; }
    const std::string chrom = a.get("chromosome"), vcfPath = a.get("vcfPath"), bamPath = a.get("bamPath"), outPath = a.get("outputPath"), sampleName = a.get("sampleName");
    const bool isDbSnp = a.has("isDbSnpVcf"), isSomatic = a.has("isSomatic");
    int minMapQ = 0;
    if (a.has("minMapQ")) { char* e = nullptr; const std::string q = a.get("minMapQ"); minMapQ = (int)strtol(q.c_str(), &e, 10); if (q.empty() || !e || *e) { fprintf(stderr, "System.FormatException: minMapQ '%s'\n", q.c_str()); return 255; } }
    // (before the file checks: in these modes -v names a folder and -b is not a BAM, Program.cs:98-106)
    { std::string lo = chrom; for (auto& ch : lo) ch = (char)tolower((unsigned char)ch);
      if (lo == "histogram" || lo == "regionhistogram") { fprintf(stderr, "CanvasSNV (MI355X): -c %s (HistogramVF developer mode) is not supported by this build\n", chrom.c_str()); return 1; } }
    if (vcfPath.empty() || !file_exists(vcfPath)) { printf("CanvasSNV.exe: File %s does not exist! Exiting.\n", vcfPath.c_str()); return 1; }
    if (bamPath.empty() || !file_exists(bamPath)) { printf("CanvasSNV.exe: File %s does not exist! Exiting.\n", bamPath.c_str()); return 1; }

    // ---- everything the reference ends with an exception for, before the context exists
    printf("Loading variants of interest from %s\n", vcfPath.c_str());
    int sampleIndex = 0;
    {
        std::vector<std::string> samples;
        if (!vcf_samples(vcfPath, samples)) { fprintf(stderr, "CanvasSNV: cannot read %s\n", vcfPath.c_str()); return 1; }
        if (!sampleName.empty() && !isDbSnp) {
            auto it = std::find(samples.begin(), samples.end(), sampleName);
            if (it == samples.end()) { fprintf(stderr, "System.ArgumentException: File '%s' should contain one genotypes column corresponding to sample %s\n", vcfPath.c_str(), sampleName.c_str()); return 255; }
            sampleIndex = (int)(it - samples.begin());
        } else if (samples.size() > 1) { fprintf(stderr, "System.ArgumentException: File '%s' contains >1 samples, name for a sample of interest must be provided\n", vcfPath.c_str()); return 255; }
    }
    int refId = -1; uint64_t voff = 0; bool anyReads = false;
    { BamAt b;
      switch (bam_open_at(bamPath, chrom, b)) {
          case BamOpen::Ok: break;
          case BamOpen::NotBam: fprintf(stderr, "CanvasSNV: %s is not a BAM file\n", bamPath.c_str()); return 1;
          case BamOpen::NoSuchRef: fprintf(stderr, "System.ArgumentException: Error: Chromosome name '%s' does not match bam file at '%s'\n", chrom.c_str(), bamPath.c_str()); return 255;
          case BamOpen::NoIndex: fprintf(stderr, "Fatal error: Bam index not found at %s.bai\n", bamPath.c_str()); return 255;
          case BamOpen::BadIndex: fprintf(stderr, "CanvasSNV: cannot read %s.bai\n", bamPath.c_str()); return 1;
      }
      refId = b.ref; voff = b.voff; anyReads = b.any; }
    ph.mark("startup");

    AsyncCtx actx;                                               // the context comes up while the VCF is parsed
    std::vector<Site> sites; long countThis = 0;
    if (int rc = load_variants(vcfPath, chrom, sampleIndex, isSomatic, sites, countThis)) return rc;
    printf("Retained %zu variants, out of %ld records for %s\n", sites.size(), countThis, chrom.c_str());
    const int32_t nsites = (int32_t)sites.size();
    std::vector<int32_t> sitePos((size_t)nsites + 1), cntRef((size_t)nsites + 1, 0), cntAlt((size_t)nsites + 1, 0);
    std::vector<uint8_t> siteRef((size_t)nsites + 1), siteAlt((size_t)nsites + 1);
    for (int32_t i = 0; i < nsites; i++) { sitePos[i] = sites[i].pos; siteRef[i] = allele_code(sites[i].ref[0]); siteAlt[i] = allele_code(sites[i].alt[0]); }
    ph.mark("vcf");

    // ---- the pileup
    printf("Looping over bam records from %s\nJump to refid %d %s\n", bamPath.c_str(), refId, chrom.c_str());
    const double tLoop0 = Phases::now();
    BamChunkLoop loop; loop.tool = "CanvasSNV"; loop.bam = bamPath; loop.voff = voff; loop.profile = "snv_count"; loop.chunk_bytes_from("CANVAS_SNV_CHUNK_BYTES");
    canvas_ctx* ctx = nullptr;
    if (anyReads && nsites > 0) {          // (no site: the reference leaves its loop at the first read that passes the filters; no read: nothing to count)
        std::unique_ptr<Dev> dPos, dRef, dAlt, dCr, dCa;
        int32_t lastPos = -1;
        loop.carried_pos = [&](int32_t p) { lastPos = p; };      // (framed on the device: the position an unsorted read follows, for the message below)
        const int rc = loop.run(actx, ctx, tLoop0,
            [&](canvas_ctx* c) -> int {
                dPos.reset(new Dev(c, ((int64_t)nsites + 1) * 4)); dRef.reset(new Dev(c, nsites + 1)); dAlt.reset(new Dev(c, nsites + 1));
                dCr.reset(new Dev(c, ((int64_t)nsites + 1) * 4)); dCa.reset(new Dev(c, ((int64_t)nsites + 1) * 4));
                if (!dPos->p || !dRef->p || !dAlt->p || !dCr->p || !dCa->p) { fprintf(stderr, "CanvasSNV: device allocation failed: %s\n", canvas_last_error(c)); return 1; }
                TOOL_TRY(c, canvas_memcpy_h2d(c, dPos->p, sitePos.data(), (int64_t)nsites * 4)); TOOL_TRY(c, canvas_memcpy_h2d(c, dRef->p, siteRef.data(), nsites)); TOOL_TRY(c, canvas_memcpy_h2d(c, dAlt->p, siteAlt.data(), nsites));
                TOOL_TRY(c, canvas_memcpy_h2d(c, dCr->p, cntRef.data(), (int64_t)nsites * 4)); TOOL_TRY(c, canvas_memcpy_h2d(c, dCa->p, cntAlt.data(), (int64_t)nsites * 4));
                return 0;
            },
            [&](const uint8_t* r, const BamFixed& fx, int32_t bs) -> BamFrame {
                const int32_t rid = fx.refID, pos = fx.pos, lseq = fx.l_seq; const uint32_t lname = fx.l_read_name, ncig = fx.n_cigar;
                if (lseq < 0 || 32ull + lname + 4ull * ncig + ((uint64_t)lseq + 1) / 2 + (uint64_t)lseq > (uint64_t)bs) { fprintf(stderr, "CanvasSNV: %s: malformed alignment record at position %d (its name, CIGAR and bases do not fit its block_size)\n", bamPath.c_str(), pos); return BamFrame::Fail; }
                if (rid < 0 || pos < 0 || rid > refId) return BamFrame::Stop;                 // past the chromosome of interest
                if (rid != refId) return BamFrame::Skip;
                if (pos < lastPos) { fprintf(stderr, "CanvasSNV (MI355X): %s is not sorted by position: read '%.*s' at %s:%d follows position %d (unsorted input is refused)\n", bamPath.c_str(), (int)(lname ? lname - 1 : 0), (const char*)(r + 32), chrom.c_str(), pos + 1, lastPos + 1); return BamFrame::Fail; }
                lastPos = pos; return BamFrame::Take;
            },
            [&](void* dRec, uint64_t used, void* dOff, int64_t nrec) -> int32_t {
                return canvas_snv_count(ctx, (const uint8_t*)dRec, used, (const uint64_t*)dOff, nrec, refId, minMapQ, 20, dPos->as<int32_t>(), dRef->as<uint8_t>(), dAlt->as<uint8_t>(),
                                        nsites, dCr->as<int32_t>(), dCa->as<int32_t>(), nullptr);
            },
            canvas_bam_frame_rule{CANVAS_BAM_FRAME_SNV, refId, 0, 0});
        if (rc) return 1;
        const double t3 = Phases::now();
        TOOL_TRY(ctx, canvas_memcpy_d2h(ctx, cntRef.data(), dCr->p, (int64_t)nsites * 4)); TOOL_TRY(ctx, canvas_memcpy_d2h(ctx, cntAlt.data(), dCa->p, (int64_t)nsites * 4));
        loop.tDevice += Phases::now() - t3;
    }
    const double tInflate = loop.tInflate, tDevice = loop.tDevice, kernelMs = loop.kernelMs; const long long overall = loop.records, chunks = loop.chunks, bytesUp = loop.bytesUp;
    printf("Looped over %lld bam records in all\n", overall);
    // (inflation and the device overlap: `inflate` is the time the main thread spent inflating and framing, `device` the time it spent queueing work and waiting for the
    // device — what of the device's work did not hide behind inflation.  Together they are the loop's wall time.)
    { const double tEnd = Phases::now(), rest = std::max(0.0, (tEnd - tLoop0) - tInflate - tDevice); ph.v.push_back({"inflate", tLoop0 + tInflate + rest}); ph.v.push_back({"device", tEnd}); }
    if (getenv("CANVAS_TOOL_TIMING")) fprintf(stderr, "[snv] {\"records\": %lld, \"chunks\": %lld, \"record_bytes\": %lld, \"kernel_ms\": %.4f, \"inflate_s\": %.4f, \"device_wait_s\": %.4f, \"threads\": %d%s}\n", overall, chunks, bytesUp, kernelMs, tInflate, tDevice, io_threads(), loop.timing_tail().c_str());

    // ---- WriteResults (:276-316), filtered by IsVariantSite (:74-81)
    std::vector<int32_t> keep;
    for (int32_t i = 0; i < nsites; i++) { const long long tot = (long long)cntRef[i] + cntAlt[i]; if (tot == 0) continue; if (isDbSnp && cntAlt[i] == 0) continue; keep.push_back(i); }
    if (!write_gz_rows(outPath, (int64_t)keep.size() + 1, [&](int64_t row, std::string& o) {
            if (row == 0) { o += "#Chromosome\tPosition\tRef\tAlt\tCountRef\tCountAlt"; return; }
            const int32_t i = keep[(size_t)row - 1];
            o += chrom; o.push_back('\t'); append_int(o, sites[i].pos); o.push_back('\t'); o += sites[i].ref; o.push_back('\t'); o += sites[i].alt; o.push_back('\t'); append_int(o, cntRef[i]); o.push_back('\t'); append_int(o, cntAlt[i]); }))
        { fprintf(stderr, "cannot write %s\n", outPath.c_str()); return 1; }
    printf("Results written to %s\n", outPath.c_str());
    {
        std::string text = "Chromosome,Position,BAF\n"; int bad = -1;
        for (int32_t i : keep) {
            if (sites[i].ref == "." || sites[i].alt == ".") continue;
            const int pr = b_allele_preference(sites[i].ref), pa = b_allele_preference(sites[i].alt);
            if (pr < 0 || pa < 0) { bad = i; break; }
            const double tot = (double)((long long)cntRef[i] + cntAlt[i]);
            const double baf = pr < pa ? (double)cntRef[i] / tot : (double)cntAlt[i] / tot;
            text += chrom; text.push_back(','); append_int(text, sites[i].pos); text.push_back(','); text += format_double(baf); text.push_back('\n');
        }
        FILE* f = fopen((outPath + ".baf").c_str(), "wb");
        if (!f || fwrite(text.data(), 1, text.size(), f) != text.size() || fclose(f) != 0) { fprintf(stderr, "cannot write %s.baf\n", outPath.c_str()); return 1; }
        if (bad >= 0) { fprintf(stderr, "System.ArgumentException: Invalid single nucleotide allele: %s\n", (b_allele_preference(sites[bad].ref) < 0 ? sites[bad].ref : sites[bad].alt).c_str()); return 255; }
    }
    printf("Results written to %s.baf\n", outPath.c_str());
    ph.mark("write");
    if (ctx && getenv("CANVAS_TOOL_FULL_TEARDOWN")) canvas_destroy(ctx);
    ph.mark("exit");
    return finish(ph, 0);
}
