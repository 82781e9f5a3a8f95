// Drop-in CanvasDiploidCaller executable on top of the C ABI: same CLI and files as CanvasDiploidCaller's Program.Main (CanvasDiploidCaller/Program.cs:27-99) and
// CanvasDiploidCaller.CallVariants (CanvasDiploidCaller.cs:273-359).
//   CanvasDiploidCaller -i S.partitioned -v S.vaf -o CNV.vcf.gz -r <folder with GenomeSize.xml> [-n sample] [-p ploidy.vcf] [-s QualityScoreParameters.json] [-d]
// Exit codes follow the reference: help, an argument nobody understands, a missing -i / -o / -v / -r -> the help, 0 (:57-72); a missing input file or GenomeSize.xml ->
// its message, 1 (:74-90).  -t (the truth report, a training aid) is not built: message, 1.  All of that is decided before a context is created.
// Reading (Segments.cs:52-144, IO.cs:134-179, PloidyInfo.cs:112-163), the call itself (canvas_call_diploid), writing (CanvasSegmentWriter.cs, CanvasSegment.cs:557-747).
// The 100 kb points of the coverage file take their upper median (and the median of 1 - max frequency) from canvas_segment_select over gathered buffers with point offsets.
#include "tool_common.hpp"
using namespace tool;

struct Seg { int chr; int begin, end; int64_t bin0, bin1; int ci[4]; };      // ci: start lower / upper, end lower / upper
struct Site { int pos, ref, alt; };

// double "F2" of .NET Core 2.x: 15 significant digits, then half-up at two decimals (format_f2 of tool_common.hpp with the precision of a double)
static std::string format_f2d(double v) {
    if (std::isnan(v)) return "NaN"; if (std::isinf(v)) return v > 0 ? "Infinity" : "-Infinity";
    std::string d; int scale; sig_digits(v, 15, d, scale);
    int pos = scale + 2;
    if (pos < 0) d.clear();
    else if (pos < (int)d.size()) { bool up = d[pos] >= '5'; d.resize(pos); if (up) { int i = pos - 1; while (i >= 0 && d[i] == '9') { d[i] = '0'; i--; } if (i >= 0) d[i]++; else { d.insert(d.begin(), '1'); scale++; } } }
    std::string ip, fp;
    for (int i = 0; i < scale; i++) ip.push_back(i < (int)d.size() ? d[i] : '0');
    if (ip.empty()) ip = "0";
    for (int i = 0; i < 2; i++) { int k = scale + i; fp.push_back(k >= 0 && k < (int)d.size() ? d[k] : '0'); }
    bool zero = true; for (char c : ip + fp) if (c != '0') zero = false;
    return std::string((std::signbit(v) && !zero) ? "-" : "") + ip + "." + fp;
}
static int half_length(int begin, int end) { return (int)((((long long)end - begin) + ((long long)end - begin >= 0 ? 1 : -1)) / 2); }      // Math.Round(Length / 2.0, AwayFromZero)
static bool ieq(const std::string& a, const std::string& b) { if (a.size() != b.size()) return false; for (size_t i = 0; i < a.size(); i++) if (tolower((unsigned char)a[i]) != tolower((unsigned char)b[i])) return false; return true; }

// plain text, or BGZF blocks with the empty end block when the path ends in .gz (BgzipOrStreamWriter)
struct VcfOut {
    FILE* f = nullptr; bool bgzf = false; std::string buf;
    bool open(const std::string& path) { f = fopen(path.c_str(), "wb"); bgzf = path.size() >= 3 && path.compare(path.size() - 3, 3, ".gz") == 0; if (f) g_open_writers++; return f != nullptr; }
    void block(const char* p, size_t n) {
        std::vector<uint8_t> out(n + 1024); z_stream z; memset(&z, 0, sizeof z);
        deflateInit2(&z, 6, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY);
        z.next_in = (Bytef*)p; z.avail_in = (uInt)n; z.next_out = out.data(); z.avail_out = (uInt)out.size(); deflate(&z, Z_FINISH); const size_t clen = z.total_out; deflateEnd(&z);
        const uint32_t crc = (uint32_t)crc32(crc32(0, nullptr, 0), (const Bytef*)p, (uInt)n), isize = (uint32_t)n; const uint16_t bsize = (uint16_t)(clen + 25);
        const uint8_t h[18] = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 'B', 'C', 2, 0, (uint8_t)(bsize & 255), (uint8_t)(bsize >> 8)};
        fwrite(h, 1, 18, f); fwrite(out.data(), 1, clen, f); fwrite(&crc, 4, 1, f); fwrite(&isize, 4, 1, f);
    }
    void write(const std::string& s) { if (!bgzf) { fwrite(s.data(), 1, s.size(), f); return; } buf += s; while (buf.size() >= 65280) { block(buf.data(), 65280); buf.erase(0, 65280); } }
    void line(const std::string& s) { write(s); write("\n"); }
    void close() { if (!f) return; if (bgzf) { if (!buf.empty()) block(buf.data(), buf.size()); block("", 0); } fclose(f); f = nullptr; g_open_writers--; }
};

// "key" : "value" or "key" : number of a flat JSON object (QualityScoreParameters); keys that are missing keep their defaults
static bool json_number(const std::string& js, const char* key, double& out) {
    const std::string k = std::string("\"") + key + "\""; size_t i = js.find(k); if (i == std::string::npos) return false;
    i = js.find(':', i + k.size()); if (i == std::string::npos) return false;
    i++; while (i < js.size() && (isspace((unsigned char)js[i]) || js[i] == '"')) i++;
    char* e = nullptr; const double v = strtod(js.c_str() + i, &e); if (e == js.c_str() + i) return false; out = v; return true;
}
static std::string attr(const std::string& el, const char* name) {
    const std::string k = std::string(name) + "=\""; size_t i = el.find(k); if (i == std::string::npos) return ""; i += k.size(); size_t j = el.find('"', i); return j == std::string::npos ? "" : el.substr(i, j - i);
}

int main(int argc, char** argv) {
    printf(">>>Command-line arguments:\n"); for (int i = 1; i < argc; i++) printf("%s ", argv[i]); printf("\n");   // Utilities.LogCommandLine
    std::vector<Opt> opts = {{"i", "infile", true}, {"v", "varfile", true}, {"o", "outfile", true}, {"r", "reference", true}, {"n", "sampleName", true}, {"p", "ploidyBed", true},
                             {"d", "dbsnpvcf", false}, {"h", "help", false}, {"s", "qscoreconfig", true}, {"t", "truth", true}};
    Parsed a = parse(argc, argv, opts);
    std::string exeDir = argv[0]; { size_t sl = exeDir.rfind('/'); exeDir = sl == std::string::npos ? "." : exeDir.substr(0, sl); }
    const std::string defaultQ = exeDir + "/QualityScoreParameters.json";
    auto help = [&]() { printf("Usage: CanvasDiploidCaller.exe [OPTIONS]+\nMake discrete-valued copy number calls assuming a diploid baseline.\n\nOptions:\n"
                               "  -i, --infile=VALUE         file containing bins, their counts, and assigned\n                               segments (obtained from CanvasPartition.exe)\n"
                               "  -v, --varfile=VALUE        file containing variant frequencies (obtained from\n                               CanvasSNV.exe)\n"
                               "  -o, --outfile=VALUE        file name prefix to ouput copy number calls to\n                               outfile.vcf\n"
                               "  -r, --reference=VALUE      reference genome folder that contains GenomeSize.xml\n"
                               "  -n, --sampleName=VALUE     sample name for output VCF header (optional)\n"
                               "  -p, --ploidyBed=VALUE      bed file specifying reference ploidy (e.g. for sex\n                               chromosomes) (optional)\n"
                               "  -d, --dbsnpvcf             flag indicating a dbSNP VCF file is used to generate\n                               the variant frequency file (Obsolete)\n"
                               "  -h, --help                 show this message and exit\n"
                               "  -s, --qscoreconfig=VALUE   parameter configuration path (default %s)\n"
                               "  -t, --truth=VALUE          path to vcf/bed with CNV truth data (optional)\n", defaultQ.c_str()); };
    bool needHelp = a.has("help");
    if (!a.extra.empty()) { printf("* Error: I don't understand the argument '%s'\n", a.extra[0].c_str()); needHelp = true; }
    if (needHelp) { help(); return 0; }
    auto last = [&](const char* k) { auto v = a.all(k); return v.empty() ? std::string() : v.back(); };
    const std::string inFile = last("infile"), outFile = last("outfile"), vafFile = last("varfile"), refFolder = last("reference");
    if (!a.has("infile") || !a.has("outfile") || vafFile.empty() || refFolder.empty()) { help(); return 0; }
    if (!file_exists(inFile)) { printf("CanvasDiploidCaller.exe: File %s does not exist! Exiting.\n", inFile.c_str()); return 1; }
    if (!file_exists(vafFile)) { printf("Canvas error: File %s does not exist! Exiting.\n", vafFile.c_str()); return 1; }
    const std::string genomeXml = refFolder + "/GenomeSize.xml";
    if (!file_exists(genomeXml)) { printf("CanvasDiploidCaller.exe: File %s does not exist! Exiting.\n", genomeXml.c_str()); return 1; }
    if (a.has("truth")) { printf("CanvasDiploidCaller (MI355X): -t (the report versus known copy numbers, a training aid) is not built\n"); return 1; }
    const std::string sampleName = a.has("sampleName") ? last("sampleName") : "SAMPLE";

    // ---- QualityScoreParameters: -s, else the file beside the executable, else the defaults of QualityScoreParameters.cs (only the LogisticGermline four are used here)
    double b4[4] = {-5.0123, 4.9801, -5.5472, -1.7914};
    { const std::string qpath = a.has("qscoreconfig") ? last("qscoreconfig") : defaultQ;
      if (a.has("qscoreconfig") && !file_exists(qpath)) { printf("CanvasDiploidCaller.exe: File %s does not exist! Exiting.\n", qpath.c_str()); return 1; }
      if (file_exists(qpath)) {
          std::string js; for_each_line(qpath, [&](const std::string& s) { js += s; js.push_back('\n'); return true; });
          json_number(js, "LogisticGermlineIntercept", b4[0]); json_number(js, "LogisticGermlineLogBinCount", b4[1]);
          json_number(js, "LogisticGermlineModelDistance", b4[2]); json_number(js, "LogisticGermlineDistanceRatio", b4[3]);
      } }

    Phases ph("CanvasDiploidCaller");
    // ---- GenomeSize.xml: every <chromosome .../> element in file order gives contigName and totalBases; nothing else is read
    std::vector<std::string> contigName; std::vector<long long> contigLen;
    { std::string xml; for_each_line(genomeXml, [&](const std::string& s) { xml += s; xml.push_back(' '); return true; });
      for (size_t i = xml.find("<chromosome"); i != std::string::npos; i = xml.find("<chromosome", i + 1)) {
          const char nx = i + 11 < xml.size() ? xml[i + 11] : ' '; if (!(isspace((unsigned char)nx) || nx == '/' || nx == '>')) continue;
          const size_t j = xml.find('>', i); const std::string el = xml.substr(i, j == std::string::npos ? std::string::npos : j - i);
          contigName.push_back(attr(el, "contigName")); contigLen.push_back(atoll(attr(el, "totalBases").c_str()));
      } }

    // ---- *.partitioned: chr, start, end, count, segment id; bins grouped by adjacent chromosome, then by adjacent segment id (Segments.cs:52-79)
    std::vector<std::string> chrName; std::vector<int64_t> chrSegOff = {0}; std::vector<Seg> segs; std::vector<float> counts;
    {   GzReader rd(inFile); if (!rd.ok()) { printf("CanvasDiploidCaller.exe: cannot read %s\n", inFile.c_str()); return 1; }
        struct Bin { int start, end; std::string id; }; std::vector<Bin> bins; std::vector<float> cnt; std::string row, cur; std::set<std::string> seen;
        auto flush = [&]() {
            if (bins.empty()) return;
            const int c = (int)chrName.size(); chrName.push_back(cur);
            size_t g0 = 0; std::vector<std::pair<size_t, size_t>> groups;
            for (size_t i = 1; i <= bins.size(); i++) if (i == bins.size() || bins[i].id != bins[g0].id) { groups.push_back({g0, i}); g0 = i; }
            for (size_t g = 0; g < groups.size(); g++) {
                const Bin& first = bins[groups[g].first]; const Bin& lastB = bins[groups[g].second - 1];
                const Bin* prev = g ? &bins[groups[g].first - 1] : nullptr; const Bin* next = g + 1 < groups.size() ? &bins[groups[g].second] : nullptr;
                Seg s; s.chr = c; s.begin = first.start; s.end = lastB.end; s.bin0 = (int64_t)counts.size() + (int64_t)groups[g].first; s.bin1 = (int64_t)counts.size() + (int64_t)groups[g].second;
                const int hf = half_length(first.start, first.end), hl = half_length(lastB.start, lastB.end);
                s.ci[0] = (!prev || prev->end != first.start) ? -hf : -half_length(prev->start, prev->end); s.ci[1] = hf;
                s.ci[2] = -hl; s.ci[3] = (!next || lastB.end != next->start) ? hl : half_length(next->start, next->end);
                segs.push_back(s);
            }
            counts.insert(counts.end(), cnt.begin(), cnt.end()); chrSegOff.push_back((int64_t)segs.size()); bins.clear(); cnt.clear();
        };
        while (rd.line(row)) {
            if (row.empty()) continue;
            auto t = split_tab(row); if (t.size() < 5) continue;
            if (bins.empty() || t[0] != cur) {
                flush();
                if (!seen.insert(t[0]).second) { fprintf(stderr, "CanvasDiploidCaller: chromosome %s comes back later in %s (the reference fails on the duplicate key)\n", t[0].c_str(), inFile.c_str()); return 1; }
                cur = t[0];
            }
            bins.push_back({atoi(t[1].c_str()), atoi(t[2].c_str()), t[4]}); cnt.push_back(strtof(t[3].c_str(), nullptr));
        }
        flush();
    }
    const int nchr = (int)chrName.size(); const int64_t nseg = (int64_t)segs.size(), nbins = (int64_t)counts.size();

    VcfOut vcf;
    auto vcf_header = [&](bool withCoverage, double overallPloidy, double diploidCoverage) {
        vcf.line("##fileformat=VCFv4.1");
        vcf.line(std::string("##source=Canvas ") + canvas_version());
        vcf.line("##reference=" + refFolder + "/genome.fa");
        if (withCoverage) { vcf.line("##OverallPloidy=" + format_f2d(overallPloidy)); vcf.line("##DiploidCoverage=" + format_f2d(diploidCoverage)); }
        for (size_t c = 0; c < contigName.size(); c++) vcf.line("##contig=<ID=" + contigName[c] + ",length=" + std::to_string(contigLen[c]) + ">");
        vcf.line("##ALT=<ID=DUP,Description=\"Region of elevated copy number relative to the reference\">");
        for (int k = 0; k <= 5; k++) if (k != 1) vcf.line("##ALT=<ID=CN" + std::to_string(k) + ",Description=\"Copy number allele: " + std::to_string(k) + " copies\">");
        vcf.line("##FILTER=<ID=q10,Description=\"Quality below 10\">");
        vcf.line("##FILTER=<ID=FailedFT,Description=\"Sample-level filter failed in all the samples\">");
        vcf.line("##INFO=<ID=CIEND,Number=2,Type=Integer,Description=\"Confidence interval around END for imprecise variants\">");
        vcf.line("##INFO=<ID=CIPOS,Number=2,Type=Integer,Description=\"Confidence interval around POS for imprecise variants\">");
        vcf.line("##INFO=<ID=CNVLEN,Number=1,Type=Integer,Description=\"Number of reference positions spanned by this CNV\">");
        vcf.line("##INFO=<ID=END,Number=1,Type=Integer,Description=\"End position of the variant described in this record\">");
        vcf.line("##INFO=<ID=SVTYPE,Number=1,Type=String,Description=\"Type of structural variant\">");
        vcf.line("##INFO=<ID=SUBCLONAL,Number=0,Type=Flag,Description=\"Subclonal variant\">");
        vcf.line("##INFO=<ID=COMMONCNV,Number=0,Type=Flag,Description=\"Common CNV variant identified from pre-specified bed intervals\">");
        vcf.line("##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">");
        vcf.line("##FORMAT=<ID=RC,Number=1,Type=Float,Description=\"Mean counts per bin in the region\">");
        vcf.line("##FORMAT=<ID=BC,Number=1,Type=Float,Description=\"Number of bins in the region\">");
        vcf.line("##FORMAT=<ID=CN,Number=1,Type=Integer,Description=\"Copy number genotype for imprecise events\">");
        vcf.line("##FORMAT=<ID=MCC,Number=1,Type=Integer,Description=\"Major chromosome count (equal to copy number for LOH regions)\">");
        vcf.line("##FORMAT=<ID=MCCQ,Number=1,Type=Float,Description=\"Major chromosome count quality score\">");
        vcf.line("##FORMAT=<ID=QS,Number=1,Type=Float,Description=\"Phred-scaled quality score. If CN is reference then this is -10log10(prob(variant)) otherwise this is -10log10(prob(no variant).\">");
        vcf.line("##FORMAT=<ID=FT,Number=1,Type=String,Description=\"Sample filter, 'PASS' indicates that all filters have passed for this sample\">");
        vcf.line("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + sampleName);
    };
    if (nseg == 0) {      // CanvasDiploidCaller.cs:285-291: the header-only VCF, without ##OverallPloidy / ##DiploidCoverage
        printf("CanvasDiploidCaller: No segments loaded; no CNV calls will be made.\n");
        if (!vcf.open(outFile)) { fprintf(stderr, "cannot write %s\n", outFile.c_str()); return 1; }
        vcf_header(false, 0, 0); vcf.close();
        return finish(ph, 0);
    }
    for (auto& s : segs) { bool known = false; for (auto& cn : contigName) known = known || ieq(cn, chrName[(size_t)s.chr]);      // SanityCheckChromosomeNames
        if (!known) { fprintf(stderr, "Unhandled Exception: System.Exception: Integrity check error: Segment found at unknown chromosome '%s'\n", chrName[(size_t)s.chr].c_str()); return 1; } }

    // ---- ploidy VCF
    std::map<std::string, std::vector<PloidyIv>> ploidy; const bool havePloidy = a.has("ploidyBed") && !last("ploidyBed").empty();
    if (havePloidy) { std::string err; if (!load_ploidy_vcf(last("ploidyBed"), ploidy, err)) { fprintf(stderr, "CanvasDiploidCaller: %s\n", err.c_str()); return 1; } }

    // ---- *.vaf: chr, position, ref, alt, ref count, alt count; records of a chromosome must come in one run and must not go backwards
    std::vector<std::vector<Site>> sitesOf((size_t)nchr);
    {   GzReader rd(vafFile); if (!rd.ok()) { printf("Canvas error: cannot read %s\n", vafFile.c_str()); return 1; }
        std::map<std::string, int> idx; for (int c = 0; c < nchr; c++) idx[chrName[(size_t)c]] = c;
        std::string row, prev; std::set<std::string> seen; int lastPos = 0; bool any = false; long long lineNo = 0;
        while (rd.line(row)) {
            lineNo++;
            if (row.empty() || row[0] == '#') continue;
            auto t = split_tab(row); if (t.size() < 6) { fprintf(stderr, "CanvasDiploidCaller: %s line %lld has fewer than six columns\n", vafFile.c_str(), lineNo); return 1; }
            const int pos = atoi(t[1].c_str());
            if (!any || t[0] != prev) {
                if (!seen.insert(t[0]).second) { fprintf(stderr, "CanvasDiploidCaller: %s is not sorted: chromosome %s comes back at line %lld (%s:%d)\n", vafFile.c_str(), t[0].c_str(), lineNo, t[0].c_str(), pos); return 1; }
                prev = t[0]; any = true;
            } else if (pos < lastPos) { fprintf(stderr, "CanvasDiploidCaller: %s is not sorted: %s:%d at line %lld comes after position %d\n", vafFile.c_str(), t[0].c_str(), pos, lineNo, lastPos); return 1; }
            lastPos = pos;
            auto it = idx.find(t[0]); if (it == idx.end()) continue;
            sitesOf[(size_t)it->second].push_back({pos, atoi(t[4].c_str()), atoi(t[5].c_str())});
        }
    }
    std::vector<int64_t> chrSiteOff((size_t)nchr + 1, 0); std::vector<int> sPos, sRef, sAlt;
    for (int c = 0; c < nchr; c++) { for (auto& s : sitesOf[(size_t)c]) { sPos.push_back(s.pos); sRef.push_back(s.ref); sAlt.push_back(s.alt); } chrSiteOff[(size_t)c + 1] = (int64_t)sPos.size(); }
    const int64_t nsites = (int64_t)sPos.size();
    // the kept sites of every segment on the host as well (the coverage file needs each run's frequencies): the forward-only pointer of IO.cs:156-176
    std::vector<float> keptF, keptM; std::vector<int64_t> hostSiteOff((size_t)nseg + 1, 0);
    for (int c = 0; c < nchr; c++) {
        int64_t index = chrSegOff[(size_t)c]; const int64_t s1 = chrSegOff[(size_t)c + 1];
        std::vector<std::vector<std::pair<float, float>>> per((size_t)(s1 - chrSegOff[(size_t)c]));
        for (auto& s : sitesOf[(size_t)c]) {
            if ((long long)s.ref + s.alt < 10) continue;
            while (index < s1 && !(segs[(size_t)index].end > s.pos)) index++;
            if (index >= s1 || segs[(size_t)index].begin > s.pos) continue;
            const int tot = s.ref + s.alt; const float f = (float)s.alt / (float)tot; const double mx = (double)std::max(s.ref, s.alt) / (double)tot;
            per[(size_t)(index - chrSegOff[(size_t)c])].push_back({f, 1.0f - (float)mx});
        }
        for (size_t k = 0; k < per.size(); k++) { for (auto& p : per[k]) { keptF.push_back(p.first); keptM.push_back(p.second); } hostSiteOff[(size_t)chrSegOff[(size_t)c] + k + 1] = (int64_t)keptF.size(); }
    }
    ph.mark("read");

    // ---- the call
    std::vector<int32_t> segBegin((size_t)nseg), segEnd((size_t)nseg); std::vector<int64_t> segBinOff((size_t)nseg + 1, 0);
    for (int64_t s = 0; s < nseg; s++) { segBegin[(size_t)s] = segs[(size_t)s].begin; segEnd[(size_t)s] = segs[(size_t)s].end; segBinOff[(size_t)s + 1] = segs[(size_t)s].bin1; }
    std::vector<double> medCount((size_t)nseg), medMaf((size_t)nseg), dist((size_t)nseg), dist2((size_t)nseg), runMed((size_t)nseg), scal(2);
    std::vector<int64_t> siteOff((size_t)nseg + 1), runFirst((size_t)nseg), runLast((size_t)nseg), info(4);
    std::vector<int32_t> inf((size_t)nseg), cn((size_t)nseg), mcc((size_t)nseg), q((size_t)nseg), runQ((size_t)nseg), runFilter((size_t)nseg);
    int64_t nruns = 0;
    AsyncCtx actx; canvas_ctx* ctx = actx.require("CanvasDiploidCaller"); if (!ctx) return 1;
    Dev dCount(ctx, nbins * 4), dPos(ctx, nsites * 4), dRef(ctx, nsites * 4), dAlt(ctx, nsites * 4);
    TOOL_TRY(ctx, canvas_memcpy_h2d(ctx, dCount.p, counts.data(), nbins * 4));
    if (nsites) { TOOL_TRY(ctx, canvas_memcpy_h2d(ctx, dPos.p, sPos.data(), nsites * 4)); TOOL_TRY(ctx, canvas_memcpy_h2d(ctx, dRef.p, sRef.data(), nsites * 4)); TOOL_TRY(ctx, canvas_memcpy_h2d(ctx, dAlt.p, sAlt.data(), nsites * 4)); }
    TOOL_TRY(ctx, canvas_call_diploid(ctx, nbins, dCount.as<float>(), nchr, chrSegOff.data(), segBegin.data(), segEnd.data(), segBinOff.data(), chrSiteOff.data(), dPos.as<int32_t>(), dRef.as<int32_t>(),
                                      dAlt.as<int32_t>(), b4, medCount.data(), siteOff.data(), inf.data(), medMaf.data(), cn.data(), mcc.data(), dist.data(), dist2.data(), q.data(), &nruns, runFirst.data(),
                                      runLast.data(), runQ.data(), runFilter.data(), runMed.data(), scal.data(), info.data()));
    if (siteOff != hostSiteOff) { fprintf(stderr, "CanvasDiploidCaller: the device and the host disagree on which sites belong to which segment\n"); return 1; }
    const double diploidCoverage = scal[0];

    // ---- merged runs
    struct Run { int chr, begin, end, cn, mcc, q, filter; int64_t bin0, bin1, site0, site1; double med; const int* ciStart; const int* ciEnd; };
    std::vector<Run> runs((size_t)nruns);
    for (int64_t r = 0; r < nruns; r++) { const Seg& f = segs[(size_t)runFirst[(size_t)r]]; const Seg& l = segs[(size_t)runLast[(size_t)r]];
        runs[(size_t)r] = {f.chr, f.begin, l.end, cn[(size_t)runFirst[(size_t)r]], mcc[(size_t)runFirst[(size_t)r]], runQ[(size_t)r], runFilter[(size_t)r], f.bin0, l.bin1,
                           siteOff[(size_t)runFirst[(size_t)r]], siteOff[(size_t)runLast[(size_t)r] + 1], runMed[(size_t)r], f.ci, l.ci + 2}; }

    // ---- <stem>.CoverageAndVariantFrequency.txt (CanvasSegment.cs:557-747): 100 kb points; the select gives every point's upper median of counts and median of 1 - max frequency
    std::string covPath = outFile; if (covPath.size() >= 7 && covPath.compare(covPath.size() - 7, 7, ".vcf.gz") == 0) covPath.resize(covPath.size() - 7);
    covPath += ".CoverageAndVariantFrequency.txt";
    {   const int pointLength = 100000;
        long long totalBins = 0, totalLength = 0; for (auto& r : runs) { totalBins += r.bin1 - r.bin0; totalLength += r.end - r.begin; }
        int minimumBins; { const float v = 0.25f * (float)totalBins / (float)(totalLength / pointLength); minimumBins = (v == v && v >= -2147483648.0f && v < 2147483648.0f) ? (int)v : (-2147483647 - 1); if (minimumBins < 1) minimumBins = 1; }
        struct Point { int chr; int start, end, majorCn, majorMcc; bool hasMcc; int64_t c0, c1, m0, m1, v0, v1; };
        std::vector<Point> points; std::vector<float> gCounts, gMaf, gVf;
        for (size_t cg = 0; cg < contigName.size(); cg++) {
            int c = -1; for (int k = 0; k < nchr; k++) if (chrName[(size_t)k] == contigName[cg]) c = k;      // (this lookup is case-sensitive in the reference: a dictionary by name)
            if (c < 0) continue;
            std::vector<const Run*> chrRuns; for (auto& r : runs) if (r.chr == c) chrRuns.push_back(&r);
            for (long long ps = 0; ps < contigLen[cg]; ps += pointLength) {
                const int start = (int)ps, end = (int)std::min<long long>(contigLen[cg], ps + pointLength);
                std::vector<std::pair<std::pair<int, int>, long long>> byPair; std::vector<std::pair<int, long long>> byCn; std::vector<const Run*> overlap;
                for (const Run* r : chrRuns) {
                    if (r->begin > end || r->end < start) continue;
                    const int w = std::min(r->end, end) - std::max(r->begin, start);
                    bool f1 = false; for (auto& e : byPair) if (e.first == std::make_pair(r->cn, r->mcc)) { e.second += w; f1 = true; } if (!f1) byPair.push_back({{r->cn, r->mcc}, w});
                    bool f2 = false; for (auto& e : byCn) if (e.first == r->cn) { e.second += w; f2 = true; } if (!f2) byCn.push_back({r->cn, w});
                    overlap.push_back(r);
                }
                long long best = 0; int major = 0; for (auto& e : byCn) if (e.second > best) { best = e.second; major = e.first; }
                bool hasMcc = false; int majorMcc = -1; { bool anyP = false; long long bw = 0; for (auto& e : byPair) if (e.first.first == major && (!anyP || e.second > bw)) { anyP = true; bw = e.second; majorMcc = e.first.second; } hasMcc = anyP && majorMcc >= 0; }
                Point P{c, start, end, major, majorMcc, hasMcc, (int64_t)gCounts.size(), 0, (int64_t)gMaf.size(), 0, (int64_t)gVf.size(), 0};
                for (const Run* r : overlap) {
                    if ((major == 2 && r->cn != 2) || (major < 2 && r->cn >= 2) || (major > 2 && r->cn <= 2)) continue;
                    const int len = r->end - r->begin; const int nb = (int)(r->bin1 - r->bin0), ns = (int)(r->site1 - r->site0);
                    auto cut = [&](int n, int& i0, int& i1) { i0 = 0; if (start > r->begin) i0 = (int)((float)n * (float)(start - r->begin) / (float)len); i1 = n; if (end < r->end) i1 = (int)((float)n * (float)(end - r->begin) / (float)len); };
                    int i0, i1; cut(nb, i0, i1); for (int i = i0; i < i1; i++) gCounts.push_back(counts[(size_t)(r->bin0 + i)]);
                    cut(ns, i0, i1); i0 = std::max(i0, 0); for (int i = i0; i < i1 && i < ns; i++) { gVf.push_back(keptF[(size_t)(r->site0 + i)]); gMaf.push_back(keptM[(size_t)(r->site0 + i)]); }
                }
                P.c1 = (int64_t)gCounts.size(); P.m1 = (int64_t)gMaf.size(); P.v1 = (int64_t)gVf.size(); points.push_back(P);
            }
        }
        const int64_t np = (int64_t)points.size(); std::vector<double> pHits((size_t)std::max<int64_t>(np, 1)), pMaf((size_t)std::max<int64_t>(np, 1));
        if (np > 0) {
            std::vector<int64_t> offC((size_t)np + 1), offM((size_t)np + 1); offC[0] = 0; offM[0] = 0;
            for (int64_t p = 0; p < np; p++) { offC[(size_t)p + 1] = points[(size_t)p].c1; offM[(size_t)p + 1] = points[(size_t)p].m1; }
            Dev dG(ctx, (int64_t)gCounts.size() * 4), dM(ctx, (int64_t)gMaf.size() * 4), dOut(ctx, np * 8);
            if (!gCounts.empty()) TOOL_TRY(ctx, canvas_memcpy_h2d(ctx, dG.p, gCounts.data(), (int64_t)gCounts.size() * 4));
            if (!gMaf.empty()) TOOL_TRY(ctx, canvas_memcpy_h2d(ctx, dM.p, gMaf.data(), (int64_t)gMaf.size() * 4));
            TOOL_TRY(ctx, canvas_segment_select(ctx, dG.as<float>(), np, offC.data(), CANVAS_SELECT_UPPER, dOut.as<double>(), nullptr));
            TOOL_TRY(ctx, canvas_memcpy_d2h(ctx, pHits.data(), dOut.p, np * 8));
            TOOL_TRY(ctx, canvas_segment_select(ctx, dM.as<float>(), np, offM.data(), CANVAS_SELECT_MEDIAN_F32, dOut.as<double>(), nullptr));
            TOOL_TRY(ctx, canvas_memcpy_d2h(ctx, pMaf.data(), dOut.p, np * 8));
        }
        ph.mark("device");
        FILE* f = fopen(covPath.c_str(), "wb"); if (!f) { fprintf(stderr, "cannot write %s\n", covPath.c_str()); return 1; }
        std::string o = "#Chromosome\tStart\tEnd\tCopyNumber\tMajorChromosomeCount\tMedianHits\tNormalizedCoverage\tMedianMinorAlleleFrequency\tReferencePloidy\t";
        for (int i = 0; i < 100; i++) o += "VariantFrequencyBin" + std::to_string(i) + "\t";
        o += "\n";
        for (int64_t p = 0; p < np; p++) {
            const Point& P = points[(size_t)p];
            o += chrName[(size_t)P.chr] + "\t" + std::to_string(P.start) + "\t" + std::to_string(P.end) + "\t";
            if (P.c1 - P.c0 >= minimumBins) {
                o += std::to_string(P.majorCn) + "\t" + (P.hasMcc ? std::to_string(P.majorMcc) : std::string()) + "\t";
                const double hits = pHits[(size_t)p];
                o += format_f2d(hits) + "\t" + format_f2d(2 * hits / diploidCoverage) + "\t";
                if (P.m1 - P.m0 >= 10) o += format_g(pMaf[(size_t)p], 15);
                o += "\t";
                int refPloidy = 2; auto it = ploidy.find(chrName[(size_t)P.chr]);
                if (havePloidy && it != ploidy.end()) for (auto& iv : it->second) if (iv.start - 1 <= P.end && iv.end >= P.start) refPloidy = iv.ploidy;
                o += std::to_string(refPloidy) + "\t";
                const int64_t nv = P.v1 - P.v0;
                if (nv >= 10) {
                    float hist[100]; for (int i = 0; i < 100; i++) hist[i] = 0.0f;
                    for (int64_t i = P.v0; i < P.v1; i++) { const int b = std::min(99, (int)std::floor((double)gVf[(size_t)i] / 0.01)); hist[b]++; }
                    for (int i = 0; i < 100; i++) { hist[i] = hist[i] / (float)nv * 100.0f; o += format_f2(hist[i]) + "\t"; }
                } else o += std::string(100, '\t');
            }
            o += "\n";
        }
        fwrite(o.data(), 1, o.size(), f); fclose(f);
    }

    // ---- the VCF (CanvasSegmentWriter.WriteSegments)
    if (!vcf.open(outFile)) { fprintf(stderr, "cannot write %s\n", outFile.c_str()); return 1; }
    { double totalPloidy = 0, totalWeight = 0; for (auto& r : runs) if (r.filter == 0) { totalWeight += r.end - r.begin; totalPloidy += (double)(r.cn * (r.end - r.begin)); }
      vcf_header(totalWeight > 0, totalWeight > 0 ? totalPloidy / totalWeight : 0, diploidCoverage); }
    const int INTMAX = 2147483647;
    for (size_t cg = 0; cg < contigName.size(); cg++)
        for (auto& r : runs) {
            const std::string& chr = chrName[(size_t)r.chr];
            if (!ieq(chr, contigName[cg])) continue;
            int refCn = 2;
            if (havePloidy) { auto it = ploidy.find(chr); refCn = reference_copy_number(it == ploidy.end() ? nullptr : &it->second, r.begin, r.end); }
            if (refCn > 2 || refCn < 0) { vcf.close(); fprintf(stderr, "Unhandled Exception: System.ArgumentException: Reference copy number > 2 is not supported\n"); return 1; }
            // GetCnvTypeAndAlleleCopyNumbers (CanvasSegment.cs:280-312)
            const char* type; std::vector<int> al; const bool hasMcc = r.mcc >= 0;
            if (r.cn == refCn) {
                if (refCn == 1) { type = "REF"; al = {1}; }
                else if (refCn == 2 && hasMcc) { if (r.mcc == 2) { type = "LOH"; al = {0, 2}; } else { type = "REF"; al = {1, 1}; } }
                else { type = "REF"; al.assign((size_t)std::max(1, refCn), -1); }
            } else if (r.cn > refCn) {
                type = "GAIN";
                if (refCn == 1) al = {r.cn};
                else if (refCn == 2) { if (hasMcc) al = {r.cn - r.mcc, r.mcc}; else al = {-1, INTMAX}; }
                else al.assign((size_t)std::max(1, refCn), -1);
            } else { type = "LOSS"; if (r.cn == 0) al.assign((size_t)refCn, 0); else al = {0, 1}; }
            // GetAltAllelesAndGenotypes for the one sample
            std::vector<int> uniq; for (int x : al) if (x != 1 && x != -1 && std::find(uniq.begin(), uniq.end(), x) == uniq.end()) uniq.push_back(x);
            std::sort(uniq.begin(), uniq.end());
            std::string alt = "."; if (!uniq.empty()) { alt.clear(); for (size_t i = 0; i < uniq.size(); i++) { if (i) alt += ","; alt += uniq[i] == INTMAX ? std::string("<DUP>") : "<CN" + std::to_string(uniq[i]) + ">"; } }
            std::vector<int> g; for (int x : al) g.push_back(x == 1 ? 0 : x == -1 ? -1 : (int)(std::find(uniq.begin(), uniq.end(), x) - uniq.begin()) + 1);
            std::stable_sort(g.begin(), g.end());
            std::string gt; for (size_t i = 0; i < g.size(); i++) { if (i) gt += "/"; gt += g[i] < 0 ? std::string(".") : std::to_string(g[i]); }
            const bool symbolic = !alt.empty() && alt.front() == '<' && alt.back() == '>';
            const bool isRef = !strcmp(type, "REF");
            std::string ft; if (r.filter & 1) ft = "q10"; if (r.filter & 2) ft += std::string(ft.empty() ? "" : ";") + "L10kb"; if (ft.empty()) ft = "PASS";
            std::string o = chr + "\t" + std::to_string(symbolic ? r.begin : r.begin + 1) + "\tCanvas:" + type + ":" + chr + ":" + std::to_string(r.begin + 1) + "-" + std::to_string(r.end) + "\t";
            o += "N\t" + alt + "\t" + format_f2d((double)r.q) + "\t" + (r.filter == 0 ? "PASS" : "FailedFT") + "\t";
            if (!isRef) o += std::string("SVTYPE=") + (!strcmp(type, "LOH") ? "LOH" : "CNV") + ";";
            o += "END=" + std::to_string(r.end);
            if (!isRef) o += ";CNVLEN=" + std::to_string(r.end - r.begin);
            o += ";CIPOS=" + std::to_string(r.ciStart[0]) + "," + std::to_string(r.ciStart[1]) + ";CIEND=" + std::to_string(r.ciEnd[0]) + "," + std::to_string(r.ciEnd[1]);
            o += "\tGT:RC:BC:CN:MCC:MCCQ:QS:FT\t" + gt + ":" + format_f2d(r.med) + ":" + std::to_string(r.bin1 - r.bin0) + ":" + std::to_string(r.cn) + ":" + (hasMcc ? std::to_string(r.mcc) : std::string(".")) + ":.:" +
                 format_f2d((double)r.q) + ":" + ft;
            vcf.line(o);
        }
    vcf.close();
    ph.mark("write");
    if (getenv("CANVAS_TOOL_FULL_TEARDOWN")) canvas_destroy(ctx);
    return finish(ph, 0);
}
