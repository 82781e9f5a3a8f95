// Drop-in CanvasNormalize executable on top of the C ABI: CLI and file formats of CanvasNormalize (CanvasNormalize/Program.cs:52-160, CanvasNormalize.cs:17-25,
// CanvasNormalizeFactory.cs:20-47).
//   CanvasNormalize -t T.binned -n N.binned [-n ...] -w W.binned -o T.ratio.binned [-m WeightedAverage|BestLR2|PCA] [-p ploidy.vcf] [-r min -r max]
// 1. the reference file -w: WeightedAverage (one -n: byte copy; several: canvas_normalize_reference, field 4 of the first control's rows replaced by "{0}" of
//    the weighted count), BestLR2 (byte copy of the control canvas_normalize_best_normal picks), PCA (-n = the model file: canvas_normalize_pca_reference,
//    written with CanvasIO.WriteToTextFile)
// 2. ratios of -t to -w read back: LSNorm for WeightedAverage / BestLR2, Raw over [min, max] of -r for PCA (canvas_normalize_ratio)
// 3. -o = RatiosToCounts with the reference copy number of every bin from the ploidy VCF (-p, absent = 2); 4. -o + ".cnd" (WriteCndFile).
// Exit codes follow Program.cs: help and missing -t / -n / -o -> 1, missing input file -> 1, every place where the reference throws -> 1 with a message.
// -f (Nextera manifest) is refused: Isas.Manifests is not part of the reference sources.
// The .cnd file is written by Illumina.Common's CSVWriter, which is not in the reference sources either: the fields are joined with commas and not quoted
// (none of them holds a comma, a quote or a line break).
#include "tool_common.hpp"
#include <algorithm>
using namespace tool;

static const char* kHelp =
    "Usage: CanvasNormalize.exe [OPTIONS]+\nNormalize coverage of genomic intervals.\n\nOptions:\n"
    "  -t, --tumor=VALUE  -n, --normal=VALUE (repeatable; in PCA mode the model file, once)  -o, --out=VALUE  -w, --weightedAverageNormal=VALUE\n"
    "  -f, --manifest=VALUE  -p, --ploidyVcfFile=VALUE  -r, --referenceBinCountRange=VALUE (twice: min and max)  -h, --help\n"
    "  -m, --mode=VALUE  normalization mode (WeightedAverage/BestLR2/PCA). Default: WeightedAverage\n";

// the rows of a .binned file as CanvasIO.ReadFromTextFile (IO.cs:26-52) or BinCounts.LoadBinCounts (BinCounts.cs:95-108) read them
struct Bins {
    std::vector<std::string> chromNames; std::vector<int32_t> chr, start, stop, gc; std::vector<double> value;
    int64_t size() const { return (int64_t)chr.size(); }
    bool same_bin(int64_t i, const Bins& o, int64_t j) const { return chromNames[chr[i]] == o.chromNames[o.chr[j]] && start[i] == o.start[j] && stop[i] == o.stop[j]; }
};
static bool read_bins(const std::string& path, int minFields, Bins& b) {
    TextRows rows; if (!read_text_rows(path, minFields, rows)) return false;
    const size_t m = rows.chr.size();
    b.chromNames = rows.chromNames; b.chr = std::move(rows.chr); b.gc = std::move(rows.gc); b.value = std::move(rows.value); b.start.resize(m); b.stop.resize(m);
    for (size_t i = 0; i < m; i++) { b.start[i] = (int32_t)rows.start[i]; b.stop[i] = (int32_t)rows.stop[i]; }
    return true;
}
static bool copy_file(const std::string& src, const std::string& dst) {
    FILE* in = fopen(src.c_str(), "rb"); if (!in) return false;
    FILE* out = fopen(dst.c_str(), "wb"); if (!out) { fclose(in); return false; }
    std::vector<char> buf(1 << 20); size_t k; bool ok = true;
    while ((k = fread(buf.data(), 1, buf.size(), in)) > 0) if (fwrite(buf.data(), 1, k, out) != k) { ok = false; break; }
    fclose(in); return (fclose(out) == 0) && ok;
}
// CanvasIO.WriteToTextFile (IO.cs:15-24): chromosome, start, stop, "{count:F2}", GC
static bool write_bins(const std::string& path, const Bins& b, const std::vector<int32_t>* rows, const std::vector<float>& count) {
    const int64_t n = rows ? (int64_t)rows->size() : (int64_t)count.size();
    return write_gz_rows(path, n, [&](int64_t k, std::string& o) {
        const int64_t i = rows ? (*rows)[k] : k;
        o += b.chromNames[b.chr[i]]; o.push_back('\t'); append_int(o, b.start[i]); o.push_back('\t'); append_int(o, b.stop[i]); o.push_back('\t');
        o += format_f2(count[k]); o.push_back('\t'); append_int(o, b.gc[i]); });
}
// PCAModel.LoadModel (PCAReferenceGenerator.cs:92-127): "chrom start stop mean axis..." per line, gzip or plain text; axes = fields of the first line - 4
static bool read_model(const std::string& path, Bins& mu, std::vector<std::vector<double>>& axes, std::string& err) {
    std::string data; if (!read_gz_all(path, data)) { err = "cannot read " + path; return false; }
    size_t p = 0; int naxes = -1; std::vector<std::string> names;
    while (p < data.size()) {
        size_t e = data.find('\n', p); if (e == std::string::npos) e = data.size();
        std::string line = data.substr(p, e - p); if (!line.empty() && line.back() == '\r') line.pop_back();
        p = e + 1;
        auto t = split_tab(line);
        if (naxes < 0) { naxes = (int)t.size() - 4; if (naxes < 0) naxes = 0; axes.assign((size_t)naxes, {}); }
        if ((int)t.size() < 4 + naxes) { err = "malformed model line: " + line; return false; }     // toks[i + 4]: IndexOutOfRangeException
        int c = -1; for (size_t k = 0; k < names.size(); k++) if (names[k] == t[0]) c = (int)k;
        if (c < 0) { c = (int)names.size(); names.push_back(t[0]); }
        mu.chr.push_back(c); mu.start.push_back(atoi(t[1].c_str())); mu.stop.push_back(atoi(t[2].c_str())); mu.gc.push_back(-1);
        mu.value.push_back((double)(float)strtod(t[3].c_str(), nullptr));                        // float.Parse
        for (int k = 0; k < naxes; k++) axes[(size_t)k].push_back(strtod(t[4 + k].c_str(), nullptr));   // double.Parse
    }
    mu.chromNames = names;
    if (naxes < 0) { err = "the model file " + path + " is empty"; return false; }
    return true;
}

int main(int argc, char** argv) {
    setenv("GPU_MAX_HW_QUEUES", "8", 0);       // (read by the HIP runtime at its first call)
    printf(">>>Command-line arguments:\n"); for (int i = 1; i < argc; i++) printf("%s ", argv[i]); printf("\n");   // Utilities.LogCommandLine
    std::vector<Opt> opts = {{"t", "tumor", true}, {"n", "normal", true}, {"o", "out", true}, {"w", "weightedAverageNormal", true}, {"f", "manifest", true},
                             {"p", "ploidyVcfFile", true}, {"r", "referenceBinCountRange", true}, {"h", "help", false}, {"m", "mode", true}};
    Parsed a = parse(argc, argv, opts);
    if (!a.extra.empty()) {
        std::string all; for (size_t i = 0; i < a.extra.size(); i++) all += (i ? "," : "") + a.extra[i];
        fprintf(stderr, "Unknown arguments: %s\n", all.c_str()); return 1;
    }
    // -m (Utilities.ParseCanvasNormalizeMode, CanvasCommon/Utilities.cs:76-89): case-insensitive, trimmed
    int mode = 0; const char* modeName[3] = {"WeightedAverage", "BestLR2", "PCA"};
    for (auto& v : a.all("mode")) {
        std::string m = v; for (auto& ch : m) ch = (char)tolower(ch);
        m.erase(0, m.find_first_not_of(" \t\r\n")); m.erase(m.find_last_not_of(" \t\r\n") + 1);
        if (m == "weightedaverage") mode = 0; else if (m == "bestlr2") mode = 1; else if (m == "pca") mode = 2;
        else { fprintf(stderr, "Invalid CanvasNormalize mode '%s'\n", v.c_str()); return 1; }
    }
    std::vector<double> range;
    for (auto& v : a.all("referenceBinCountRange")) {          // double.Parse
        char* end = nullptr; const double d = strtod(v.c_str(), &end);
        if (v.empty() || *end) { fprintf(stderr, "Input string was not in a correct format: -r %s\n", v.c_str()); return 1; }
        range.push_back(d);
    }
    const std::string tumorFile = a.get("tumor"), outFile = a.get("out"), refFile = a.get("weightedAverageNormal");
    const auto normals = a.all("normal");
    bool needHelp = a.has("help");
    if (!a.has("tumor")) { fprintf(stderr, "Please specify the tumor bed file.\n"); needHelp = true; }
    else if (normals.empty()) { fprintf(stderr, mode == 2 ? "Please specify a model file.\n" : "Please specify at least one normal bed file.\n"); needHelp = true; }
    else if (!a.has("out")) { fprintf(stderr, "Please specify an output file name.\n"); needHelp = true; }
    if (range.empty()) range = {1.0, HUGE_VAL};
    else if (range.size() != 2) { fprintf(stderr, "Please specify -r exactly twice.\n"); needHelp = true; }
    if (needHelp) { printf("%s", kHelp); return 1; }
    if (!file_exists(tumorFile)) { printf("CanvasNormalize.exe: File %s does not exist! Exiting.\n", tumorFile.c_str()); return 1; }
    for (auto& f : normals) if (!file_exists(f)) { printf("CanvasNormalize.exe: File %s does not exist! Exiting.\n", f.c_str()); return 1; }
    if (a.has("manifest") && !file_exists(a.get("manifest"))) { printf("CanvasNormalize.exe: File %s does not exist! Exiting.\n", a.get("manifest").c_str()); return 1; }
    const std::string ploidyVcf = a.get("ploidyVcfFile");
    if (a.has("ploidyVcfFile") && !file_exists(ploidyVcf)) { printf("CanvasNormalize.exe: File %s does not exist! Exiting.\n", ploidyVcf.c_str()); return 1; }
    if (mode == 2 && normals.size() > 1) { printf("CanvasNormalize.exe: Please specify only one model file.\n"); return 1; }
    if (a.has("manifest")) { fprintf(stderr, "CanvasNormalize (MI355X): -f/--manifest is not supported by this build\n"); return 1; }
    if (refFile.empty()) { fprintf(stderr, "CanvasNormalize: -w/--weightedAverageNormal is required (the reference file is written there)\n"); return 1; }
    const double minRef = std::min(range[0], range[1]), maxRef = std::max(range[0], range[1]);
    printf("CanvasNormalize (MI355X) mode %s\n", modeName[mode]);

    Phases ph("CanvasNormalize");
    AsyncCtx actx;                                              // the context comes up while the files are read
    // PloidyInfo.LoadPloidyFromVcfFileNoSampleId (CanvasNormalizeUtilities.cs:35-41)
    std::map<std::string, std::vector<PloidyIv>> ploidyByChrom; const bool havePloidy = a.has("ploidyVcfFile");
    if (havePloidy) { std::string err; if (!load_ploidy_vcf(ploidyVcf, ploidyByChrom, err)) { fprintf(stderr, "CanvasNormalize: %s\n", err.c_str()); return 1; } }
    auto need_ctx = [&]() -> canvas_ctx* { return actx.require("CanvasNormalize"); };

    // ---- 1. the reference file
    if (mode == 0 || mode == 1) {
        if (normals.size() == 1) {
            if (!copy_file(normals[0], refFile)) { fprintf(stderr, "cannot copy %s to %s\n", normals[0].c_str(), refFile.c_str()); return 1; }
        } else if (normals.size() > 64) {
            fprintf(stderr, "CanvasNormalize (MI355X): at most 64 control samples are supported (%zu given)\n", normals.size()); return 1;
        } else {
            std::vector<Bins> nb(normals.size());
            for (size_t s = 0; s < normals.size(); s++) if (!read_bins(normals[s], 4, nb[s])) { fprintf(stderr, "cannot read %s\n", normals[s].c_str()); return 1; }
            const int64_t n = nb[0].size();
            for (auto& b : nb) if (b.size() != n) { fprintf(stderr, "CanvasNormalize: the control files have different numbers of bins\n"); return 1; }
            Bins tb;
            if (mode == 1) {
                if (!read_bins(tumorFile, 4, tb)) { fprintf(stderr, "cannot read %s\n", tumorFile.c_str()); return 1; }
                if (tb.size() != n) { fprintf(stderr, "CanvasNormalize: the tumour and the control files have different numbers of bins\n"); return 1; }
            }
            ph.mark("read_controls");
            canvas_ctx* ctx = need_ctx(); if (!ctx || n == 0) { if (ctx) fprintf(stderr, "CanvasNormalize: empty control files\n"); return 1; }
            std::vector<Dev*> dn; std::vector<const double*> ptrs;
            for (auto& b : nb) { dn.push_back(new Dev(ctx, n * 8)); ptrs.push_back(dn.back()->as<double>()); TOOL_TRY(ctx, canvas_memcpy_h2d(ctx, dn.back()->p, b.value.data(), n * 8)); }
            if (mode == 0) {
                // WeightedAverageReferenceGenerator.Run (WeightedAverageReferenceGenerator.cs:34-68)
                Dev dw(ctx, n * 8); std::vector<double> w(normals.size()), weighted((size_t)n);
                TOOL_TRY(ctx, canvas_normalize_reference(ctx, (int32_t)normals.size(), ptrs.data(), n, nullptr, 0, dw.as<double>(), w.data()));
                TOOL_TRY(ctx, canvas_memcpy_d2h(ctx, weighted.data(), dw.p, n * 8));
                for (auto* d : dn) delete d;
                ph.mark("device_reference");
                // every line of the first control file keeps its tokens, field 4 becomes String.Format("{0}", w) (G15)
                std::string data; if (!read_gz_all(normals[0], data)) { fprintf(stderr, "cannot read %s\n", normals[0].c_str()); return 1; }
                std::vector<std::pair<size_t, size_t>> lines;
                for (size_t p = 0; p < data.size();) { size_t e = data.find('\n', p); if (e == std::string::npos) e = data.size(); size_t le = e; if (le > p && data[le - 1] == '\r') le--; lines.push_back({p, le}); p = e + 1; }
                if ((int64_t)lines.size() != n) { fprintf(stderr, "CanvasNormalize: %s has lines with fewer than four fields\n", normals[0].c_str()); return 1; }
                if (!write_gz_rows(refFile, n, [&](int64_t i, std::string& o) {
                        auto t = split_tab(data.substr(lines[i].first, lines[i].second - lines[i].first));
                        t[3] = format_g(weighted[i], 15);
                        for (size_t k = 0; k < t.size(); k++) { if (k) o.push_back('\t'); o += t[k]; } }))
                    { fprintf(stderr, "cannot write %s\n", refFile.c_str()); return 1; }
            } else {
                // BestLR2ReferenceGenerator.Run (BestLR2ReferenceGenerator.cs:31-80)
                Dev dt(ctx, n * 8); TOOL_TRY(ctx, canvas_memcpy_h2d(ctx, dt.p, tb.value.data(), n * 8));
                int32_t best = -1, replayed = 0; std::vector<double> msl(normals.size()); std::vector<int64_t> ign(normals.size());
                TOOL_TRY(ctx, canvas_normalize_best_normal(ctx, dt.as<double>(), (int32_t)normals.size(), ptrs.data(), n, nullptr, 0, &best, msl.data(), ign.data(), &replayed));
                for (auto* d : dn) delete d;
                printf("BestLR2: normal %d of %zu chosen (%d replayed exactly)\n", best + 1, normals.size(), replayed);
                ph.mark("device_reference");
                if (!copy_file(normals[(size_t)best], refFile)) { fprintf(stderr, "cannot copy %s to %s\n", normals[(size_t)best].c_str(), refFile.c_str()); return 1; }
            }
        }
    }
    // the tumour as CanvasIO reads it (float.Parse of the count)
    Bins tumor; if (!read_bins(tumorFile, 5, tumor)) { fprintf(stderr, "cannot read %s\n", tumorFile.c_str()); return 1; }
    if (mode == 2) {
        // PCAReferenceGenerator.Run (PCAReferenceGenerator.cs:32-69)
        Bins mu; std::vector<std::vector<double>> axes; std::string err;
        if (!read_model(normals[0], mu, axes, err)) { fprintf(stderr, "CanvasNormalize: %s\n", err.c_str()); return 1; }
        const int64_t nm = mu.size();
        for (int64_t i = 0; i < std::min(nm, tumor.size()); i++)       // VerifyBinOrder (:74-81) over the zipped prefix
            if (!tumor.same_bin(i, mu, i)) { fprintf(stderr, "CanvasNormalize: Bins must be in the same order as those in the model file.\n"); return 1; }
        if (axes.empty()) { fprintf(stderr, "CanvasNormalize: No axes to project onto.\n"); return 1; }
        if (axes.size() > 64) { fprintf(stderr, "CanvasNormalize (MI355X): at most 64 axes are supported (%zu in the model)\n", axes.size()); return 1; }
        if (nm > tumor.size()) { fprintf(stderr, "CanvasNormalize: Vector and the axes must be of the same dimension.\n"); return 1; }   // Project: the model is longer than the sample
        if (nm == 0) { fprintf(stderr, "CanvasNormalize: the model file has no bins\n"); return 1; }
        ph.mark("read_model");
        canvas_ctx* ctx = need_ctx(); if (!ctx) return 1;
        // (a sample longer than the model is cut to the model's length, as Enumerable.Zip does)
        std::vector<float> cnt((size_t)nm), muf((size_t)nm), ref((size_t)nm);
        for (int64_t i = 0; i < nm; i++) { cnt[i] = (float)tumor.value[i]; muf[i] = (float)mu.value[i]; }
        Dev dc(ctx, nm * 4), dm(ctx, nm * 4), dr(ctx, nm * 4);
        TOOL_TRY(ctx, canvas_memcpy_h2d(ctx, dc.p, cnt.data(), nm * 4)); TOOL_TRY(ctx, canvas_memcpy_h2d(ctx, dm.p, muf.data(), nm * 4));
        std::vector<Dev*> da; std::vector<const double*> ptrs;
        for (auto& ax : axes) { da.push_back(new Dev(ctx, nm * 8)); ptrs.push_back(da.back()->as<double>()); TOOL_TRY(ctx, canvas_memcpy_h2d(ctx, da.back()->p, ax.data(), nm * 8)); }
        double medianRatio = 0; std::vector<double> sizes(axes.size()); int32_t orth = 0;
        TOOL_TRY(ctx, canvas_normalize_pca_reference(ctx, nm, dc.as<float>(), dm.as<float>(), (int32_t)axes.size(), ptrs.data(), minRef, maxRef, dr.as<float>(), &medianRatio, sizes.data(), &orth));
        for (auto* d : da) delete d;
        if (!orth) { fprintf(stderr, "CanvasNormalize: Axes are not orthogonal to each other in %s.\n", normals[0].c_str()); return 1; }
        TOOL_TRY(ctx, canvas_memcpy_d2h(ctx, ref.data(), dr.p, nm * 4));
        ph.mark("device_reference");
        if (!write_bins(refFile, tumor, nullptr, ref)) { fprintf(stderr, "cannot write %s\n", refFile.c_str()); return 1; }
    }
    ph.mark("write_reference");

    // ---- 2. ratios of the tumour to the reference file read back (LSNormRatioCalculator / RawRatioCalculator)
    Bins refBins; if (!read_bins(refFile, 5, refBins)) { fprintf(stderr, "cannot read %s\n", refFile.c_str()); return 1; }
    int64_t n = std::min(tumor.size(), refBins.size());
    if (mode != 2 && tumor.size() != refBins.size()) { fprintf(stderr, "CanvasNormalize (MI355X): the tumour (%lld bins) and the reference (%lld bins) differ in length\n", (long long)tumor.size(), (long long)refBins.size()); return 1; }
    std::vector<int32_t> ploidy((size_t)n, 2);
    if (havePloidy) {
        for (int64_t i = 0; i < n; i++) {
            auto it = ploidyByChrom.find(tumor.chromNames[tumor.chr[i]]);
            const int cn = reference_copy_number(it == ploidyByChrom.end() ? nullptr : &it->second, tumor.start[i], tumor.stop[i]);
            if (cn < 0) { fprintf(stderr, "CanvasNormalize: reference ploidy outside 0..4 on %s (the reference throws IndexOutOfRangeException)\n", tumor.chromNames[tumor.chr[i]].c_str()); return 1; }
            ploidy[i] = cn;
        }
    }
    ph.mark("read_ratio_inputs");
    std::vector<int32_t> keep; std::vector<float> ratio, count;
    if (n > 0) {
        canvas_ctx* ctx = need_ctx(); if (!ctx) return 1;
        std::vector<float> s((size_t)n), r((size_t)n);
        for (int64_t i = 0; i < n; i++) { s[i] = (float)tumor.value[i]; r[i] = (float)refBins.value[i]; }
        Dev ds(ctx, n * 4), dr(ctx, n * 4), dp(ctx, n * 4), dk(ctx, n * 4), dra(ctx, n * 4), dco(ctx, n * 4);
        TOOL_TRY(ctx, canvas_memcpy_h2d(ctx, ds.p, s.data(), n * 4)); TOOL_TRY(ctx, canvas_memcpy_h2d(ctx, dr.p, r.data(), n * 4));
        TOOL_TRY(ctx, canvas_memcpy_h2d(ctx, dp.p, ploidy.data(), n * 4));
        int64_t k = 0; double lsf = 1;
        TOOL_TRY(ctx, canvas_normalize_ratio(ctx, n, ds.as<float>(), dr.as<float>(), nullptr, 0, mode == 2 ? 1 : 0, mode == 2 ? minRef : 1.0, mode == 2 ? maxRef : HUGE_VAL,
                                             dp.as<int32_t>(), dk.as<int32_t>(), dra.as<float>(), dco.as<float>(), &k, &lsf));
        keep.resize((size_t)k); ratio.resize((size_t)k); count.resize((size_t)k);
        if (k > 0) { TOOL_TRY(ctx, canvas_memcpy_d2h(ctx, keep.data(), dk.p, k * 4)); TOOL_TRY(ctx, canvas_memcpy_d2h(ctx, ratio.data(), dra.p, k * 4)); TOOL_TRY(ctx, canvas_memcpy_d2h(ctx, count.data(), dco.p, k * 4)); }
    }
    ph.mark("device_ratio");
    // ---- 3. RatiosToCounts -> -o (CanvasIO.WriteToTextFile)
    if (!write_bins(outFile, tumor, &keep, count)) { fprintf(stderr, "cannot write %s\n", outFile.c_str()); return 1; }
    // ---- 4. WriteCndFile (CanvasNormalizeUtilities.cs:47-90): fragment count, reference count, chromosome, start, end, ratio; floats as float.ToString() (G7)
    {
        for (int32_t i : keep) if (!tumor.same_bin(i, refBins, i)) { fprintf(stderr, "CanvasNormalize: Reference bins and ratio bins are not in the same order.\n"); return 1; }
        const std::string cnd = outFile + ".cnd";
        FILE* f = fopen(cnd.c_str(), "wb"); if (!f) { fprintf(stderr, "cannot write %s\n", cnd.c_str()); return 1; }
        std::string o = "Fragment Count,Reference Count,Chromosome,Start,End,Unsmoothed Log Ratio\n";
        for (size_t k = 0; k < keep.size(); k++) {
            const int32_t i = keep[k];
            o += format_g((double)(float)tumor.value[i], 7); o.push_back(','); o += format_g((double)(float)refBins.value[i], 7); o.push_back(',');
            o += tumor.chromNames[tumor.chr[i]]; o.push_back(','); append_int(o, tumor.start[i]); o.push_back(','); append_int(o, tumor.stop[i]); o.push_back(',');
            o += format_g((double)ratio[k], 7); o.push_back('\n');
            if (o.size() > (1u << 20)) { fwrite(o.data(), 1, o.size(), f); o.clear(); }
        }
        const bool ok = fwrite(o.data(), 1, o.size(), f) == o.size();
        if (fclose(f) != 0 || !ok) { fprintf(stderr, "cannot write %s\n", cnd.c_str()); return 1; }
    }
    ph.mark("write");
    return finish(ph, 0);
}
