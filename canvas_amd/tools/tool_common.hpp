// Shared host code of the drop-in tool drivers (CanvasBin / CanvasClean / CanvasPartition / CanvasNormalize / CanvasSNV / FlagUniqueKmers): option parsing in the reference's NDesk OptionSet
// style, gzip text I/O of the intermediate files (CanvasCommon/IO.cs), .NET Core 2.x number formatting, and the
// IsAutosome assumption (Isas.SequencingFiles is not in /root/reference: "optional chr prefix + integer").
// The drivers use ONLY the C ABI of include/canvas_hip.h (what the C# hosts would P/Invoke).
#pragma once
#include <zlib.h>
#include <time.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <functional>
#include <map>
#include <memory>
#include <atomic>
#include <set>
#include <string>
#include <thread>
#include <vector>
#include <unistd.h>
#include <sys/mman.h>
#include <mutex>
#include <new>
#include "../../include/canvas_hip.h"
#include "fast_io.hpp"

#ifndef CANVAS_SRC_HASH
#define CANVAS_SRC_HASH "unhashed-build-0000000000000000"
#endif
__attribute__((used)) static const char tool_src_hash_marker[] = "CANVAS_SRC_HASH=" CANVAS_SRC_HASH;

// ---- big host buffers (bases, hits, fragment lengths: gigabytes per run) come from 2 MB-aligned anonymous mappings advised to transparent huge pages: the box runs THP
// in "madvise" mode, and 4 KB pages cost a fault per page while a file is read plus 0.5 s of page freeing when the process leaves.  Everything below 8 MB is malloc's.
// (each tool is one translation unit: the replaced global operators live here.)  CANVAS_TOOL_NO_HUGEPAGES=1 keeps malloc for everything.
// This header DEFINES the global operators: it must be part of exactly one translation unit per executable.  A second inclusion is a duplicate-symbol error at link time
// (the definition below has external linkage on purpose) instead of an ODR violation nobody sees.  Memory released by a library that carries its own allocator never
// reaches these operators (libcanvas_hip.so hands out no ownership of host memory); blocks of 8 MB and more that such a library allocates for itself are its own business.
extern "C" { int canvas_tool_common_hpp_is_in_one_translation_unit = 1; }
namespace tool { struct BigAllocs { std::mutex m; std::map<void*, size_t> len; }; static inline BigAllocs& big_allocs() { static BigAllocs* b = new BigAllocs; return *b; } }
void* operator new(size_t n) {
    static const bool huge = !getenv("CANVAS_TOOL_NO_HUGEPAGES");
    const size_t H = (size_t)2 << 20;
    if (huge && n >= ((size_t)8 << 20)) {
        const size_t len = (n + H - 1) & ~(H - 1);
        char* p = (char*)mmap(nullptr, len + H, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (p != (char*)MAP_FAILED) {
            char* q = (char*)(((uintptr_t)p + H - 1) & ~(uintptr_t)(H - 1));
            if (q > p) munmap(p, (size_t)(q - p));
            if (q + len < p + len + H) munmap(q + len, (size_t)((p + len + H) - (q + len)));
            madvise(q, len, MADV_HUGEPAGE);
            { auto& B = tool::big_allocs(); std::lock_guard<std::mutex> g(B.m); B.len[q] = len; }
            return q;
        }
    }
    void* r = malloc(n ? n : 1); if (!r) throw std::bad_alloc(); return r;
}
void operator delete(void* p) noexcept {
    if (!p) return;
    if (((uintptr_t)p & (((uintptr_t)2 << 20) - 1)) == 0) {
        auto& B = tool::big_allocs(); size_t len = 0;
        { std::lock_guard<std::mutex> g(B.m); auto it = B.len.find(p); if (it != B.len.end()) { len = it->second; B.len.erase(it); } }
        if (len) { munmap(p, len); return; }
    }
    free(p);
}
void operator delete(void* p, size_t) noexcept { operator delete(p); }

namespace tool {

// ---- NDesk.OptionSet-like parsing: -x value, -x=value, --long value, --long=value, /x value; flags without value
struct Opt { std::string shortName, longName; bool takesValue; };
struct Parsed { std::multimap<std::string, std::string> values; std::vector<std::string> extra; bool has(const std::string& k) const { return values.count(k) > 0; }
    std::string get(const std::string& k, const std::string& d = "") const { auto it = values.find(k); return it == values.end() ? d : it->second; }
    std::vector<std::string> all(const std::string& k) const { std::vector<std::string> r; auto rg = values.equal_range(k); for (auto it = rg.first; it != rg.second; ++it) r.push_back(it->second); return r; } };
static Parsed parse(int argc, char** argv, const std::vector<Opt>& opts) {
    Parsed p;
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i], name, val; bool hasVal = false;
        if (a.rfind("--", 0) == 0) name = a.substr(2); else if (a.size() > 1 && (a[0] == '-' || a[0] == '/')) name = a.substr(1); else { p.extra.push_back(a); continue; }
        size_t eq = name.find_first_of("=:");
        if (eq != std::string::npos) { val = name.substr(eq + 1); name = name.substr(0, eq); hasVal = true; }
        const Opt* o = nullptr;
        for (auto& c : opts) if (c.shortName == name || c.longName == name) o = &c;
        if (!o) { p.extra.push_back(a); continue; }
        std::string key = o->longName.empty() ? o->shortName : o->longName;
        if (o->takesValue) { if (!hasVal) { if (i + 1 < argc) val = argv[++i]; else { p.extra.push_back(a); continue; } } p.values.insert({key, val}); }
        else p.values.insert({key, "1"});
    }
    return p;
}

// ---- gzip text
struct GzReader { gzFile f; explicit GzReader(const std::string& path) { f = gzopen(path.c_str(), "rb"); } ~GzReader() { if (f) gzclose(f); }
    bool ok() const { return f != nullptr; }
    bool line(std::string& out) { out.clear(); char buf[1 << 16]; bool any = false;
        while (gzgets(f, buf, sizeof buf)) { any = true; out += buf; if (!out.empty() && out.back() == '\n') break; }
        while (!out.empty() && (out.back() == '\n' || out.back() == '\r')) out.pop_back();
        return any; } };
static std::atomic<int> g_open_writers{0};      // output objects that still hold buffered data: finish() leaves without unwinding only when there is none
struct GzWriter { gzFile f; explicit GzWriter(const std::string& path) { f = gzopen(path.c_str(), "wb"); if (f) g_open_writers++; } ~GzWriter() { close(); }
    bool ok() const { return f != nullptr; } void line(const std::string& s) { gzwrite(f, s.data(), (unsigned)s.size()); gzputc(f, '\n'); }
    void close() { if (f) { gzclose(f); f = nullptr; g_open_writers--; } } };
static std::vector<std::string> split(const std::string& s, char sep) { std::vector<std::string> r; size_t a = 0; for (;;) { size_t b = s.find(sep, a); r.push_back(s.substr(a, b == std::string::npos ? b : b - a)); if (b == std::string::npos) break; a = b + 1; } return r; }
static std::vector<std::string> split_tab(const std::string& s) { return split(s, '\t'); }
// the sample's value of a FORMAT key (VCF columns 9 and 10+: "GT:GQX" and "0/1:30"); nullptr: the record has no such key
struct VcfFormat { std::vector<std::string> keys, vals; VcfFormat(const std::string& format, const std::string& sample) : keys(split(format, ':')), vals(split(sample, ':')) {}
    const std::string* find(const char* k) const { for (size_t i = 0; i < keys.size() && i < vals.size(); i++) if (keys[i] == k) return &vals[i]; return nullptr; } };
// every line of a text file without its line end, until fn returns false
static bool for_each_line(const std::string& path, const std::function<bool(const std::string&)>& fn) {
    FILE* f = fopen(path.c_str(), "rb"); if (!f) return false;
    char buf[1 << 14]; bool go = true;
    while (go && fgets(buf, sizeof buf, f)) { std::string s(buf); while (!s.empty() && (s.back() == '\n' || s.back() == '\r')) s.pop_back(); go = fn(s); }
    fclose(f); return true;
}
static bool file_exists(const std::string& p) { FILE* f = fopen(p.c_str(), "rb"); if (f) { fclose(f); return true; } return false; }

// ---- .NET Core 2.x formatting: float "F2" (7 significant digits, then half-up at 2 decimals) and double "G15"
static void sig_digits(double v, int prec, std::string& digits, int& scale) {
    char buf[64]; snprintf(buf, sizeof buf, "%.*e", prec - 1, std::fabs(v));
    digits.clear(); const char* p = buf;
    for (; *p && *p != 'e'; p++) if (*p >= '0' && *p <= '9') digits.push_back(*p);
    scale = atoi(p + 1) + 1;
    while (!digits.empty() && digits.back() == '0') digits.pop_back();
    if (digits.empty()) scale = 0;
}
static std::string format_f2(float v) {
    if (std::isnan(v)) return "NaN"; if (std::isinf(v)) return v > 0 ? "Infinity" : "-Infinity";
    std::string d; int scale; sig_digits((double)v, 7, d, scale);
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
static std::string format_g(double v, int prec) {
    if (std::isnan(v)) return "NaN"; if (std::isinf(v)) return v > 0 ? "Infinity" : "-Infinity";
    std::string d; int scale; sig_digits(v, prec, d, scale);
    if (d.empty()) return "0";
    std::string out = std::signbit(v) ? "-" : ""; int e10 = scale - 1;
    if (e10 >= prec || e10 < -5) { out.push_back(d[0]); if (d.size() > 1) { out.push_back('.'); out += d.substr(1); } char eb[16]; snprintf(eb, sizeof eb, "E%c%02d", e10 < 0 ? '-' : '+', std::abs(e10)); return out + eb; }
    if (scale <= 0) return out + "0." + std::string(-scale, '0') + d;
    for (int i = 0; i < scale; i++) out.push_back(i < (int)d.size() ? d[i] : '0');
    if ((int)d.size() > scale) { out.push_back('.'); out += d.substr(scale); }
    return out;
}

static bool is_autosome(std::string name) {
    if (name.rfind("chr", 0) == 0) name = name.substr(3);
    if (name.empty()) return false;
    for (char c : name) if (c < '0' || c > '9') return false;
    return true;
}

// excluded intervals of a BED file (Utilities.LoadBedFile, CanvasCommon/Utilities.cs:793-829): chr -> (start, stop) in file order
static bool load_bed(const std::string& path, std::map<std::string, std::vector<std::pair<int, int>>>& out) {
    return for_each_line(path, [&](const std::string& s) { auto t = split_tab(s); if (t.size() >= 3) out[t[0]].push_back({atoi(t[1].c_str()), atoi(t[2].c_str())}); return true; });
}

// PloidyInterval (PloidyInfo.cs:182-198): one-based Start = POS, End = INFO/END, Ploidy = the sample's CN field ("." = 2)
struct PloidyIv { int start, end, ploidy; };
// the single-sample ploidy VCF as Isas' VcfReader exposes it to PloidyInfo.LoadPloidyFromVcfFileNoSampleId (PloidyInfo.cs:112-165; no genotype column or more
// than one is refused); plain or gzip text.  CanvasPartition -p and CanvasNormalize -p
static bool load_ploidy_vcf(const std::string& path, std::map<std::string, std::vector<PloidyIv>>& out, std::string& err) {
    GzReader rd(path); if (!rd.ok()) { err = "cannot open ploidy VCF '" + path + "'"; return false; }
    std::string row; int samples = -1;
    auto one_sample = [&]() {
        if (samples < 0) err = "File '" + path + "' has no #CHROM header line";
        else if (samples == 0) err = "File '" + path + "' does not contain any genotype column";
        else if (samples > 1) err = "File '" + path + "' cannot have more than one genotype columns when no sample ID provided";
        return samples == 1; };
    while (rd.line(row)) {
        if (row.empty()) continue;
        if (row[0] == '#') { if (row.rfind("#CHROM", 0) == 0) { auto h = split_tab(row); samples = (int)h.size() > 9 ? (int)h.size() - 9 : 0; } continue; }
        if (!one_sample()) return false;
        auto f = split_tab(row);
        if (f.size() < 10) { err = "malformed ploidy VCF record: " + row; return false; }
        PloidyIv iv; iv.start = atoi(f[1].c_str()); iv.end = -1; iv.ploidy = 2;
        bool haveEnd = false;
        for (auto& kv : split(f[7], ';')) if (kv.rfind("END=", 0) == 0) { iv.end = atoi(kv.c_str() + 4); haveEnd = true; }
        if (!haveEnd) { err = "ploidy VCF record without INFO/END: " + row; return false; }            // InfoFields["END"] throws KeyNotFoundException
        const VcfFormat fmt(f[8], f[9]); const std::string* cn = fmt.find("CN");
        if (!cn) { err = "File '" + path + "' must contain one genotype CN column!"; return false; }
        iv.ploidy = *cn == "." ? 2 : atoi(cn->c_str());
        out[f[0]].push_back(iv);
    }
    return one_sample();
}
// PloidyInfo.GetReferenceCopyNumber of the bin [start, stop) (PloidyInfo.cs:56-75, through CanvasNormalizeUtilities.GetPloidy, :13-20): the copy number that
// covers most bases, 2 on a chromosome the VCF does not list; -1: a ploidy outside 0..4 indexes past baseCounts (the reference throws)
static int reference_copy_number(const std::vector<PloidyIv>* ivs, int start, int stop) {
    if (!ivs) return 2;
    int baseCounts[5] = {0, 0, stop - start, 0, 0};
    for (auto& iv : *ivs) {
        if (iv.ploidy == 2) continue;
        const int overlapStart = std::max(start, iv.start - 1);
        if (overlapStart > iv.end) continue;
        const int overlapBases = std::min(stop, iv.end) - overlapStart;
        if (overlapBases <= 0) continue;
        if (iv.ploidy < 0 || iv.ploidy > 4) return -1;
        baseCounts[2] -= overlapBases; baseCounts[iv.ploidy] += overlapBases;
    }
    int best = 0, cn = 2;
    for (int c = 0; c < 5; c++) if (baseCounts[c] > best) { best = baseCounts[c]; cn = c; }
    return cn;
}

struct Dev {      // tiny RAII around the ABI's device memory
    canvas_ctx* ctx; void* p = nullptr;
    Dev(canvas_ctx* c, int64_t bytes) : ctx(c) { p = canvas_device_malloc(c, bytes > 0 ? bytes : 1); }
    ~Dev() { if (p) canvas_device_free(ctx, p); }
    Dev(const Dev&) = delete; Dev& operator=(const Dev&) = delete;
    template <class T> T* as() { return (T*)p; }
};
// wall-clock phases of a tool run, printed as one JSON line on stderr when CANVAS_TOOL_TIMING is set (bench.py's `executables` leg: what part of a run is file I/O)
struct Phases {
    const char* tool; std::vector<std::pair<std::string, double>> v; double t0;
    static double now() { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec; }
    explicit Phases(const char* name) : tool(name), t0(now()) {}
    void mark(const char* phase) { v.push_back({phase, now()}); }
    bool reported = false;
    ~Phases() { report(); }
    void report() {
        if (reported || !getenv("CANVAS_TOOL_TIMING")) return;
        reported = true;
        std::string js = std::string("{\"tool\": \"") + tool + "\", \"phases\": {"; double prev = t0;
        for (size_t i = 0; i < v.size(); i++) { char b[96]; snprintf(b, sizeof b, "%s\"%s\": %.4f", i ? ", " : "", v[i].first.c_str(), v[i].second - prev); js += b; prev = v[i].second; }
        // (wall-clock stamps of the first and the last statement of main: what lies outside them — the loader in front, the kernel's teardown of the process behind — is the
        // difference to the caller's own clock around the process, tools/exe_probe.sh)
        struct timespec tr; clock_gettime(CLOCK_REALTIME, &tr); const double real = (double)tr.tv_sec + 1e-9 * (double)tr.tv_nsec;
        char b[160]; snprintf(b, sizeof b, "}, \"total\": %.4f, \"main_entered_unix\": %.4f, \"leaving_unix\": %.4f}", now() - t0, real - (now() - t0), real); js += b;
        fprintf(stderr, "%s\n", js.c_str());
        if (FILE* f = fopen("/proc/self/smaps_rollup", "r")) {      // how much of the process is resident, and how much of that in transparent huge pages (what leaving the process has to give back)
            char line[256]; std::string rss, thp;
            while (fgets(line, sizeof line, f)) { if (!strncmp(line, "Rss:", 4)) rss = line + 4; if (!strncmp(line, "AnonHugePages:", 14)) thp = line + 14; }
            fclose(f);
            auto trim = [](std::string v) { while (!v.empty() && (v.back() == '\n' || v.back() == ' ')) v.pop_back(); size_t a = v.find_first_not_of(' '); return a == std::string::npos ? std::string() : v.substr(a); };
            fprintf(stderr, "[memory] resident %s, of it in transparent huge pages %s\n", trim(rss).c_str(), trim(thp).c_str());
        }
    }
};
// The GPU context is created on a helper thread while the main thread reads and parses the input files (HIP initialisation + the context's pinned buffers and streams
// take 0.15-0.3 s on a cold process; no file of a tool depends on it).  get() joins.
struct AsyncCtx {
    std::thread th; canvas_ctx* ctx = nullptr;
    // warm (optional): run on the helper thread behind canvas_create — e.g. a CBS call on a toy sample, so that the code objects are loaded and the launcher threads, streams
    // and engine buffers of the method exist by the time the real coverage has been read (a cold process paid 0.45 s in the device phase of -m CBS for 0.1 s of work)
    explicit AsyncCtx(std::function<void(canvas_ctx*)> warm = nullptr) { th = std::thread([this, warm] { ctx = canvas_create(0); if (ctx && !getenv("CANVAS_TOOL_KEEP_PINNING")) (void)canvas_set_one_shot(ctx, 1);      // (one OS process per sample: nothing amortises pinned staging)
                                                                                              if (ctx && warm && !getenv("CANVAS_TOOL_NO_WARMUP")) warm(ctx); }); }
    canvas_ctx* get() { if (th.joinable()) th.join(); return ctx; }
    // get(), with the one message of a tool that finds no device
    canvas_ctx* require(const char* toolName) { if (!get()) fprintf(stderr, "%s (MI355X): no usable GPU (this build has no CPU fallback)\n", toolName); return ctx; }
    ~AsyncCtx() { if (th.joinable()) th.join(); }
};
// End of a successful run: every output file is closed by now; the process leaves without unwinding (freeing gigabytes of host vectors, the context's device buffers and
// the HIP runtime's own teardown cost 0.1-0.6 s of wall time and change nothing on disk).  CANVAS_TOOL_FULL_TEARDOWN=1 returns through main instead.
static inline int finish(Phases& ph, int rc) {
    ph.report(); fflush(stdout); fflush(stderr);
    if (g_open_writers.load() != 0) return rc;      // (a writer that is still open flushes in its destructor: leave through main)
    // Leaving costs CanvasBin as much as its longest phase, and nothing done here changes it (measured, tools/exe_probe.sh + tools/exit_probe.sh: stamps of main's last
    // statement against the caller's clock): 0.43 s pass between _exit and the caller's wait returning, of which 0.26 s is the kernel giving back 7.6 GB of resident host
    // pages — 37 ms per GB, with or without a GPU in the process — and 0.07-0.09 s the driver's release of a process that has used the device.  Freeing the device buffers and
    // destroying the context first (4 ms) leaves the figure where it is, handing the pages to a forked child makes it worse (0.47 s), and unwinding main frees the same pages in
    // user space for the same price.  What would help is holding less anonymous memory: binning straight from the mapped .dat / FASTA files.
    if (!getenv("CANVAS_TOOL_FULL_TEARDOWN")) _exit(rc);
    return rc;
}
// (CANVAS_TOOL_FULL_TEARDOWN + CANVAS_TOOL_TIMING: where the unwinding of main spends its time — declared BEFORE the object whose destruction it reports)
struct ExitStamp { const char* what; explicit ExitStamp(const char* w) : what(w) {}
    ~ExitStamp() { if (getenv("CANVAS_TOOL_TIMING") && getenv("CANVAS_TOOL_FULL_TEARDOWN")) fprintf(stderr, "[teardown] %.4f s  %s\n", Phases::now(), what); } };
#define TOOL_TRY(ctx, expr) do { int32_t rc_ = (expr); if (rc_ != 0) { fprintf(stderr, "%s failed (%d): %s\n", #expr, rc_, canvas_last_error(ctx)); return 1; } } while (0)

// ---- a BAM as chunks of raw record bytes on the device (CanvasSNV's pileup, CanvasBin -c): the chunk format of canvas_snv_count / canvas_hits_from_bam.
// The file is mapped, the BGZF blocks of a chunk are inflated on the worker threads straight into one of two staging buffers (registered with the runtime), the
// block_size chain is walked once for the byte offset of every record the tool takes, a record the chunk ends inside is carried over to the next one, and the chunk is
// uploaded asynchronously: chunk k + 1 is inflated while chunk k is uploaded and consumed.  What the tools differ in comes as three callables:
//   setup(ctx)                        once, when the staging buffers exist and before the first chunk is framed (the tool's own device arrays); 0 or the exit code
//   frame(r, fx, block_size)          one record: r = its 32 fixed bytes (the whole record lies behind them), fx = the same decoded (block_size >= 32 is checked)
//   consume(dRec, used, dOff, nrec)   queue the device work of a chunk of nrec taken records (nrec > 0); the library's return code
// CANVAS_TOOL_DEVICE_INFLATE=1 (configuration of the executables, like the chunk size; off by default): the chunk's compressed bytes and a table of its blocks go up
// instead, canvas_bgzf_inflate writes the record bytes straight into the buffer consume reads, and they are copied DOWN into the staging buffer for the framing, which
// is the same code.  No host thread inflates and no inflated chunk is uploaded; only the carried tail (less than one record) goes up from the host copy.  A block the
// device refuses is a block that "does not inflate to its recorded size".  The chunks are not overlapped in this form.
// CANVAS_TOOL_DEVICE_FRAME=1 (configuration as well, off by default, implies device inflation): the framing moves to the device too.  `rule` restates the tool's `frame`
// for canvas_bam_frame (csrc/bam_frame.hpp); the call leaves the offsets of the taken records in the buffer consume reads and says how many there are, where the carried
// tail starts and whether the chain met a record that stops or fails the tool.  The tail moves to the front of the other buffer on the device: no inflated chunk and no
// offset table crosses PCIe in either direction, and no staging buffer is pinned.  For a malformed or unsorted record the loop copies that one record's head down and
// lets `frame` say what it says on the host path (carried_pos hands it the position the record was compared with); messages and exit codes are the same.
// CANVAS_TOOL_CHECK_CRC=1 (bam_io.hpp; configuration, off by default): on the host path the worker thread that inflated a block sums it with zlib's crc32(); on the two
// device paths canvas_bgzf_crc32 is queued behind canvas_bgzf_inflate on the same descriptors, with its statuses, and its summary is read where the inflate's is.  The
// compressed stretch that goes up is 8 bytes longer: the last block's trailer.  A block that fails ends the loop as one that does not inflate does.
enum class BamFrame { Take, Skip, TakeAndStop, Stop, Fail };      // TakeAndStop / Stop: nothing behind this record is read; Fail: the tool has said why (unless quiet)
struct BamChunkLoop {
    const char* tool; std::string bam; uint64_t voff = 0; size_t chunkBytes = (size_t)32 << 20;
    bool quiet = false;               // no message for input the loop itself refuses (the caller has an answer of its own for such a file)
    const char* profile = nullptr;    // with CANVAS_TOOL_TIMING: the library scope whose device time goes to kernelMs
    double tInflate = 0, tDevice = 0, kernelMs = 0; long long records = 0, chunks = 0, bytesUp = 0;
    bool deviceInflate = false; double inflateKernelMs = 0;      // CANVAS_TOOL_DEVICE_INFLATE; with CANVAS_TOOL_TIMING the device time of canvas_bgzf_inflate
    bool deviceFrame = false; double frameKernelMs = 0; long long framedWrong = 0;      // CANVAS_TOOL_DEVICE_FRAME; the device time of canvas_bam_frame, tiles it walked twice
    bool checkCrc = false; double crcKernelMs = 0;                // CANVAS_TOOL_CHECK_CRC; on the device paths the device time of canvas_bgzf_crc32
    std::function<void(int32_t)> carried_pos;                   // device framing, an unsorted record: the position it was compared with, before `frame` sees the record
    // the end of the tool's timing line
    std::string timing_tail() const { char b[288]; snprintf(b, sizeof b, ", \"device_inflate\": %d, \"inflate_kernel_ms\": %.4f, \"device_frame\": %d, \"frame_kernel_ms\": %.4f, \"check_crc\": %d, \"crc_kernel_ms\": %.4f",
                                                             deviceInflate ? 1 : 0, inflateKernelMs, deviceFrame ? 1 : 0, frameKernelMs, checkCrc ? 1 : 0, crcKernelMs); return b; }
    void chunk_bytes_from(const char* envName) { if (const char* e = getenv(envName)) { const long long v = atoll(e); if (v >= 65536) chunkBytes = (size_t)v; } }
    // 0: the file was read to its end or to the record that stopped it, everything is queued and waited for.  1: the device or the runtime failed (message printed).
    // 2: the input was refused (message printed unless quiet, or by frame).  Any other value: what setup returned.
    template <class Setup, class Frame, class Consume>
    int run(AsyncCtx& actx, canvas_ctx*& ctx, double tLoop0, Setup setup, Frame frame, Consume consume, const canvas_bam_frame_rule& rule) {
        MappedFile mf; if (!mf.open(bam)) { fprintf(stderr, "%s: cannot map %s\n", tool, bam.c_str()); return 1; }
        const uint8_t* F = (const uint8_t*)mf.p; const size_t FN = mf.n;
        // blocks of the first chunk: sizes the buffers (a small file gets small ones: pinning costs time per megabyte)
        size_t fileAt = (size_t)(voff >> 16); size_t skip = (size_t)(voff & 0xFFFF);
        std::vector<BgzfBlock> blocks; bool eof = false;          // (`in` made an offset in the file)
        auto collect = [&](size_t& total) -> bool {
            blocks.clear(); total = 0;
            while (total < chunkBytes) {
                if (fileAt >= FN) { eof = true; break; }
                BgzfBlock b; const size_t size = bgzf_parse(F + fileAt, FN - fileAt, b);
                if (size == 0 || size > FN - fileAt) { if (!quiet) fprintf(stderr, "%s: %s: truncated or damaged BGZF block at byte %zu\n", tool, bam.c_str(), fileAt); return false; }
                b.in += fileAt; blocks.push_back(b); total += b.isize; fileAt += size;
            }
            return true;
        };
        size_t total = 0; if (!collect(total)) return 2;
        const size_t cap = 2 * std::min(chunkBytes + 65536, std::max<size_t>(total, 65536)) + 2 * 65536, offCap = cap / 36 + 16;
        if (!(ctx = actx.require(tool))) return 1;
        const bool timing = getenv("CANVAS_TOOL_TIMING") != nullptr;
        if (timing && profile) (void)canvas_profile_enable(ctx, 1);
        { const char* e = getenv("CANVAS_TOOL_DEVICE_FRAME"); deviceFrame = e && atoi(e) == 1; }
        { const char* e = getenv("CANVAS_TOOL_DEVICE_INFLATE"); deviceInflate = deviceFrame || (e && atoi(e) == 1); }
        checkCrc = bgzf_check_crc();
        if (timing && checkCrc && deviceInflate) (void)canvas_profile_enable(ctx, 1);
        const size_t hostCap = deviceFrame ? 1 : cap, hostOffCap = deviceFrame ? 1 : offCap;      // (framed on the device: no staging buffers)
        std::unique_ptr<uint8_t[]> hRec[2] = {std::unique_ptr<uint8_t[]>(new uint8_t[hostCap]), std::unique_ptr<uint8_t[]>(new uint8_t[hostCap])};
        std::unique_ptr<uint64_t[]> hOff[2] = {std::unique_ptr<uint64_t[]>(new uint64_t[hostOffCap]), std::unique_ptr<uint64_t[]>(new uint64_t[hostOffCap])};
        struct Registered { canvas_ctx* c; std::vector<void*> v; ~Registered() { for (void* p : v) (void)canvas_host_unregister(c, p); } } reg{ctx, {}};
        for (int i = 0; i < 2 && !deviceFrame; i++) { TOOL_TRY(ctx, canvas_host_register(ctx, hRec[i].get(), (int64_t)cap)); reg.v.push_back(hRec[i].get());
                                      TOOL_TRY(ctx, canvas_host_register(ctx, hOff[i].get(), (int64_t)(offCap * 8))); reg.v.push_back(hOff[i].get()); }
        Dev dRec0(ctx, (int64_t)cap), dRec1(ctx, (int64_t)cap), dOff0(ctx, (int64_t)(offCap * 8)), dOff1(ctx, (int64_t)(offCap * 8));
        if (!dRec0.p || !dRec1.p || !dOff0.p || !dOff1.p) { fprintf(stderr, "%s: device allocation failed: %s\n", tool, canvas_last_error(ctx)); return 1; }
        void* dRec[2] = {dRec0.p, dRec1.p}; void* dOff[2] = {dOff0.p, dOff1.p};
        if (int rc = setup(ctx)) return rc;
        std::unique_ptr<Dev> dFrameState;      // (only when the records are framed on the device)
        if (deviceFrame) {
            dFrameState.reset(new Dev(ctx, 32));
            if (!dFrameState->p) { fprintf(stderr, "%s: device allocation failed: %s\n", tool, canvas_last_error(ctx)); return 1; }
            const int64_t zero[4] = {0, 0, 0, 0};
            TOOL_TRY(ctx, canvas_memcpy_h2d(ctx, dFrameState->p, zero, 32));
            if (timing) (void)canvas_profile_enable(ctx, 1);
        }
        // device inflation: the chunk's stretch of the file, its block table and the statuses, grown as chunks need them (a level-0 block is larger than what it holds)
        std::unique_ptr<Dev> dComp, dBlk, dStatus, dCrc, dCrcStatus; size_t compCap = 0, blkCap = 0; std::vector<canvas_bgzf_block> table;
        tDevice += Phases::now() - tLoop0;

        size_t carry = 0; int cur = 0; bool done = false; std::vector<size_t> pre;
        for (;;) {
            const double t0 = Phases::now();
            uint8_t* buf = hRec[cur].get(); uint64_t* offs = hOff[cur].get();
            if (carry + total > cap) { if (!quiet) fprintf(stderr, "%s: %s: an alignment record larger than %zu bytes\n", tool, bam.c_str(), cap / 2); (void)canvas_synchronize(ctx); return 2; }
            pre.assign(blocks.size() + 1, carry);
            for (size_t i = 0; i < blocks.size(); i++) pre[i + 1] = pre[i] + blocks[i].isize;
            std::atomic<bool> ok(true), crcFailed(false);
            if (deviceInflate) {
                table.clear();                                                   // (a block of ISIZE 0 is not inflated here either)
                const size_t compAt = blocks.empty() ? 0 : blocks.front().in, compBytes = blocks.empty() ? 0 : blocks.back().in + blocks.back().clen + (checkCrc ? 8 : 0) - compAt;      // (with the last trailer: inside the file, bgzf_parse has seen to it)
                for (size_t i = 0; i < blocks.size(); i++) if (blocks[i].isize) table.push_back({(uint64_t)(blocks[i].in - compAt), (uint64_t)pre[i], (uint32_t)blocks[i].clen, blocks[i].isize});
                if (!table.empty()) {
                    if (!dComp || compBytes > compCap || table.size() > blkCap) {      // (!dComp: a first chunk whose blocks hold no deflate data at all)
                        TOOL_TRY(ctx, canvas_synchronize(ctx));                  // chunk k - 1 may still read the buffers that go
                        if (!dComp || compBytes > compCap) { compCap = compBytes + compBytes / 4; dComp.reset(); dComp.reset(new Dev(ctx, (int64_t)compCap)); }
                        if (table.size() > blkCap) { blkCap = 2 * table.size(); dBlk.reset(); dStatus.reset(); dBlk.reset(new Dev(ctx, (int64_t)(blkCap * sizeof(canvas_bgzf_block)))); dStatus.reset(new Dev(ctx, (int64_t)(blkCap * 4)));
                                                     if (checkCrc) { dCrc.reset(); dCrcStatus.reset(); dCrc.reset(new Dev(ctx, (int64_t)(blkCap * 4))); dCrcStatus.reset(new Dev(ctx, (int64_t)(blkCap * 4))); } }
                        if (!dComp->p || !dBlk->p || !dStatus->p || (checkCrc && (!dCrc->p || !dCrcStatus->p))) { fprintf(stderr, "%s: device allocation failed: %s\n", tool, canvas_last_error(ctx)); return 1; }
                    }
                    TOOL_TRY(ctx, canvas_memcpy_h2d_async(ctx, dComp->p, F + compAt, (int64_t)compBytes));
                    TOOL_TRY(ctx, canvas_memcpy_h2d_async(ctx, dBlk->p, table.data(), (int64_t)(table.size() * sizeof(canvas_bgzf_block))));
                    if (carry && !deviceFrame) TOOL_TRY(ctx, canvas_memcpy_h2d_async(ctx, dRec[cur], buf, (int64_t)carry));      // (framed on the device: the tail is there already)
                    int64_t info[4];
                    TOOL_TRY(ctx, canvas_bgzf_inflate(ctx, dComp->as<uint8_t>(), compBytes, dBlk->as<canvas_bgzf_block>(), (int64_t)table.size(), (uint8_t*)dRec[cur], cap,
                                                      dStatus->as<int32_t>(), info));
                    if (info[1] == 0 && checkCrc) {
                        int64_t ci[4];
                        TOOL_TRY(ctx, canvas_bgzf_crc32(ctx, dComp->as<uint8_t>(), compBytes, dBlk->as<canvas_bgzf_block>(), (int64_t)table.size(), (const uint8_t*)dRec[cur], cap,
                                                        dStatus->as<int32_t>(), dCrc->as<uint32_t>(), dCrcStatus->as<int32_t>(), ci));
                        if (ci[1] != 0) crcFailed = true;
                    }
                    if (info[1] != 0) ok = false;
                    else if (!crcFailed && !deviceFrame) TOOL_TRY(ctx, canvas_memcpy_d2h(ctx, buf + carry, (uint8_t*)dRec[cur] + carry, (int64_t)total));
                }
            } else
            parallel_for((int64_t)blocks.size(), [&](int64_t i) {
                const BgzfBlock& b = blocks[(size_t)i];
                if (b.isize && !inflate_raw(F + b.in, b.clen, buf + pre[(size_t)i], b.isize)) ok = false;
                else if (b.isize && checkCrc && !bgzf_crc_ok(buf + pre[(size_t)i], b.isize, b.crc)) crcFailed = true;
            });
            const bool crcBad = ok && crcFailed;      // (a block that does not inflate comes first on every path)
            if (crcBad) ok = false;
            const size_t len = carry + total;
            // the block_size chain: one offset per record the tool takes; the shape of every record is checked here (the kernels check it again)
            size_t at = skip; skip = 0; int64_t nrec = 0; bool failed = false;
            if (at > len) { if (!quiet) fprintf(stderr, "%s: %s.bai points behind the end of a block\n", tool, bam.c_str()); (void)canvas_synchronize(ctx); return 2; }
            if (ok && deviceFrame) {
                int64_t fi[8];
                TOOL_TRY(ctx, canvas_bam_frame(ctx, (const uint8_t*)dRec[cur], (uint64_t)len, (uint64_t)at, &rule, (uint64_t*)dOff[cur], (int64_t)offCap, dFrameState->as<int64_t>(), fi));
                if (fi[3] == CANVAS_BAM_FRAME_CAPACITY) { fprintf(stderr, "%s: %s: %lld records in a chunk sized for %zu\n", tool, bam.c_str(), (long long)fi[1], offCap); return 1; }
                nrec = fi[1]; at = (size_t)fi[2]; framedWrong += fi[6];
                if (fi[3] == CANVAS_BAM_FRAME_STOPPED) done = true;
                if (fi[3] == CANVAS_BAM_FRAME_MALFORMED || fi[3] == CANVAS_BAM_FRAME_UNSORTED) {
                    // that one record's head comes down (block_size, the fixed fields, the name, the first CIGAR word), and the tool's `frame` says what it has to say
                    uint8_t head[4 + 32 + 255 + 4] = {0};
                    const size_t n = std::min(sizeof head, len - (size_t)fi[4]);
                    TOOL_TRY(ctx, canvas_memcpy_d2h(ctx, head, (const uint8_t*)dRec[cur] + fi[4], (int64_t)n));
                    const int32_t bs = (int32_t)le32(head); BamFixed fx;
                    if (!fx.decode(head + 4, bs)) { if (!quiet) fprintf(stderr, "%s: %s: malformed alignment record (block_size %d)\n", tool, bam.c_str(), bs); }
                    else { if (fi[3] == CANVAS_BAM_FRAME_UNSORTED && carried_pos) carried_pos((int32_t)fi[5]); (void)frame(head + 4, fx, bs); }
                    failed = true;
                }
            } else
            if (ok) while (at + 4 <= len) {
                const int32_t bs = (int32_t)le32(buf + at);
                if (bs >= 32 && (size_t)bs > len - at - 4) break;                            // completed by the next chunk
                const uint8_t* r = buf + at + 4; BamFixed fx;
                if (!fx.decode(r, bs)) { if (!quiet) fprintf(stderr, "%s: %s: malformed alignment record (block_size %d)\n", tool, bam.c_str(), bs); failed = true; break; }
                const BamFrame f = frame(r, fx, bs);
                if (f == BamFrame::Fail) { failed = true; break; }
                if (f == BamFrame::Stop) { done = true; break; }
                if (f != BamFrame::Skip) offs[nrec++] = (uint64_t)at;
                at += 4 + (size_t)bs;
                if (f == BamFrame::TakeAndStop) { done = true; break; }
            }
            if (!ok && !quiet) fprintf(stderr, crcBad ? "%s: %s: a BGZF block fails its CRC32\n" : "%s: %s: a BGZF block does not inflate to its recorded size\n", tool, bam.c_str());
            if (!ok || failed) { (void)canvas_synchronize(ctx); return 2; }
            const size_t used = at;
            if (!done && eof && at < len) { if (!quiet) fprintf(stderr, "%s: %s: the file ends inside an alignment record (truncated)\n", tool, bam.c_str()); (void)canvas_synchronize(ctx); return 2; }
            carry = done ? 0 : len - at;
            const double t1 = Phases::now(); tInflate += t1 - t0;
            TOOL_TRY(ctx, canvas_synchronize(ctx));                            // chunk k - 1 ran while this one was inflated
            if (carry && !deviceFrame) memcpy(hRec[cur ^ 1].get(), buf + at, carry);          // only now: the other buffer was the source of chunk k - 1's upload until the wait above
            if (carry && deviceFrame) TOOL_TRY(ctx, canvas_memcpy_d2d_async(ctx, dRec[cur ^ 1], (const uint8_t*)dRec[cur] + at, (int64_t)carry));      // (consume below only reads [0, used))
            if (nrec > 0) {
                if (!deviceInflate) TOOL_TRY(ctx, canvas_memcpy_h2d_async(ctx, dRec[cur], buf, (int64_t)used));      // (inflated on the device: the bytes are there)
                if (!deviceFrame) TOOL_TRY(ctx, canvas_memcpy_h2d_async(ctx, dOff[cur], offs, nrec * 8));
                TOOL_TRY(ctx, consume(dRec[cur], (uint64_t)used, dOff[cur], nrec));
                records += nrec; chunks++; bytesUp += (long long)used;
            }
            tDevice += Phases::now() - t1;
            if (done || eof) break;
            cur ^= 1;
            const double t2 = Phases::now();
            if (!collect(total)) { (void)canvas_synchronize(ctx); return 2; }
            tInflate += Phases::now() - t2;
        }
        const double t3 = Phases::now();
        TOOL_TRY(ctx, canvas_synchronize(ctx));
        if (timing && profile) { int32_t launches = 0; (void)canvas_profile_get(ctx, profile, &kernelMs, &launches, 1); }
        if (timing && deviceInflate) { int32_t launches = 0; (void)canvas_profile_get(ctx, "bgzf_inflate", &inflateKernelMs, &launches, 1); }
        if (timing && deviceFrame) { int32_t launches = 0; (void)canvas_profile_get(ctx, "bam_frame", &frameKernelMs, &launches, 1); }
        if (timing && checkCrc && deviceInflate) { int32_t launches = 0; (void)canvas_profile_get(ctx, "bgzf_crc32", &crcKernelMs, &launches, 1); }
        tDevice += Phases::now() - t3;
        return 0;
    }
};

}  // namespace tool
