// The host comparator of tools/inflate_probe.py: the BGZF blocks of a file from offset AT until their inflated sizes reach MAX_OUT, through inflate_raw
// (canvas_amd/tools/bam_io.hpp) on the tools' own thread pool (fast_io.hpp: parallel_for, CANVAS_TOOL_THREADS), straight into one buffer: what BamChunkLoop does per
// chunk.  One warm-up pass, then REPEATS timed ones; prints one JSON line.
// build: g++ -O2 -std=c++17 -pthread tools/probe_src/inflate_raw_host.cpp -lz -o inflate_raw_host
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include "../../canvas_amd/tools/fast_io.hpp"

int main(int argc, char** argv) {
    if (argc != 5) { fprintf(stderr, "usage: inflate_raw_host FILE AT MAX_OUT REPEATS\n"); return 2; }
    tool::MappedFile mf; if (!mf.open(argv[1])) { fprintf(stderr, "cannot map %s\n", argv[1]); return 2; }
    const uint8_t* F = (const uint8_t*)mf.p; size_t at = strtoull(argv[2], nullptr, 10); const size_t maxOut = strtoull(argv[3], nullptr, 10); const int repeats = atoi(argv[4]);
    std::vector<BgzfBlock> blocks; std::vector<size_t> pre; size_t total = 0;
    while (total < maxOut && at < mf.n) {
        BgzfBlock b; const size_t size = bgzf_parse(F + at, mf.n - at, b);
        if (size == 0 || size > mf.n - at) { fprintf(stderr, "damaged block at %zu\n", at); return 2; }
        b.in += at; blocks.push_back(b); pre.push_back(total); total += b.isize; at += size;
    }
    std::vector<uint8_t> out(total);
    std::vector<double> ms;
    for (int r = 0; r <= repeats; r++) {
        std::atomic<bool> ok(true);
        const auto t0 = std::chrono::steady_clock::now();
        tool::parallel_for((int64_t)blocks.size(), [&](int64_t i) { const BgzfBlock& b = blocks[(size_t)i]; if (b.isize && !inflate_raw(F + b.in, b.clen, out.data() + pre[(size_t)i], b.isize)) ok = false; });
        const double t = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (!ok) { fprintf(stderr, "a block does not inflate to its recorded size\n"); return 2; }
        if (r) ms.push_back(t);
    }
    std::sort(ms.begin(), ms.end());
    printf("{\"blocks\": %zu, \"inflated_bytes\": %zu, \"threads\": %d, \"ms_median\": %.3f, \"ms_min\": %.3f}\n", blocks.size(), total, tool::io_threads(), ms[ms.size() / 2], ms[0]);
    return 0;
}
