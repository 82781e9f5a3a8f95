// The framing loop of BamChunkLoop::run (canvas_amd/tools/tool_common.hpp) on one inflated chunk in host memory, with the three tools' `frame` callables restated:
// what the host path spends per chunk on the walk of the block_size chain, for tools/frame_probe.py to set beside canvas_bam_frame.  One thread, as in the tools.
// usage: frame_walk_host CHUNK_FILE KIND(1 snv, 2 hits, 3 fragments) REF_ID SORTED REPEATS  ->  one JSON line
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../canvas_amd/tools/bam_io.hpp"

static bool passes_read_filters(const uint8_t* r, const BamFixed& a, bool pairedEnd) {
    if (a.flag & 0x4) return false;
    if (a.flag & 0x200) return false;
    if (a.flag & 0x400) return false;
    if (a.flag & 0x10) return false;
    if (a.flag & 0x900) return false;
    if (a.n_cigar == 0) return false;
    const uint32_t c0 = le32(r + 32 + a.l_read_name);
    if ((c0 & 0xF) != 0 || (c0 >> 4) < 35) return false;
    if (pairedEnd && !(a.flag & 0x2)) return false;
    return true;
}

int main(int argc, char** argv) {
    if (argc != 6) { fprintf(stderr, "usage: frame_walk_host CHUNK_FILE KIND REF_ID SORTED REPEATS\n"); return 2; }
    FILE* f = fopen(argv[1], "rb"); if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    fseek(f, 0, SEEK_END); const size_t len = (size_t)ftell(f); fseek(f, 0, SEEK_SET);
    std::vector<uint8_t> chunk(len); if (fread(chunk.data(), 1, len, f) != len) return 2;
    fclose(f);
    const int kind = atoi(argv[2]), refId = atoi(argv[3]), sorted = atoi(argv[4]), repeats = atoi(argv[5]);
    std::vector<uint64_t> offs(len / 36 + 16);
    std::vector<double> ms; long long nrec = 0, seen = 0; size_t used = 0; int event = 0;
    for (int rep = 0; rep <= repeats; rep++) {
        const auto t0 = std::chrono::steady_clock::now();
        const uint8_t* buf = chunk.data(); size_t at = 0; nrec = 0; seen = 0; event = 0; int32_t last = kind == 1 ? -1 : INT32_MIN;
        while (at + 4 <= len) {
            const int32_t bs = (int32_t)le32(buf + at);
            if (bs >= 32 && (size_t)bs > len - at - 4) break;
            const uint8_t* r = buf + at + 4; BamFixed fx;
            if (!fx.decode(r, bs)) { event = 2; break; }
            seen++;
            int f = 0;                                   // 0 take, 1 skip, 2 take and stop, 3 stop, 4 fail
            if (kind == 1) {
                if (fx.l_seq < 0 || 32ull + fx.l_read_name + 4ull * fx.n_cigar + ((uint64_t)fx.l_seq + 1) / 2 + (uint64_t)fx.l_seq > (uint64_t)bs) f = 4;
                else if (fx.refID < 0 || fx.pos < 0 || fx.refID > refId) f = 3;
                else if (fx.refID != refId) f = 1;
                else if (fx.pos < last) f = 4;
                else last = fx.pos;
            } else if (kind == 2) {
                if (!fx.name_and_cigar_fit(bs)) f = 4;
                else if (fx.refID == refId && !sorted) f = 0;
                else if (!passes_read_filters(r, fx, true)) f = 0;
                else if (fx.refID != refId) f = 2;
                else if (fx.pos < last) f = 4;
                else last = fx.pos;
            } else {
                if (!fx.name_and_cigar_fit(bs)) f = 4;
                else if (fx.refID != refId) f = 2;
            }
            if (f == 4) { event = 2; break; }
            if (f == 3) { event = 1; break; }
            if (f != 1) offs[(size_t)nrec++] = (uint64_t)at;
            at += 4 + (size_t)bs;
            if (f == 2) { event = 1; break; }
        }
        used = at;
        if (rep) ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(ms.begin(), ms.end());
    printf("{\"records\": %lld, \"taken\": %lld, \"used\": %zu, \"event\": %d, \"ms_median\": %.4f, \"ms_min\": %.4f, \"checksum\": %llu}\n", seen, nrec, used, event,
           ms[ms.size() / 2], ms.front(), (unsigned long long)(nrec ? offs[(size_t)nrec - 1] : 0));
    return 0;
}
