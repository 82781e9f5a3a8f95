// canvas_amd/csrc/ws_layout.hpp on the host (tests/test_ws_layout_host.py builds this with AddressSanitizer and UndefinedBehaviorSanitizer).
//   ws_layout_host           every check below; one "ok <what>" line each, a message and exit status 1 at the first one that fails
//   ws_layout_host overrun   carves into a heap block of exactly the measured size and writes one byte past the last buffer: AddressSanitizer ends the program
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../canvas_amd/csrc/ws_layout.hpp"

#define CHECK(cond) do { if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

struct S24 { char b[24]; };
static_assert(sizeof(S24) == 24, "a 24-byte element");
static const size_t COUNTS[] = {0, 1, 255, 256, 257};
struct Range { uintptr_t at; size_t bytes; };

template <class T> static void takes(WsCarver& ws, std::vector<Range>& out) {
    for (size_t n : COUNTS) { T* p; ws.take(p, n); out.push_back({(uintptr_t)p, n * sizeof(T)}); }
}
static void layout_all(WsCarver& ws, std::vector<Range>& out) { out.clear(); takes<uint8_t>(ws, out); takes<double>(ws, out); takes<S24>(ws, out); }

// a heap block of exactly `bytes` (256-aligned, as the device allocations are): a byte behind it is AddressSanitizer's
struct Block {
    void* p = nullptr; size_t bytes = 0;
    ~Block() { free(p); }
    int32_t reserve(size_t n, void** base) { free(p); p = nullptr; bytes = n; if (posix_memalign(&p, 256, n ? n : 1) != 0) return -99; *base = p; return 0; }
    bool holds(const void* q) const { return (uintptr_t)q >= (uintptr_t)p && (uintptr_t)q < (uintptr_t)p + bytes; }
};

// aligned, in order, disjoint, ending at `end` (offsets from `base`)
static bool well_formed(const std::vector<Range>& r, uintptr_t base, size_t end) {
    uintptr_t at = base;
    for (const Range& x : r) { if (x.at % 256 != 0 || x.at < at) return false; at = x.at + x.bytes; }
    return at == base + end;
}

int main(int argc, char** argv) {
    const bool overrun = argc > 1 && !strcmp(argv[1], "overrun");
    std::string err;
    {   // an empty layout measures 0 bytes
        size_t asked = 1, bytes = 1; int calls = 0;
        const int32_t rc = ws_layout_carve("empty", 0, -7, &err, [&](size_t n, void** base) { asked = n; *base = nullptr; return 0; }, [&](WsCarver&) { calls++; }, &bytes);
        CHECK(rc == 0 && asked == 0 && bytes == 0 && calls == 2 && err.empty());
        printf("ok empty\n");
    }
    {   // the measuring pass alone: offsets from null, nothing for UndefinedBehaviorSanitizer to report
        WsCarver m(nullptr); std::vector<Range> r; layout_all(m, r);
        CHECK(r.size() == 15 && well_formed(r, 0, m.off) && r[0].at == 0);
        printf("ok measure %zu\n", m.off);
    }
    {   // measured bytes == carved end; every byte of every range written inside a block of exactly that size; the site's slack is added to the reservation only
        Block blk; std::vector<Range> r; size_t asked = 0, bytes = 0;
        int32_t rc = ws_layout_carve("slack", 4096, -7, &err, [&](size_t n, void** base) { asked = n; return blk.reserve(n, base); }, [&](WsCarver& ws) { layout_all(ws, r); }, &bytes);
        CHECK(rc == 0 && asked == bytes + 4096);
        rc = ws_layout_carve("exact", 0, -7, &err, [&](size_t n, void** base) { asked = n; return blk.reserve(n, base); }, [&](WsCarver& ws) { layout_all(ws, r); }, &bytes);
        CHECK(rc == 0 && err.empty() && asked == bytes && blk.bytes == bytes);
        CHECK(well_formed(r, (uintptr_t)blk.p, bytes));
        for (const Range& x : r) memset((void*)x.at, 0xA5, x.bytes);
        if (overrun) { memset((void*)r.back().at, 0x5A, r.back().bytes + 1); printf("the write past the block went unnoticed\n"); return 1; }
        printf("ok carve %zu\n", bytes);
    }
    {   // a status of the reserve callback is passed on, and the layout is not run on a base
        int calls = 0;
        const int32_t rc = ws_layout_carve("refused", 0, -7, &err, [&](size_t, void**) { return -3; }, [&](WsCarver&) { calls++; });
        CHECK(rc == -3 && calls == 1);
        printf("ok refused\n");
    }
    for (int grow = 0; grow < 2; grow++) {   // counts that differ between the passes: the error names the site, and nothing the caller holds points into the block
        Block blk; int pass = 0; double* a = nullptr; uint8_t* b = nullptr; size_t bytes = 77;
        err.clear();
        const int32_t rc = ws_layout_carve("site_under_test", 0, -7, &err, [&](size_t n, void** base) { return blk.reserve(n, base); },
                                           [&](WsCarver& ws) { const bool second = pass++ == 1; ws.take(a, 100); ws.take(b, second ? (grow ? 300 : 3) : 30); }, &bytes);
        CHECK(rc == -7 && err.find("site_under_test") != std::string::npos && bytes == 77);
        CHECK(!blk.holds(a) && !blk.holds(b) && pass == 3);
        printf("ok mismatch %d\n", grow);
    }
    {   // one layout on two bases (the device workspace and its pinned image): equal offsets
        Block d, h; std::vector<Range> rd, rh; size_t nd = 0, nh = 0;
        CHECK(ws_layout_carve("device", 0, -7, &err, [&](size_t n, void** base) { return d.reserve(n, base); }, [&](WsCarver& ws) { layout_all(ws, rd); }, &nd) == 0);
        CHECK(ws_layout_carve("pinned", 0, -7, &err, [&](size_t n, void** base) { return h.reserve(n, base); }, [&](WsCarver& ws) { layout_all(ws, rh); }, &nh) == 0);
        CHECK(nd == nh && rd.size() == rh.size() && d.p != h.p);
        for (size_t i = 0; i < rd.size(); i++) CHECK(rd[i].at - (uintptr_t)d.p == rh[i].at - (uintptr_t)h.p && rd[i].bytes == rh[i].bytes);
        printf("ok mirror\n");
    }
    return 0;
}
