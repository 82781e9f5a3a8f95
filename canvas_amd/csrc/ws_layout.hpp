// Workspace layouts (plain C++, no HIP): a list of buffers is declared ONCE, as a callable that does nothing but take() from a WsCarver.
// ws_layout_carve runs it on a measuring carver to learn its size, reserves, and runs it again on the arena.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

// bump allocator over a workspace: every take starts on a 256-byte boundary.  With a null base it only measures: `off` advances and the pointers
// it hands out are offsets from null.  The carver itself forms every address in uintptr_t, never by arithmetic on a null pointer; a layout may go on
// to derive values from what it was handed (`A.cq = dCq + s`), which in the measuring pass are offsets as well and are overwritten by the second pass.
struct WsCarver {
    uintptr_t base; size_t off = 0;
    explicit WsCarver(void* p) : base((uintptr_t)p) {}
    template <class T> T* take(size_t n) { off = (off + 255) & ~size_t(255); T* r = (T*)(base + off); off += n * sizeof(T); return r; }
    template <class T> void take(T*& p, size_t n) { p = take<T>(n); }      // the element type comes from the pointer it fills
};

// A layout runs twice, the first time on a null base: it may only assign pointers and values derived from them (no HIP call, no dereference, no side
// effect that is not idempotent).  reserve(bytes, &base) makes the arena hold `bytes` and returns its base; a non-zero status of its own is passed on.
// Returns mismatch_code with *err naming the site when the two passes end at different offsets; the pointers are then re-derived from null, so that
// the caller is left with nothing that points into the arena.
template <class Reserve, class Layout>
static inline int32_t ws_layout_carve(const char* site, size_t slack, int32_t mismatch_code, std::string* err, Reserve&& reserve, Layout&& layout, size_t* bytes_out = nullptr) {
    WsCarver measure(nullptr); layout(measure);
    void* base = nullptr;
    const int32_t rc = reserve(measure.off + slack, &base); if (rc) return rc;
    WsCarver carve(base); layout(carve);
    if (carve.off != measure.off) {
        WsCarver none(nullptr); layout(none);
        if (err) *err = std::string(site) + ": the workspace layout measured " + std::to_string(measure.off) + " bytes and carved " + std::to_string(carve.off);
        return mismatch_code;
    }
    if (bytes_out) *bytes_out = carve.off;
    return 0;
}
