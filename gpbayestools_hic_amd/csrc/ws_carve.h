// ws_carve.h — the one way a buffer is split into pieces: sizes and pointers come from the same list of take() calls.
// Host-only and free of HIP, so that a stand-alone program can check every layout (tests/host/ws_carve_check.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace gpb {

// Carves pieces off a buffer of element type B (the DevBuf's T), front to back.  With a null base it only counts: every piece
// is null and total() is what the same calls will need — ctx_carve (gpb_internal.h) runs a layout once that way, sizes the
// buffer, and runs it again over the buffer's pointer.
template <typename B>
struct Carver {
    B* base;
    int64_t used = 0;              // elements of B handed out so far

    explicit Carver(B* b = nullptr) : base(b) {}
    // the next n elements of T: the piece's size is rounded up to whole B's, then to `granule` B's.  n == 0: null, no size.
    template <typename T>
    T* take(int64_t n, int64_t granule = 1) {
        if (n <= 0) return nullptr;
        int64_t sz = ((int64_t)sizeof(T) * n + (int64_t)sizeof(B) - 1) / (int64_t)sizeof(B);
        sz = (sz + granule - 1) / granule * granule;
        T* p = base ? reinterpret_cast<T*>(base + used) : nullptr;
        used += sz;
        return p;
    }
    int64_t total() const { return used; }
};

}  // namespace gpb
