// dev_buf_check.cpp — stand-alone host check of gpb::DevBuf (csrc/dev_buf.h): the buffer cache is played by malloc / free with a
// live counter and a "fail the next call" switch.  Built with the address and undefined-behaviour sanitizers by
// tests/test_dev_buf_host.py; exit status 0 = every check held and nothing leaked.
#include <stdio.h>
#include <stdlib.h>
#include <type_traits>
#include "../../gpbayestools_hic_amd/csrc/dev_buf.h"

static long g_live = 0;             // buffers handed out and not yet returned
static bool g_fail_next = false;
static void* g_last_freed = nullptr;

namespace gpb {
hipError_t pool_malloc(void** p, size_t bytes) {
    *p = nullptr;
    if (g_fail_next) { g_fail_next = false; return hipErrorOutOfMemory; }
    *p = malloc(bytes);
    if (!*p) return hipErrorOutOfMemory;
    ++g_live;
    return hipSuccess;
}
void pool_free(void* p) {
    if (!p) return;
    g_last_freed = p;
    --g_live;
    free(p);
}
void pool_trim() {}
}  // namespace gpb

static int g_failed = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); ++g_failed; } \
    } while (0)

using gpb::DevBuf;
static_assert(!std::is_copy_constructible<DevBuf<double>>::value, "DevBuf must not be copy-constructible");
static_assert(!std::is_copy_assignable<DevBuf<double>>::value, "DevBuf must not be copy-assignable");

int main() {
    {
        DevBuf<double> b;
        CHECK(b.p == nullptr && b.cap == 0 && !b && b.get() == nullptr);
        CHECK(b.alloc(37) == hipSuccess);
        CHECK(b.p != nullptr && b.cap == 37 && g_live == 1);
        double* q = b;                                  // reads like the pointer it replaces
        CHECK(q == b.get() && b + 5 == q + 5);
        for (int i = 0; i < 37; ++i) b[i] = i;          // every element is ours (the sanitizer watches the bounds)
        CHECK(b[36] == 36.0);

        CHECK(b.alloc(0) == hipSuccess);                // an empty request still gives one element
        CHECK(b.p != nullptr && b.cap == 1 && g_live == 1);
        b[0] = 1.0;

        double* held = b.p;                             // a failing alloc on a held buffer: the old one goes back, nothing is left
        g_fail_next = true;
        CHECK(b.alloc(64) != hipSuccess);
        CHECK(b.p == nullptr && b.cap == 0 && g_live == 0 && g_last_freed == held);

        CHECK(b.alloc(8) == hipSuccess && b.cap == 8 && g_live == 1);
        b.release();
        CHECK(b.p == nullptr && b.cap == 0 && g_live == 0);
        b.release();                                    // twice is harmless
        CHECK(b.p == nullptr && b.cap == 0 && g_live == 0);

        DevBuf<int> a, c;                               // the destructor returns what is held at the end of the scope
        CHECK(a.alloc(3) == hipSuccess && c.alloc(5) == hipSuccess && b.alloc(2) == hipSuccess && g_live == 3);
    }
    CHECK(g_live == 0);
    if (g_failed) return 1;
    puts("dev_buf_check: ok");
    return 0;
}
