// dispatch_check.cpp — stand-alone host check of csrc/dispatch.h, the one place where a run-time value becomes a kernel's
// template argument.  with_int calls its lambda exactly once with the listed value that was asked for and not at all for a value
// outside the list, which comes back as NO_CASE; pick_dpad(d) is the smallest listed width >= d and every width it returns
// dispatches; with_kind covers the three kernel ids and nothing else.  The widths are restated here, not read from the header.
// Built with the address and undefined-behaviour sanitizers by tests/test_dispatch_host.py; exit status 0 = every check held.
#include <stdio.h>
#include <vector>
#include "../../gpbayestools_hic_amd/csrc/dispatch.h"

using namespace gpb;

static int g_failed = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); ++g_failed; } \
    } while (0)

static const int WIDTHS[] = {8, 16, 20, 24, 32, 48, 64};
static const int N_WIDTHS = 7;

static_assert(MAX_D == 64, "MAX_D is the last width");
static_assert(pick_dpad(20) == 20 && pick_dpad(21) == 24 && pick_dpad(65) == -1, "pick_dpad at compile time");

// `with` dispatches v over a list: for v in `listed` one call, with v; for every other v of [lo, hi] none and NO_CASE
template <class With>
static void check_list(const char* what, With with, const std::vector<int>& listed, int64_t lo, int64_t hi) {
    for (int64_t v = lo; v <= hi; ++v) {
        bool in = false;
        for (int l : listed) in = in || l == v;
        int calls = 0, seen = -12345;
        const int rc = with(v, [&](auto C) {
            ++calls;
            seen = decltype(C)::value;
            return 1000 + decltype(C)::value;          // (the lambda's result is handed back)
        });
        const bool ok = in ? (calls == 1 && seen == v && rc == 1000 + v) : (calls == 0 && rc == NO_CASE);
        if (!ok) {
            fprintf(stderr, "%s: v = %lld: %d calls, saw %d, returned %d\n", what, (long long)v, calls, seen, rc);
            ++g_failed;
        }
    }
}

int main() {
    const std::vector<int> widths(WIDTHS, WIDTHS + N_WIDTHS);
    check_list("with_dpad", [](int64_t v, auto f) { return with_dpad(v, f); }, widths, -2, 130);
    check_list("with_kind", [](int64_t v, auto f) { return with_kind((int)v, f); },
               {GPB_KERNEL_RBF, GPB_KERNEL_MATERN15, GPB_KERNEL_MATERN25}, -3, 6);
    CHECK(GPB_KERNEL_RBF == 0 && GPB_KERNEL_MATERN15 == 1 && GPB_KERNEL_MATERN25 == 2);
    // the lists written at the launch sites
    check_list("planes", [](int64_t v, auto f) { return with_int<0, 6, 7>(v, f); }, {0, 6, 7}, -1, 9);
    check_list("walkers per lane", [](int64_t v, auto f) { return with_int<1, 2>(v, f); }, {1, 2}, -1, 4);
    check_list("walker tile", [](int64_t v, auto f) { return with_int<32, 64, 128>(v, f); }, {32, 64, 128}, 0, 260);
    check_list("GPs", [](int64_t v, auto f) { return with_int<1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16>(v, f); },
               {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16}, -1, 18);
    // a value that only equals a listed one after truncation to 32 bits is not listed
    CHECK(with_dpad(((int64_t)1 << 32) + 8, [](auto) { return 0; }) == NO_CASE);
    // a failure inside the lambda is not mistaken for a missing case, nor the reverse
    CHECK(with_dpad(8, [](auto) { return GPB_E_HIP; }) == GPB_E_HIP);
    CHECK(NO_CASE != 0 && NO_CASE != GPB_E_ARG && NO_CASE != GPB_E_STATE && NO_CASE != GPB_E_HIP && NO_CASE != GPB_E_NODEV &&
          NO_CASE != GPB_E_ALLOC && NO_CASE != GPB_E_RCCL);

    // pick_dpad: the smallest listed width >= d, -1 above the last; whatever it returns dispatches
    for (int64_t d = 1; d <= 200; ++d) {
        int want = -1;
        for (int i = N_WIDTHS - 1; i >= 0; --i)
            if (WIDTHS[i] >= d) want = WIDTHS[i];
        const int got = pick_dpad(d);
        if (got != want) { fprintf(stderr, "pick_dpad(%lld) = %d, expected %d\n", (long long)d, got, want); ++g_failed; }
        CHECK((d <= 64) == (got > 0));
        if (got < 0) continue;
        int seen = 0;
        CHECK(with_dpad(got, [&](auto D) { seen = decltype(D)::value; return 0; }) == 0);
        CHECK(seen == got);
    }
    if (g_failed) {
        fprintf(stderr, "dispatch_check: %d checks failed\n", g_failed);
        return 1;
    }
    printf("dispatch_check: ok\n");
    return 0;
}
