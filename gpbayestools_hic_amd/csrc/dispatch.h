// dispatch.h — from a run-time value to a kernel's template argument.  Host only, plain C++17 with no HIP in it
// (tests/host/dispatch_check.cpp builds it alone).
#pragma once
#include <limits.h>
#include <stdint.h>
#include <type_traits>
#include <utility>
#include "../../include/gpbayes.h"

namespace gpb {

constexpr int NO_CASE = INT_MIN;      // with_int: the value is not in the list (no GPB_E_* code and no LAPACK info is INT_MIN)

// f(std::integral_constant<int, V>{}) for the listed V that equals v, and f's int handed back:
//     with_int<0, 6, 7>(planes, [&](auto S) { constexpr int SLICE = decltype(S)::value; ... k<SLICE> ...; return 0; })
// A value that is not listed calls nothing and returns NO_CASE, which the launch sites make GPB_E_STATE (dispatched,
// gpb_internal.h): an incomplete list fails loudly, it does not run some other instantiation.
template <int... Vs, class F>
inline int with_int(int64_t v, F&& f) {
    int rc = NO_CASE;
    (void)((v == Vs && (rc = f(std::integral_constant<int, Vs>{}), true)) || ...);
    return rc;
}

// The padded input widths: every kernel that forms a scaled distance is instantiated or sized on one of them (ascending;
// 20: the reference's analyses have 17-20 model parameters).  tests/test_width_cases.py reads this line.
using Widths = std::integer_sequence<int, 8, 16, 20, 24, 32, 48, 64>;

template <int... Vs, class F>
inline int with_listed(std::integer_sequence<int, Vs...>, int64_t v, F&& f) { return with_int<Vs...>(v, f); }
template <int... Vs>
constexpr int first_at_least(std::integer_sequence<int, Vs...>, int64_t d) {       // of an ascending list; -1: none
    int r = -1;
    (void)((d <= Vs && (r = Vs, true)) || ...);
    return r;
}
template <int... Vs>
constexpr int last_of(std::integer_sequence<int, Vs...>) {
    int r = -1;
    ((r = Vs), ...);
    return r;
}

constexpr int MAX_D = last_of(Widths{});
constexpr int pick_dpad(int64_t d) { return first_at_least(Widths{}, d); }      // the width of a design with d inputs, -1: d > MAX_D
template <class F>
inline int with_dpad(int64_t dpad, F&& f) { return with_listed(Widths{}, dpad, f); }
template <class F>
inline int with_kind(int kind, F&& f) { return with_int<GPB_KERNEL_RBF, GPB_KERNEL_MATERN15, GPB_KERNEL_MATERN25>(kind, f); }

}  // namespace gpb
