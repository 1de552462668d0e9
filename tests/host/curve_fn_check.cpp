// curve_fn_check.cpp — stand-alone host run of csrc/curve_fn.h (tests/test_curve_fn_host.py builds it with the address and
// undefined-behaviour sanitizers and -ffp-contract=off and compares every printed value with the numpy model): all four functions
// at every branch boundary (0, 0.2, 0.4, 2, 4, g == T0) with both one-ulp neighbours, and at negative g.  One line per value, the
// inputs and the result as hex floats:
//   fn <fn> g <g> p <p0> <p1> <p2> <p3> v <value>            fn 0 .. 2
//   fn 3 d <d> theta <d values> aux <2 d values> v <value>   fn 3
#include <math.h>
#include <stdio.h>
#include <vector>

#include "../../gpbayestools_hic_amd/csrc/curve_fn.h"

int main() {
    const double T0s[] = {0.2, 0.17, 0.2345678901234567};
    std::vector<double> gs;
    for (const double b : {0.0, 0.2, 0.4, 2.0, 4.0, T0s[1], T0s[2], 6.2, 0.6, 0.5}) {
        gs.push_back(nextafter(b, -INFINITY));
        gs.push_back(b);
        gs.push_back(nextafter(b, INFINITY));
    }
    for (const double g : {-0.1, -1.0, -4.0, 1e-300, 0.1, 0.3, 1.0, 3.0, 5.0}) gs.push_back(g);
    // amplitudes of both signs; the widths positive
    const double pars[][4] = {{0.13, T0s[0], 0.09, 0.031}, {-0.07, T0s[1], 0.012, 0.1}, {0.19999, T0s[2], 0.15, 0.005},
                              {0.001, 0.3, 0.2, 0.0123}, {1.7, 2.9, -3.3, 0.05}, {0.2, 0.1, 0.3, 0.07}};
    int n = 0;
    for (int fn = 0; fn < 3; ++fn)
        for (const auto& p : pars) {
            if (fn == 0 && !(p[2] > 0.0 && p[3] > 0.0)) continue;
            for (const double g : gs) {
                const double v = gpb::curve_value(fn, p, nullptr, g);
                printf("fn %d g %a p %a %a %a %a v %a\n", fn, g, p[0], p[1], p[2], p[3], v);
                ++n;
            }
        }
    for (int d = 1; d <= 20; d += (d < 5 ? 1 : 5)) {
        std::vector<double> theta(d), aux(2 * d);
        for (int rep = 0; rep < 4; ++rep) {
            for (int j = 0; j < d; ++j) {
                theta[j] = 0.1 + 0.37 * j + 0.011 * rep * (j + 1);
                aux[j] = rep == 3 ? theta[j] : 0.3 + 0.29 * j;               // (rep 3: the truth itself, delta = 0)
                aux[d + j] = 0.1 + 1.3 * ((j * 7 + rep) % 5);
            }
            const double v = gpb::curve_value(3, theta.data(), aux.data(), 0.0, d);
            printf("fn 3 d %d theta", d);
            for (int j = 0; j < d; ++j) printf(" %a", theta[j]);
            printf(" aux");
            for (int j = 0; j < 2 * d; ++j) printf(" %a", aux[j]);
            printf(" v %a\n", v);
            ++n;
        }
    }
    printf("curve_fn_check: ok %d\n", n);
    return 0;
}
