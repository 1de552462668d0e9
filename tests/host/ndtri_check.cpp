// ndtri_check.cpp — stand-alone host run of csrc/ndtri.h (tests/test_ndtri_host.py builds it with the address and
// undefined-behaviour sanitizers and compares every printed value with scipy.special.ndtri): Phi^-1(p) on
//   both tails, log-spaced: p = 10^-e and 1 - 10^-e for e = 10 ... 1 in steps of 1/16;
//   the middle, dense: p = k / 4096 for k = 1 ... 4095, and the switch |p - 1/2| = 0.425 with both one-ulp neighbours on both sides;
//   the switch r = 5 of the tails (p = exp(-25)) with both one-ulp neighbours, and its mirror image;
//   the rank transform's own arguments (r - 3/8) / (n + 1/4) for n = 2048, r = 1 ... 32, n - 31 ... n and every half rank between.
// Then the special values 1/2, 0, 1, -1, 2, NaN.  One line per value, both numbers as hex floats:   p <p> z <z>
#include <math.h>
#include <stdio.h>
#include <vector>

#include "../../gpbayestools_hic_amd/csrc/ndtri.h"

int main() {
    std::vector<double> ps;
    for (int i = 0; i <= 9 * 16; ++i) {
        const double t = pow(10.0, -10.0 + i / 16.0);
        ps.push_back(t);
        ps.push_back(1.0 - t);
    }
    for (int k = 1; k < 4096; ++k) ps.push_back(k / 4096.0);
    for (const double c : {0.5 - 0.425, 0.5 + 0.425, exp(-25.0), 1.0 - exp(-25.0)}) {
        ps.push_back(nextafter(c, 0.0));
        ps.push_back(c);
        ps.push_back(nextafter(c, 1.0));
    }
    const double n = 2048.0;
    for (int r2 = 2; r2 <= 64; ++r2) {
        ps.push_back((0.5 * r2 - 0.375) / (n + 0.25));
        ps.push_back((0.5 * (2.0 * n + 2.0 - r2) - 0.375) / (n + 0.25));
    }
    int cnt = 0;
    for (const double p : ps) {
        printf("p %a z %a\n", p, gpb::ndtri(p));
        ++cnt;
    }
    for (const double p : {0.5, 0.0, 1.0, -1.0, 2.0, (double)NAN}) {
        printf("p %a z %a\n", p, gpb::ndtri(p));
        ++cnt;
    }
    printf("ndtri_check: ok %d\n", cnt);
    return 0;
}
