// chi2_sf_check.cpp — stand-alone host run of csrc/chi2_sf.h (tests/test_chi2_sf_host.py builds it with the address and
// undefined-behaviour sanitizers and -ffp-contract=off and compares every printed value with mpmath): Q(ndf / 2, x / 2) on the grid
// ndf in {1, 2, 3, 16, 55, 64, 540, 2048} times x / ndf in {0, 1e-3, 0.3, 0.9, 1, 1.1, 2, 5, 40}, and at the switch between the
// series and the continued fraction, x / 2 = ndf / 2 + 1, with both one-ulp neighbours.  Then the special values.  One line per
// value, the inputs and the result as hex floats:
//   ndf <ndf> x <x> q <Q> iters <steps of the loop that ran>
#include <math.h>
#include <stdio.h>
#include <vector>

#include "../../gpbayestools_hic_amd/csrc/chi2_sf.h"

int main() {
    int n = 0, worst = 0;
    for (const double ndf : {1.0, 2.0, 3.0, 16.0, 55.0, 64.0, 540.0, 2048.0}) {
        std::vector<double> xs;
        for (const double r : {0.0, 1e-3, 0.3, 0.9, 1.0, 1.1, 2.0, 5.0, 40.0}) xs.push_back(r * ndf);
        const double sw = ndf + 2.0;                     // x / 2 == ndf / 2 + 1
        xs.push_back(nextafter(sw, -INFINITY));
        xs.push_back(sw);
        xs.push_back(nextafter(sw, INFINITY));
        for (const double x : xs) {
            int it = -1;
            const double q = gpb::chi2_sf(x, ndf, &it);
            printf("ndf %a x %a q %a iters %d\n", ndf, x, q, it);
            if (it > worst) worst = it;
            ++n;
        }
    }
    for (const double x : {(double)NAN, -1.0, -0.0, (double)INFINITY}) {
        int it = -1;
        printf("ndf %a x %a q %a iters %d\n", 3.0, x, gpb::chi2_sf(x, 3.0, &it), it);
        ++n;
    }
    printf("chi2_sf_check: ok %d max_iter %d bound %d\n", n, worst, GPB_CHI2_SF_MAX_ITER);
    return 0;
}
