// chi2_sf.h — the survival function of the chi-square distribution, Q(ndf / 2, x / 2) with Q the regularised upper incomplete
// gamma function: one function for the host and the device, included alone by tests/host/chi2_sf_check.cpp.
//   a = ndf / 2, t = x / 2.  NaN in gives NaN out; x <= 0 gives 1; ndf must be positive (NaN otherwise).
//   t <  a + 1:  P = pre * sum_{n >= 0} t^n / (a (a + 1) ... (a + n)),  Q = 1 - P      (the series; P stays below ~0.92 here)
//   t >= a + 1:  Q = pre / (t + 1 - a - 1 (1 - a) / (t + 3 - a - 2 (2 - a) / (t + 5 - a - ...)))   (modified Lentz)
//   pre = exp(a ln t - t - lgamma(a)).
// Both loops are bounded by GPB_CHI2_SF_MAX_ITER.  The series' terms fall like exp(-n^2 / (2 a)) at t = a + 1, so it ends after
// about sqrt(2 a ln(1 / eps)) terms: 275 at a = 1024; the fraction needs fewest steps far above a and about as many as
// the series just above the switch (measured on the test grid, a <= 1024: 272 at most).  A loop that runs out returns what it has:
// its error is then the size of its last term, not a failure.
// Accuracy: the prefactor's argument carries the rounding of a ln t, t and lgamma(a), each up to ~1e4 at a = 1024, so the relative
// error of Q grows to ~1e-12 there; below a ~ 30 it is a few 1e-15.
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GPB_CHI2_HD __host__ __device__
#else
#define GPB_CHI2_HD
#endif

#define GPB_CHI2_SF_MAX_ITER 600

namespace gpb {

// iters (optional): the steps of the loop that ran
GPB_CHI2_HD inline double chi2_sf(double x, double ndf, int* iters = nullptr) {
    if (iters) *iters = 0;
    if (x != x || !(ndf > 0.0)) return NAN;
    if (x <= 0.0) return 1.0;
    const double a = 0.5 * ndf, t = 0.5 * x;
    if (t == INFINITY) return 0.0;
    const double pre = exp(a * log(t) - t - lgamma(a));
    const double eps = 1.1102230246251565e-16;             // 2^-53
    if (t < a + 1.0) {
        double ap = a, del = 1.0 / a, sum = del;
        int n = 0;
        for (n = 1; n <= GPB_CHI2_SF_MAX_ITER; ++n) {
            ap += 1.0;
            del *= t / ap;
            sum += del;
            if (fabs(del) < fabs(sum) * eps) break;
        }
        if (iters) *iters = n;
        const double q = 1.0 - pre * sum;
        return q < 0.0 ? 0.0 : q;
    }
    const double tiny = 1e-300;
    double b = t + 1.0 - a, c = 1.0 / tiny, d = 1.0 / b, h = d;
    int n = 0;
    for (n = 1; n <= GPB_CHI2_SF_MAX_ITER; ++n) {
        const double an = -(double)n * ((double)n - a);
        b += 2.0;
        d = an * d + b;
        if (fabs(d) < tiny) d = tiny;
        c = b + an / c;
        if (fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (fabs(del - 1.0) < 2.0 * eps) break;
    }
    if (iters) *iters = n;
    const double q = pre * h;
    return q > 1.0 ? 1.0 : q;
}

}  // namespace gpb
