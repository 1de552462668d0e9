// curve_fn.h — the parametrised curves whose posterior bands gpb_chain_curves selects (examples/PlotMCMC.ipynb: zeta/s (T),
// eta/s (mu_B), <y_loss> (y_init)) and the closure distance delta, one value at a time.  Host- and device-compilable; nothing
// but <math.h> is needed.  Every function body runs under `fp contract(off)`: each operation is rounded on its own, exactly as
// numpy's vectorised forms round them (a device build contracts a * b + c into one fma by default, which is another number).
// The forms are the notebook's vectorised ones: they differ from the emulator's scalar parameter map (gpb_pmap.hip) at and
// below g = 0.
//   fn 0  zeta/s   p = (zmax, T0, sigma+, sigma-):  zmax exp(-((g - T0) (g - T0)) / (2 (s s))),  s = sigma- if g < T0 else sigma+
//   fn 1  eta/s    p = (e0, e2, e4):    0 <= g <= 0.2: e0 + (e2 - e0) (g / 0.2);  0.2 < g < 0.4: e2 + (e4 - e2) ((g - 0.2) / 0.2);
//                                       g >= 0.4: e4;  g < 0: 0
//   fn 2  y_loss   p = (y2, y4, y6):    0 <= g <= 2: y2 (g / 2);  2 < g < 4: y2 + (y4 - y2) ((g - 2) / 2);
//                                       g >= 4: y4 + (y6 - y4) ((g - 4) / 2);  g < 0: 0
//   fn 3  delta    (sum_j ((theta_j - truth_j) / width_j)^2) / d, j ascending, one add after the other; aux = truth [d] | width [d]
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CURVE_HD __host__ __device__ inline
#else
#define CURVE_HD inline
#endif

namespace gpb {

constexpr int CURVE_FN_ZETA = 0, CURVE_FN_ETA = 1, CURVE_FN_YLOSS = 2, CURVE_FN_DELTA = 3;

// fn 0 .. 2 from the curve's (up to four) parameters
CURVE_HD double curve_param(int fn, double p0, double p1, double p2, double p3, double g) {
#pragma clang fp contract(off)
    if (fn == CURVE_FN_ZETA) {
        const double s = g < p1 ? p3 : p2;
        const double dt = g - p1;
        const double num = -(dt * dt);
        const double den = 2.0 * (s * s);
        return p0 * exp(num / den);
    }
    if (fn == CURVE_FN_ETA) {
        if (g >= 0.0 && g <= 0.2) return p0 + (p1 - p0) * (g / 0.2);
        if (g > 0.2 && g < 0.4) return p1 + (p2 - p1) * ((g - 0.2) / 0.2);
        if (g >= 0.4) return p2;
        return 0.0;
    }
    if (g >= 0.0 && g <= 2.0) return p0 * (g / 2.0);
    if (g > 2.0 && g < 4.0) return p0 + (p1 - p0) * ((g - 2.0) / 2.0);
    if (g >= 4.0) return p1 + (p2 - p1) * ((g - 4.0) / 2.0);
    return 0.0;
}

// fn 3 from a sample's d parameters
CURVE_HD double curve_delta(const double* theta, const double* aux, int d) {
#pragma clang fp contract(off)
    double sum = 0.0;
    for (int j = 0; j < d; ++j) {
        const double z = (theta[j] - aux[j]) / aux[d + j];
        sum = sum + z * z;
    }
    return sum / (double)d;
}

// par: the curve's parameters in order (fn 0: four, fn 1 and 2: three), or for fn 3 the sample's d parameters
CURVE_HD double curve_value(int fn, const double* par, const double* aux, double g, int d = 0) {
    if (fn == CURVE_FN_DELTA) return curve_delta(par, aux, d);
    return curve_param(fn, par[0], par[1], par[2], fn == CURVE_FN_ZETA ? par[3] : 0.0, g);
}

}  // namespace gpb
