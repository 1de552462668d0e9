// hmc_step.h — the arithmetic of one Hamiltonian Monte Carlo step with a diagonal metric in a hard prior box (gpb_hmc.hip), one
// set of functions for the host and the device, included alone by tests/host/hmc_step_check.cpp.  Every rounding is written
// out (no product is meant to be fused into a sum: compile with -ffp-contract=off), so that tests/hmc_reference.py restates
// the kick, the drift with its wall rule and the kinetic energy bit for bit; only the step size, the accept probability and the
// dual-averaging update call a transcendental function.
//   kick      p = p + h g                                       (h = eps / 2, g the gradient of the log-posterior)
//   drift     x = x + eps (minv p), then the wall rule: while x lies outside [lo, hi], at most HMC_MAX_REFLECT times,
//             x = lo + (lo - x) or x = hi - (x - hi) and p = -p  (the trajectory reflects: volume preserving and reversible,
//             Neal 2011, section 5.1); a coordinate still outside after that marks the trajectory as escaped
//   kinetic   K = 1/2 sum_j (p_j p_j) minv_j in index order
//   dual averaging (Hoffman & Gelman 2014, algorithm 5; gamma = 0.05, t0 = 10, kappa = 0.75) on the state block
//             [0] ln eps  [1] ln eps-bar  [2] H-bar  [3] mu  [4] the update count
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GPB_HMC_HD __host__ __device__
#else
#define GPB_HMC_HD
#endif

#define GPB_HMC_MAX_REFLECT 8
#define GPB_HMC_ESCAPED 16          /* hmc_drift's return value: the reflections made, plus this when the coordinate escaped */

namespace gpb {

constexpr double HMC_DA_GAMMA = 0.05, HMC_DA_T0 = 10.0, HMC_DA_KAPPA = 0.75;
constexpr double HMC_DIVERGENT = 1000.0;      // a trajectory whose energy error exceeds this (or is NaN) counts as divergent
constexpr double HMC_A_SCALE = 4294967296.0;  // accept probabilities are summed over the chains as integers of 2^-32

GPB_HMC_HD inline double hmc_kick(double p, double h, double g) { return p + h * g; }

// -> reflections made (0 .. 8) | GPB_HMC_ESCAPED.  A NaN coordinate compares false with both walls: it is left alone and
// does not count as escaped (its row evaluates as outside the box and the trajectory is rejected there).
GPB_HMC_HD inline int hmc_drift(double& x, double& p, double eps, double minv, double lo, double hi) {
    double xx = x + eps * (minv * p), pp = p;
    int n = 0;
    for (int r = 0; r < GPB_HMC_MAX_REFLECT; ++r) {
        if (xx < lo) {
            xx = lo + (lo - xx);
            pp = -pp;
            ++n;
        } else if (xx > hi) {
            xx = hi - (xx - hi);
            pp = -pp;
            ++n;
        } else {
            break;
        }
    }
    x = xx;
    p = pp;
    return (xx < lo || xx > hi) ? (n | GPB_HMC_ESCAPED) : n;
}

GPB_HMC_HD inline double hmc_kinetic(const double* p, const double* minv, int d) {
    double s = 0.0;
    for (int j = 0; j < d; ++j) s = s + (p[j] * p[j]) * minv[j];
    return 0.5 * s;
}

// the step size of one step: eps (1 + jitter (2 u - 1)), u uniform in [0, 1)
GPB_HMC_HD inline double hmc_step_size(double ln_eps, double jitter, double u) {
    return exp(ln_eps) * (1.0 + jitter * (2.0 * u - 1.0));
}

// min(1, exp(-dH)); 0 for a NaN energy error
GPB_HMC_HD inline double hmc_accept_prob(double dH) {
    if (dH != dH) return 0.0;
    const double a = exp(-dH);
    return a < 1.0 ? a : 1.0;
}

// what a chain adds to the integer sum of the accept probabilities (a in [0, 1])
GPB_HMC_HD inline unsigned long long hmc_a_fixed(double a) { return (unsigned long long)(a * HMC_A_SCALE); }
GPB_HMC_HD inline double hmc_a_mean(unsigned long long sum, long long C) { return ((double)sum / HMC_A_SCALE) / (double)C; }

// one update with the mean accept probability a_mean of a step towards the target delta
GPB_HMC_HD inline void hmc_dual_average(double* st, double a_mean, double delta) {
    const double t = st[4] + 1.0;
    const double w = 1.0 / (t + HMC_DA_T0);
    const double hbar = (1.0 - w) * st[2] + w * (delta - a_mean);
    const double le = st[3] - (sqrt(t) / HMC_DA_GAMMA) * hbar;
    const double eta = pow(t, -HMC_DA_KAPPA);
    st[1] = eta * le + (1.0 - eta) * st[1];
    st[0] = le;
    st[2] = hbar;
    st[4] = t;
}

}  // namespace gpb
