// hmc_step_check.cpp — csrc/hmc_step.h on the host, included alone: every function at fixed and pseudo-random inputs, the
// inputs and results printed as hex floats for tests/test_hmc_step_host.py, which restates them with tests/hmc_reference.py.
// Built with -fsanitize=address,undefined -ffp-contract=off and run as a child process.
#include "../../gpbayestools_hic_amd/csrc/hmc_step.h"

#include <cstdint>
#include <cstdio>
#include <vector>

namespace {

uint64_t lcg_state = 0x243F6A8885A308D3ull;
double uniform() {                                   // 53 bits of a 64-bit LCG's high half (Knuth's MMIX constants)
    lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(lcg_state >> 11) * (1.0 / 9007199254740992.0);
}

int n_lines = 0;

void drift_case(double x, double p, double eps, double minv, double lo, double hi) {
    double xx = x, pp = p;
    const int r = gpb::hmc_drift(xx, pp, eps, minv, lo, hi);
    std::printf("drift %a %a %a %a %a %a -> %a %a %d\n", x, p, eps, minv, lo, hi, xx, pp, r);
    ++n_lines;
}

void kick_case(double p, double h, double g) {
    std::printf("kick %a %a %a -> %a\n", p, h, g, gpb::hmc_kick(p, h, g));
    ++n_lines;
}

void kinetic_case(const std::vector<double>& p, const std::vector<double>& minv) {
    std::printf("kinetic %d", (int)p.size());
    for (double v : p) std::printf(" %a", v);
    for (double v : minv) std::printf(" %a", v);
    std::printf(" -> %a\n", gpb::hmc_kinetic(p.data(), minv.data(), (int)p.size()));
    ++n_lines;
}

void dual_case(double* st, double a_mean, double delta) {
    std::printf("dual %a %a %a %a %a %a %a ->", st[0], st[1], st[2], st[3], st[4], a_mean, delta);
    gpb::hmc_dual_average(st, a_mean, delta);
    std::printf(" %a %a %a %a %a\n", st[0], st[1], st[2], st[3], st[4]);
    ++n_lines;
}

}  // namespace

int main() {
    const double nan = NAN, inf = INFINITY;
    // the wall rule in the unit box: no reflection, one at each wall, two in one drift, eight and still inside, the escape,
    // exactly on a wall (from inside and at rest), NaN in x and in p
    drift_case(0.5, 0.3, 0.1, 1.0, 0.0, 1.0);
    drift_case(0.01, -1.0, 0.1, 1.0, 0.0, 1.0);
    drift_case(0.95, 1.0, 0.1, 1.0, 0.0, 1.0);
    drift_case(0.5, 1.0, 1.8, 1.0, 0.0, 1.0);
    drift_case(0.5, -1.0, 1.8, 1.0, 0.0, 1.0);
    drift_case(0.5, 1.0, 7.7, 1.0, 0.0, 1.0);
    drift_case(0.5, 1.0, 100.0, 1.0, 0.0, 1.0);
    drift_case(0.5, -1.0, 8.75, 1.0, 0.0, 1.0);
    drift_case(0.5, 1.0, 0.5, 1.0, 0.0, 1.0);
    drift_case(0.5, -1.0, 0.5, 1.0, 0.0, 1.0);
    drift_case(0.0, 0.0, 0.1, 1.0, 0.0, 1.0);
    drift_case(1.0, 0.0, 0.1, 1.0, 0.0, 1.0);
    drift_case(nan, 1.0, 0.1, 1.0, 0.0, 1.0);
    drift_case(0.5, nan, 0.1, 1.0, 0.0, 1.0);
    drift_case(0.5, inf, 0.1, 1.0, 0.0, 1.0);
    // a start outside the box, a box away from the origin, a narrow box
    drift_case(1.2, 0.1, 0.1, 1.0, 0.0, 1.0);
    drift_case(-0.004, -0.1, 0.1, 1.0, 0.0, 1.0);
    drift_case(3.2, 0.7, 0.3, 0.37, -2.5, 3.25);
    drift_case(-2.4, -0.7, 0.9, 0.37, -2.5, 3.25);
    drift_case(0.3000001, 1.0, 1e-6, 1.0, 0.3, 0.3000004);
    for (int i = 0; i < 400; ++i) {
        const double lo = 4.0 * uniform() - 2.0, hi = lo + 0.05 + 3.0 * uniform();
        const double x = lo + (hi - lo) * uniform();
        const double scale = i % 4 == 0 ? 40.0 : (i % 4 == 1 ? 4.0 : 0.5);
        drift_case(x, 2.0 * uniform() - 1.0, scale * uniform(), 0.01 + 2.0 * uniform(), lo, hi);
    }
    kick_case(0.5, 0.05, -3.25);
    kick_case(-1.0, 0.0, inf);
    kick_case(nan, 0.1, 1.0);
    for (int i = 0; i < 100; ++i) kick_case(4.0 * uniform() - 2.0, 0.3 * uniform(), 200.0 * uniform() - 100.0);
    for (int d : {1, 2, 3, 20, 71, 127, 256}) {
        std::vector<double> p(d), m(d);
        for (int j = 0; j < d; ++j) {
            p[j] = 6.0 * uniform() - 3.0;
            m[j] = 0.001 + uniform();
        }
        kinetic_case(p, m);
    }
    kinetic_case({1.0, nan}, {1.0, 1.0});
    // dual averaging: 60 updates in a row with accept probabilities all over [0, 1], then two restarts
    double st[5] = {-2.0, 0.0, 0.0, -2.0 + 2.302585092994046, 0.0};
    for (int i = 0; i < 60; ++i) dual_case(st, i < 5 ? 0.0 : (i < 10 ? 1.0 : uniform()), 0.8);
    double st2[5] = {0.25, 0.0, 0.0, 2.5, 0.0};
    for (int i = 0; i < 20; ++i) dual_case(st2, uniform(), 0.65);
    for (double dH : {0.0, -1.0, 1.0, 0.3, 1000.5, -inf, inf, nan, 745.2, 1e-17}) {
        std::printf("accept %a -> %a\n", dH, gpb::hmc_accept_prob(dH));
        ++n_lines;
    }
    for (int i = 0; i < 20; ++i) {
        const double le = 4.0 * uniform() - 5.0, jit = 0.9 * uniform(), u = uniform();
        std::printf("eps %a %a %a -> %a\n", le, jit, u, gpb::hmc_step_size(le, jit, u));
        ++n_lines;
    }
    for (int i = 0; i < 20; ++i) {
        const double a = i == 0 ? 0.0 : (i == 1 ? 1.0 : uniform());
        std::printf("afixed %a -> %llu\n", a, gpb::hmc_a_fixed(a));
        ++n_lines;
    }
    std::printf("amean %llu %lld -> %a\n", 123456789012345ull, 70ll, gpb::hmc_a_mean(123456789012345ull, 70ll));
    ++n_lines;
    std::printf("hmc_step_check: ok %d\n", n_lines);
    return 0;
}
