// Host check of csrc/coupled_setup.h (the joint factorisation of a coupled chain likelihood), built with the address and
// undefined-behaviour sanitizers by tests/test_coupled_setup_host.py.  For random block structures the closed form
//     loglike = -1/2 (c_perp + v^T S^-1 v) - 1/2 (logdet0 + log det S),  S = I + R diag(g) R^T,  v = R m + v0
// is compared with a dense long-double Cholesky of C0 + A^T diag(g) A written here; an indefinite C0 and a repeated row of A
// must be reported as "does not apply".
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../../gpbayestools_hic_amd/csrc/coupled_setup.h"

typedef long double ld;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static double urand() {                       // splitmix64 -> (0, 1)
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    z ^= z >> 31;
    return ((double)(z >> 11) + 0.5) / 9007199254740992.0;
}
static double nrand() { return sqrt(-2.0 * log(urand())) * cos(6.283185307179586 * urand()); }

#define CHECK(c)                                                                   \
    do {                                                                           \
        if (!(c)) {                                                                \
            printf("coupled_setup_check: FAILED %s (line %d)\n", #c, __LINE__);    \
            exit(1);                                                               \
        }                                                                          \
    } while (0)

// lower Cholesky of the n x n matrix a in place; false when not positive definite
static bool chol(std::vector<ld>& a, int64_t n) {
    for (int64_t j = 0; j < n; ++j) {
        ld d = a[j * n + j];
        for (int64_t k = 0; k < j; ++k) d -= a[j * n + k] * a[j * n + k];
        if (!(d > 0.0L)) return false;
        a[j * n + j] = sqrtl(d);
        for (int64_t i = j + 1; i < n; ++i) {
            ld v = a[i * n + j];
            for (int64_t k = 0; k < j; ++k) v -= a[i * n + k] * a[j * n + k];
            a[i * n + j] = v / a[j * n + j];
        }
    }
    return true;
}

// -1/2 y^T C^-1 y - 1/2 log det C by a dense Cholesky
static ld dense_loglike(std::vector<ld> C, std::vector<ld> y, int64_t n) {
    CHECK(chol(C, n));
    ld q = 0.0L, logdet = 0.0L;
    for (int64_t i = 0; i < n; ++i) {
        ld v = y[i];
        for (int64_t k = 0; k < i; ++k) v -= C[i * n + k] * y[k];
        y[i] = v / C[i * n + i];
        q += y[i] * y[i];
        logdet += 2.0L * logl(C[i * n + i]);
    }
    return -0.5L * q - 0.5L * logdet;
}

struct Problem {
    std::vector<int64_t> Ms, Ps;
    std::vector<std::vector<double>> A, mu, C0;
    std::vector<double> yexp, cexp;
    std::vector<gpb::CoupledBlock> blk;
    int64_t MT = 0, PT = 0;
};

static Problem make(const std::vector<int64_t>& Ms, const std::vector<int64_t>& Ps, bool with_trunc) {
    Problem pr;
    pr.Ms = Ms; pr.Ps = Ps;
    const int E = (int)Ms.size();
    pr.A.resize(E); pr.mu.resize(E); pr.C0.resize(E);
    for (int e = 0; e < E; ++e) {
        const int64_t M = Ms[e], P = Ps[e];
        pr.MT += M; pr.PT += P;
        pr.A[e].resize(P * M);
        for (auto& x : pr.A[e]) x = nrand();
        pr.mu[e].resize(M);
        for (auto& x : pr.mu[e]) x = 2.0 + nrand();
        if (with_trunc) {                       // a small symmetric positive semi-definite block: B B^T with B [M][2]
            std::vector<double> B(M * 2);
            for (auto& x : B) x = 0.1 * nrand();
            pr.C0[e].assign(M * M, 0.0);
            for (int64_t i = 0; i < M; ++i)
                for (int64_t j = 0; j < M; ++j) pr.C0[e][i * M + j] = B[i * 2] * B[j * 2] + B[i * 2 + 1] * B[j * 2 + 1];
        }
    }
    const int64_t MT = pr.MT;
    pr.yexp.resize(MT);
    for (auto& x : pr.yexp) x = 2.0 + nrand();
    // diag(sigma^2) + a fully correlated source + a source over the middle half (it straddles the blocks) + an exponential kernel
    std::vector<double> sig(MT), s1(MT), s2(MT, 0.0);
    for (int64_t i = 0; i < MT; ++i) { sig[i] = 0.05 + 0.1 * urand(); s1[i] = 0.03 * pr.yexp[i]; }
    for (int64_t i = MT / 4; i < MT - MT / 4; ++i) s2[i] = 0.05 * pr.yexp[i];
    pr.cexp.assign(MT * MT, 0.0);
    for (int64_t i = 0; i < MT; ++i)
        for (int64_t j = 0; j < MT; ++j)
            pr.cexp[i * MT + j] = (i == j ? sig[i] * sig[i] : 0.0) + s1[i] * s1[j] + s2[i] * s2[j] +
                                  0.3 * sig[i] * sig[j] * exp(-fabs((double)(i - j)) / 5.0);
    for (int e = 0; e < E; ++e)
        pr.blk.push_back(gpb::CoupledBlock{Ms[e], Ps[e], pr.A[e].data(), pr.mu[e].data(), with_trunc ? pr.C0[e].data() : nullptr});
    return pr;
}

static double check_structure(const std::vector<int64_t>& Ms, const std::vector<int64_t>& Ps, bool with_trunc) {
    Problem pr = make(Ms, Ps, with_trunc);
    const int E = (int)Ms.size();
    const int64_t MT = pr.MT, PT = pr.PT;
    gpb::CoupledTables t;
    CHECK(gpb::coupled_setup(pr.blk.data(), E, pr.yexp.data(), pr.cexp.data(), t));
    CHECK(t.PT == PT && t.MT == MT && (int64_t)t.R.size() == PT * PT && (int64_t)t.v0.size() == PT);
    for (int64_t i = 0; i < PT; ++i)
        for (int64_t j = 0; j < i; ++j) CHECK(t.R[i * PT + j] == 0.0);
    double worst = 0.0;
    for (int trial = 0; trial < 20; ++trial) {
        std::vector<double> m(PT), g(PT);
        for (int64_t p = 0; p < PT; ++p) { m[p] = nrand(); g[p] = 0.01 + urand(); }
        // dense: C = C0 + A^T diag(g) A, y = A^T m + mu - yexp
        std::vector<ld> C(MT * MT), y(MT);
        for (int64_t i = 0; i < MT * MT; ++i) C[i] = pr.cexp[i];
        for (int64_t e = 0, o = 0, po = 0; e < E; o += Ms[e], po += Ps[e], ++e) {
            const int64_t M = Ms[e], P = Ps[e];
            for (int64_t i = 0; i < M; ++i) {
                ld yi = (ld)pr.mu[e][i] - (ld)pr.yexp[o + i];
                for (int64_t p = 0; p < P; ++p) yi += (ld)pr.A[e][p * M + i] * (ld)m[po + p];
                y[o + i] = yi;
                for (int64_t j = 0; j < M; ++j) {
                    ld c = with_trunc ? (ld)pr.C0[e][i * M + j] : 0.0L;
                    for (int64_t p = 0; p < P; ++p) c += (ld)pr.A[e][p * M + i] * (ld)g[po + p] * (ld)pr.A[e][p * M + j];
                    C[(o + i) * MT + o + j] += c;
                }
            }
        }
        const ld ref = dense_loglike(C, y, MT);
        // closed form from the tables
        std::vector<ld> S(PT * PT, 0.0L), v(PT);
        for (int64_t i = 0; i < PT; ++i) {
            ld vi = t.v0[i];
            for (int64_t p = i; p < PT; ++p) vi += (ld)t.R[i * PT + p] * (ld)m[p];
            v[i] = vi;
            for (int64_t j = 0; j <= i; ++j) {
                ld s = i == j ? 1.0L : 0.0L;
                for (int64_t p = i; p < PT; ++p) s += (ld)t.R[i * PT + p] * (ld)g[p] * (ld)t.R[j * PT + p];
                S[i * PT + j] = s;
            }
        }
        const ld got = dense_loglike(S, v, PT) - 0.5L * ((ld)t.cperp + (ld)t.logdet0);
        const double rel = (double)(fabsl(got - ref) / fabsl(ref));
        if (rel > worst) worst = rel;
        CHECK(rel < 1e-13);
    }
    return worst;
}

int main() {
    const struct { std::vector<int64_t> Ms, Ps; } cases[] = {
        {{7, 5, 9}, {3, 2, 4}}, {{12}, {5}}, {{6, 4}, {6, 4}}, {{12, 20}, {3, 5}}, {{1, 8, 3, 5}, {1, 2, 3, 1}}, {{30, 25, 33}, {6, 4, 5}},
    };
    for (const auto& c : cases)
        for (int trunc = 0; trunc < 2; ++trunc) {
            const double w = check_structure(c.Ms, c.Ps, trunc != 0);
            printf("E = %d, with_trunc = %d: worst relative error %.3g\n", (int)c.Ms.size(), trunc, w);
        }
    gpb::CoupledTables t;
    {   // an indefinite C0: one off-block pair correlated beyond 1
        Problem pr = make({7, 5, 9}, {3, 2, 4}, false);
        const int64_t MT = pr.MT, a = 2, b = 15;
        const double big = 1.5 * sqrt(pr.cexp[a * MT + a] * pr.cexp[b * MT + b]);
        pr.cexp[a * MT + b] = pr.cexp[b * MT + a] = big;
        CHECK(!gpb::coupled_setup(pr.blk.data(), 3, pr.yexp.data(), pr.cexp.data(), t));
    }
    {   // a repeated row of A
        Problem pr = make({7, 5, 9}, {3, 2, 4}, true);
        for (int64_t i = 0; i < 9; ++i) pr.A[2][3 * 9 + i] = pr.A[2][1 * 9 + i];
        CHECK(!gpb::coupled_setup(pr.blk.data(), 3, pr.yexp.data(), pr.cexp.data(), t));
    }
    {   // beyond the limits, and more GPs than observables
        Problem pr = make({140}, {129}, false);
        CHECK(!gpb::coupled_setup(pr.blk.data(), 1, pr.yexp.data(), pr.cexp.data(), t));
        Problem pq = make({4}, {4}, false);
        pq.blk[0].P = 5;
        CHECK(!gpb::coupled_setup(pq.blk.data(), 1, pq.yexp.data(), pq.cexp.data(), t));
    }
    printf("coupled_setup_check: ok\n");
    return 0;
}
