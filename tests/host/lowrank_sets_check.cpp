// Host check of csrc/lowrank_setup.h (the factorisation of the low-rank block likelihood and the data terms of one data vector
// against it), built with the address and undefined-behaviour sanitizers by tests/test_lowrank_sets_host.py.  For shapes
// (M, P) and K = 6 data vectors against ONE factorisation, the closed form
//     loglike = -1/2 (c_perp_k + v^T S^-1 v) - 1/2 (logdet0 + log det S),  S = I + R diag(g) R^T,  v = R m + v0_k
// is compared with a dense long-double Cholesky of C0 + A^T diag(g) A and dY_k = A^T m + mu - yexp_k written here; the terms of
// set k must be, bit for bit, those of a factorisation of its own followed by the data terms of yexp_k alone (what a single-set
// installation computes); an indefinite C0 and a repeated row of A must be reported as "does not apply".
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../gpbayestools_hic_amd/csrc/lowrank_setup.h"

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
            printf("lowrank_sets_check: FAILED %s (line %d)\n", #c, __LINE__);     \
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
    int64_t M, P, K;
    std::vector<double> A, mu, c0, cexp, data;       // [P][M], [M], [M][M], [M][M], [K][M]
};

static Problem make(int64_t M, int64_t P, int64_t K) {
    Problem pr;
    pr.M = M; pr.P = P; pr.K = K;
    pr.A.resize(P * M);
    for (auto& x : pr.A) x = nrand();
    pr.mu.resize(M);
    for (auto& x : pr.mu) x = 2.0 + nrand();
    std::vector<double> B(M * 2);                    // truncation covariance: B B^T with B [M][2]
    for (auto& x : B) x = 0.1 * nrand();
    pr.c0.assign(M * M, 0.0);
    for (int64_t i = 0; i < M; ++i)
        for (int64_t j = 0; j < M; ++j) pr.c0[i * M + j] = B[i * 2] * B[j * 2] + B[i * 2 + 1] * B[j * 2 + 1];
    std::vector<double> sig(M);
    for (auto& x : sig) x = 0.05 + 0.1 * urand();
    pr.cexp.assign(M * M, 0.0);
    for (int64_t i = 0; i < M; ++i)
        for (int64_t j = 0; j < M; ++j)
            pr.cexp[i * M + j] = (i == j ? sig[i] * sig[i] : 0.0) + 0.3 * sig[i] * sig[j] * exp(-fabs((double)(i - j)) / 5.0);
    pr.data.resize(K * M);
    for (auto& x : pr.data) x = 2.0 + nrand();
    for (int64_t i = 0; i < M; ++i) pr.data[(K - 1) * M + i] += 40.0;      // one set far from the others
    return pr;
}

static double check_shape(int64_t M, int64_t P, int64_t K) {
    Problem pr = make(M, P, K);
    gpb::LowrankFactor f;
    CHECK(gpb::lowrank_factor(M, P, pr.A.data(), pr.c0.data(), pr.cexp.data(), f));
    CHECK(f.ok && f.M == M && f.P == P && (int64_t)f.L.size() == M * M && (int64_t)f.Q.size() == P * M);
    double R[256];
    gpb::lowrank_R16(f, R);
    for (int i = 0; i < 16; ++i)
        for (int j = 0; j < 16; ++j)
            if (j < i || i >= P || j >= P) CHECK(R[i * 16 + j] == 0.0);
    std::vector<double> v0(K * 16, 0.0), cperp(K);
    for (int64_t k = 0; k < K; ++k) gpb::lowrank_data_terms(f, pr.mu.data(), pr.data.data() + k * M, v0.data() + k * 16, &cperp[k]);
    // bit for bit what a single-set set-up of data[k] gives: its own factorisation, then its data terms
    for (int64_t k = 0; k < K; ++k) {
        gpb::LowrankFactor f1;
        CHECK(gpb::lowrank_factor(M, P, pr.A.data(), pr.c0.data(), pr.cexp.data(), f1));
        double v1[16] = {0.0}, c1, R1[256];
        gpb::lowrank_data_terms(f1, pr.mu.data(), pr.data.data() + k * M, v1, &c1);
        gpb::lowrank_R16(f1, R1);
        CHECK(memcmp(v1, v0.data() + k * 16, sizeof(v1)) == 0);
        CHECK(memcmp(&c1, &cperp[k], sizeof(double)) == 0);
        CHECK(memcmp(R1, R, sizeof(R)) == 0);
        CHECK(f1.logdet0 == f.logdet0);
        for (int64_t i = P; i < 16; ++i) CHECK(v0[k * 16 + i] == 0.0);
    }
    double worst = 0.0;
    for (int64_t k = 0; k < K; ++k)
        for (int trial = 0; trial < 20; ++trial) {
            std::vector<double> m(P), g(P);
            for (int64_t p = 0; p < P; ++p) { m[p] = nrand(); g[p] = 0.01 + urand(); }
            std::vector<ld> C(M * M), y(M);
            for (int64_t i = 0; i < M; ++i) {
                ld yi = (ld)pr.mu[i] - (ld)pr.data[k * M + i];
                for (int64_t p = 0; p < P; ++p) yi += (ld)pr.A[p * M + i] * (ld)m[p];
                y[i] = yi;
                for (int64_t j = 0; j < M; ++j) {
                    ld c = (ld)pr.c0[i * M + j] + (ld)pr.cexp[i * M + j];
                    for (int64_t p = 0; p < P; ++p) c += (ld)pr.A[p * M + i] * (ld)g[p] * (ld)pr.A[p * M + j];
                    C[i * M + j] = c;
                }
            }
            const ld ref = dense_loglike(C, y, M);
            std::vector<ld> S(P * P, 0.0L), v(P);
            for (int64_t i = 0; i < P; ++i) {
                ld vi = v0[k * 16 + i];
                for (int64_t p = i; p < P; ++p) vi += (ld)R[i * 16 + p] * (ld)m[p];
                v[i] = vi;
                for (int64_t j = 0; j <= i; ++j) {
                    ld s = i == j ? 1.0L : 0.0L;
                    for (int64_t p = i; p < P; ++p) s += (ld)R[i * 16 + p] * (ld)g[p] * (ld)R[j * 16 + p];
                    S[i * P + j] = s;
                }
            }
            const ld got = dense_loglike(S, v, P) - 0.5L * ((ld)cperp[k] + (ld)(double)f.logdet0);
            const double rel = (double)(fabsl(got - ref) / fabsl(ref));
            if (rel > worst) worst = rel;
            CHECK(rel < 1e-13);
        }
    return worst;
}

int main() {
    const int64_t shapes[][2] = {{7, 3}, {12, 12}, {40, 16}, {5, 1}};
    for (const auto& s : shapes) {
        const double w = check_shape(s[0], s[1], 6);
        printf("M = %d, P = %d, K = 6: worst relative error %.3g\n", (int)s[0], (int)s[1], w);
    }
    gpb::LowrankFactor f;
    {   // an indefinite C0: one pair correlated beyond 1
        Problem pr = make(7, 3, 1);
        const int64_t M = pr.M, a = 2, b = 5;
        const double big = 1.5 * sqrt((pr.c0[a * M + a] + pr.cexp[a * M + a]) * (pr.c0[b * M + b] + pr.cexp[b * M + b]));
        pr.cexp[a * M + b] = pr.cexp[b * M + a] = big;
        CHECK(!gpb::lowrank_factor(M, 3, pr.A.data(), pr.c0.data(), pr.cexp.data(), f));
        CHECK(!f.ok);
    }
    {   // a repeated row of A
        Problem pr = make(12, 5, 1);
        for (int64_t i = 0; i < 12; ++i) pr.A[3 * 12 + i] = pr.A[1 * 12 + i];
        CHECK(!gpb::lowrank_factor(12, 5, pr.A.data(), pr.c0.data(), pr.cexp.data(), f));
        CHECK(!f.ok);
    }
    {   // more GPs than observables
        Problem pr = make(4, 4, 1);
        CHECK(!gpb::lowrank_factor(4, 5, pr.A.data(), pr.c0.data(), pr.cexp.data(), f));
    }
    printf("lowrank_sets_check: ok\n");
    return 0;
}
