// lowrank_setup.h — host set-up of the low-rank block likelihood (plain C++, no HIP: tests/host/lowrank_sets_check.cpp includes
// this header alone).
//   PCA mode (src/emulator.py:584-587 + src/mcmc.py:23-65): the covariance of every walker is C = C0 + A^T D A with the SAME
//   C0 = C_trunc + C_exp and a walker-dependent D = diag(var_p) of rank P << M.  With C0 = L0 L0^T and the thin QR
//   factorisation L0^-1 A^T = Q R (M x P, P x P):
//       L0^-1 C L0^-T = I + Q (R D R^T) Q^T
//       log det C = log det C0 + log det S,                 S = I_P + R D R^T
//       y^T C^-1 y = |(I - Q Q^T) L0^-1 y|^2 + v^T S^-1 v,  v = Q^T L0^-1 y = R m + v0
//   because y = A^T m + (mu - yexp) and L0^-1 A^T m = Q R m lies in the span of Q: the first term is a constant of the
//   emulator.  No difference of large numbers anywhere (unlike the Woodbury identity); against 40-digit arithmetic the form
//   is as accurate as the dense Cholesky (1e-15 relative).  Per walker this is a P x P Cholesky instead of an M x M one.
//   Two pieces:
//     lowrank_factor      L0, log det C0, Q, R — everything that does NOT depend on the data.  Long double, O(M^3), once per
//                         experimental covariance.
//     lowrank_data_terms  v0 = Q^T L0^-1 (mu - yexp) [P] and c_perp = |(I - Q Q^T) L0^-1 (mu - yexp)|^2 of ONE data vector,
//                         given a factorisation: O(M^2).  A second data set against the same covariance (a closure study:
//                         gpb_chain_like_sets) costs this and no second Cholesky.
//   A covariance PER data set is out of scope: it would need a factorisation (and an R, a log det C0) per set.
#pragma once
#include <math.h>
#include <stdint.h>
#include <vector>

namespace gpb {

struct LowrankFactor {
    int64_t M = 0, P = 0;
    std::vector<long double> L;    // [M][M] lower triangle of the Cholesky factor of C0
    std::vector<long double> Q;    // [P][M] the orthonormal columns of Q, one per row
    std::vector<long double> R;    // [P][P] upper triangle, row-major
    long double logdet0 = 0.0L;
    bool ok = false;
    void clear() { M = P = 0; L.clear(); Q.clear(); R.clear(); logdet0 = 0.0L; ok = false; }
};

// x <- L0^-1 x
inline void lowrank_fwd(const LowrankFactor& f, long double* x) {
    const int64_t M = f.M;
    const long double* L = f.L.data();
    for (int64_t i = 0; i < M; ++i) {
        long double v = x[i];
        for (int64_t k = 0; k < i; ++k) v -= L[i * M + k] * x[k];
        x[i] = v / L[i * M + i];
    }
}

// A [P][M], c0 [M][M] (the truncation covariance), cexp [M][M].  false (f.ok likewise): the form does not apply — C0 not
// positive definite, or A (numerically) rank deficient.
inline bool lowrank_factor(int64_t M, int64_t P, const double* A, const double* c0, const double* cexp, LowrankFactor& f) {
    f.clear();
    if (M < 1 || P < 1 || P > M) return false;
    f.M = M; f.P = P;
    f.L.assign((size_t)(M * M), 0.0L);
    long double* L = f.L.data();
    for (int64_t i = 0; i < M; ++i)
        for (int64_t j = 0; j <= i; ++j) {                         // symmetrised lower triangle of C0
            const double a = c0[i * M + j] + cexp[i * M + j], b = c0[j * M + i] + cexp[j * M + i];
            L[i * M + j] = 0.5L * ((long double)a + (long double)b);
        }
    long double logdet = 0.0L;
    for (int64_t j = 0; j < M; ++j) {                              // Cholesky, column by column
        long double dsum = L[j * M + j];
        for (int64_t k = 0; k < j; ++k) dsum -= L[j * M + k] * L[j * M + k];
        if (!(dsum > 0.0L)) return false;
        const long double ljj = sqrtl(dsum);
        L[j * M + j] = ljj;
        logdet += 2.0L * logl(ljj);
        for (int64_t i = j + 1; i < M; ++i) {
            long double v = L[i * M + j];
            for (int64_t k = 0; k < j; ++k) v -= L[i * M + k] * L[j * M + k];
            L[i * M + j] = v / ljj;
        }
    }
    f.Q.assign((size_t)(P * M), 0.0L);
    f.R.assign((size_t)(P * P), 0.0L);
    long double* R = f.R.data();
    for (int64_t j = 0; j < P; ++j) {                              // column j of L0^-1 A^T, then Gram-Schmidt twice
        long double* q = f.Q.data() + j * M;
        for (int64_t i = 0; i < M; ++i) q[i] = A[j * M + i];
        lowrank_fwd(f, q);
        long double norm0 = 0.0L;
        for (int64_t i = 0; i < M; ++i) norm0 += q[i] * q[i];
        for (int pass = 0; pass < 2; ++pass)
            for (int64_t i = 0; i < j; ++i) {
                const long double* qi = f.Q.data() + i * M;
                long double r = 0.0L;
                for (int64_t k = 0; k < M; ++k) r += qi[k] * q[k];
                for (int64_t k = 0; k < M; ++k) q[k] -= r * qi[k];
                R[i * P + j] += r;
            }
        long double nrm = 0.0L;
        for (int64_t i = 0; i < M; ++i) nrm += q[i] * q[i];
        if (!(nrm > 1e-24L * norm0) || !(norm0 > 0.0L)) return false;      // A (numerically) rank deficient
        nrm = sqrtl(nrm);
        R[j * P + j] = nrm;
        for (int64_t i = 0; i < M; ++i) q[i] /= nrm;
    }
    f.logdet0 = logdet;
    f.ok = true;
    return true;
}

// The data terms of one yexp [M] against a factorisation: v0 [P] and c_perp, rounded to double once at the end.
inline void lowrank_data_terms(const LowrankFactor& f, const double* mu, const double* yexp, double* v0_out, double* cperp_out) {
    const int64_t M = f.M, P = f.P;
    std::vector<long double> w((size_t)M);
    for (int64_t i = 0; i < M; ++i) w[i] = (long double)mu[i] - (long double)yexp[i];
    lowrank_fwd(f, w.data());
    std::vector<long double> v0((size_t)P, 0.0L);
    for (int64_t j = 0; j < P; ++j)
        for (int64_t k = 0; k < M; ++k) v0[j] += f.Q[j * M + k] * w[k];
    long double cperp = 0.0L;
    for (int64_t k = 0; k < M; ++k) {
        long double t = w[k];
        for (int64_t j = 0; j < P; ++j) t -= f.Q[j * M + k] * v0[j];
        cperp += t * t;
    }
    for (int64_t i = 0; i < P; ++i) v0_out[i] = (double)v0[i];
    *cperp_out = (double)cperp;
}

// R as the kernels take it: [16][16] doubles, upper triangle, zero padded (P <= 16)
inline void lowrank_R16(const LowrankFactor& f, double* Rh) {
    for (int i = 0; i < 256; ++i) Rh[i] = 0.0;
    for (int64_t i = 0; i < f.P; ++i)
        for (int64_t j = i; j < f.P; ++j) Rh[i * 16 + j] = (double)f.R[i * f.P + j];
}

}  // namespace gpb
