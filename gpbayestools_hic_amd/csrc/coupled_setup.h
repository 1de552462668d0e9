// coupled_setup.h — host set-up of the coupled chain likelihood (plain C++, no HIP: tests/host/coupled_setup_check.cpp includes
// this header alone).
//   The experimental covariance of a chain may couple its emulators (a shared normalisation uncertainty, errors correlated
//   across the emulators' observables; the reference adds whatever expdata_cov holds, src/mcmc.py:288-293).  The covariance
//   of a row is then
//       C = C0 + A^T diag(g) A,   C0 = blockdiag(C_trunc,e) + C_exp  (MT x MT, full),   A = blockdiag(A_e)  (PT x MT),
//   with MT = sum M_e observables, PT = sum P_e GPs, g the GPs' variances — lowrank_setup's form (gpb_api.hip) with joint
//   matrices.  With C0 = L0 L0^T, the thin QR factorisation L0^-1 A^T = Q R and w0 = L0^-1 (mu - yexp):
//       v0 = Q^T w0        c_perp = |w0 - Q v0|^2        logdet0 = log det C0
//       S  = I + R diag(g) R^T        v = R m + v0
//       loglike = -1/2 (c_perp + v^T S^-1 v) - 1/2 (logdet0 + log det S)
//   R is a dense upper triangle of order PT; c_perp, v0 and logdet0 belong to the chain.  All in long double, once per
//   experiment: O(MT^3).
#pragma once
#include <math.h>
#include <stdint.h>
#include <vector>

namespace gpb {

constexpr int64_t COUPLED_MAX_PT = 128;     // GPs of a coupled chain (the kernels' largest padded order)
constexpr int64_t COUPLED_MAX_MT = 2048;    // observables of a coupled chain

struct CoupledBlock {          // one emulator of the chain
    int64_t M, P;
    const double* A;           // [P][M]
    const double* mu;          // [M]
    const double* C0;          // [M][M] truncation covariance (nullptr: zeros)
};

struct CoupledTables {
    int64_t PT = 0, MT = 0;
    std::vector<double> R;     // [PT][PT] upper triangle, row-major (zero below the diagonal)
    std::vector<double> v0;    // [PT]
    double cperp = 0.0, logdet0 = 0.0;
};

// false: the form does not apply — C0 not positive definite, A numerically rank deficient (lowrank_setup's tests), or the
// chain beyond the limits.  yexp [MT], cexp [MT][MT] in emuList order.
inline bool coupled_setup(const CoupledBlock* blk, int E, const double* yexp, const double* cexp, CoupledTables& out) {
    int64_t MT = 0, PT = 0;
    for (int e = 0; e < E; ++e) {
        if (blk[e].M < 1 || blk[e].P < 1 || blk[e].P > blk[e].M) return false;
        MT += blk[e].M;
        PT += blk[e].P;
    }
    if (E < 1 || PT > COUPLED_MAX_PT || MT > COUPLED_MAX_MT) return false;
    std::vector<long double> L((size_t)(MT * MT), 0.0L);
    for (int64_t i = 0; i < MT; ++i)
        for (int64_t j = 0; j <= i; ++j)                               // symmetrised lower triangle of C_exp ...
            L[i * MT + j] = 0.5L * ((long double)cexp[i * MT + j] + (long double)cexp[j * MT + i]);
    for (int64_t e = 0, o = 0; e < E; o += blk[e].M, ++e) {            // ... + the emulators' truncation blocks
        if (!blk[e].C0) continue;
        const int64_t M = blk[e].M;
        for (int64_t i = 0; i < M; ++i)
            for (int64_t j = 0; j <= i; ++j)
                L[(o + i) * MT + o + j] += 0.5L * ((long double)blk[e].C0[i * M + j] + (long double)blk[e].C0[j * M + i]);
    }
    long double logdet = 0.0L;
    for (int64_t j = 0; j < MT; ++j) {                                 // Cholesky, column by column
        long double dsum = L[j * MT + j];
        for (int64_t k = 0; k < j; ++k) dsum -= L[j * MT + k] * L[j * MT + k];
        if (!(dsum > 0.0L)) return false;
        const long double ljj = sqrtl(dsum);
        L[j * MT + j] = ljj;
        logdet += 2.0L * logl(ljj);
        for (int64_t i = j + 1; i < MT; ++i) {
            long double v = L[i * MT + j];
            for (int64_t k = 0; k < j; ++k) v -= L[i * MT + k] * L[j * MT + k];
            L[i * MT + j] = v / ljj;
        }
    }
    auto fwd = [&](std::vector<long double>& x, int64_t from) {        // x <- L0^-1 x for an x that is zero in front of `from`
        for (int64_t i = from; i < MT; ++i) {
            long double v = x[i];
            for (int64_t k = from; k < i; ++k) v -= L[i * MT + k] * x[k];
            x[i] = v / L[i * MT + i];
        }
    };
    // Column j of A^T is non-zero only in its emulator's rows [o, o + M): L0^-1 of it starts at row o, and so does every
    // column of Q of that emulator or a later one (from[]: the first row a column of Q can be non-zero in).
    std::vector<std::vector<long double>> Q((size_t)PT, std::vector<long double>((size_t)MT, 0.0L));
    std::vector<int64_t> from((size_t)PT, 0);
    std::vector<long double> R((size_t)(PT * PT), 0.0L);
    int64_t j = 0;
    for (int64_t e = 0, o = 0; e < E; o += blk[e].M, ++e) {
        const int64_t M = blk[e].M;
        for (int64_t p = 0; p < blk[e].P; ++p, ++j) {                  // column j of L0^-1 A^T, then Gram-Schmidt twice
            std::vector<long double>& q = Q[j];
            for (int64_t i = 0; i < M; ++i) q[o + i] = blk[e].A[p * M + i];
            fwd(q, o);
            int64_t qfrom = o;
            long double norm0 = 0.0L;
            for (int64_t i = o; i < MT; ++i) norm0 += q[i] * q[i];
            for (int pass = 0; pass < 2; ++pass)
                for (int64_t i = 0; i < j; ++i) {
                    const int64_t k0 = from[i] > qfrom ? from[i] : qfrom;
                    long double r = 0.0L;
                    for (int64_t k = k0; k < MT; ++k) r += Q[i][k] * q[k];
                    for (int64_t k = from[i]; k < MT; ++k) q[k] -= r * Q[i][k];
                    if (from[i] < qfrom) qfrom = from[i];
                    R[i * PT + j] += r;
                }
            long double nrm = 0.0L;
            for (int64_t i = qfrom; i < MT; ++i) nrm += q[i] * q[i];
            if (!(nrm > 1e-24L * norm0) || !(norm0 > 0.0L)) return false;      // A (numerically) rank deficient
            nrm = sqrtl(nrm);
            R[j * PT + j] = nrm;
            for (int64_t i = qfrom; i < MT; ++i) q[i] /= nrm;
            from[j] = qfrom;
        }
    }
    std::vector<long double> w((size_t)MT);
    for (int64_t e = 0, o = 0; e < E; o += blk[e].M, ++e)
        for (int64_t i = 0; i < blk[e].M; ++i) w[o + i] = (long double)blk[e].mu[i] - (long double)yexp[o + i];
    fwd(w, 0);
    std::vector<long double> v0((size_t)PT, 0.0L);
    for (int64_t c = 0; c < PT; ++c)
        for (int64_t k = from[c]; k < MT; ++k) v0[c] += Q[c][k] * w[k];
    for (int64_t c = 0; c < PT; ++c)                                   // w <- w0 - Q v0
        for (int64_t k = from[c]; k < MT; ++k) w[k] -= Q[c][k] * v0[c];
    long double cperp = 0.0L;
    for (int64_t k = 0; k < MT; ++k) cperp += w[k] * w[k];
    out.PT = PT;
    out.MT = MT;
    out.R.assign((size_t)(PT * PT), 0.0);
    out.v0.assign((size_t)PT, 0.0);
    for (int64_t i = 0; i < PT; ++i) {
        out.v0[i] = (double)v0[i];
        for (int64_t c = i; c < PT; ++c) out.R[i * PT + c] = (double)R[i * PT + c];
    }
    out.cperp = (double)cperp;
    out.logdet0 = (double)logdet;
    return true;
}

}  // namespace gpb
