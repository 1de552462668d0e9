// psis_fit.h — the pieces of Pareto-smoothed importance sampling that are arithmetic on one sorted tail: the tail length, the
// Zhang-Stephens fit of the generalised Pareto distribution and its quantile function (Vehtari, Simpson, Gelman, Yao, Gabry,
// JMLR 2024; Zhang & Stephens, Technometrics 2009).  One set of functions for the host and the device, included alone by
// tests/host/psis_fit_check.cpp; gpb_psis.hip has the whole procedure in its header.
//   t [n] ascending: the tail's excesses over the cutoff, t_j = exp(x_j) - exp(cutoff), 0-based here, 1-based t_[.] in the formulas.
//   m_est = 30 + floor(sqrt(n)) candidates, i = 1 .. m_est:
//     b_i = (1 - sqrt(m_est / (i - 1/2))) / (3 t_[floor(n / 4 + 1/2)]) + 1 / t_[n]
//     k_i = (1 / n) sum_j log1p(-b_i t_j),   L_i = n (ln(-(b_i / k_i)) - k_i - 1),   w_i = 1 / sum_j exp(L_j - L_i)
//   candidates with w_i < 10 eps are dropped, the rest divided by their sum;  bhat = sum_i w_i b_i,
//   k = (1 / n) sum_j log1p(-bhat t_j),  sigma = -k / bhat,  khat = (n k + 5) / (n + 10)   (the prior: ten observations of k = 1/2)
//   quantile at p: sigma expm1(-khat log1p(-p)) / khat, and -sigma log1p(-p) at khat == 0.
// Every sum runs in a tree fixed by n and m_est alone: a sum over the tail is GPB_PSIS_LANES strided partial sums, lane l taking
// j = l, l + 64, ... in ascending order, folded by halving (lane l += lane l + 32, then + 16, ... + 1), which is what a wave's
// __shfl_down ladder computes; the sums over the candidates run in index order.  psis_fit_serial is that tree on one thread: the
// host's check and the device's kernel compute the same operations in the same order (both are compiled with -ffp-contract=off).
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GPB_PSIS_HD __host__ __device__
#else
#define GPB_PSIS_HD
#endif

#define GPB_PSIS_MAX_S (1 << 24)        // samples per row: the tail is then at most ceil(3 sqrt(S)) = 12288 values
#define GPB_PSIS_MAX_TAIL 12288
#define GPB_PSIS_MAX_CAND 140           // 30 + floor(sqrt(12288))
#define GPB_PSIS_MIN_TAIL 5             // a tail of four or fewer values is not fitted: khat = +inf
#define GPB_PSIS_LANES 64

namespace gpb {

// M = min(S // 5, ceil(3 sqrt(S))): the cutoff is the (M + 1)-th largest value
GPB_PSIS_HD inline int64_t psis_tail_max(int64_t S) {
    const int64_t a = S / 5, b = (int64_t)ceil(3.0 * sqrt((double)S));
    return a < b ? a : b;
}
GPB_PSIS_HD inline int psis_m_est(int n) { return 30 + (int)sqrt((double)n); }
// the order statistic the candidates are scaled by, 0-based: floor(n / 4 + 1/2) - 1
GPB_PSIS_HD inline int psis_quartile_index(int n) { return (int)((double)n / 4.0 + 0.5) - 1; }

// b_i, i = 1 .. m_est
GPB_PSIS_HD inline double psis_candidate(int i, int m_est, double t_quart, double t_last) {
    double b = 1.0 - sqrt((double)m_est / ((double)i - 0.5));
    b = b / (3.0 * t_quart);
    return b + 1.0 / t_last;
}
// lane's share of sum_j log1p(-b t_j)
GPB_PSIS_HD inline double psis_lane_sum(const double* t, int n, double b, int lane) {
    double s = 0.0;
    for (int j = lane; j < n; j += GPB_PSIS_LANES) s = s + log1p(-b * t[j]);
    return s;
}
GPB_PSIS_HD inline double psis_profile(int n, double b, double k) { return (double)n * (log(-(b / k)) - k - 1.0); }
// w_i from the profile values L [m]
GPB_PSIS_HD inline double psis_weight(const double* L, int m, int i) {
    double s = 0.0;
    for (int j = 0; j < m; ++j) s = s + exp(L[j] - L[i]);
    return 1.0 / s;
}
// bhat from the candidates and their weights
GPB_PSIS_HD inline double psis_bhat(const double* b, const double* w, int m) {
    const double thr = 10.0 * DBL_EPSILON;
    double sum = 0.0;
    for (int i = 0; i < m; ++i)
        if (w[i] >= thr) sum = sum + w[i];
    double bh = 0.0;
    for (int i = 0; i < m; ++i)
        if (w[i] >= thr) bh = bh + b[i] * (w[i] / sum);
    return bh;
}
// from ksum = sum_j log1p(-bhat t_j): sigma and the prior-shrunk khat
GPB_PSIS_HD inline void psis_finish(int n, double bhat, double ksum, double* khat, double* sigma) {
    const double k = ksum / (double)n;
    *sigma = -k / bhat;
    *khat = ((double)n * k + 5.0) / ((double)n + 10.0);
}
// the generalised Pareto quantile at p in (0, 1)
GPB_PSIS_HD inline double psis_gpd_quantile(double p, double khat, double sigma) {
    if (khat == 0.0) return -sigma * log1p(-p);
    return expm1(-khat * log1p(-p)) / khat * sigma;
}
// the value that replaces the j-th smallest (0-based) of n tail values, before the truncation at 0
GPB_PSIS_HD inline double psis_smoothed(int j, int n, double khat, double sigma, double exp_cutoff) {
    const double p = ((double)j + 0.5) / (double)n;
    return log(psis_gpd_quantile(p, khat, sigma) + exp_cutoff);
}

// folds GPB_PSIS_LANES lane values as a wave's __shfl_down ladder does; the sum is left in v[0]
inline double psis_fold(double* v) {
    for (int off = GPB_PSIS_LANES / 2; off > 0; off >>= 1)
        for (int l = 0; l < off; ++l) v[l] = v[l] + v[l + off];
    return v[0];
}
inline double psis_tail_sum(const double* t, int n, double b) {
    double v[GPB_PSIS_LANES];
    for (int l = 0; l < GPB_PSIS_LANES; ++l) v[l] = psis_lane_sum(t, n, b, l);
    return psis_fold(v);
}
// the whole fit on one thread, n >= GPB_PSIS_MIN_TAIL; b_out, w_out [psis_m_est(n)] (optional): the candidates and their weights
inline void psis_fit_serial(const double* t, int n, double* khat, double* sigma, double* b_out = nullptr, double* w_out = nullptr) {
    const int m = psis_m_est(n);
    double b[GPB_PSIS_MAX_CAND + 64], L[GPB_PSIS_MAX_CAND + 64], w[GPB_PSIS_MAX_CAND + 64];
    const double tq = t[psis_quartile_index(n)], tl = t[n - 1];
    for (int i = 0; i < m; ++i) {
        b[i] = psis_candidate(i + 1, m, tq, tl);
        L[i] = psis_profile(n, b[i], psis_tail_sum(t, n, b[i]) / (double)n);
    }
    for (int i = 0; i < m; ++i) w[i] = psis_weight(L, m, i);
    const double bh = psis_bhat(b, w, m);
    psis_finish(n, bh, psis_tail_sum(t, n, bh), khat, sigma);
    for (int i = 0; i < m; ++i) {
        if (b_out) b_out[i] = b[i];
        if (w_out) w_out[i] = w[i];
    }
}

}  // namespace gpb
