// gpb_diag.hip — convergence diagnostics of a resident chain (gpb_mcmc_diag): the walker-averaged normalised autocorrelation
// function, the integrated autocorrelation time with emcee's automatic window, and split-R-hat, per parameter, of a chain that
// lies in HBM as [nsteps, nwalkers, d] (the stretch sampler's store) or [nwalkers, nsteps, d] (the pickles), through strides.
// What emcee's autocorr.integrated_time does with one zero-padded FFT per (walker, parameter) in a Python loop is here ONE banded
// fp64 matrix product per parameter: with y_w the centred series of walker w scaled to unit length and Y[t][w] = y_w(t),
//     sum_w  sum_t y_w(t) y_w(t + k)  =  the sum of the k-th diagonal of  Y Y^T,
// a product with the walkers as the inner dimension; only the 64 x 64 blocks (I, J), J >= I, within max_lag of the diagonal exist.
//   k_diag_pack    one lane per (walker, parameter): two-pass mean, c0 = sum of squares of the centred series, the means and sample
//                  variances of the two halves; writes Y[j][t][w] (walker-contiguous; t padded to 64, w to 16, padding and the walkers
//                  that never moved — all values equal, decided by comparing them — exactly zero)
//   k_diag_stats   one workgroup per parameter: grand mean, W, B, split-R-hat, the number of constant walkers
//   k_diag_gram    one workgroup per (parameter, block of the band): gemm_tile_loop<64> over the walkers, both operands rows of Y;
//                  the accumulator tile goes to LDS and 127 lanes sum one diagonal each in row order -> per-block lag partials
//   k_diag_lags    one lane per lag: its block partials added in block-row order (an order that depends on nsteps alone, so rho[k]
//                  has the same bits for every max_lag >= k), divided by the number of walkers that moved
//   k_diag_scan    one lane per parameter: taus[m] = 2 sum_{k <= m} rho[k] - 1 sequentially, the first m >= c taus[m]
// Nothing accumulates in place, no floating-point atomics, no workgroup waits for another: every sum has one fixed order.
#include "gpb_internal.h"
#include "diag_gram.h"
#include "block_reduce.h"
#include <math.h>

namespace gpb {

namespace {

constexpr int DIAG_THREADS = REDUCE_THREADS;      // Kahan, block_sum: block_reduce.h
constexpr int DIAG_STATS = 6;                 // per (parameter, walker): mean | moved (0 / 1) | mean, variance of half 1 | of half 2
constexpr int64_t DIAG_WS_BYTES = (int64_t)GPB_DIAG_WS_MB << 20;

// ---------------------------------------------------------------------------------------------------------------- pack
// element (t, w, j) of the chain at x[t * ss + w * ws + j]; lane = (w, jj) with jj fastest: a wave reads whole parameter rows
__global__ __launch_bounds__(DIAG_THREADS) void k_diag_pack(const double* __restrict__ x, int64_t n, int64_t nw, int64_t ss, int64_t ws,
                                                            int64_t j0, int64_t dg, int64_t nsp, int64_t nwp, double* __restrict__ Y,
                                                            double* __restrict__ stats) {
    const int64_t idx = (int64_t)blockIdx.x * DIAG_THREADS + threadIdx.x;
    if (idx >= nwp * dg) return;
    const int64_t w = idx / dg, jj = idx % dg;
    double* y = Y + jj * nsp * nwp + w;
    if (w >= nw) {
        for (int64_t t = 0; t < nsp; ++t) y[t * nwp] = 0.0;
        return;
    }
    const double* p = x + w * ws + j0 + jj;
    const int64_t h = n / 2;
    // A walker all of whose values are equal never moved.  Decided by comparing the values: the rounded mean of a constant series
    // fl(fl(n v) / n) is often not v, and a c0 about it would be n ulp^2 > 0 — the walker would enter the average as the constant
    // series 1 / sqrt(n).  Its means are its value, so that its c0 and its halves' variances come out exactly 0.
    const double v0 = p[0];
    bool differs = false;
    Kahan a, a1, a2;
    for (int64_t t = 0; t < n; ++t) {
        const double v = p[t * ss];
        differs |= v != v0;
        a.add(v);
        if (t < h) a1.add(v);
        if (t >= n - h) a2.add(v);
    }
    const double mean = differs ? a.s / (double)n : v0, m1 = differs ? a1.s / (double)h : v0, m2 = differs ? a2.s / (double)h : v0;
    Kahan c, c1, c2;
    for (int64_t t = 0; t < n; ++t) {
        const double v = p[t * ss];
        const double e = v - mean;
        c.add(e * e);
        if (t < h) {
            const double e1 = v - m1;
            c1.add(e1 * e1);
        }
        if (t >= n - h) {
            const double e2 = v - m2;
            c2.add(e2 * e2);
        }
    }
    const double c0 = c.s;
    const bool moved = differs && c0 > 0.0;               // (c0 > 0: differences whose squares underflow count as none)
    const double rs = moved ? 1.0 / sqrt(c0) : 0.0;
    for (int64_t t = 0; t < n; ++t) y[t * nwp] = moved ? (p[t * ss] - mean) * rs : 0.0;
    for (int64_t t = n; t < nsp; ++t) y[t * nwp] = 0.0;
    double* st = stats + (jj * nwp + w) * DIAG_STATS;
    st[0] = mean;
    st[1] = moved ? 1.0 : 0.0;
    st[2] = m1;
    st[3] = c1.s / (double)(h - 1);
    st[4] = m2;
    st[5] = c2.s / (double)(h - 1);
}

// ---------------------------------------------------------------------------------------------------------------- moments, R-hat
__global__ __launch_bounds__(DIAG_THREADS) void k_diag_stats(const double* __restrict__ stats, int64_t n, int64_t nw, int64_t nwp,
                                                             int64_t j0, double* __restrict__ moments, double* __restrict__ rhat,
                                                             int* __restrict__ nconst) {
    __shared__ double sw[REDUCE_WAVES];
    const int tid = threadIdx.x;
    const int64_t jj = blockIdx.x, j = j0 + jj;
    const double* st = stats + jj * nwp * DIAG_STATS;
    const double h = (double)(n / 2), n2 = 2.0 * (double)nw;
    Kahan am, amv, ahm, ahv;
    for (int64_t w = tid; w < nw; w += DIAG_THREADS) {
        const double* s = st + w * DIAG_STATS;
        am.add(s[0]);
        amv.add(s[1]);
        ahm.add(s[2]);
        ahm.add(s[4]);
        ahv.add(s[3]);
        ahv.add(s[5]);
    }
    const double mean = block_sum(am.s, sw) / (double)nw;
    const double nmov = block_sum(amv.s, sw);                 // (a sum of zeros and ones: exact)
    const double hm = block_sum(ahm.s, sw) / n2;
    const double W = block_sum(ahv.s, sw) / n2;
    Kahan ab;
    for (int64_t w = tid; w < nw; w += DIAG_THREADS) {
        const double* s = st + w * DIAG_STATS;
        const double e1 = s[2] - hm, e2 = s[4] - hm;
        ab.add(e1 * e1);
        ab.add(e2 * e2);
    }
    const double B = h * (block_sum(ab.s, sw) / (n2 - 1.0));
    if (tid == 0) {
        moments[j * 3 + 0] = mean;
        moments[j * 3 + 1] = W;
        moments[j * 3 + 2] = B;
        rhat[j] = nmov > 0.0 ? sqrt(((h - 1.0) / h * W + B / h) / W) : NAN;
        nconst[j] = (int)((double)nw - nmov);
    }
}

// (the band of Y Y^T, k_diag_gram: diag_gram.h — gpb_rank.hip takes its lag sums from the same kernel)

// ---------------------------------------------------------------------------------------------------------------- lags
// rho[j][k]: lag k = 64 D + r lives on diagonal r of the blocks of block diagonal D and, for r > 0, on diagonal r - 64 of those
// of D + 1; block row by block row, D before D + 1.  nb = padded nsteps / 64 fixes the order — max_lag only decides which lags exist.
__global__ __launch_bounds__(DIAG_THREADS) void k_diag_lags(const double* __restrict__ part, const int* __restrict__ nconst, int64_t nw,
                                                            int64_t nb, int64_t pstride, int64_t max_lag, int64_t j0,
                                                            double* __restrict__ rho) {
    const int64_t k = (int64_t)blockIdx.x * DIAG_THREADS + threadIdx.x;
    if (k > max_lag) return;
    const int64_t jj = blockIdx.y, j = j0 + jj;
    const int64_t D = k / 64, r = k % 64;
    const double* p0 = part + (jj * pstride + D * nb) * 128 + 63 + r;
    const double* p1 = part + (jj * pstride + (D + 1) * nb) * 128 + 63 + r - 64;
    double s = 0.0;
    for (int64_t I = 0; I + D < nb; ++I) {
        s += p0[I * 128];
        if (r > 0 && I + D + 1 < nb) s += p1[I * 128];
    }
    const int nmov = (int)nw - nconst[j];
    rho[j * (max_lag + 1) + k] = nmov > 0 ? s / (double)nmov : NAN;
}

// ---------------------------------------------------------------------------------------------------------------- window
__global__ __launch_bounds__(64) void k_diag_scan(const double* __restrict__ rho, const int* __restrict__ nconst, int64_t nw,
                                                  int64_t max_lag, double c, int64_t j0, int64_t dg,
                                                  double* __restrict__ tau, int* __restrict__ window) {
    const int64_t jj = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (jj >= dg) return;
    const int64_t j = j0 + jj;
    if ((int)nw - nconst[j] <= 0) {
        tau[j] = NAN;
        window[j] = -1;
        return;
    }
    const double* f = rho + j * (max_lag + 1);
    double cum = 0.0, taus = 0.0;
    for (int64_t m = 0; m <= max_lag; ++m) {
        cum += f[m];
        taus = 2.0 * cum - 1.0;
        if ((double)m >= c * taus) {
            tau[j] = taus;
            window[j] = (int)m;
            return;
        }
    }
    tau[j] = taus;
    window[j] = (int)max_lag | GPB_DIAG_NO_WINDOW;
}

}  // namespace

// results of all d parameters into the staging block res: rho [d][max_lag + 1] | tau [d] | moments [d][3] | rhat [d] | window [d]
// (int) | nconst [d] (int)
int launch_mcmc_diag(gpb_ctx* ctx, const double* x, int64_t n, int64_t nw, int64_t d, int64_t ss, int64_t ws, int64_t max_lag,
                     double c, bool need_acf, double* rho, double* tau, double* moments, double* rhat, int* window, int* nconst) {
    const int64_t nsp = round_up(n, 64), nwp = round_up(nw, 16), nb = nsp / 64;
    const int64_t nd = need_acf ? imin64((max_lag + 63) / 64, nb - 1) + 1 : 0;      // block diagonals of the band
    const int64_t nblk = nd * nb;
    if (nblk > 0x7fffffffLL) GPB_FAIL(GPB_E_ARG, "gpb_mcmc_diag: more than 2^31 - 1 blocks in the band");
    // one parameter: Y, the lag partials of its blocks (one diagonal more is addressed, never read, by the last lags), the statistics
    DiagWs dw;
    Carver<double> one;
    dw.lay(one, 1, nsp, nwp, nblk + nb, DIAG_STATS);
    const int64_t per = one.total();
    int64_t G = DIAG_WS_BYTES / (8 * per);
    G = G < 1 ? 1 : (G > d ? d : G);
    if (G > 65535) G = 65535;
    if ((nwp * G + DIAG_THREADS - 1) / DIAG_THREADS > 0x7fffffffLL) GPB_FAIL(GPB_E_ARG, "gpb_mcmc_diag: too many walkers");
    if (const int rc = ctx_carve(ctx, ctx->diag_ws, [&](Carver<double>& cv) { dw.lay(cv, G, nsp, nwp, nblk + nb, DIAG_STATS); }))
        return rc;
    double *Y = dw.Y, *part = dw.part, *stats = dw.stats;
    for (int64_t j0 = 0; j0 < d; j0 += G) {
        const int64_t dg = imin64(G, d - j0);
        hipLaunchKernelGGL(k_diag_pack, dim3((unsigned)((nwp * dg + DIAG_THREADS - 1) / DIAG_THREADS)), dim3(DIAG_THREADS), 0,
                           ctx->stream, x, n, nw, ss, ws, j0, dg, nsp, nwp, Y, stats);
        hipLaunchKernelGGL(k_diag_stats, dim3((unsigned)dg), dim3(DIAG_THREADS), 0, ctx->stream, stats, n, nw, nwp, j0, moments, rhat,
                           nconst);
        if (!need_acf) continue;
        hipLaunchKernelGGL(k_diag_gram, dim3((unsigned)nblk, (unsigned)dg), dim3(GEMM_THREADS), 0, ctx->stream, Y, nsp, nwp, nb,
                           nblk + nb, part);
        hipLaunchKernelGGL(k_diag_lags, dim3((unsigned)((max_lag + DIAG_THREADS) / DIAG_THREADS), (unsigned)dg), dim3(DIAG_THREADS), 0,
                           ctx->stream, part, nconst, nw, nb, nblk + nb, max_lag, j0, rho);
        hipLaunchKernelGGL(k_diag_scan, dim3((unsigned)((dg + 63) / 64)), dim3(64), 0, ctx->stream, rho, nconst, nw, max_lag, c, j0, dg,
                           tau, window);
    }
    GPB_HIP(hipGetLastError());
    return 0;
}

}  // namespace gpb

using namespace gpb;

extern "C" int gpb_mcmc_diag(gpb_ctx* ctx, const double* x_dev, int64_t nsteps, int64_t nwalkers, int64_t d, int64_t step_stride,
                             int64_t walker_stride, int64_t max_lag, double c, int on_device, double* rho, double* tau,
                             int32_t* window, double* moments, double* rhat, int32_t* nconst) {
    if (!ctx || !x_dev) return GPB_E_ARG;
    if (nsteps < 4) GPB_FAIL(GPB_E_ARG, "gpb_mcmc_diag: need nsteps >= 4");
    if (nwalkers < 1 || d < 1) GPB_FAIL(GPB_E_ARG, "gpb_mcmc_diag: need nwalkers >= 1 and d >= 1");
    if (nsteps > 0x7fffffffLL || nwalkers > 0x7fffffffLL || d > 0x7fffffffLL)
        GPB_FAIL(GPB_E_ARG, "gpb_mcmc_diag: more than 2^31 - 1 steps, walkers or parameters");
    if (max_lag < 0 || max_lag > nsteps - 1) GPB_FAIL(GPB_E_ARG, "gpb_mcmc_diag: max_lag outside [0, nsteps - 1]");
    if (!(c > 0.0) || !isfinite(c)) GPB_FAIL(GPB_E_ARG, "gpb_mcmc_diag: c must be positive and finite");
    if (walker_stride < d || step_stride < d) GPB_FAIL(GPB_E_ARG, "gpb_mcmc_diag: a stride below d (elements would alias)");
    // (both factors below 2^31 times a stride the caller could address: the products are compared as 128-bit integers)
    const bool steps_outer = (__int128)step_stride >= (__int128)walker_stride * nwalkers;
    const bool walkers_outer = (__int128)walker_stride >= (__int128)step_stride * nsteps;
    if (!steps_outer && !walkers_outer)
        GPB_FAIL(GPB_E_ARG, "gpb_mcmc_diag: neither stride spans the other axis (elements would alias)");
    if (!rho && !tau && !window && !moments && !rhat && !nconst) return 0;
    GPB_HIP(hipSetDevice(ctx->device));
    const bool need_acf = rho || tau || window;
    const int64_t L1 = max_lag + 1;
    const int64_t n_rho = need_acf ? d * L1 : 0;
    // the kernels write every statistic, wanted or not, into the stage; what the caller wants is copied from there
    DiagStage s;
    if (const int rc = ctx_carve(ctx, ctx->out_stage, [&](Carver<double>& cv) { s.lay(cv, n_rho, d); })) return rc;
    if (const int rc = launch_mcmc_diag(ctx, x_dev, nsteps, nwalkers, d, step_stride, walker_stride, max_lag, c, need_acf, s.rho, s.tau,
                                        s.moments, s.rhat, s.window, s.nconst))
        return rc;
    HostOut so(ctx, on_device != 0, true);
    so.at(rho, s.rho, n_rho);
    so.at(tau, s.tau, d);
    so.at(window, s.window, d);
    so.at(moments, s.moments, 3 * d);
    so.at(rhat, s.rhat, d);
    so.at(nconst, s.nconst, d);
    return so.finish();
}
