// gpb_smc.hip — a tempered sequential Monte Carlo sampler over a chain of emulators, resident on the device
// (Chain.run_SMC, smc.py).  The outer algorithm is the one pocoMC runs — adaptive tempering from the prior to the
// posterior, resampling, MCMC moves, a running evidence — with the particle covariance in place of a normalizing flow.
//   k_smc_reweight   one workgroup: the bisection for the next beta at the target effective sample size, the evidence
//                    increment (log-sum-exp), the weights and their inclusive normalised scan
//   k_smc_resample   systematic resampling: a binary search per position, the gather of x and logl by ancestor
//   k_smc_mean       the mean of the resampled particles, one workgroup per column
//   k_smc_moments    their covariance (divided by N), one workgroup per entry of the lower triangle
//   k_smc_chol       the d x d lower Cholesky factor in LDS; a non-positive pivot only sets a flag
//   k_smc_propose    z ~ N(0, I) (Philox + Box-Muller), x' = x + exp(log_sigma) Lc z, one wave per particle, Lc in LDS
//   (evaluation)     chain_eval: gpb_chain_logpost or the per-emulator sequence, all N proposals in one batch
//   k_smc_accept     log u < beta (logl' - logl), the particles replaced in place, the counters, the log_sigma step
// Written with contraction off and sums in index order where tests/smc_reference.py restates them.
#include "gpb_internal.h"
#include "philox.h"
#include <math.h>

namespace gpb {
namespace {

constexpr uint32_t SMC_TAG_RESAMPLE = 8u, SMC_TAG_NORMAL = 9u, SMC_TAG_ACCEPT = 10u;
constexpr int64_t SMC_MAX_N = 1 << 20;  // particles
constexpr int SMC_MAX_D = 128;          // parameters: Lc [d, d] and four rows of normals in LDS, 8 d^2 + 32 d <= 160 KiB
constexpr int SMC_RW_T = 1024;          // threads of the reweight workgroup
constexpr int SMC_RW_LDS = 16384;       // log-likelihoods kept in LDS across the halvings (128 KiB; the rest stay in L2)
constexpr int SMC_BISECT = 60;          // halvings of [beta_prev, 1]
constexpr double SMC_TARGET_ACC = 0.234;
// the state block [GPB_SMC_STATE_WORDS] of 8-byte words: doubles, then 64-bit counters
enum { SB_BETA = 0, SB_LOGZ, SB_LOG_SIGMA, SB_ESS, SB_DLOGZ, SB_STEP_ACC = 8, SB_TICKET, SB_NACCEPT, SB_NAN_MOVE, SB_NAN_WEIGHT,
       SB_FLAG };

__device__ __forceinline__ double smc_resample_u(uint64_t seed, uint32_t stage) {
    const U4 r = philox(seed, stage, 0u, 0u, SMC_TAG_RESAMPLE);
    return u01(r.x, r.y);
}

__device__ __forceinline__ double smc_accept_logu(uint64_t seed, uint32_t i, uint32_t k) {
    const U4 r = philox(seed, i, k, 0u, SMC_TAG_ACCEPT);
    return log(u01(r.x, r.y));
}

// sums of a and b over the 1024 threads in a fixed order (lanes by the shuffle tree, then the 16 waves in index order);
// every thread returns with the same totals
__device__ __forceinline__ void rw_sum2(double& a, double& b, double* sh /*[32]*/) {
#pragma clang fp contract(off)
    for (int o = 32; o > 0; o >>= 1) {
        a = a + __shfl_down(a, o);
        b = b + __shfl_down(b, o);
    }
    const int w = threadIdx.x >> 6;
    __syncthreads();                                           // the previous use of sh is over
    if ((threadIdx.x & 63) == 0) {
        sh[w] = a;
        sh[16 + w] = b;
    }
    __syncthreads();
    a = 0.0;
    b = 0.0;
    for (int i = 0; i < SMC_RW_T / 64; ++i) {
        a = a + sh[i];
        b = b + sh[16 + i];
    }
}

// sum of w = exp(db (logl - max)) and of w^2 over the particles (NaN: weight 0); dls holds logl - max of the first 16384
__device__ __forceinline__ void rw_ess_sums(const double* dls, const double* __restrict__ logl, int64_t N, double mx, double db,
                                            double* sh, double& s1, double& s2) {
#pragma clang fp contract(off)
    s1 = 0.0;
    s2 = 0.0;
    for (int64_t i = threadIdx.x; i < N; i += SMC_RW_T) {
        const double l = i < SMC_RW_LDS ? dls[i] : logl[i] - mx;
        const double w = l == l ? exp(db * l) : 0.0;
        s1 = s1 + w;
        s2 = s2 + w * w;
    }
    rw_sum2(s1, s2, sh);
}

// one workgroup.  wgt [N]: the unnormalised weights; cum [N]: their inclusive scan divided by its last entry
__global__ __launch_bounds__(SMC_RW_T) void k_smc_reweight(const double* __restrict__ logl, int64_t N, double ess_fraction,
                                                           double* __restrict__ state, double* __restrict__ wgt,
                                                           double* __restrict__ cum) {
#pragma clang fp contract(off)
    __shared__ double dls[SMC_RW_LDS];
    __shared__ double sh[32];
    __shared__ double cbase[SMC_RW_T];
    const int t = threadIdx.x;
    double mx = -INFINITY, nnan = 0.0;
    for (int64_t i = t; i < N; i += SMC_RW_T) {
        const double l = logl[i];
        if (i < SMC_RW_LDS) dls[i] = l;
        if (l != l) nnan = nnan + 1.0;
        if (l > mx) mx = l;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double y = __shfl_down(mx, o);
        if (y > mx) mx = y;
    }
    if ((t & 63) == 0) sh[t >> 6] = mx;
    __syncthreads();
    mx = sh[0];
    for (int i = 1; i < SMC_RW_T / 64; ++i)
        if (sh[i] > mx) mx = sh[i];
    double zero = 0.0;
    rw_sum2(nnan, zero, sh);
    for (int64_t i = t; i < imin64(N, SMC_RW_LDS); i += SMC_RW_T) dls[i] = dls[i] - mx;       // (a thread's own entries)
    const double beta_prev = state[SB_BETA];
    const double target = ess_fraction * (double)N;
    double s1, s2;
    rw_ess_sums(dls, logl, N, mx, 1.0 - beta_prev, sh, s1, s2);
    double beta = 1.0;
    if (!((s1 * s1) / s2 >= target)) {
        double lo = beta_prev, hi = 1.0;
        for (int it = 0; it < SMC_BISECT; ++it) {
            const double mid = 0.5 * (lo + hi);
            rw_ess_sums(dls, logl, N, mx, mid - beta_prev, sh, s1, s2);
            if ((s1 * s1) / s2 > target) lo = mid;
            else hi = mid;
        }
        beta = hi;
        rw_ess_sums(dls, logl, N, mx, beta - beta_prev, sh, s1, s2);
    }
    const double db = beta - beta_prev;
    for (int64_t i = t; i < N; i += SMC_RW_T) {
        const double l = i < SMC_RW_LDS ? dls[i] : logl[i] - mx;
        wgt[i] = l == l ? exp(db * l) : 0.0;
    }
    __syncthreads();
    // the scan, monotone by construction: a contiguous chunk per thread; the chunks' bases are one sequential scan of the
    // chunk totals, so that a chunk ends exactly where the next begins (cum never steps back over a run of zero weights)
    const int64_t C = (N + SMC_RW_T - 1) / SMC_RW_T;
    const int64_t i0 = imin64((int64_t)t * C, N), i1 = imin64(i0 + C, N);
    double part = 0.0;
    for (int64_t i = i0; i < i1; ++i) part = part + wgt[i];
    cbase[t] = part;
    __syncthreads();
    if (t == 0) {
        double r = 0.0;
        for (int i = 0; i < SMC_RW_T; ++i) {
            const double p = cbase[i];
            cbase[i] = r;
            r = r + p;
        }
        sh[0] = r;
    }
    __syncthreads();
    const double total = sh[0], base = cbase[t];
    double local = 0.0;
    for (int64_t i = i0; i < i1; ++i) {
        local = local + wgt[i];
        cum[i] = (base + local) / total;
    }
    if (t == 0) {
        const double dlogz = (db * mx + log(s1)) - log((double)N);
        state[SB_BETA] = beta;
        state[SB_LOGZ] = state[SB_LOGZ] + dlogz;
        state[SB_ESS] = (s1 * s1) / s2;
        state[SB_DLOGZ] = dlogz;
        unsigned long long* cnt = reinterpret_cast<unsigned long long*>(state);
        cnt[SB_NAN_WEIGHT] = (unsigned long long)nnan;
        if (!(total > 0.0)) cnt[SB_FLAG] |= 2ull;              // no particle with a finite log-likelihood
    }
}

// 256 positions per workgroup: the ancestor of each, then the rows gathered with coalesced copies
__global__ __launch_bounds__(256) void k_smc_resample(const double* __restrict__ cum, const double* __restrict__ x,
                                                      const double* __restrict__ logl, int64_t N, int d, uint64_t seed,
                                                      uint32_t stage, double* __restrict__ xo, double* __restrict__ loglo,
                                                      long long* __restrict__ anc_out) {
#pragma clang fp contract(off)
    __shared__ int anc[256];
    const int t = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * 256, i = base + t;
    if (i < N) {
        double pos = (smc_resample_u(seed, stage) + (double)i) / (double)N;
        if (pos > 0.99999999999999989) pos = 0.99999999999999989;       // 1 - 2^-53: cum[N - 1] = 1 exceeds every position
        int64_t lo = 0, hi = N - 1;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (cum[mid] > pos) hi = mid;
            else lo = mid + 1;
        }
        anc[t] = (int)lo;
        loglo[i] = logl[lo];
        if (anc_out) anc_out[i] = lo;
    }
    __syncthreads();
    const int64_t rows = imin64(256, N - base);
    for (int64_t e = t; e < rows * d; e += 256) {
        const int64_t p = e / d, j = e - p * d;
        xo[(base + p) * d + j] = x[(int64_t)anc[p] * d + j];
    }
}

// sum over the N rows of column a (shifted by the first row's entry), in a fixed order; every thread gets the total
__device__ __forceinline__ double mom_colsum(const double* __restrict__ x, int64_t N, int d, int a, double* sh) {
#pragma clang fp contract(off)
    const double x0 = x[a];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < N; i += 256) s = s + (x[i * d + a] - x0);
    for (int o = 32; o > 0; o >>= 1) s = s + __shfl_down(s, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// mean_a = x_0a + sum_i (x_ia - x_0a) / N, workgroup a (the shift makes the mean of equal rows exact, so that a degenerate
// ensemble has a covariance of exactly zero)
__global__ __launch_bounds__(256) void k_smc_mean(const double* __restrict__ x, int64_t N, int d, double* __restrict__ mean) {
#pragma clang fp contract(off)
    __shared__ double sh[4];
    const int a = blockIdx.x;
    const double ma = x[a] + mom_colsum(x, N, d, a, sh) / (double)N;
    if (threadIdx.x == 0) mean[a] = ma;
}

// workgroup e of the d (d + 1) / 2 entries (a, b), b <= a, of the lower triangle, row by row:
// cov[a, b] = cov[b, a] = sum_i (x_ia - mean_a)(x_ib - mean_b) / N.  The columns are read at stride d: a reweighting costs
// d^2 N / 2 strided loads: little at the sizes the sampler is run at (d ~ 15, N ~ 4096), but it grows with d^2 N up to
// the limits
__global__ __launch_bounds__(256) void k_smc_moments(const double* __restrict__ x, int64_t N, int d,
                                                     const double* __restrict__ mean, double* __restrict__ cov) {
#pragma clang fp contract(off)
    __shared__ double sh[4];
    int a = 0;
    while ((a + 1) * (a + 2) / 2 <= (int)blockIdx.x) ++a;
    const int b = (int)blockIdx.x - a * (a + 1) / 2;
    const double ma = mean[a], mb = mean[b];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < N; i += 256) s = s + (x[i * d + a] - ma) * (x[i * d + b] - mb);
    for (int o = 32; o > 0; o >>= 1) s = s + __shfl_down(s, o);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double c = (((sh[0] + sh[1]) + sh[2]) + sh[3]) / (double)N;
        cov[(int64_t)a * d + b] = c;
        cov[(int64_t)b * d + a] = c;
    }
}

// one workgroup, the matrix in LDS (d * d doubles of dynamic LDS): right-looking Cholesky, Lc lower with zeros above
__global__ __launch_bounds__(256) void k_smc_chol(const double* __restrict__ cov, int d, double* __restrict__ Lc,
                                                  double* __restrict__ state) {
#pragma clang fp contract(off)
    extern __shared__ double A[];
    __shared__ int bad;
    const int t = threadIdx.x;
    if (t == 0) bad = 0;
    for (int e = t; e < d * d; e += 256) A[e] = cov[e];
    __syncthreads();
    for (int k = 0; k < d; ++k) {
        const double piv = A[k * d + k];
        __syncthreads();
        if (!(piv > 0.0)) {                                    // non-positive (or NaN): flagged; the host raises at the stage boundary
            if (t == 0) bad = 1;
        }
        const double r = sqrt(piv);
        if (t == 0) A[k * d + k] = r;
        for (int i = k + 1 + t; i < d; i += 256) A[i * d + k] = A[i * d + k] / r;
        __syncthreads();
        const int m = d - k - 1;
        for (int e = t; e < m * m; e += 256) {
            const int i = k + 1 + e / m, j = k + 1 + e % m;
            if (j <= i) A[i * d + j] = A[i * d + j] - A[i * d + k] * A[j * d + k];
        }
        __syncthreads();
    }
    for (int e = t; e < d * d; e += 256) Lc[e] = (e % d) <= (e / d) ? A[e] : 0.0;
    if (t == 0 && bad) reinterpret_cast<unsigned long long*>(state)[SB_FLAG] |= 1ull;
}

// four waves per workgroup, one wave per particle at a time; Lc transposed in LDS so that the lanes read neighbours
__global__ __launch_bounds__(256) void k_smc_propose(const double* __restrict__ x, const double* __restrict__ Lc,
                                                    const double* __restrict__ state, int64_t N, int d, uint64_t seed,
                                                    uint32_t k, double* __restrict__ xp) {
#pragma clang fp contract(off)
    extern __shared__ double sm[];
    double* LT = sm;                                           // LT[j * d + i] = Lc[i, j]
    const int t = threadIdx.x, w = t >> 6, lane = t & 63;
    double* z = sm + (int64_t)d * d + w * d;
    for (int e = t; e < d * d; e += 256) LT[(e % d) * d + e / d] = Lc[e];
    const double step = exp(state[SB_LOG_SIGMA]);
    for (int64_t base = (int64_t)blockIdx.x * 4; base < N; base += (int64_t)gridDim.x * 4) {
        const int64_t p = base + w;
        __syncthreads();                                       // LT is loaded; the last particle's z has been read
        if (p < N)
            for (int j = lane; 2 * j < d; j += 64) {
                double n0, n1;
                normal_pair(seed, (uint32_t)p, k, (uint32_t)j, SMC_TAG_NORMAL, n0, n1);
                z[2 * j] = n0;
                if (2 * j + 1 < d) z[2 * j + 1] = n1;
            }
        __syncthreads();
        if (p < N)
            for (int i = lane; i < d; i += 64) {
                double s = 0.0;
                for (int j = 0; j <= i; ++j) s = s + LT[j * d + i] * z[j];
                xp[p * d + i] = x[p * d + i] + step * s;
            }
    }
}

// 256 particles per workgroup: the decisions, the accepted rows copied, the counters; the last workgroup to finish adapts
// log_sigma from the step's count and re-arms the two scratch counters
__global__ __launch_bounds__(256) void k_smc_accept(double* __restrict__ x, double* __restrict__ logl,
                                                   const double* __restrict__ xp, const double* __restrict__ lp,
                                                   double* __restrict__ state, int64_t N, int d, uint64_t seed, uint32_t k,
                                                   double outside, double sdiv /* s + 1 */) {
#pragma clang fp contract(off)
    __shared__ int take[256];
    __shared__ int nacc, nnan;
    const int t = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * 256, i = base + t;
    if (t == 0) { nacc = 0; nnan = 0; }
    __syncthreads();
    int tk = 0;
    if (i < N) {
        const double l1 = lp[i], l0 = logl[i];
        const bool isnan_ = l1 != l1;
        // outside the box (lp = outside_value) and NaN: rejected whatever beta is
        tk = !isnan_ && l1 > outside && smc_accept_logu(seed, (uint32_t)i, k) < state[SB_BETA] * (l1 - l0);
        if (tk) {
            logl[i] = l1;
            atomicAdd(&nacc, 1);
        }
        if (isnan_) atomicAdd(&nnan, 1);
    }
    take[t] = tk;
    __syncthreads();
    const int64_t rows = imin64(256, N - base);
    for (int64_t e = t; e < rows * d; e += 256) {
        const int64_t p = e / d;
        if (take[p]) x[base * d + e] = xp[base * d + e];
    }
    if (t == 0) {
        unsigned long long* cnt = reinterpret_cast<unsigned long long*>(state);
        if (nacc) {
            atomicAdd(&cnt[SB_STEP_ACC], (unsigned long long)nacc);
            atomicAdd(&cnt[SB_NACCEPT], (unsigned long long)nacc);
        }
        if (nnan) atomicAdd(&cnt[SB_NAN_MOVE], (unsigned long long)nnan);
        __threadfence();
        if (atomicAdd(&cnt[SB_TICKET], 1ull) == (unsigned long long)gridDim.x - 1ull) {
            __threadfence();
            const unsigned long long acc = atomicExch(&cnt[SB_STEP_ACC], 0ull);
            atomicExch(&cnt[SB_TICKET], 0ull);
            state[SB_LOG_SIGMA] = state[SB_LOG_SIGMA] + ((double)acc / (double)N - SMC_TARGET_ACC) / sdiv;
        }
    }
}

#ifdef GPB_DEBUG_VARIANTS
__global__ void k_smc_draws(int64_t N, int d, uint64_t seed, uint32_t stage, uint32_t k, double* __restrict__ normals,
                            double* __restrict__ lu_acc, double* __restrict__ u_res) {
    const int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const int64_t np = (d + 1) / 2;
    if (g < N * np) {
        const int64_t c = g / np, j = g - c * np;
        double n0, n1;
        normal_pair(seed, (uint32_t)c, k, (uint32_t)j, SMC_TAG_NORMAL, n0, n1);
        normals[c * d + 2 * j] = n0;
        if (2 * j + 1 < d) normals[c * d + 2 * j + 1] = n1;
    }
    if (g < N) lu_acc[g] = smc_accept_logu(seed, (uint32_t)g, k);
    if (g == 0) u_res[0] = smc_resample_u(seed, stage);
}
#endif

// the argument checks both entry points share (need_like: the move evaluates the chain, the reweighting only its contexts' sizes)
int smc_check(gpb_ctx* const* ctxs, int E, int64_t N, const char* who, bool need_like, int64_t& nd) {
    gpb_ctx* ctx = ctxs[0];
    if (N < 2 || N > SMC_MAX_N) GPB_FAIL(GPB_E_ARG, std::string(who) + ": 2 .. 1048576 particles");
    if (int rc = chain_ctx_check(ctxs, E, who, need_like)) return rc;
    nd = sampler_ndim(ctx);
    if (nd < 1 || nd > SMC_MAX_D) GPB_FAIL(GPB_E_ARG, std::string(who) + ": 1 .. 128 parameters");
    return 0;
}

// workspace of the chain's first context (SmcWs, ws_layout.h)
int smc_workspace(gpb_ctx* ctx, int64_t N, int64_t nd, SmcWs& ws) {
    return ctx_carve(ctx, ctx->smc_ws, [&](Carver<double>& c) { ws.lay(c, N, nd); });
}
}  // namespace
}  // namespace gpb

using namespace gpb;

extern "C" int gpb_chain_smc_reweight(gpb_ctx* const* ctxs, int E, int64_t N, uint64_t stage, uint64_t seed,
                                      double ess_fraction, double* x_dev, double* logl_dev, double* state_dev, double* Lc_dev,
                                      int64_t* ancestors_dev, double* mean_dev) {
    if (!chain_args_ok(ctxs, E)) return GPB_E_ARG;
    gpb_ctx* ctx = ctxs[0];
    if (!x_dev || !logl_dev || !state_dev || !Lc_dev) GPB_FAIL(GPB_E_ARG, "gpb_chain_smc_reweight: null pointer");
    if (!(ess_fraction > 0.0 && ess_fraction < 1.0)) GPB_FAIL(GPB_E_ARG, "gpb_chain_smc_reweight: 0 < ess_fraction < 1");
    if (stage > 0xFFFFFFFFull) GPB_FAIL(GPB_E_ARG, "gpb_chain_smc_reweight: stages are numbered below 2^32");
    int64_t nd;
    int rc;
    if ((rc = smc_check(ctxs, E, N, "gpb_chain_smc_reweight", false, nd))) return rc;
    GPB_HIP(hipSetDevice(ctx->device));
    SmcWs ws;
    if ((rc = smc_workspace(ctx, N, nd, ws))) return rc;
    double *wgt = ws.wgt, *cum = ws.cum, *lg = ws.lp, *xg = ws.xp, *cov = ws.cov, *mean = ws.mean;
    const int d = (int)nd;
    hipLaunchKernelGGL(k_smc_reweight, dim3(1), dim3(SMC_RW_T), 0, ctx->stream, logl_dev, N, ess_fraction, state_dev, wgt, cum);
    hipLaunchKernelGGL(k_smc_resample, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, ctx->stream, cum, x_dev, logl_dev, N, d,
                       seed, (uint32_t)stage, xg, lg, reinterpret_cast<long long*>(ancestors_dev));
    GPB_HIP(hipMemcpyAsync(x_dev, xg, sizeof(double) * (size_t)(N * nd), hipMemcpyDeviceToDevice, ctx->stream));
    GPB_HIP(hipMemcpyAsync(logl_dev, lg, sizeof(double) * (size_t)N, hipMemcpyDeviceToDevice, ctx->stream));
    hipLaunchKernelGGL(k_smc_mean, dim3(d), dim3(256), 0, ctx->stream, x_dev, N, d, mean);
    hipLaunchKernelGGL(k_smc_moments, dim3((unsigned)(d * (d + 1) / 2)), dim3(256), 0, ctx->stream, x_dev, N, d, mean, cov);
    const size_t lds = sizeof(double) * (size_t)(nd * nd);
    if (lds > 65536)
        GPB_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_smc_chol), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_smc_chol, dim3(1), dim3(256), lds, ctx->stream, cov, d, Lc_dev, state_dev);
    if (mean_dev) GPB_HIP(hipMemcpyAsync(mean_dev, mean, sizeof(double) * (size_t)nd, hipMemcpyDeviceToDevice, ctx->stream));
    GPB_HIP(hipGetLastError());
    return 0;
}

extern "C" int gpb_chain_smc_move(gpb_ctx* const* ctxs, int E, int64_t N, int64_t nsteps, uint64_t step0, uint64_t stage_step0,
                                  uint64_t seed, double* x_dev, double* logl_dev, double* state_dev, const double* Lc_dev,
                                  const double* lo_dev, const double* hi_dev, double outside_value, double inside_const) {
    if (!chain_args_ok(ctxs, E)) return GPB_E_ARG;
    gpb_ctx* ctx = ctxs[0];
    if (!x_dev || !logl_dev || !state_dev || !Lc_dev || !lo_dev || !hi_dev || nsteps < 0)
        GPB_FAIL(GPB_E_ARG, "gpb_chain_smc_move: null pointer or negative size");
    if (step0 + (uint64_t)nsteps > 0xFFFFFFFFull || stage_step0 + (uint64_t)nsteps > 0xFFFFFFFFull)
        GPB_FAIL(GPB_E_ARG, "gpb_chain_smc_move: steps are numbered below 2^32");
    int64_t nd;
    int rc;
    if ((rc = smc_check(ctxs, E, N, "gpb_chain_smc_move", true, nd))) return rc;      // (all the state checks chain_eval has)
    if (nsteps == 0) return 0;
    GPB_HIP(hipSetDevice(ctx->device));
    SmcWs ws;
    if ((rc = smc_workspace(ctx, N, nd, ws))) return rc;
    double *lp = ws.lp, *xp = ws.xp;
    const int d = (int)nd;
    const size_t lds = sizeof(double) * (size_t)(nd * nd + 4 * nd);
    if (lds > 65536)
        GPB_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_smc_propose), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int64_t quads = (N + 3) / 4;
    const unsigned gp = (unsigned)imin64(quads, 2 * (int64_t)ctx->num_cu), ga = (unsigned)((N + 255) / 256);
    for (int64_t n = 0; n < nsteps; ++n) {
        const uint32_t k = (uint32_t)(step0 + (uint64_t)n);
        hipLaunchKernelGGL(k_smc_propose, dim3(gp), dim3(256), lds, ctx->stream, x_dev, Lc_dev, state_dev, N, d, seed, k, xp);
        if ((rc = chain_eval(ctxs, E, xp, N, lp, lo_dev, hi_dev, outside_value, inside_const))) return rc;
        hipLaunchKernelGGL(k_smc_accept, dim3(ga), dim3(256), 0, ctx->stream, x_dev, logl_dev, xp, lp, state_dev, N, d, seed, k,
                           outside_value, (double)(stage_step0 + (uint64_t)n + 1));
    }
    GPB_HIP(hipGetLastError());
    return 0;
}

#ifdef GPB_DEBUG_VARIANTS      // test hook (include/gpbayes_debug.h)
extern "C" int gpb_test_smc_draws(gpb_ctx* ctx, int64_t N, int64_t d, uint64_t seed, uint64_t stage, uint64_t step,
                                  double* normals_dev, double* logu_accept_dev, double* u_resample_dev) {
    if (!ctx || N < 2 || N > SMC_MAX_N || d < 1 || d > SMC_MAX_D || !normals_dev || !logu_accept_dev || !u_resample_dev)
        return GPB_E_ARG;
    GPB_HIP(hipSetDevice(ctx->device));
    const int64_t n = N * ((d + 1) / 2);
    hipLaunchKernelGGL(k_smc_draws, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, N, (int)d, seed,
                       (uint32_t)stage, (uint32_t)step, normals_dev, logu_accept_dev, u_resample_dev);
    GPB_HIP(hipGetLastError());
    return 0;
}
#endif  // GPB_DEBUG_VARIANTS
