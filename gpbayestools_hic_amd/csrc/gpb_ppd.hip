// gpb_ppd.hip — posterior-predictive summaries of a whole chain (gpb_ppd_summary): reductions over the sample axis of the
// observable-major arrays gpb_emu_predict_diag writes, mu_T / var_T [M][ld] with the S samples of an observable contiguous.
// What the reference does with fifteen samples on the host (examples/ClosureTest.ipynb, PlotMCMC.ipynb over Chain._predict,
// src/mcmc.py:153-166, src/emulator.py:553-605) for all S of them, per observable m:
//   k_ppd_moments   E_s mu, E_s sigma^2 (the emulator part) and E_s (mu - E mu)^2 (the parameter part, two passes): by the law of
//                   total variance the last two sum to the predictive variance
//   k_ppd_order     the order statistics mu_(k), mu_(min(k + 1, S - 1)), k = floor(q (S - 1)) — the two neighbours numpy's default
//                   percentile interpolates between — by a most-significant-digit radix select on the order-preserving 64-bit key:
//                   eight passes of 8 bits, counted with integer LDS atomics, all 2 nq ranks in the same passes; nothing is sorted
//   k_ppd_mix       quantiles of the predictive mixture F(y) = 1/S sum_s Phi((y - mu_s) / tau_s), tau_s^2 = max(sigma_s^2 + vadd, 0),
//                   by exactly 64 halvings of [min_s(mu_s - 9 tau_s), max_s(mu_s + 9 tau_s)] (F(mid) < q moves the lower end, the
//                   result is the upper end), all levels advancing together: one pass over the row per halving; and the PIT
//                   F(yobs).  A sample with tau_s = 0 contributes the step y >= mu_s.
// One workgroup per row and kernel.  Every sum is a per-thread compensated sum over the thread's strided samples followed by a
// fixed tree (wave butterfly, then the waves in order): its shape depends on S alone, so a row's bits depend on nothing but the
// row — not on M, the other rows, ld, or the outputs that share the call.  No floating-point atomics.
#include "gpb_internal.h"
#include "block_reduce.h"
#include "order_key.h"
#include <math.h>

namespace gpb {

namespace {

constexpr int PPD_THREADS = REDUCE_THREADS;      // Kahan, wave_sum, block_sum: block_reduce.h
constexpr int PPD_WAVES = REDUCE_WAVES;
constexpr int PPD_RANKS = 2 * PPD_MAX_Q;

// ---------------------------------------------------------------------------------------------------------------- moments
__global__ __launch_bounds__(PPD_THREADS) void k_ppd_moments(const double* __restrict__ mu_T, const double* __restrict__ var_T,
                                                             int64_t S, int64_t ld, double* __restrict__ moments) {
    __shared__ double sw[PPD_WAVES];
    const int tid = threadIdx.x;
    const int64_t m = blockIdx.x;
    const double* mu = mu_T + m * ld;
    const double* var = var_T ? var_T + m * ld : nullptr;
    Kahan a, b;
    for (int64_t s = tid; s < S; s += PPD_THREADS) {
        a.add(mu[s]);
        if (var) b.add(var[s]);
    }
    const double mean = block_sum(a.s, sw) / (double)S;
    const double ev = block_sum(b.s, sw) / (double)S;
    Kahan c;
    for (int64_t s = tid; s < S; s += PPD_THREADS) {
        const double d = mu[s] - mean;
        c.add(__dmul_rn(d, d));
    }
    const double pv = block_sum(c.s, sw) / (double)S;
    if (tid == 0) {
        moments[m * 3 + 0] = mean;
        moments[m * 3 + 1] = ev;
        moments[m * 3 + 2] = pv;
    }
}

// ---------------------------------------------------------------------------------------------------------------- order statistics
// (ppd_key / ppd_unkey, the unsigned keys in the order of the doubles: order_key.h)
// Rank r keeps the digits found so far (prefix[r], the undecided bits zero) and its rank among the keys that share them (rem[r]).
// Ranks with equal prefixes form a group and share one 256-bin histogram: a pass costs one LDS atomic per key and GROUP that the
// key belongs to (one group in the first pass, at most 2 nq in the last).
__global__ __launch_bounds__(PPD_THREADS) void k_ppd_order(const double* __restrict__ mu_T, int64_t S, int64_t ld, PpdLevels lv,
                                                           double* __restrict__ order) {
    __shared__ unsigned hist[PPD_RANKS][256];
    __shared__ unsigned long long prefix[PPD_RANKS], gprefix[PPD_RANKS];
    __shared__ long long rem[PPD_RANKS];
    __shared__ int grp[PPD_RANKS];
    __shared__ int ngrp;
    const int tid = threadIdx.x;
    const int64_t m = blockIdx.x;
    const double* mu = mu_T + m * ld;
    const int nr = 2 * lv.nq;
    if (tid == 0) {
#pragma unroll
        for (int r = 0; r < PPD_RANKS; ++r) {       // (constant indices: the by-value argument stays in the kernel-argument segment)
            rem[r] = lv.k[r];
            prefix[r] = 0ull;
        }
    }
    for (int pass = 0; pass < 8; ++pass) {
        const int shift = 56 - 8 * pass;
        const unsigned long long mask = pass == 0 ? 0ull : ~0ull << (shift + 8);
        __syncthreads();
        if (tid == 0) {
            int ng = 0;
            for (int r = 0; r < nr; ++r) {
                int g = 0;
                while (g < ng && gprefix[g] != prefix[r]) ++g;
                if (g == ng) gprefix[ng++] = prefix[r];
                grp[r] = g;
            }
            ngrp = ng;
        }
        __syncthreads();
        const int ng = ngrp;
        for (int e = tid; e < ng * 256; e += PPD_THREADS) (&hist[0][0])[e] = 0u;
        __syncthreads();
        for (int64_t s = tid; s < S; s += PPD_THREADS) {
            const unsigned long long key = ppd_key(mu[s]);
            const unsigned long long kp = key & mask;
            const int bin = (int)((key >> shift) & 255ull);
            for (int g = 0; g < ng; ++g)
                if (kp == gprefix[g]) atomicAdd(&hist[g][bin], 1u);
        }
        __syncthreads();
        if (tid < nr) {
            const int g = grp[tid];
            const long long want = rem[tid];
            long long cum = 0;
            int b = 0;
            for (; b < 255; ++b) {
                const long long c = (long long)hist[g][b];
                if (want < cum + c) break;
                cum += c;
            }
            prefix[tid] |= (unsigned long long)b << shift;
            rem[tid] = want - cum;
        }
    }
    __syncthreads();
    if (tid < nr) order[m * nr + tid] = ppd_unkey(prefix[tid]);
}

// ---------------------------------------------------------------------------------------------------------------- mixture quantiles, PIT
struct MixLds {
    double q[PPD_MAX_Q], a[PPD_MAX_Q], b[PPD_MAX_Q], mid[PPD_MAX_Q], F[PPD_MAX_Q];
    double sw[PPD_MAX_Q][PPD_WAVES];
    double mm[2][PPD_WAVES];
    int live[PPD_MAX_Q];
};

// F at s.mid[i] for the live levels i < nlev -> s.F[i]; acc / cmp [nlev][PPD_THREADS]: each thread's compensated partial sums
__device__ __forceinline__ void mix_eval(MixLds& s, int nlev, const double* __restrict__ mu, const double* __restrict__ var,
                                         double va, int64_t S, double* acc, double* cmp) {
    const int tid = threadIdx.x;
    for (int i = 0; i < nlev; ++i) {
        acc[i * PPD_THREADS + tid] = 0.0;
        cmp[i * PPD_THREADS + tid] = 0.0;
    }
    for (int64_t k = tid; k < S; k += PPD_THREADS) {
        const double m = mu[k];
        const double tau = sqrt(fmax((var ? var[k] : 0.0) + va, 0.0));
        const double r = 1.0 / (tau * 1.4142135623730951);
        for (int i = 0; i < nlev; ++i) {
            if (!s.live[i]) continue;
            const double y = s.mid[i];
            const double term = tau > 0.0 ? 0.5 * erfc((m - y) * r) : (y >= m ? 1.0 : 0.0);
            const double c0 = cmp[i * PPD_THREADS + tid], a0 = acc[i * PPD_THREADS + tid];
            const double yk = term - c0, t = a0 + yk;
            cmp[i * PPD_THREADS + tid] = (t - a0) - yk;
            acc[i * PPD_THREADS + tid] = t;
        }
    }
    for (int i = 0; i < nlev; ++i) {
        if (!s.live[i]) continue;
        const double v = wave_sum(acc[i * PPD_THREADS + tid]);
        if ((tid & 63) == 0) s.sw[i][tid >> 6] = v;
    }
    __syncthreads();
    if (tid < nlev && s.live[tid]) s.F[tid] = ((s.sw[tid][0] + s.sw[tid][1]) + (s.sw[tid][2] + s.sw[tid][3])) / (double)S;
    __syncthreads();
}

__global__ __launch_bounds__(PPD_THREADS) void k_ppd_mix(const double* __restrict__ mu_T, const double* __restrict__ var_T, int64_t S,
                                                         int64_t ld, PpdLevels lv, const double* __restrict__ vadd,
                                                         const double* __restrict__ yobs, double* __restrict__ mixq,
                                                         double* __restrict__ pit) {
    extern __shared__ __attribute__((aligned(16))) double dyn[];      // acc | cmp, [max(nq, 1)][PPD_THREADS] each
    __shared__ MixLds s;
    const int tid = threadIdx.x;
    const int64_t m = blockIdx.x;
    const double* mu = mu_T + m * ld;
    const double* var = var_T ? var_T + m * ld : nullptr;
    const double va = vadd ? vadd[m] : 0.0;
    const int nq = lv.nq;
    double* acc = dyn;
    double* cmp = dyn + (size_t)nq * PPD_THREADS;
    if (tid == 0) {
#pragma unroll
        for (int i = 0; i < PPD_MAX_Q; ++i) s.q[i] = lv.q[i];
    }
    if (mixq) {
        // the bracket: exact minimum / maximum, whatever the order
        double lo = INFINITY, hi = -INFINITY;
        for (int64_t k = tid; k < S; k += PPD_THREADS) {
            const double tau = sqrt(fmax((var ? var[k] : 0.0) + va, 0.0));
            lo = fmin(lo, fma(-9.0, tau, mu[k]));
            hi = fmax(hi, fma(9.0, tau, mu[k]));
        }
        for (int o = 32; o >= 1; o >>= 1) {
            lo = fmin(lo, __shfl_xor(lo, o, 64));
            hi = fmax(hi, __shfl_xor(hi, o, 64));
        }
        if ((tid & 63) == 0) {
            s.mm[0][tid >> 6] = lo;
            s.mm[1][tid >> 6] = hi;
        }
        __syncthreads();
        if (tid < nq) {
            s.a[tid] = fmin(fmin(s.mm[0][0], s.mm[0][1]), fmin(s.mm[0][2], s.mm[0][3]));
            s.b[tid] = fmax(fmax(s.mm[1][0], s.mm[1][1]), fmax(s.mm[1][2], s.mm[1][3]));
            s.live[tid] = s.q[tid] > 0.0 && s.q[tid] < 1.0;
        }
        for (int h = 0; h < 64; ++h) {
            __syncthreads();
            if (tid < nq && s.live[tid]) {
                const double a = s.a[tid], b = s.b[tid], mid = 0.5 * (a + b);
                if (a < mid && mid < b) s.mid[tid] = mid;
                else s.live[tid] = 0;                  // the bracket's ends are neighbours: nothing left to halve
            }
            __syncthreads();
            int any = 0;
            for (int i = 0; i < nq; ++i) any |= s.live[i];
            if (!any) break;                           // (s.live is the same for every thread: a uniform exit)
            mix_eval(s, nq, mu, var, va, S, acc, cmp);
            if (tid < nq && s.live[tid]) {
                if (s.F[tid] < s.q[tid]) s.a[tid] = s.mid[tid];
                else s.b[tid] = s.mid[tid];
            }
        }
        __syncthreads();
        if (tid < nq) {
            const double q = s.q[tid];
            mixq[m * nq + tid] = q <= 0.0 ? -INFINITY : (q >= 1.0 ? INFINITY : s.b[tid]);
        }
    }
    if (pit) {
        __syncthreads();
        if (tid == 0) {
            s.mid[0] = yobs[m];
            s.live[0] = 1;
        }
        __syncthreads();
        mix_eval(s, 1, mu, var, va, S, acc, cmp);
        if (tid == 0) pit[m] = s.F[0];
    }
}

}  // namespace

int launch_ppd(gpb_ctx* ctx, const double* mu_T, const double* var_T, int64_t M, int64_t S, int64_t ld, const PpdLevels& lv,
               const double* vadd, const double* yobs, double* moments, double* order, double* mixq, double* pit) {
    const dim3 grid((unsigned)M), block(PPD_THREADS);
    if (moments) hipLaunchKernelGGL(k_ppd_moments, grid, block, 0, ctx->stream, mu_T, var_T, S, ld, moments);
    if (order) hipLaunchKernelGGL(k_ppd_order, grid, block, 0, ctx->stream, mu_T, S, ld, lv, order);
    if (mixq || pit) {
        const size_t lds = sizeof(double) * 2 * (size_t)lv.nq * PPD_THREADS;
        GPB_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_ppd_mix), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k_ppd_mix, grid, block, lds, ctx->stream, mu_T, var_T, S, ld, lv, vadd, yobs, mixq, pit);
    }
    GPB_HIP(hipGetLastError());
    return 0;
}

}  // namespace gpb

using namespace gpb;

extern "C" int gpb_ppd_summary(gpb_ctx* ctx, const double* mu_T, const double* var_T, int64_t M, int64_t S, int64_t ld,
                               const double* q_host, int nq, const double* vadd_dev, const double* yobs_dev, int on_device,
                               double* moments, double* order, double* mixq, double* pit) {
    if (!ctx || !mu_T || !q_host) return GPB_E_ARG;
    if (M < 1 || S < 1) GPB_FAIL(GPB_E_ARG, "gpb_ppd_summary: need M >= 1 and S >= 1");
    if (M > 0x7fffffffLL || S > 0x7fffffffLL) GPB_FAIL(GPB_E_ARG, "gpb_ppd_summary: more than 2^31 - 1 rows or samples");
    if (ld < S) GPB_FAIL(GPB_E_ARG, "gpb_ppd_summary: ld < S");
    if (nq < 1 || nq > PPD_MAX_Q) GPB_FAIL(GPB_E_ARG, "gpb_ppd_summary: need 1 <= nq <= 16 levels");
    PpdLevels lv;
    for (int i = 0; i < PPD_MAX_Q; ++i) {
        lv.q[i] = 0.0;
        lv.k[2 * i] = lv.k[2 * i + 1] = 0;
    }
    lv.nq = nq;
    for (int i = 0; i < nq; ++i) {
        const double q = q_host[i];
        if (!(q >= 0.0 && q <= 1.0)) GPB_FAIL(GPB_E_ARG, "gpb_ppd_summary: a level outside [0, 1]");
        if (mixq && ((q > 0.0 && q < 1e-15) || (q < 1.0 && q > 1.0 - 1e-15)))
            GPB_FAIL(GPB_E_ARG, "gpb_ppd_summary: a mixture quantile strictly within 1e-15 of 0 or 1 (outside the starting bracket's reach)");
        lv.q[i] = q;
        const long long k = (long long)floor(q * (double)(S - 1));       // numpy's virtual index (n - 1) q, floored
        lv.k[2 * i] = k;
        lv.k[2 * i + 1] = k + 1 < S ? k + 1 : S - 1;
    }
    if (mixq && !var_T && !vadd_dev) GPB_FAIL(GPB_E_ARG, "gpb_ppd_summary: mixture quantiles need var_T or vadd (a width)");
    if (pit && !yobs_dev) GPB_FAIL(GPB_E_ARG, "gpb_ppd_summary: pit needs yobs");
    if (!moments && !order && !mixq && !pit) return 0;
    GPB_HIP(hipSetDevice(ctx->device));
    HostOut so(ctx, on_device != 0);
    double *d_mo, *d_or, *d_mq, *d_pi;
    so.out(d_mo, moments, 3 * M);
    so.out(d_or, order, 2 * nq * M);
    so.out(d_mq, mixq, nq * M);
    so.out(d_pi, pit, M);
    if (const int rc = so.reserve()) return rc;
    if (const int rc = launch_ppd(ctx, mu_T, var_T, M, S, ld, lv, vadd_dev, yobs_dev, d_mo, d_or, d_mq, d_pi)) return rc;
    return so.finish();
}
