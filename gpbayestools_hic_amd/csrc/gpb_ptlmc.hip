// gpb_ptlmc.hip — the reference's parallel-tempered Langevin sampler (surmise's PTLMC, src/mcmc.py:623-692) as a
// device-resident step loop over a chain of emulators.
//   k_ptl_propose    rvalo ~ N(0, 1) (Philox + Box-Muller), thetap = theta + sqrt2 adjrho (rvalo @ hc)
//                    [+ adjrho^2 (dfval @ covmat0)]                                    src/mcmc.py:626-633
//   (evaluation)     gpb_chain_logpost / the per-emulator sequence, or gpb_chain_logpost_grad
//   k_ptl_accept     fvalp = lp / temps, the Langevin correction qadj, log u < fvalp - fval + qadj    src/mcmc.py:634-655
//   k_ptl_exchange   tempexchange(iters = 5) in one lane, the reorder out of place, numtimes, the tau update and the
//                    saved sample                                                   src/mcmc.py:657-670,679-692
// Every kernel is written with contraction off and in the reference's order of operations, so that
// tests/ptlmc_reference.py can restate a step operation for operation.
#include "gpb_internal.h"
#include "philox.h"
#include <math.h>

namespace gpb {
namespace {

// the fourth Philox counter word of PTLMC's draws (the stretch move uses 0, 1 and 7)
constexpr uint32_t PTL_TAG_NORMAL = 2u, PTL_TAG_ACCEPT = 3u, PTL_TAG_SWAP = 4u;
constexpr int PTL_MAX_D = 256;          // parameters of a row held in LDS by the propose / accept kernels
constexpr int64_t PTL_MAX_T = 4096;     // ladder rungs: the exchange keeps the order and the tempered values in LDS
constexpr int PTL_ITERS = 5;            // tempexchange(..., iters=5), src/mcmc.py:658
constexpr int PTL_CHUNK = 256;          // exchange picks drawn in parallel per round of the serial lane

__device__ __forceinline__ void ptl_normal_pair(uint64_t seed, uint32_t c, uint32_t k, uint32_t j, double& n0,
                                                double& n1) {
    normal_pair(seed, c, k, j, PTL_TAG_NORMAL, n0, n1);
}

__device__ __forceinline__ void ptl_pick(uint64_t seed, uint32_t i, uint32_t k, int64_t T, int& rt, double& lu) {
    const U4 r = philox(seed, i, k, 0u, PTL_TAG_SWAP);
    rt = 1 + (int)(((uint64_t)r.x * (uint64_t)(T - 1)) >> 32);
    lu = log(u01(r.y, r.z));
}

__device__ __forceinline__ double ptl_accept_logu(uint64_t seed, uint32_t c, uint32_t k) {
    const U4 r = philox(seed, c, k, 0u, PTL_TAG_ACCEPT);
    return log(u01(r.x, r.y));
}

// rho = 2 (1 + tanh tau) as the reference writes it (src/mcmc.py:619,666)
__device__ __forceinline__ double ptl_rho(double tau) {
#pragma clang fp contract(off)
    const double e = exp(2.0 * tau);
    return 2.0 * (1.0 + (e - 1.0) / (e + 1.0));
}

// one wave per chain c
__global__ __launch_bounds__(64) void k_ptl_propose(const double* __restrict__ theta, const double* __restrict__ dfval,
                                                   const double* __restrict__ tune, const double* __restrict__ temps13,
                                                   const double* __restrict__ hc, const double* __restrict__ cov0, int d,
                                                   uint64_t seed, uint32_t k, double* __restrict__ rvalo,
                                                   double* __restrict__ thetap) {
#pragma clang fp contract(off)
    __shared__ double rv[PTL_MAX_D], df[PTL_MAX_D];
    const int64_t c = blockIdx.x;
    const int t = threadIdx.x;
    for (int j = t; 2 * j < d; j += 64) {
        double n0, n1;
        ptl_normal_pair(seed, (uint32_t)c, k, (uint32_t)j, n0, n1);
        rv[2 * j] = n0;
        if (2 * j + 1 < d) rv[2 * j + 1] = n1;
    }
    if (dfval)
        for (int i = t; i < d; i += 64) df[i] = dfval[c * d + i];
    __syncthreads();
    const double adj = ptl_rho(tune[0]) * temps13[c];
    const double sc = 1.4142135623730951 * adj;                // np.sqrt(2) * adjrho
    const double a2 = adj * adj;                               // adjrho ** 2
    for (int i = t; i < d; i += 64) {
        double s = 0.0;
        for (int j = 0; j < d; ++j) s = s + rv[j] * hc[(int64_t)j * d + i];
        double x = theta[c * d + i] + sc * s;
        if (dfval) {
            double g = 0.0;
            for (int j = 0; j < d; ++j) g = g + df[j] * cov0[(int64_t)j * d + i];
            x = x + a2 * g;
        }
        thetap[c * d + i] = x;
        rvalo[c * d + i] = rv[i];
    }
}

// one wave per chain c: the Metropolis-Hastings decision, the chain's state replaced in place where it accepts
__global__ __launch_bounds__(64) void k_ptl_accept(double* __restrict__ theta, double* __restrict__ fval,
                                                  double* __restrict__ dfval, const double* __restrict__ thetap,
                                                  const double* __restrict__ lp, const double* __restrict__ grad,
                                                  const double* __restrict__ rvalo, const double* __restrict__ tune,
                                                  const double* __restrict__ temps, const double* __restrict__ temps13,
                                                  const double* __restrict__ hc, int d, uint64_t seed, uint32_t k,
                                                  int* __restrict__ acc, long long* __restrict__ naccept) {
#pragma clang fp contract(off)
    __shared__ double dsum[PTL_MAX_D], t2[PTL_MAX_D];
    __shared__ double qadj_s;
    const int64_t c = blockIdx.x;
    const int t = threadIdx.x;
    const double tc = temps[c];
    const double fvalp = lp[c] / tc;
    const double f0 = fval[c];
    double qadj = 0.0;
    if (dfval) {
        for (int i = t; i < d; i += 64) dsum[i] = dfval[c * d + i] + grad[c * d + i] / tc;
        __syncthreads();
        const double h = (ptl_rho(tune[0]) * temps13[c]) / 2.0;          // adjrho / 2
        for (int i = t; i < d; i += 64) {
            double s = 0.0;
            for (int j = 0; j < d; ++j) s = s + dsum[j] * hc[(int64_t)j * d + i];
            t2[i] = h * s;
        }
        __syncthreads();
        if (t == 0) {
            double s1 = 0.0, s2 = 0.0;
            for (int i = 0; i < d; ++i) {
                const double term1 = rvalo[c * d + i] / 1.4142135623730951;
                s1 = s1 + term1 * t2[i];
                s2 = s2 + t2[i] * t2[i];
            }
            qadj_s = -(2.0 * s1 + s2);
        }
        __syncthreads();
        qadj = qadj_s;
    }
    const bool take = ptl_accept_logu(seed, (uint32_t)c, k) < (fvalp - f0) + qadj;   // NaN / -inf - -inf reject
    __syncthreads();                                           // every lane has read fval / dfval before they change
    if (take) {
        for (int i = t; i < d; i += 64) {
            theta[c * d + i] = thetap[c * d + i];
            if (dfval) dfval[c * d + i] = grad[c * d + i] / tc;
        }
    }
    if (t == 0) {
        if (take) {
            fval[c] = fvalp;
            if (naccept) naccept[c] += 1;
        }
        acc[c] = take ? 1 : 0;
    }
}

// one workgroup: the temperature exchange (serial in lane 0, as tempexchange is), then the reorder into the other buffers
__global__ __launch_bounds__(256) void k_ptl_exchange(const double* __restrict__ theta, const double* __restrict__ fval,
                                                     const double* __restrict__ dfval, double* __restrict__ theta_o,
                                                     double* __restrict__ fval_o, double* __restrict__ dfval_o,
                                                     const double* __restrict__ temps, const int* __restrict__ acc,
                                                     double* __restrict__ tune, int64_t T, int d, int64_t numtemps,
                                                     uint64_t seed, uint32_t k, int tune_now, double taracc,
                                                     double* __restrict__ save, int64_t nsave, int64_t save_idx,
                                                     long long* __restrict__ nswap) {
#pragma clang fp contract(off)
    __shared__ int order[PTL_MAX_T];
    __shared__ double fo[PTL_MAX_T];           // fvaln[order[i]]: the tempered values follow their chains
    __shared__ int pick[PTL_CHUNK];
    __shared__ double rhoh[PTL_CHUNK], lu[PTL_CHUNK];
    __shared__ int swp[PTL_CHUNK];
    __shared__ int nacc;
    const int t = threadIdx.x;
    if (t == 0) nacc = 0;
    for (int64_t i = t; i < T; i += 256) {
        order[i] = (int)i;
        fo[i] = fval[i] * temps[i];                            // fvaln = fval * temps
    }
    __syncthreads();
    int a = 0;
    for (int64_t i = t; i < T; i += 256) a += acc[i];
    atomicAdd(&nacc, a);
    const int64_t npick = PTL_ITERS * T;
    for (int64_t b = 0; b < npick; b += PTL_CHUNK) {
        const int64_t i = b + t;
        if (i < npick) {
            int rt;
            double l;
            ptl_pick(seed, (uint32_t)i, k, T, rt, l);
            pick[t] = rt;
            rhoh[t] = 1.0 / temps[rt - 1] - 1.0 / temps[rt];
            lu[t] = l;
        }
        __syncthreads();
        if (t == 0) {
            const int n = (int)(npick - b < PTL_CHUNK ? npick - b : PTL_CHUNK);
            for (int q = 0; q < n; ++q) {
                const int rt = pick[q];
                const double hi = fo[rt], lo = fo[rt - 1];
                const int s = (hi - lo) * rhoh[q] > lu[q];
                if (s) {
                    fo[rt - 1] = hi;
                    fo[rt] = lo;
                    const int o = order[rt - 1];
                    order[rt - 1] = order[rt];
                    order[rt] = o;
                }
                swp[q] = s;
            }
        }
        __syncthreads();
        if (nswap && i < npick && swp[t]) atomicAdd(reinterpret_cast<unsigned long long*>(nswap + (pick[t] - 1)), 1ull);
        __syncthreads();
    }
    for (int64_t e = t; e < T * d; e += 256) {
        const int64_t idx = e / d, j = e - idx * d, src = order[idx];
        theta_o[e] = theta[src * d + j];
        if (dfval) dfval_o[e] = (1.0 / temps[idx]) * (temps[src] * dfval[src * d + j]);
    }
    for (int64_t idx = t; idx < T; idx += 256) fval_o[idx] = fo[idx] / temps[idx];
    if (save && save_idx >= 0 && save_idx < nsave) {
        const int64_t numchain = T - numtemps;
        for (int64_t e = t; e < numchain * d; e += 256) {
            const int64_t m = e / d, j = e - m * d;
            save[(m * nsave + save_idx) * d + j] = theta[(int64_t)order[numtemps + m] * d + j];
        }
    }
    if (t == 0) {
        double nt = tune[1] + (double)nacc / (double)T;
        double tau = tune[0];
        if (tune_now) {
            tau = tau + 1.0 / sqrt(1.0 + (double)k / 10.0) * (nt / 10.0 - taracc);
            nt = 0.0;
        }
        tune[0] = tau;
        tune[1] = nt;
    }
}

#ifdef GPB_DEBUG_VARIANTS
__global__ void k_ptl_draws(int64_t T, int d, uint64_t seed, uint32_t k, double* __restrict__ normals,
                            double* __restrict__ lu_acc, long long* __restrict__ picks, double* __restrict__ lu_swap) {
    const int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const int64_t np = (d + 1) / 2;
    if (g < T * np) {
        const int64_t c = g / np, j = g - c * np;
        double n0, n1;
        ptl_normal_pair(seed, (uint32_t)c, k, (uint32_t)j, n0, n1);
        normals[c * d + 2 * j] = n0;
        if (2 * j + 1 < d) normals[c * d + 2 * j + 1] = n1;
    }
    if (g < T) lu_acc[g] = ptl_accept_logu(seed, (uint32_t)g, k);
    if (g < PTL_ITERS * T) {
        int rt;
        double l;
        ptl_pick(seed, (uint32_t)g, k, T, rt, l);
        picks[g] = rt;
        lu_swap[g] = l;
    }
}
#endif

}  // namespace
}  // namespace gpb

using namespace gpb;

extern "C" int gpb_chain_ptlmc_run(gpb_ctx* const* ctxs, int E, int64_t numtemps, int64_t numchain, int64_t nsteps,
                                   uint64_t step0, uint64_t seed, int64_t samptunning, double taracc, double* theta_dev,
                                   double* fval_dev, double* dfval_dev, double* tune_dev, const double* temps_dev,
                                   const double* temps13_dev, const double* hc_dev, const double* covmat0_dev,
                                   const double* lo_dev, const double* hi_dev, double outside_value, double inside_const,
                                   double* save_dev, int64_t nsave, int64_t* naccept_dev, int64_t* nswap_dev) {
    if (!chain_args_ok(ctxs, E)) return GPB_E_ARG;
    gpb_ctx* ctx = ctxs[0];
    if (!theta_dev || !fval_dev || !tune_dev || !temps_dev || !temps13_dev || !hc_dev || !covmat0_dev || !lo_dev ||
        !hi_dev || nsteps < 0 || samptunning < 0 || (save_dev && nsave < 1))
        GPB_FAIL(GPB_E_ARG, "gpb_chain_ptlmc_run: null pointer or negative size");
    const int64_t T = numtemps + numchain;
    if (numtemps < 0 || numchain < 1 || T < 2 || T > PTL_MAX_T)
        GPB_FAIL(GPB_E_ARG, "gpb_chain_ptlmc_run: numtemps + numchain must be 2 .. 4096 with numchain >= 1");
    if (step0 + (uint64_t)nsteps > 0xFFFFFFFFull) GPB_FAIL(GPB_E_ARG, "gpb_chain_ptlmc_run: steps are numbered below 2^32");
    int rc;
    if ((rc = chain_ctx_check(ctxs, E, "gpb_chain_ptlmc_run"))) return rc;
    const int64_t nd = sampler_ndim(ctx);
    if (nd < 1 || nd > PTL_MAX_D) GPB_FAIL(GPB_E_ARG, "gpb_chain_ptlmc_run: 1 .. 256 parameters");
    const bool grad = dfval_dev != nullptr;
    // the gradient's own state checks before anything is enqueued (no rows: nothing runs); chain_eval has none beyond the above
    double probe = 0.0;
    if (grad && (rc = gpb_chain_logpost_grad(ctxs, E, &probe, 0, &probe, &probe, lo_dev, hi_dev, outside_value, inside_const)))
        return rc;
    if (nsteps == 0) return 0;
    GPB_HIP(hipSetDevice(ctx->device));
    PtlWs ws;
    if ((rc = ctx_carve(ctx, ctx->ptl_ws, [&](Carver<double>& c) { ws.lay(c, T, nd); }))) return rc;
    double *rvalo = ws.rvalo, *thetap = ws.thetap, *gbuf = ws.grad, *thetaB = ws.thetaB, *dfvalB = ws.dfvalB, *lp = ws.lp,
           *fvalB = ws.fvalB;
    int* acc = ws.acc;
    double *th = theta_dev, *fv = fval_dev, *df = dfval_dev;          // the state alternates between the two buffers
    double *th2 = thetaB, *fv2 = fvalB, *df2 = grad ? dfvalB : nullptr;
    const dim3 gT((unsigned)T);
    for (int64_t n = 0; n < nsteps; ++n) {
        const uint64_t kk = step0 + (uint64_t)n;
        const uint32_t k = (uint32_t)kk;
        hipLaunchKernelGGL(k_ptl_propose, gT, dim3(64), 0, ctx->stream, th, df, tune_dev, temps13_dev, hc_dev, covmat0_dev,
                           (int)nd, seed, k, rvalo, thetap);
        if (grad) {
            if ((rc = gpb_chain_logpost_grad(ctxs, E, thetap, T, lp, gbuf, lo_dev, hi_dev, outside_value, inside_const)))
                return rc;
        } else if ((rc = chain_eval(ctxs, E, thetap, T, lp, lo_dev, hi_dev, outside_value, inside_const))) {
            return rc;
        }
        hipLaunchKernelGGL(k_ptl_accept, gT, dim3(64), 0, ctx->stream, th, fv, df, thetap, lp, grad ? gbuf : nullptr,
                           rvalo, tune_dev, temps_dev, temps13_dev, hc_dev, (int)nd, seed, k, acc,
                           reinterpret_cast<long long*>(naccept_dev));
        const bool tuning = (int64_t)kk < samptunning;
        const int tune_now = tuning && kk % 10 == 0;
        const int64_t save_idx = (!tuning && save_dev) ? (int64_t)kk - samptunning : -1;
        hipLaunchKernelGGL(k_ptl_exchange, dim3(1), dim3(256), 0, ctx->stream, th, fv, df, th2, fv2, df2, temps_dev, acc,
                           tune_dev, T, (int)nd, numtemps, seed, k, tune_now, taracc, save_dev, nsave, save_idx,
                           reinterpret_cast<long long*>(nswap_dev));
        std::swap(th, th2);
        std::swap(fv, fv2);
        std::swap(df, df2);
    }
    GPB_HIP(hipGetLastError());
    if (th != theta_dev) {
        GPB_HIP(hipMemcpyAsync(theta_dev, th, sizeof(double) * (size_t)(T * nd), hipMemcpyDeviceToDevice, ctx->stream));
        GPB_HIP(hipMemcpyAsync(fval_dev, fv, sizeof(double) * (size_t)T, hipMemcpyDeviceToDevice, ctx->stream));
        if (grad)
            GPB_HIP(hipMemcpyAsync(dfval_dev, df, sizeof(double) * (size_t)(T * nd), hipMemcpyDeviceToDevice, ctx->stream));
    }
    return 0;
}

#ifdef GPB_DEBUG_VARIANTS      // test hook (include/gpbayes_debug.h)
extern "C" int gpb_test_ptlmc_draws(gpb_ctx* ctx, int64_t T, int64_t d, uint64_t seed, uint64_t step, double* normals_dev,
                                    double* logu_accept_dev, int64_t* picks_dev, double* logu_swap_dev) {
    if (!ctx || T < 2 || T > PTL_MAX_T || d < 1 || d > PTL_MAX_D || !normals_dev || !logu_accept_dev || !picks_dev ||
        !logu_swap_dev)
        return GPB_E_ARG;
    GPB_HIP(hipSetDevice(ctx->device));
    const int64_t n = T * ((d + 1) / 2) > PTL_ITERS * T ? T * ((d + 1) / 2) : PTL_ITERS * T;
    hipLaunchKernelGGL(k_ptl_draws, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, T, (int)d, seed,
                       (uint32_t)step, normals_dev, logu_accept_dev, reinterpret_cast<long long*>(picks_dev), logu_swap_dev);
    GPB_HIP(hipGetLastError());
    return 0;
}
#endif  // GPB_DEBUG_VARIANTS
