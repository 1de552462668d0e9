// gpb_hmc.hip — Hamiltonian Monte Carlo over many independent chains as a device-resident step loop over a chain of emulators
// (DESIGN.md section 30).  A diagonal metric, L leapfrog steps per trajectory, the hard prior box as reflecting walls, the step
// size adapted by dual averaging on the mean accept probability of all chains.  One gpb_chain_logpost_grad of C rows per
// leapfrog: the batch the gradient kernels were built for.
//   k_hmc_eps        the step's step size eps_k = eps (1 + jitter (2 u - 1)), one lane, shared by all chains
//   k_hmc_begin      momenta p = z msqrt (Philox + Box-Muller), the trajectory's start, H0 = -lp + K0       one wave per chain
//   k_hmc_leap       [second kick of the leapfrog before,] first kick, drift, walls                  one thread per (chain, j)
//   (evaluation)     gpb_chain_logpost_grad at the C trajectory points
//   k_hmc_finish     last kick, H1, the accept test, the state replaced in place, counters, the saved sample  one wave per chain
//   k_hmc_adapt      the dual-averaging update from the integer sum of the accept probabilities, one lane
// The arithmetic is that of hmc_step.h, built with -ffp-contract=off (build.py), every sum over the parameters in index order
// in one lane, so that tests/hmc_reference.py restates a step operation for operation.  No kernel waits for another
// workgroup; the only loop whose trip count depends on data is the wall rule's, bounded by GPB_HMC_MAX_REFLECT.
#include "gpb_internal.h"
#include "hmc_step.h"
#include "philox.h"
#include <math.h>

namespace gpb {
namespace {

// the fourth Philox counter word of HMC's draws (philox.h lists the tags in use)
constexpr uint32_t HMC_TAG_MOM = 12u, HMC_TAG_EPS = 13u, HMC_TAG_ACC = 14u;
constexpr int HMC_MAX_D = 256;               // parameters of a chain held in LDS by k_hmc_begin / k_hmc_finish
constexpr int64_t HMC_MAX_C = 1048576;
constexpr int64_t HMC_MAX_L = 1024;
// the state block's 8-byte slots behind the five doubles of hmc_step.h
constexpr int HMC_ST_ACCEPTED = 5, HMC_ST_DIVERGENT = 6, HMC_ST_ESCAPED = 7, HMC_ST_NAN = 8, HMC_ST_ASUM = 9;

__device__ __forceinline__ void count(double* state, int slot, unsigned long long n) {
    atomicAdd(reinterpret_cast<unsigned long long*>(state) + slot, n);
}

__global__ __launch_bounds__(64) void k_hmc_eps(const double* __restrict__ state, double jitter, uint64_t seed, uint32_t k,
                                                double* __restrict__ eps, double* __restrict__ eps_out) {
    if (threadIdx.x != 0) return;
    const U4 r = philox(seed, 0u, k, 0u, HMC_TAG_EPS);
    const double e = hmc_step_size(state[0], jitter, u01(r.x, r.y));
    eps[0] = e;
    eps[1] = e / 2.0;
    if (eps_out) eps_out[0] = e;
}

// one wave per chain c
__global__ __launch_bounds__(64) void k_hmc_begin(const double* __restrict__ x, const double* __restrict__ lp,
                                                  const double* __restrict__ minv, const double* __restrict__ msqrt, int d,
                                                  uint64_t seed, uint32_t k, double* __restrict__ p, double* __restrict__ xt,
                                                  double* __restrict__ h0, int* __restrict__ esc, double* __restrict__ p0_out) {
    __shared__ double ps[HMC_MAX_D];
    const int64_t c = blockIdx.x;
    const int t = threadIdx.x;
    for (int j = t; 2 * j < d; j += 64) {
        double n0, n1;
        normal_pair(seed, (uint32_t)c, k, (uint32_t)j, HMC_TAG_MOM, n0, n1);
        ps[2 * j] = n0 * msqrt[2 * j];
        if (2 * j + 1 < d) ps[2 * j + 1] = n1 * msqrt[2 * j + 1];
    }
    __syncthreads();
    for (int i = t; i < d; i += 64) {
        p[c * d + i] = ps[i];
        if (p0_out) p0_out[c * d + i] = ps[i];
        xt[c * d + i] = x[c * d + i];
    }
    if (t == 0) {
        h0[c] = -lp[c] + hmc_kinetic(ps, minv, d);
        esc[c] = 0;
    }
}

// one thread per (chain, parameter): g is the state's gradient for the trajectory's first leapfrog (and no second kick is
// pending then), the trajectory's own gradient gt afterwards
__global__ __launch_bounds__(256) void k_hmc_leap(double* __restrict__ p, double* __restrict__ xt, const double* __restrict__ g,
                                                  const double* __restrict__ gt, const double* __restrict__ eps,
                                                  const double* __restrict__ minv, const double* __restrict__ lo,
                                                  const double* __restrict__ hi, int64_t n, int d, int first,
                                                  int* __restrict__ esc, double* __restrict__ traj_out) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t c = i / d;
    const int j = (int)(i - c * d);
    const double e = eps[0], h = eps[1];
    double pp = p[i];
    if (!first) pp = hmc_kick(pp, h, gt[i]);
    pp = hmc_kick(pp, h, first ? g[i] : gt[i]);
    double xx = xt[i];
    const int r = hmc_drift(xx, pp, e, minv[j], lo[j], hi[j]);
    p[i] = pp;
    xt[i] = xx;
    if (r & GPB_HMC_ESCAPED) esc[c] = 1;                      // (every writer writes the same value)
    if (traj_out) traj_out[i] = xx;
}

// one wave per chain c: the last kick, the energy error, the decision; where the chain accepts, x, lp and grad are replaced
__global__ __launch_bounds__(64) void k_hmc_finish(double* __restrict__ x, double* __restrict__ lp, double* __restrict__ grad,
                                                   const double* __restrict__ p, const double* __restrict__ xt,
                                                   const double* __restrict__ gt, const double* __restrict__ lpt,
                                                   const double* __restrict__ h0, const int* __restrict__ esc,
                                                   const double* __restrict__ eps, const double* __restrict__ minv, int d,
                                                   int64_t C, uint64_t seed, uint32_t k, int adapt, double* __restrict__ state,
                                                   long long* __restrict__ naccept, double* __restrict__ save,
                                                   double* __restrict__ lpsave, int64_t save_idx, double* __restrict__ logu_out,
                                                   double* __restrict__ dh_out, double* __restrict__ a_out) {
    __shared__ double ps[HMC_MAX_D];
    __shared__ int take_s;
    const int64_t c = blockIdx.x;
    const int t = threadIdx.x;
    const double h = eps[1];
    for (int i = t; i < d; i += 64) ps[i] = hmc_kick(p[c * d + i], h, gt[c * d + i]);
    __syncthreads();
    if (t == 0) {
        const double l1 = lpt[c];
        const double h1 = -l1 + hmc_kinetic(ps, minv, d);
        const double dH = h1 - h0[c];
        const U4 r = philox(seed, (uint32_t)c, k, 0u, HMC_TAG_ACC);
        const double lu = log(u01(r.x, r.y));
        const bool escaped = esc[c] != 0;
        const bool take = (lu < -dH) && !escaped;             // NaN rejects: the comparison is false
        const double a = escaped ? 0.0 : hmc_accept_prob(dH);
        take_s = take ? 1 : 0;
        if (take) {
            lp[c] = l1;
            if (naccept) naccept[c] += 1;
            count(state, HMC_ST_ACCEPTED, 1ull);
        }
        if (dH > HMC_DIVERGENT || dH != dH) count(state, HMC_ST_DIVERGENT, 1ull);
        if (escaped) count(state, HMC_ST_ESCAPED, 1ull);
        if (l1 != l1) count(state, HMC_ST_NAN, 1ull);
        if (adapt) count(state, HMC_ST_ASUM, hmc_a_fixed(a));
        if (logu_out) logu_out[c] = lu;
        if (dh_out) dh_out[c] = dH;
        if (a_out) a_out[c] = a;
    }
    __syncthreads();
    const bool take = take_s != 0;
    for (int i = t; i < d; i += 64) {
        double xi = x[c * d + i];
        if (take) {
            xi = xt[c * d + i];
            x[c * d + i] = xi;
            grad[c * d + i] = gt[c * d + i];
        }
        if (save_idx >= 0) save[(save_idx * C + c) * d + i] = xi;
    }
    if (t == 0 && save_idx >= 0 && lpsave) lpsave[save_idx * C + c] = lp[c];
}

__global__ __launch_bounds__(64) void k_hmc_adapt(double* __restrict__ state, int64_t C, double target) {
    if (threadIdx.x != 0) return;
    unsigned long long* u = reinterpret_cast<unsigned long long*>(state);
    hmc_dual_average(state, hmc_a_mean(u[HMC_ST_ASUM], (long long)C), target);
    u[HMC_ST_ASUM] = 0ull;
}

}  // namespace
}  // namespace gpb

using namespace gpb;

extern "C" int gpb_chain_hmc_run(gpb_ctx* const* ctxs, int E, int64_t C, int64_t nsteps, uint64_t step0, uint64_t seed, int64_t L,
                                 double jitter, int adapt, double target_accept, double* x_dev, double* lp_dev, double* grad_dev,
                                 double* state_dev, const double* minv_dev, const double* msqrt_dev, const double* lo_dev,
                                 const double* hi_dev, double outside_value, double inside_const, double* save_dev,
                                 double* lpsave_dev, int64_t nsave, uint64_t save0, int64_t thin, int64_t* naccept_dev,
                                 const gpb_hmc_diag* diag) {
    if (!chain_args_ok(ctxs, E)) return GPB_E_ARG;
    gpb_ctx* ctx = ctxs[0];
    if (!x_dev || !lp_dev || !grad_dev || !state_dev || !minv_dev || !msqrt_dev || !lo_dev || !hi_dev || nsteps < 0 ||
        (save_dev && (nsave < 1 || thin < 1)))
        GPB_FAIL(GPB_E_ARG, "gpb_chain_hmc_run: null pointer, negative size, or nsave / thin below 1 with save_dev");
    if (C < 1 || C > HMC_MAX_C) GPB_FAIL(GPB_E_ARG, "gpb_chain_hmc_run: 1 .. 1048576 chains");
    if (L < 1 || L > HMC_MAX_L) GPB_FAIL(GPB_E_ARG, "gpb_chain_hmc_run: 1 .. 1024 leapfrog steps");
    if (!(jitter >= 0.0 && jitter < 1.0)) GPB_FAIL(GPB_E_ARG, "gpb_chain_hmc_run: 0 <= jitter < 1");
    if (adapt && !(target_accept > 0.0 && target_accept < 1.0)) GPB_FAIL(GPB_E_ARG, "gpb_chain_hmc_run: 0 < target_accept < 1");
    // steps step0 .. step0 + nsteps - 1 are all below 2^32 (step0 first: the sum must not wrap)
    if (step0 > 0xFFFFFFFFull || (uint64_t)nsteps > 0x100000000ull - step0)
        GPB_FAIL(GPB_E_ARG, "gpb_chain_hmc_run: steps are numbered below 2^32");
    if (diag && nsteps != 1) GPB_FAIL(GPB_E_ARG, "gpb_chain_hmc_run: diag reports one step (nsteps == 1)");
    int rc;
    if ((rc = chain_ctx_check(ctxs, E, "gpb_chain_hmc_run"))) return rc;
    const int64_t nd = sampler_ndim(ctx);
    if (nd < 1 || nd > HMC_MAX_D) GPB_FAIL(GPB_E_ARG, "gpb_chain_hmc_run: 1 .. 256 parameters");
    // the gradient's own state checks before anything is enqueued (no rows: nothing runs)
    double probe = 0.0;
    if ((rc = gpb_chain_logpost_grad(ctxs, E, &probe, 0, &probe, &probe, lo_dev, hi_dev, outside_value, inside_const))) return rc;
    if (nsteps == 0) return 0;
    GPB_HIP(hipSetDevice(ctx->device));
    HmcWs ws;
    if ((rc = ctx_carve(ctx, ctx->hmc_ws, [&](Carver<double>& c) { ws.lay(c, C, nd); }))) return rc;
    const int64_t n = C * nd;
    const dim3 gC((unsigned)C), gN((unsigned)((n + 255) / 256));
    for (int64_t s = 0; s < nsteps; ++s) {
        const uint64_t kk = step0 + (uint64_t)s;
        const uint32_t k = (uint32_t)kk;
        hipLaunchKernelGGL(k_hmc_eps, dim3(1), dim3(64), 0, ctx->stream, state_dev, jitter, seed, k, ws.eps,
                           diag ? diag->eps_dev : nullptr);
        hipLaunchKernelGGL(k_hmc_begin, gC, dim3(64), 0, ctx->stream, x_dev, lp_dev, minv_dev, msqrt_dev, (int)nd, seed, k, ws.p,
                           ws.xt, ws.h0, ws.esc, diag ? diag->p0_dev : nullptr);
        for (int64_t l = 0; l < L; ++l) {
            hipLaunchKernelGGL(k_hmc_leap, gN, dim3(256), 0, ctx->stream, ws.p, ws.xt, grad_dev, ws.gt, ws.eps, minv_dev, lo_dev,
                               hi_dev, n, (int)nd, l == 0 ? 1 : 0, ws.esc,
                               (diag && diag->traj_dev) ? diag->traj_dev + l * n : nullptr);
            if ((rc = gpb_chain_logpost_grad(ctxs, E, ws.xt, C, ws.lpt, ws.gt, lo_dev, hi_dev, outside_value, inside_const)))
                return rc;
        }
        int64_t save_idx = -1;
        if (save_dev && kk >= save0 && (kk - save0) % (uint64_t)thin == 0 && (int64_t)((kk - save0) / (uint64_t)thin) < nsave)
            save_idx = (int64_t)((kk - save0) / (uint64_t)thin);
        hipLaunchKernelGGL(k_hmc_finish, gC, dim3(64), 0, ctx->stream, x_dev, lp_dev, grad_dev, ws.p, ws.xt, ws.gt, ws.lpt, ws.h0,
                           ws.esc, ws.eps, minv_dev, (int)nd, C, seed, k, adapt ? 1 : 0, state_dev,
                           reinterpret_cast<long long*>(naccept_dev), save_dev, lpsave_dev, save_idx,
                           diag ? diag->logu_dev : nullptr, diag ? diag->dh_dev : nullptr, diag ? diag->a_dev : nullptr);
        if (adapt) hipLaunchKernelGGL(k_hmc_adapt, dim3(1), dim3(64), 0, ctx->stream, state_dev, C, target_accept);
    }
    GPB_HIP(hipGetLastError());
    return 0;
}
