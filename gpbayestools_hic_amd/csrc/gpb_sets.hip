// gpb_sets.hip — one chain of emulators calibrated against MANY data vectors in one resident run (a closure study: the
// experiment replaced by the model's own output at K held-out design points, examples/ClosureTest.ipynb once per point).
//   gpb_chain_like_sets        per emulator the data terms (v0[k][16], cperp[k]) of K data vectors against the covariance that
//                              gpb_chain_like_set installed: O(M^2) host work per vector, no second Cholesky (lowrank_setup.h)
//   gpb_chain_logpost_sets     rows that belong to different data sets: chain_rows with the last stage replaced
//                              (chain_rows_sets, gpb_chain.hip; k_loglike_lowrank_sets, gpb_like.hip)
//   gpb_chain_emcee_sets_run   the stretch move over K independent ensembles whose proposals form ONE batch of K nw/2 rows per
//                              half-step.  Set s draws exactly what a stand-alone gpb_chain_emcee_run with seed = seeds[s]
//                              draws (the device functions of stretch_move.h with the set's own Ensemble and offset
//                              pointers), so its walkers are that run's, bit for bit.
// The covariance is shared by all sets; a covariance per set would need a factorisation per set and is out of scope.
#include "gpb_internal.h"
#include "stretch_move.h"

namespace gpb {
namespace {

// K ensembles of 2 nhalf walkers each: pos [K][2 nhalf][d], set s keyed by seeds[s]
struct SetsEnsembles {
    const uint64_t* seeds;             // [K] (device)
    int64_t nhalf;
    int d, hb, randomize;
};

// grid (walker groups of one set, sets): k_propose on set blockIdx.y.  The batch's rows are numbered across the sets — slot k
// of set s is row s nhalf + k — which propose_slot forms as k - r0: r0 = -(s nhalf), and every slot of the set is "mine".
__global__ void k_propose_sets(const double* __restrict__ pos, SetsEnsembles se, int half, uint32_t step, double a,
                               double* __restrict__ q, double* __restrict__ factor, ProposeBox box) {
    const int64_t gid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const int64_t k = gid >> 5;
    if (k >= se.nhalf) return;
    const int64_t o = (int64_t)blockIdx.y * se.nhalf;              // the set's first row of the batch
    const Ensemble en{se.nhalf, se.d, se.seeds[blockIdx.y], se.hb, se.randomize};
    const double* ps = pos + 2 * o * se.d;
    box.r0 = -o;
    box.chunk = o + se.nhalf;
    if (box.ll) box.ll += o;
    propose_slot(en, k, (int)(gid & 31), half, step, a, q + o * se.d, factor + o, box, [&](int64_t w) { return ps + w * se.d; });
}

// k_accept on set blockIdx.y: the set's own permutation, draws and lp; the counter of the finished batch is re-armed once
__global__ void k_accept_sets(double* __restrict__ pos, double* __restrict__ lp, SetsEnsembles se, int half, uint32_t step,
                              const double* __restrict__ q, const double* __restrict__ factor, const double* __restrict__ lpq,
                              long long* __restrict__ naccept, long long* __restrict__ n_nan, BatchCount done) {
    const int64_t gid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const int64_t k = gid >> 5;
    const int t0 = (int)(gid & 31), d = se.d;
    if (done.cmp && gid == 0 && blockIdx.y == 0) done.report_and_rearm();
    if (k >= se.nhalf) return;
    const int64_t o = (int64_t)blockIdx.y * se.nhalf;
    const uint64_t seed = se.seeds[blockIdx.y];
    double* ps = pos + 2 * o * d;
    double* lps = lp + 2 * o;
    const double* qs = q + o * d;
    const int64_t idx = make_perm(seed, step, 2 * se.nhalf, se.hb, se.randomize)(2 * k + half);
    LpSource src{};
    src.lpq = lpq + o;
    double lpq_k;
    const bool take = accept_decision(PendingAccept{qs, factor + o, lps, src, seed, step, half}, k, idx, lpq_k);
    // a NaN log-probability is rejected and counted, as in k_accept
    if (n_nan && t0 == 0 && lpq_k != lpq_k) atomicAdd(reinterpret_cast<unsigned long long*>(n_nan), 1ull);
    __builtin_amdgcn_wave_barrier();                                 // keep the loads above the stores below
    if (take) {
        for (int t = t0; t < d; t += 32) ps[idx * d + t] = qs[k * d + t];
        if (t0 == 0) {
            lps[idx] = lpq_k;
            if (naccept) naccept[2 * o + idx] += 1;
        }
    }
}

__global__ void k_store_sets(const double* __restrict__ pos, const double* __restrict__ lp, double* __restrict__ chain,
                             double* __restrict__ lpchain, int64_t nw, int d) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (chain && i < nw * d) chain[i] = pos[i];
    if (lpchain && i < nw) lpchain[i] = lp[i];
}

}  // namespace
}  // namespace gpb

using namespace gpb;

extern "C" int gpb_chain_like_sets(gpb_ctx* const* ctxs, int E, int64_t K, const double* yexp_host) {
    if (!chain_args_ok(ctxs, E)) return GPB_E_ARG;
    gpb_ctx* ctx = ctxs[0];
    for (int e = 0; e < E; ++e)
        if (!ctxs[e]) GPB_FAIL(GPB_E_ARG, "gpb_chain_like_sets: null context");
    if (K == 0) {                                      // the tables are dropped
        for (int e = 0; e < E; ++e) ctxs[e]->lrs_K = 0;
        return 0;
    }
    if (K < 1 || K > MAX_LIKE_SETS) GPB_FAIL(GPB_E_ARG, "gpb_chain_like_sets: 1 <= K <= 65536 data sets (0 drops the tables)");
    if (!yexp_host) GPB_FAIL(GPB_E_ARG, "gpb_chain_like_sets: null pointer");
    int64_t MT = 0;
    for (int e = 0; e < E; ++e) {
        if (!ctxs[e]->have_like) GPB_FAIL(GPB_E_STATE, "gpb_chain_like_sets before gpb_chain_like_set");
        if (ctxs[e]->device != ctx->device || ctxs[e]->stream != ctx->stream)
            GPB_FAIL(GPB_E_STATE, "gpb_chain_like_sets: the emulators' contexts must share one device and stream");
        MT += ctxs[e]->M;
    }
    int rc = lowrank_sets_check(ctxs, E, "gpb_chain_like_sets");
    if (rc) return rc;
    GPB_HIP(hipSetDevice(ctx->device));
    GPB_HIP(hipStreamSynchronize(ctx->stream));        // (nothing enqueued still reads the tables that are replaced)
    for (int e = 0; e < E; ++e) ctxs[e]->lrs_K = 0;
    std::vector<double> v0, cperp((size_t)K);
    for (int64_t e = 0, o = 0; e < E; o += ctxs[e]->M, ++e) {
        gpb_ctx* c = ctxs[e];
        v0.assign((size_t)(K * 16), 0.0);              // zero padded beyond P like lr_v0
        for (int64_t k = 0; k < K; ++k)
            lowrank_data_terms(c->lr_fac, c->h_mu.data(), yexp_host + k * MT + o, v0.data() + k * 16, &cperp[(size_t)k]);
        if ((rc = ctx_replace(c, c->lrs_v0, K * 16)) || (rc = ctx_replace(c, c->lrs_cperp, K))) {
            if (e) ctx->err = c->err;
            return rc;
        }
        GPB_HIP(hipMemcpy(c->lrs_v0, v0.data(), sizeof(double) * (size_t)(K * 16), hipMemcpyHostToDevice));
        GPB_HIP(hipMemcpy(c->lrs_cperp, cperp.data(), sizeof(double) * (size_t)K, hipMemcpyHostToDevice));
    }
    for (int e = 0; e < E; ++e) ctxs[e]->lrs_K = K;
    return 0;
}

#ifdef GPB_DEBUG_VARIANTS      // test hook (include/gpbayes_debug.h)
extern "C" int gpb_debug_like_tables(gpb_ctx* ctx, int64_t K, double* v0_host, double* cperp_host) {
    if (!ctx || !v0_host || !cperp_host || K < 0) return GPB_E_ARG;
    GPB_HIP(hipSetDevice(ctx->device));
    GPB_HIP(hipStreamSynchronize(ctx->stream));
    if (K == 0) {
        if (!ctx->have_like || !ctx->lr_ok) GPB_FAIL(GPB_E_STATE, "gpb_debug_like_tables: no low-rank likelihood installed");
        GPB_HIP(hipMemcpy(v0_host, ctx->lr_v0, sizeof(double) * 16, hipMemcpyDeviceToHost));
        *cperp_host = ctx->lr_cperp;
        return 0;
    }
    if (ctx->lrs_K < 1) GPB_FAIL(GPB_E_STATE, "gpb_debug_like_tables: no per-data-set tables (gpb_chain_like_sets)");
    if (K != ctx->lrs_K) GPB_FAIL(GPB_E_ARG, "gpb_debug_like_tables: K is not the tables' K");
    GPB_HIP(hipMemcpy(v0_host, ctx->lrs_v0, sizeof(double) * (size_t)(K * 16), hipMemcpyDeviceToHost));
    GPB_HIP(hipMemcpy(cperp_host, ctx->lrs_cperp, sizeof(double) * (size_t)K, hipMemcpyDeviceToHost));
    return 0;
}
#endif  // GPB_DEBUG_VARIANTS

extern "C" int gpb_chain_logpost_sets(gpb_ctx* const* ctxs, int E, const double* Xs_dev, int64_t W, int64_t rows_per_set,
                                      double* ll_dev, const double* lo_dev, const double* hi_dev, double outside_value,
                                      double inside_const) {
    if (!chain_args_ok(ctxs, E)) return GPB_E_ARG;
    gpb_ctx* ctx = ctxs[0];
    if (!Xs_dev || !ll_dev || !lo_dev || !hi_dev || W < 0) GPB_FAIL(GPB_E_ARG, "gpb_chain_logpost_sets: null pointer or negative size");
    if (rows_per_set < 1 || W % rows_per_set || W >= (1ll << 31))
        GPB_FAIL(GPB_E_ARG, "gpb_chain_logpost_sets: W must be a multiple of rows_per_set >= 1, below 2^31");
    int rc = sets_check(ctxs, E, W / rows_per_set, "gpb_chain_logpost_sets");
    if (rc) return rc;
    if (W == 0) return 0;
    GPB_HIP(hipSetDevice(ctx->device));
    return chain_rows_sets(ctxs, E, Xs_dev, W, rows_per_set, ll_dev, lo_dev, hi_dev, outside_value, inside_const);
}

extern "C" int gpb_chain_emcee_sets_run(gpb_ctx* const* ctxs, int E, double* pos_dev, double* lp_dev, int64_t K, int64_t nwalkers,
                                        int64_t nsteps, const uint64_t* seeds_host, uint64_t step0, double a, int randomize_split,
                                        const double* lo_dev, const double* hi_dev, double outside_value, double inside_const,
                                        double* chain_dev, double* lpchain_dev, int64_t* naccept_dev) {
    if (!chain_args_ok(ctxs, E)) return GPB_E_ARG;
    gpb_ctx* ctx = ctxs[0];
    // ---- every check and every workspace before the first launch
    if (!pos_dev || !lp_dev || !lo_dev || !hi_dev || !seeds_host || nsteps < 0)
        GPB_FAIL(GPB_E_ARG, "gpb_chain_emcee_sets_run: null pointer or negative size");
    if (K < 1 || K > 65535) GPB_FAIL(GPB_E_ARG, "gpb_chain_emcee_sets_run: 1 <= K <= 65535 ensembles (the sets are a grid dimension)");
    if (nwalkers < 2 || (nwalkers & 1) || nwalkers > (1ll << 30) || K * nwalkers > (1ll << 30))
        GPB_FAIL(GPB_E_ARG, "gpb_chain_emcee_sets_run: nwalkers must be even, 2 .. 2^30, and K nwalkers <= 2^30");
    if (ctx->comm) GPB_FAIL(GPB_E_STATE, "gpb_chain_emcee_sets_run: a communicator is installed (the K-set move is not sharded)");
    int rc = sets_check(ctxs, E, K, "gpb_chain_emcee_sets_run");
    if (rc) return rc;
    GPB_HIP(hipSetDevice(ctx->device));
    const int64_t nh = nwalkers / 2, d = sampler_ndim(ctx), W = K * nh;
    for (int e = 0; e < E; ++e)
        if ((rc = ensure_wcap(ctxs[e], W))) { if (e) ctx->err = ctxs[e]->err; return rc; }
    if ((rc = ensure_lr_blocks(ctx, E))) return rc;
    McWs mc{};
    if ((rc = ctx_carve(ctx, ctx->mc_ws, [&](Carver<double>& c) { mc.lay(c, W, d); }))) return rc;
    if ((rc = ensure_cmp_rows(ctx, d))) return rc;
    if ((rc = ctx_grow(ctx, ctx->sets_seeds, K))) return rc;
    // emcee_plan's size rule (gpb_stretch.hip): the proposal kernel gathers the rows inside the box itself (premark 2) while
    // the batch is small enough for it; beyond that, or with tune key 29 below 2, launch_compact marks and gathers
    const int pre = (ctx->premark >= 2 && W <= 16384) ? 2 : 0;
    if (nsteps == 0) return 0;
    GPB_HIP(hipMemcpyAsync(ctx->sets_seeds, seeds_host, sizeof(uint64_t) * (size_t)K, hipMemcpyHostToDevice, ctx->stream));
    if (pre) GPB_HIP(hipMemsetAsync(ctx->cmp_idx, 0, 2 * sizeof(int), ctx->stream));
    const SetsEnsembles se{ctx->sets_seeds, nh, (int)d, half_bits(nwalkers), randomize_split ? 1 : 0};
    const dim3 grid((unsigned)((nh * 32 + 255) / 256), (unsigned)K);
    double *q = mc.q[0], *factor = mc.factor[0], *lpq = mc.lpq[0];
    int* cmpv = ctx->cmp_idx;
    ProposeBox box{};
    BatchCount done{};
    if (pre) {
        box.lo = lo_dev; box.hi = hi_dev; box.outside = outside_value;
        box.ll = lpq; box.Xc = ctx->cmp_X; box.cmp = cmpv;
        done = BatchCount{cmpv, ctx->live_hint, W, ctx->profile ? ctx->rows_live : (unsigned long long*)nullptr};
    }
    const int64_t nrow = K * nwalkers;
    // ---- the unfused sequence per half-step: propose -> evaluate -> accept [-> store]
    for (int64_t g = 0; g < 2 * nsteps; ++g) {
        const int64_t n = g >> 1;
        const int half = (int)(g & 1);
        const uint32_t step = (uint32_t)(step0 + (uint64_t)n);
        hipLaunchKernelGGL(k_propose_sets, grid, dim3(256), 0, ctx->stream, pos_dev, se, half, step, a, q, factor, box);
        if ((rc = chain_rows_sets(ctxs, E, q, W, nh, lpq, lo_dev, hi_dev, outside_value, inside_const, pre, cmpv))) return rc;
        hipLaunchKernelGGL(k_accept_sets, grid, dim3(256), 0, ctx->stream, pos_dev, lp_dev, se, half, step, q, factor, lpq,
                           reinterpret_cast<long long*>(naccept_dev), reinterpret_cast<long long*>(ctx->n_nan.get()), done);
        if (half == 1 && (chain_dev || lpchain_dev))
            hipLaunchKernelGGL(k_store_sets, dim3((unsigned)((nrow * d + 255) / 256)), dim3(256), 0, ctx->stream, pos_dev, lp_dev,
                               chain_dev ? chain_dev + n * nrow * d : nullptr, lpchain_dev ? lpchain_dev + n * nrow : nullptr,
                               nrow, (int)d);
    }
    GPB_HIP(hipGetLastError());
    return 0;
}
