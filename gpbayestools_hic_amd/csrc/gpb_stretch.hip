// gpb_stretch.hip — the emcee-equivalent stretch move and its device-resident loop over a chain of emulators.
//   k_propose / k_accept   emcee StretchMove (a=2) as driven by     src/mcmc.py:68-92,372-412
//   gpb_chain_emcee_run: the log-posterior batches are those of gpb_chain.hip (chain_rows, whose compaction the proposal
//   kernels here take over; chain_eval for one uncompacted emulator), as for the other samplers (gpb_ptlmc.hip, gpb_smc.hip)
#include "gpb_internal.h"
#include "stretch_move.h"

namespace gpb {

__global__ void k_propose(const double* __restrict__ pos, Ensemble en, int half, uint32_t step, double a,
                          double* __restrict__ q, double* __restrict__ factor, ProposeBox box) {
    const int64_t gid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const int64_t k = gid >> 5;
    if (k >= en.nhalf) return;
    propose_slot(en, k, (int)(gid & 31), half, step, a, q, factor, box, [&](int64_t w) { return pos + w * en.d; });
}


__global__ void k_accept(double* __restrict__ pos, double* __restrict__ lp, Ensemble en, int half, uint32_t step,
                         const double* __restrict__ q, const double* __restrict__ factor, LpSource lpq,
                         long long* __restrict__ naccept, long long* __restrict__ n_nan, BatchCount done) {
    // 32 lanes per walker, all inside one wave: every lane takes the same decision from the OLD lp[idx]
    // (the load precedes lane 0's store in program order), then moves its own parameters
    const int64_t gid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const int64_t k = gid >> 5;
    const int t0 = (int)(gid & 31), d = en.d;
    if (done.cmp && gid == 0) done.report_and_rearm();
    if (k >= en.nhalf) return;
    const int64_t idx = make_perm(en.seed, step, 2 * en.nhalf, en.hb, en.randomize)(2 * k + half);
    double lpq_k;
    const bool take = accept_decision(PendingAccept{q, factor, lp, lpq, en.seed, step, half}, k, idx, lpq_k);
    // emcee raises "Probability function returned NaN" at the step it happens (emcee/ensemble.py compute_log_prob);
    // here the proposal is rejected (NaN compares false) and counted, and the host raises at its next check
    if (n_nan && t0 == 0 && lpq_k != lpq_k) atomicAdd(reinterpret_cast<unsigned long long*>(n_nan), 1ull);
    __builtin_amdgcn_wave_barrier();                                 // keep the loads above the stores below
    if (take) {
        for (int t = t0; t < d; t += 32) pos[idx * d + t] = q[k * d + t];
        if (t0 == 0) {
            lp[idx] = lpq_k;
            if (naccept) naccept[idx] += 1;
        }
    }
}

// The accept of one half-step and the proposal of the next in ONE launch (gpb_chain_emcee_run): a proposal needs the
// positions AFTER the pending accept, of its own walker and of its partner; instead of waiting for another kernel to
// have moved them, a walker group looks both walkers up — the inverse split permutation tells whether a walker is in the
// pending half and in which slot — and takes that slot's accept decision itself (same draws, same arithmetic as the
// group that owns the slot).  Accepted walkers are read from the pending proposals q_a, all others from pos, which this
// kernel writes for accepted walkers only: no read of a location another group writes.  lp is ping-ponged (lp_in is
// read by every decision, lp_out written once per walker), q / factor / lpq alternate between two sets.
__global__ void k_accept_propose(double* __restrict__ pos, const double* __restrict__ lp_in, double* __restrict__ lp_out,
                                 Ensemble en, int half_a, uint32_t step_a, const double* __restrict__ q_a,
                                 const double* __restrict__ factor_a, LpSource lpq_a, long long* __restrict__ naccept,
                                 long long* __restrict__ n_nan, BatchCount done, int half_p, uint32_t step_p, double a,
                                 double* __restrict__ q_p, double* __restrict__ factor_p, ProposeBox box) {
    const int64_t gid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const int64_t k = gid >> 5;
    const int t0 = (int)(gid & 31), d = en.d;
    if (gid == 0) done.report_and_rearm();
    if (k >= en.nhalf) return;
    const SplitPerm pa = make_perm(en.seed, step_a, 2 * en.nhalf, en.hb, en.randomize);
    const PendingAccept A{q_a, factor_a, lp_in, lpq_a, en.seed, step_a, half_a};
    {   // ---- the accept of slot k (k_accept, with lp written to the other buffer)
        const int64_t idx = pa(2 * k + half_a);
        double lpq_k;
        const bool take = accept_decision(A, k, idx, lpq_k);
        if (n_nan && t0 == 0 && lpq_k != lpq_k) atomicAdd(reinterpret_cast<unsigned long long*>(n_nan), 1ull);
        if (take)
            for (int t = t0; t < d; t += 32) pos[idx * d + t] = q_a[k * d + t];
        if (t0 == 0) {
            lp_out[idx] = take ? lpq_k : lp_in[idx];
            if (take && naccept) naccept[idx] += 1;
            const int64_t other = pa(2 * k + (1 - half_a));           // the walker of the resting half with this slot
            lp_out[other] = lp_in[other];
        }
    }
    // ---- the proposal of slot k for (step_p, half_p): k_propose on the positions after the pending accept
    propose_slot(en, k, t0, half_p, step_p, a, q_p, factor_p, box, [&](int64_t w) -> const double* {
        const int64_t y = pa.inv(w);
        if ((int)(y & 1) == half_a) {
            double unused;
            if (accept_decision(A, y >> 1, w, unused)) return q_a + (y >> 1) * d;
        }
        return pos + w * d;
    });
}

// Balanced sharding of a batch over the ranks (gpb_chain_emcee_run with a communicator).  A rank's contiguous share of
// the proposals holds a varying number of rows inside the prior box (256 proposals: 120 +- 8), and the step waits for the
// rank with the most — which, more often than not, needs one walker tile more than the others.  Every rank knows all
// proposals, so every rank ranks ALL live rows in order here (flags from the proposal kernel; counts of integers: any
// order) and takes the `r`-th of R equal slices of that list: rows with rank g in [r per, (r + 1) per), per =
// ceil(live / R), gathered into Xc.  The slices are padded to the collective's fixed size (per <= nhalf / R), so the
// all-gather is the one of the contiguous scheme; the accept kernels find a live row's value through rank_of (LpSource).
//   flags[nhalf] in; rank_of[nhalf] out (-1 outside the box); meta = {live, per}; cmp[0] = rows of this rank's slice,
//   cmp[4 + i] = i (the likelihood kernel's scatter list: results land densely in the send buffer)
__global__ __launch_bounds__(256) void k_balance_gather(const double* __restrict__ q, int64_t nhalf, int d,
                                                        const int* __restrict__ flags, int* __restrict__ rank_of,
                                                        int R, int r, double* __restrict__ Xc, int* __restrict__ cmp,
                                                        int* __restrict__ meta) {
    __shared__ int wsum[4], wbase[4], wtot[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t w0 = (int64_t)blockIdx.x * 256;
    int before = 0, total = 0;
    for (int64_t w = tid; w < nhalf; w += 256) {
        const int f = flags[w];
        total += f;
        if (w < w0) before += f;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        before += __shfl_xor(before, o);
        total += __shfl_xor(total, o);
    }
    const bool in = w0 + tid < nhalf && flags[w0 + tid] != 0;
    const unsigned long long m = __ballot(in);
    if (lane == 0) { wsum[wave] = __popcll(m); wbase[wave] = before; wtot[wave] = total; }
    __syncthreads();
    int off = (wbase[0] + wbase[1]) + (wbase[2] + wbase[3]);
    const int live = (wtot[0] + wtot[1]) + (wtot[2] + wtot[3]);
    for (int i = 0; i < wave; ++i) off += wsum[i];
    const int g = in ? off + __popcll(m & ((1ull << lane) - 1ull)) : -1;
    const int per = live > 0 ? (live + R - 1) / R : 1;
    const int lo = r * per, hi = min(lo + per, live);
    if (w0 + tid < nhalf) rank_of[w0 + tid] = g;
    if (g >= lo && g < hi) {
        const int64_t src = (w0 + tid) * d, dst = (int64_t)(g - lo) * d;
        for (int k = 0; k < d; ++k) Xc[dst + k] = q[src + k];
        cmp[4 + (g - lo)] = g - lo;
    }
    if (blockIdx.x == 0 && tid == 0) {
        cmp[0] = hi > lo ? hi - lo : 0;
        meta[0] = live;
        meta[1] = per;
    }
}

#ifdef GPB_DEBUG_VARIANTS
// test hooks: the generator and the draws of a (seed, step, half), for the parity tests against the oracle
__global__ void k_philox_test(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int64_t n) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t* v = in + 6 * i;
    const U4 r = philox((uint64_t)v[0] | ((uint64_t)v[1] << 32), v[2], v[3], v[4], v[5]);
    out[4 * i + 0] = r.x; out[4 * i + 1] = r.y; out[4 * i + 2] = r.z; out[4 * i + 3] = r.w;
}
__global__ void k_stretch_draws(int64_t nhalf, int half, uint64_t seed, uint32_t step, int hb, int randomize,
                                double* __restrict__ u_z, long long* __restrict__ jj, double* __restrict__ u_acc,
                                long long* __restrict__ perm) {
    const int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (k >= 2 * nhalf) return;
    perm[k] = make_perm(seed, step, 2 * nhalf, hb, randomize)(k);
    if (k >= nhalf) return;
    const U4 r = philox(seed, (uint32_t)k, step, (uint32_t)half, 0u);           // as k_propose
    u_z[k] = u01(r.x, r.y);
    jj[k] = (long long)(((uint64_t)r.z * (uint64_t)nhalf) >> 32);
    const U4 ra = philox(seed, (uint32_t)k, step, (uint32_t)half, 1u);          // as k_accept
    u_acc[k] = u01(ra.x, ra.y);
}

// test hook: out[i] = pi_step(i)
__global__ void k_perm(long long* __restrict__ out, int64_t n, uint64_t seed, uint32_t step, int hb) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = make_perm(seed, step, n, hb, 1)(i);
}
#endif  // GPB_DEBUG_VARIANTS


}  // namespace gpb

using namespace gpb;


extern "C" int gpb_stretch_propose(gpb_ctx* ctx, const double* pos_dev, int64_t nwalkers, int64_t d, int half,
                                   uint64_t seed, uint64_t step, double a, double* q_dev, double* factor_dev,
                                   int randomize_split) {
    if (!ctx || nwalkers < 2 || (nwalkers & 1) || nwalkers > (1ll << 30) || d < 1 || (half != 0 && half != 1))
        return GPB_E_ARG;
    const int64_t nh = nwalkers / 2;
    const Ensemble en{nh, (int)d, seed, half_bits(nwalkers), randomize_split ? 1 : 0};
    hipLaunchKernelGGL(k_propose, dim3((unsigned)((nh * 32 + 255) / 256)), dim3(256), 0, ctx->stream, pos_dev, en, half,
                       (uint32_t)step, a, q_dev, factor_dev, ProposeBox{});
    GPB_HIP(hipGetLastError());
    return 0;
}

extern "C" int gpb_stretch_accept(gpb_ctx* ctx, double* pos_dev, double* lp_dev, int64_t nwalkers, int64_t d,
                                  int half, uint64_t seed, uint64_t step, const double* q_dev,
                                  const double* factor_dev, const double* lpq_dev, int64_t* naccept_dev,
                                  int randomize_split) {
    if (!ctx || nwalkers < 2 || (nwalkers & 1) || nwalkers > (1ll << 30) || d < 1 || (half != 0 && half != 1))
        return GPB_E_ARG;
    const int64_t nh = nwalkers / 2;
    const Ensemble en{nh, (int)d, seed, half_bits(nwalkers), randomize_split ? 1 : 0};
    LpSource lpq{};
    lpq.lpq = lpq_dev;
    hipLaunchKernelGGL(k_accept, dim3((unsigned)((nh * 32 + 255) / 256)), dim3(256), 0, ctx->stream, pos_dev, lp_dev, en, half,
                       (uint32_t)step, q_dev, factor_dev, lpq, reinterpret_cast<long long*>(naccept_dev),
                       reinterpret_cast<long long*>(ctx->n_nan.get()), BatchCount{});
    GPB_HIP(hipGetLastError());
    return 0;
}

extern "C" int gpb_stretch_nan_count(gpb_ctx* ctx, int64_t* count_host, int reset) {
    if (!ctx || !count_host) return GPB_E_ARG;
    GPB_HIP(hipSetDevice(ctx->device));
    long long v = 0;
    GPB_HIP(hipMemcpyAsync(&v, ctx->n_nan, sizeof(v), hipMemcpyDeviceToHost, ctx->stream));
    GPB_HIP(hipStreamSynchronize(ctx->stream));
    if (reset) GPB_HIP(hipMemsetAsync(ctx->n_nan, 0, sizeof(long long), ctx->stream));
    *count_host = (int64_t)v;
    return 0;
}

// ---------------------------------------------------------------------------- device-resident sampling loop
__global__ void k_store_step(const double* __restrict__ pos, const double* __restrict__ lp, double* __restrict__ chain,
                             double* __restrict__ lpchain, int64_t nw, int d) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (chain && i < nw * d) chain[i] = pos[i];
    if (lpchain && i < nw) lpchain[i] = lp[i];
}

__global__ void k_fill(double* __restrict__ x, int64_t n, double v) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i < n) x[i] = v;
}

namespace {
// What gpb_chain_emcee_run decides before it enqueues anything: argument checks, the share of every batch this rank
// evaluates, which of the step's kernels are fused, and every workspace it needs — all of which can fail on ONE rank only
// (bad state, hipMalloc).  gpb_chain_emcee_prepare runs exactly this and nothing else, so that the ranks of a sharded run
// can agree that all of them are ready BEFORE any of them enqueues a collective the others would wait in.
struct EmceePlan {
    int64_t nh = 0, d = 0, chunk = 0, r0 = 0;
    int R = 1;
    bool sim = false, plain = false, premark = false, fuse_ap = false, balanced = false;
    int pre = 0;
    McWs mc{};                     // the proposal workspace (ctx->mc_ws)
    BalWs bal{};                   // balanced: the flags / ranks / scatter lists (ctx->bal_ws), else null
};

int emcee_plan(gpb_ctx* const* ctxs, int E, int64_t nwalkers, EmceePlan& pl) {
    gpb_ctx* ctx = ctxs[0];
    if (nwalkers < 2 || (nwalkers & 1) || nwalkers > (1ll << 30)) GPB_FAIL(GPB_E_ARG, "gpb_chain_emcee_run: nwalkers must be even, 2 .. 2^30");
    // one emulator without a parameter map may also run uncompacted (tune key 27 = 0, non-PCA modes): chain_eval's gpb_logpost
    pl.plain = E == 1 && ctx->pmap_d_in == 0 && !compaction_applies(ctx);
    int rc;
    if (pl.plain) {
        if (!ctx->have_like) GPB_FAIL(GPB_E_STATE, "gpb_emcee_run before gpb_like_set");
    } else if ((rc = chain_check(ctxs, E, "gpb_chain_emcee_run"))) {
        return rc;
    }
    GPB_HIP(hipSetDevice(ctx->device));
    const int64_t nh = nwalkers / 2, d = sampler_ndim(ctx);
    int R = ctx->comm ? ctx->nranks : 1;
    const int rank = ctx->comm ? ctx->rank : 0;
    // measurement / test hook (tune keys 26, 32): behave like rank `sim_rank` of `sim_ranks` on a single GPU — evaluate
    // that rank's nh / sim_ranks rows of every batch only (the other rows keep -inf: rejected) and still issue the collective
    pl.sim = ctx->sim_ranks > 1 && R == 1;
    if (pl.sim) R = ctx->sim_ranks;
    if (nh % R) GPB_FAIL(GPB_E_ARG, "gpb_chain_emcee_run: half the ensemble must divide evenly over the ranks");
    if (pl.sim && ctx->sim_rank >= R) GPB_FAIL(GPB_E_ARG, "gpb_chain_emcee_run: tune key 32 (simulated rank) must be below key 26 (ranks)");
    pl.nh = nh; pl.d = d; pl.R = R;
    pl.chunk = nh / R;
    pl.r0 = (pl.sim ? ctx->sim_rank : rank) * pl.chunk;
    const int64_t chunk = pl.chunk;
    for (int e = 0; e < E; ++e)                        // all workspaces now: the loop holds pointers into them
        if ((rc = ensure_wcap(ctxs[e], chunk))) { if (e) ctx->err = ctxs[e]->err; return rc; }
    if (!pl.plain && (rc = ensure_lr_blocks(ctx, E))) return rc;
    if ((rc = ctx_carve(ctx, ctx->mc_ws, [&](Carver<double>& c) { pl.mc.lay(c, nh, d); }))) return rc;
    // the gather kernel counts the flags in front of each of its workgroups itself: fine for a rank's rows of an
    // ensemble, quadratic for very large batches, which keep the marking kernel with its per-workgroup counts
    pl.premark = !pl.plain && ctx->premark && chunk <= 16384;
    // ... premark 2 (default): the proposal kernel gathers the rows as well (slots from a counter that the accept kernel
    // re-arms), no compaction kernel at all; 1: flags only, k_compact_gather follows
    pl.pre = pl.premark ? (ctx->premark >= 2 ? 2 : 1) : 0;
    // ... and with that, tune key 30 (default on): the accept of a half-step and the proposal of the next are one launch
    pl.fuse_ap = pl.pre == 2 && ctx->fuse_accept_propose;
    // sharded (or playing one rank of several): equal slices of the ordered list of ALL live rows instead of the live rows
    // of a contiguous share (k_balance_gather; tune key 36)
    // Worth its extra launch (k_balance_gather + the rank look-ups of the accept step: +11 us per half-step, measured) only
    // where the ranks' live counts straddle a walker-tile boundary often: 256 proposals per rank hold 120 +- 8 live rows, so
    // at 8 ranks three half-steps in four have a rank with a fifth 64x32 tile (+23 us, measured per tile); at 2 and 4 ranks
    // the contiguous shares rarely differ by a tile.  0 = never (default), 1 = from 8 ranks on, 2 = always.
    pl.balanced = pl.pre == 2 && R > 1 && nh <= 16384 &&
                  (ctx->balance_shards == 2 || (ctx->balance_shards == 1 && R >= 8));
    if (pl.balanced && (rc = ctx_carve(ctx, ctx->bal_ws, [&](Carver<int>& c) { pl.bal.lay(c, nh, chunk); }))) return rc;
    if (pl.pre && (rc = ensure_cmp_rows(ctx, d))) return rc;
    return 0;
}
}  // namespace

extern "C" int gpb_chain_emcee_prepare(gpb_ctx* const* ctxs, int E, int64_t nwalkers) {
    if (!chain_args_ok(ctxs, E)) return GPB_E_ARG;
    EmceePlan pl;
    return emcee_plan(ctxs, E, nwalkers, pl);
}

extern "C" int gpb_chain_emcee_run(gpb_ctx* const* ctxs, int E, double* pos_dev, double* lp_dev, int64_t nwalkers,
                                   int64_t nsteps, uint64_t seed, uint64_t step0, double a, int randomize_split,
                                   const double* lo_dev, const double* hi_dev, double outside_value, double inside_const,
                                   double* chain_dev, double* lpchain_dev, int64_t* naccept_dev) {
    if (!chain_args_ok(ctxs, E)) return GPB_E_ARG;
    gpb_ctx* ctx = ctxs[0];
    if (!pos_dev || !lp_dev || !lo_dev || !hi_dev || nsteps < 0) GPB_FAIL(GPB_E_ARG, "gpb_chain_emcee_run: null pointer or negative size");
    EmceePlan pl;
    int rc = emcee_plan(ctxs, E, nwalkers, pl);
    if (rc) return rc;
    const int64_t nh = pl.nh, d = pl.d, chunk = pl.chunk, r0 = pl.r0;
    const int R = pl.R, pre = pl.pre;
    const bool sim = pl.sim, plain = pl.plain, premark = pl.premark, fuse_ap = pl.fuse_ap, balanced = pl.balanced;
    double *const *qs = pl.mc.q, *const *factors = pl.mc.factor, *const *lpqs = pl.mc.lpq, *lp2 = pl.mc.lp2;
    const Ensemble en{nh, (int)d, seed, half_bits(nwalkers), randomize_split ? 1 : 0};
    const dim3 g32((unsigned)((nh * 32 + 255) / 256));
    int *const *bal_flags = pl.bal.flags, *const *bal_rank = pl.bal.rank, *const *bal_cmp = pl.bal.cmp, *const *bal_meta = pl.bal.meta;
    if (balanced) GPB_HIP(hipMemsetAsync(ctx->bal_ws, 0, sizeof(int) * (size_t)pl.bal.n, ctx->stream));
    if (pre) GPB_HIP(hipMemsetAsync(ctx->cmp_idx, 0, 2 * sizeof(int), ctx->stream));
    if (sim) hipLaunchKernelGGL(k_fill, dim3((unsigned)((pl.mc.n_sets + 255) / 256)), dim3(256), 0, ctx->stream, qs[0], pl.mc.n_sets,
                                -INFINITY);
    unsigned long long* const live = pre == 2 && ctx->profile ? ctx->rows_live : (unsigned long long*)nullptr;
    double* lp_cur = lp_dev;                           // fuse_ap: lp alternates between the caller's vector and lp2
    double* lp_alt = lp2;
    const int64_t nhalfsteps = 2 * nsteps;
    // the counter + index list of the rows inside the box of the batch in buffer set b: two views one int apart, so that the
    // fused kernel can re-arm the finished batch's counter while it fills the next one's
    auto cmp_view = [&](int b) { return balanced ? bal_cmp[b] : (ctx->cmp_idx ? ctx->cmp_idx + b : (int*)nullptr); };
    // What the proposal kernel does beside proposing, for the batch in buffer set b.  balanced: the flags of every row,
    // k_balance_gather ranks them and takes this rank's slice; premark: the prior-box test of this rank's rows, with their
    // flags for k_compact_gather (1) or gathered at once (2); else nothing.
    auto propose_box = [&](int b) {
        ProposeBox box{};
        if (!balanced && !premark) return box;
        box.lo = lo_dev; box.hi = hi_dev; box.outside = outside_value;
        if (balanced) {
            box.flags = bal_flags[b]; box.chunk = nh;
        } else {
            box.ll = lpqs[b]; box.r0 = r0; box.chunk = chunk;
            if (pre == 1) box.flags = ctx->cmp_idx + 4 + ctx->Wcap;
            if (pre == 2) { box.Xc = ctx->cmp_X; box.cmp = cmp_view(b); }
        }
        return box;
    };
    for (int64_t g = 0; g < nhalfsteps; ++g) {
        const int64_t n = g >> 1;
        const int half = (int)(g & 1), b = fuse_ap ? (int)(g & 1) : 0;
        const uint32_t step = (uint32_t)(step0 + (uint64_t)n);
        double *q = qs[b], *factor = factors[b], *lpq = lpqs[b];
        int* cmpv = cmp_view(b);
        // where the accept step finds this batch's log-probabilities, and the batch's counter it re-arms
        const LpSource lp_src{lpq, bal_rank[b], bal_meta[b], chunk, outside_value};
        BatchCount done{};
        if (pre == 2) done = BatchCount{cmpv, ctx->live_hint, chunk, live};
        if (!fuse_ap || g == 0)
            hipLaunchKernelGGL(k_propose, g32, dim3(256), 0, ctx->stream, pos_dev, en, half, step, a, q, factor, propose_box(b));
        if (balanced)
            hipLaunchKernelGGL(k_balance_gather, dim3((unsigned)((nh + 255) / 256)), dim3(256), 0, ctx->stream, q, nh, (int)d,
                               bal_flags[b], bal_rank[b], R, (int)(r0 / chunk), ctx->cmp_X, cmpv, bal_meta[b]);
        // this rank's rows of the batch: [compaction to the rows inside the box,] per emulator K*^T + mean partials,
        // V = L^-1 K*^T with the fused sum of squares, block log-likelihood (+ prior box + constant)
        if (plain) {
            if ((rc = chain_eval(ctxs, E, q + r0 * d, chunk, lpq + r0, lo_dev, hi_dev, outside_value, inside_const))) return rc;
        } else if ((rc = chain_rows(ctxs, E, q + r0 * d, chunk, lpq + r0, lo_dev, hi_dev, outside_value, inside_const, pre,
                                    cmpv))) {
            return rc;
        }
        if (sim ? ctx->comm != nullptr : R > 1)                      // in place, on this stream
            if ((rc = gpb_dist_allgather(ctx, lpq + r0, lpq, chunk))) return rc;
        if (fuse_ap && g + 1 < nhalfsteps) {
            const int64_t g1 = g + 1;
            hipLaunchKernelGGL(k_accept_propose, g32, dim3(256), 0, ctx->stream, pos_dev, lp_cur, lp_alt, en, half, step, q, factor,
                               lp_src, reinterpret_cast<long long*>(naccept_dev), reinterpret_cast<long long*>(ctx->n_nan.get()), done,
                               (int)(g1 & 1), (uint32_t)(step0 + (uint64_t)(g1 >> 1)), a, qs[1 - b], factors[1 - b],
                               propose_box(1 - b));
            double* sw = lp_cur; lp_cur = lp_alt; lp_alt = sw;
        } else {
            hipLaunchKernelGGL(k_accept, g32, dim3(256), 0, ctx->stream, pos_dev, lp_cur, en, half, step, q, factor, lp_src,
                               reinterpret_cast<long long*>(naccept_dev), reinterpret_cast<long long*>(ctx->n_nan.get()), done);
        }
        if (half == 1 && (chain_dev || lpchain_dev))
            hipLaunchKernelGGL(k_store_step, dim3((unsigned)((nwalkers * d + 255) / 256)), dim3(256), 0, ctx->stream, pos_dev,
                               lp_cur, chain_dev ? chain_dev + n * nwalkers * d : nullptr,
                               lpchain_dev ? lpchain_dev + n * nwalkers : nullptr, nwalkers, (int)d);
    }
    if (lp_cur != lp_dev)
        GPB_HIP(hipMemcpyAsync(lp_dev, lp_cur, sizeof(double) * (size_t)nwalkers, hipMemcpyDeviceToDevice, ctx->stream));
    GPB_HIP(hipGetLastError());
    return 0;
}


extern "C" int gpb_emcee_run(gpb_ctx* ctx, double* pos_dev, double* lp_dev, int64_t nwalkers, int64_t nsteps,
                             uint64_t seed, uint64_t step0, double a, int randomize_split, const double* lo_dev,
                             const double* hi_dev, double outside_value, double inside_const, double* chain_dev,
                             double* lpchain_dev, int64_t* naccept_dev) {
    if (!ctx) return GPB_E_ARG;
    if (ctx->pmap_d_in > 0 && !compaction_applies(ctx))
        GPB_FAIL(GPB_E_STATE, "gpb_emcee_run: an emulator with a parameter map needs the block likelihood kernels");
    gpb_ctx* one[1] = {ctx};
    return gpb_chain_emcee_run(one, 1, pos_dev, lp_dev, nwalkers, nsteps, seed, step0, a, randomize_split, lo_dev, hi_dev,
                               outside_value, inside_const, chain_dev, lpchain_dev, naccept_dev);
}

#ifdef GPB_DEBUG_VARIANTS      // test hooks (include/gpbayes_debug.h)
extern "C" int gpb_test_split_perm(gpb_ctx* ctx, int64_t n, uint64_t seed, uint64_t step, int64_t* out_dev) {
    if (!ctx || n < 2 || n > (1ll << 30) || !out_dev) return GPB_E_ARG;
    hipLaunchKernelGGL(k_perm, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream,
                       reinterpret_cast<long long*>(out_dev), n, seed, (uint32_t)step, half_bits(n));
    GPB_HIP(hipGetLastError());
    return 0;
}

extern "C" int gpb_test_philox(gpb_ctx* ctx, int64_t n, const uint32_t* in_host, uint32_t* out_host) {
    if (!ctx || n < 1 || n > (1 << 20) || !in_host || !out_host) return GPB_E_ARG;
    GPB_HIP(hipSetDevice(ctx->device));
    uint32_t *din = nullptr, *dout = nullptr;
    GPB_HIP(hipMalloc(&din, sizeof(uint32_t) * 6 * n));
    GPB_HIP(hipMalloc(&dout, sizeof(uint32_t) * 4 * n));
    GPB_HIP(hipMemcpy(din, in_host, sizeof(uint32_t) * 6 * n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_philox_test, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, din, dout, n);
    hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = hipMemcpy(out_host, dout, sizeof(uint32_t) * 4 * n, hipMemcpyDeviceToHost);
    (void)hipFree(din); (void)hipFree(dout);
    GPB_HIP(e);
    return 0;
}

extern "C" int gpb_test_stretch_draws(gpb_ctx* ctx, int64_t nwalkers, int half, uint64_t seed, uint64_t step,
                                      int randomize_split, double* u_z_dev, int64_t* j_dev, double* u_acc_dev,
                                      int64_t* perm_dev) {
    if (!ctx || nwalkers < 2 || (nwalkers & 1) || nwalkers > (1ll << 30) || (half != 0 && half != 1) || !u_z_dev ||
        !j_dev || !u_acc_dev || !perm_dev)
        return GPB_E_ARG;
    hipLaunchKernelGGL(k_stretch_draws, dim3((unsigned)((nwalkers + 255) / 256)), dim3(256), 0, ctx->stream,
                       nwalkers / 2, half, seed, (uint32_t)step, half_bits(nwalkers), randomize_split ? 1 : 0, u_z_dev,
                       reinterpret_cast<long long*>(j_dev), u_acc_dev, reinterpret_cast<long long*>(perm_dev));
    GPB_HIP(hipGetLastError());
    return 0;
}
#endif  // GPB_DEBUG_VARIANTS
