// gpb_chain.hip — the log-posterior of a chain of emulators: what every sampler and the gradient evaluate.
//   Chain._predict concatenates the emulators' observables and the covariance is block-diagonal over them
//   (src/mcmc.py:153-166), so the log-likelihood is the sum of the emulators' blocks; all emulators see the same rows of
//   the same parameter space (those with a parameter map, src/emulator.py:492-551, through gpb_param_map).
//   chain_ctx_check   what every entry point that takes a list of contexts asks of it
//   chain_rows        the compacted chain call: the rows inside the prior box only, the emulators' launches batched
//   chain_rows_sets   chain_rows for rows that belong to different data sets (gpb_chain_like_sets; gpb_sets.hip)
//   chain_eval        the chain call where it applies, else the per-emulator sequence
#include "gpb_internal.h"

namespace gpb {
namespace {
// parameters of the CHAIN (a parameter map's d_in; the GPs' own d is bounded by 64 in gpb_gp_set).  The proposal kernels
// take any number; k_compact_mark stages 256 rows of it in LDS in tiles, so the bound is only a sanity limit.
constexpr int64_t MAX_CHAIN_NDIM = 512;

// Why not (why == nullptr: no objection).  `why` continues the caller's name.
struct ChainRefusal {
    int code;
    const char* why;
};
// the contexts can be evaluated as one chain: same device, stream and parameter space; likelihood installed
ChainRefusal ctx_refusal(gpb_ctx* const* ctxs, int E, bool need_like) {
    const gpb_ctx* c0 = ctxs[0];
    for (int e = 0; e < E; ++e) {
        const gpb_ctx* c = ctxs[e];
        if (!c) return {GPB_E_ARG, ": null context"};
        if (need_like && !c->have_like) return {GPB_E_STATE, " before gpb_like_set"};
        if (c->device != c0->device || c->stream != c0->stream)
            return {GPB_E_STATE, ": the emulators' contexts must share one device and stream"};
        if (sampler_ndim(c) != sampler_ndim(c0)) return {GPB_E_ARG, ": the emulators disagree on the number of parameters"};
        if (c->pmap_d_in > 0 && c->pmap_d_out != c->d) return {GPB_E_STATE, ": a parameter map's output must be the GPs' input"};
    }
    return {0, nullptr};
}
// ... and the compacted chain path admits them: a block likelihood kernel applies to every emulator
ChainRefusal chain_refusal(gpb_ctx* const* ctxs, int E) {
    const ChainRefusal r = ctx_refusal(ctxs, E, true);
    if (r.why) return r;
    for (int e = 0; e < E; ++e)
        if (!compaction_applies(ctxs[e]))
            return {GPB_E_STATE, ": needs the block likelihood kernels (PCA mode, M <= 64 or npc <= 16) for every emulator"};
    if (sampler_ndim(ctxs[0]) > MAX_CHAIN_NDIM) return {GPB_E_ARG, ": more than 512 chain parameters"};
    return {0, nullptr};
}
int refuse(gpb_ctx* ctx, const char* who, const ChainRefusal& r) {
    if (r.why) GPB_FAIL(r.code, std::string(who) + r.why);
    return 0;
}
}  // namespace

int chain_ctx_check(gpb_ctx* const* ctxs, int E, const char* who, bool need_like) {
    return refuse(ctxs[0], who, ctx_refusal(ctxs, E, need_like));
}
int chain_check(gpb_ctx* const* ctxs, int E, const char* who) { return refuse(ctxs[0], who, chain_refusal(ctxs, E)); }

// Passes (1) and (2) of a compacted chain batch (chain_rows has the list), over the rows gathered in ctxs[0]->cmp_X
static int chain_predict_passes(gpb_ctx* const* ctxs, int E, int64_t W, const int* cmpv) {
    gpb_ctx* c0 = ctxs[0];
    int rc;
    const double* Xg[MAX_CHAIN_CTX];
    gpb_ctx* mapped[MAX_CHAIN_CTX];
    int nmapped = 0;
    for (int e = 0; e < E; ++e) {
        gpb_ctx* c = ctxs[e];
        Xg[e] = c0->cmp_X;
        c->hint_from = c0;
        if (c->pmap_d_in > 0) {                        // this emulator's GPs see the PCA-reduced parameters
            mapped[nmapped++] = c;
            Xg[e] = c->Xs;
        }
    }
    if (nmapped > 1 && c0->chain_batch) {              // the maps of all mapped emulators over the gathered rows: one launch
        if ((rc = launch_param_maps(mapped, nmapped, c0->cmp_X, W))) { c0->err = mapped[0]->err; return rc; }
    } else {
        for (int i = 0; i < nmapped; ++i)
            if ((rc = gpb_param_map(mapped[i], c0->cmp_X, W, mapped[i]->Xs))) { c0->err = mapped[i]->err; return rc; }
    }
    for (int e = 0; e < E;) {              // K*^T: one launch per run of emulators of equal padded size and PADDED input
        int n = 1;                                     // count (parameterTrafoPCA emulators keep 17-19 of 20 inputs each: one launch)
        while (c0->chain_batch && e + n < E && ctxs[e + n]->Np == ctxs[e]->Np && ctxs[e + n]->dpad == ctxs[e]->dpad && n < 32) ++n;
        if ((rc = launch_kcross_group(ctxs + e, Xg + e, n, W, cmpv))) { c0->err = ctxs[e]->err; return rc; }
        e += n;
    }
    for (int e = 0; e < E;) {
        int n = 1, gps = (int)ctxs[e]->P;
        while (c0->chain_batch && e + n < E && ctxs[e + n]->Np == ctxs[e]->Np && gps + (int)ctxs[e + n]->P <= GPB_MAX_MULTI_GP) {
            gps += (int)ctxs[e + n]->P;
            ++n;
        }
        if ((rc = launch_vsq(ctxs + e, n, W, cmpv))) { c0->err = ctxs[e]->err; return rc; }
        e += n;
    }
    return 0;
}

// log-posterior of rows X[W][ndim] over all emulators, rows inside the box only (ctxs[0] owns the compaction)
int chain_rows(gpb_ctx* const* ctxs, int E, const double* X_dev, int64_t W, double* ll_dev, const double* lo_dev,
               const double* hi_dev, double outside, double inside_const, int premarked, const int* cmpv) {
    gpb_ctx* c0 = ctxs[0];
    int rc;
    if ((rc = coupling_check(ctxs, E, "gpb_chain_logpost"))) return rc;
    for (int e = 0; e < E; ++e)
        if ((rc = ensure_wcap(ctxs[e], W))) { if (e) c0->err = ctxs[e]->err; return rc; }
    if ((rc = ensure_lr_blocks(c0, E))) return rc;
    if ((rc = launch_compact(c0, X_dev, W, sampler_ndim(c0), lo_dev, hi_dev, outside, ll_dev, premarked))) return rc;
    if (!cmpv) cmpv = c0->cmp_idx;                     // (count, -, -, -, indices ...) of the rows inside the box
    // Three passes over the emulators (each kernel sees what it would see in its own emulator's sequence: same bits):
    // (1) parameter maps, then K*^T and the mean partials — ONE launch per run of emulators of equal padded size
    //     (k_kcross_multi);
    // (2) V = L^-1 K*^T with the fused sum of squares: ONE launch for each run of emulators whose designs pad to the same
    //     Np (the reference's analyses: nine emulators on one design) instead of one partly filled launch per emulator;
    // (3) the block log-likelihoods, added up in emuList order: one launch that walks the emulators (k_loglike_lowrank_multi)
    //     when every block takes the low-rank kernel, else one launch per emulator.  A chain whose experimental covariance
    //     couples its emulators (gpb_chain_like_set) has no blocks to add: the GPs' sums per emulator (k_finalize), then
    //     one launch of the joint kernel (gpb_coupled.hip).
    if ((rc = chain_predict_passes(ctxs, E, W, cmpv))) return rc;
    if (coupling_installed(c0)) {
        for (int e = 0; e < E; ++e)
            if ((rc = launch_finalize(ctxs[e], W, true))) { c0->err = ctxs[e]->err; return rc; }
        return launch_loglike_coupled(ctxs, E, W, ll_dev, cmpv, inside_const);
    }
    bool taken;
    if ((rc = launch_loglike_lowrank_chain(ctxs, E, W, ll_dev, cmpv, inside_const, &taken)) || taken) return rc;
    for (int e = 0; e < E; ++e) {
        gpb_ctx* c = ctxs[e];
        const bool fused = loglike_fuses_finalize(c, W);
        if ((!fused && (rc = launch_finalize(c, W, true))) ||
            (rc = launch_loglike(c, W, ll_dev, e > 0, fused, nullptr, nullptr, nullptr, outside,
                                 e == E - 1 ? inside_const : 0.0, cmpv))) {
            c0->err = c->err;
            return rc;
        }
    }
    return 0;
}

// chain_rows for rows that belong to different data sets (row w: set w / rows_per_set of gpb_chain_like_sets' tables): the
// same compaction and passes (1)-(2) — the prediction does not depend on the data — then the sets' likelihood kernel
int chain_rows_sets(gpb_ctx* const* ctxs, int E, const double* X_dev, int64_t W, int64_t rows_per_set, double* ll_dev,
                    const double* lo_dev, const double* hi_dev, double outside, double inside_const, int premarked, const int* cmpv) {
    gpb_ctx* c0 = ctxs[0];
    int rc;
    for (int e = 0; e < E; ++e)
        if ((rc = ensure_wcap(ctxs[e], W))) { if (e) c0->err = ctxs[e]->err; return rc; }
    if ((rc = ensure_lr_blocks(c0, E))) return rc;
    if ((rc = launch_compact(c0, X_dev, W, sampler_ndim(c0), lo_dev, hi_dev, outside, ll_dev, premarked))) return rc;
    if (!cmpv) cmpv = c0->cmp_idx;
    if ((rc = chain_predict_passes(ctxs, E, W, cmpv))) return rc;
    return launch_loglike_lowrank_sets(ctxs, E, W, rows_per_set, ll_dev, cmpv, inside_const);
}

int sets_check(gpb_ctx* const* ctxs, int E, int64_t nsets, const char* who) {
    gpb_ctx* ctx = ctxs[0];
    int rc = chain_check(ctxs, E, who);
    if (rc) return rc;
    if ((rc = lowrank_sets_check(ctxs, E, who))) return rc;
    for (int e = 0; e < E; ++e)
        if (ctxs[e]->lrs_K < 1 || ctxs[e]->lrs_K != ctx->lrs_K)
            GPB_FAIL(GPB_E_STATE, std::string(who) + " before gpb_chain_like_sets (a new gpb_like_set drops its tables)");
    if (nsets > ctx->lrs_K) GPB_FAIL(GPB_E_ARG, std::string(who) + ": more data sets than gpb_chain_like_sets installed");
    return 0;
}

// The C counterpart of Chain.log_prob_device (mcmc.py), which makes the same per-emulator sequence of public calls from
// Python (use_chain_call = False: what the tests compare this against); a change of the rule goes into both.
int chain_eval(gpb_ctx* const* ctxs, int E, const double* X, int64_t W, double* lp, const double* lo, const double* hi,
               double outside, double inside_const) {
    if (gpb_chain_supported(ctxs, E) == 1) return gpb_chain_logpost(ctxs, E, X, W, lp, lo, hi, outside, inside_const);
    if (coupling_installed(ctxs[0])) {                 // the sum of the emulators' blocks below is not this chain's likelihood
        gpb_ctx* ctx = ctxs[0];
        GPB_FAIL(GPB_E_STATE, "gpb: a coupled chain likelihood is installed (gpb_chain_like_set), but the contexts no longer "
                              "take the compacted chain call");
    }
    // The sum of the emulators' block likelihoods in emuList order (accumulate from the second on), the prior box over the
    // ORIGINAL parameters with the last: gpb_logpost, or gpb_loglike + gpb_box_finish where the last emulator's GPs see mapped
    // parameters.  Those go into the emulator's own staging buffer, as in chain_rows (sized here, on the caller's device).
    gpb_ctx* c0 = ctxs[0];
    const int64_t nd = sampler_ndim(c0);
    int rc = 0;
    for (int e = 0; e < E && !rc; ++e) {
        gpb_ctx* c = ctxs[e];
        const bool mapped = c->pmap_d_in > 0, last = e == E - 1;
        if (mapped) {
            if (!(rc = ensure_wcap(c, W)) && !(rc = gpb_param_map(c, X, W, c->Xs)) &&
                !(rc = gpb_loglike(c, c->Xs, W, 1, lp, e > 0, nullptr)) && last)
                rc = gpb_box_finish(c, X, W, nd, lo, hi, outside, inside_const, lp);
        } else {
            rc = last ? gpb_logpost(c, X, W, lp, e > 0, lo, hi, outside, inside_const) : gpb_loglike(c, X, W, 1, lp, e > 0, nullptr);
        }
        if (rc) c0->err = c->err;
    }
    return rc;
}

}  // namespace gpb

using namespace gpb;

extern "C" int gpb_chain_supported(gpb_ctx* const* ctxs, int E) {
    if (!chain_args_ok(ctxs, E)) return GPB_E_ARG;
    int n = 1;
    while (n < E && ctxs[n]) ++n;                      // the contexts before the first null one are judged first, in order
    if (chain_refusal(ctxs, n).why) return 0;
    return n < E ? GPB_E_ARG : 1;                      // a null context is the caller's error, all else an answer
}

extern "C" int gpb_chain_logpost(gpb_ctx* const* ctxs, int E, const double* Xs_dev, int64_t W, double* ll_dev,
                                 const double* lo_dev, const double* hi_dev, double outside_value, double inside_const) {
    if (!chain_args_ok(ctxs, E)) return GPB_E_ARG;
    gpb_ctx* ctx = ctxs[0];
    if (!Xs_dev || !ll_dev || !lo_dev || !hi_dev || W < 0) GPB_FAIL(GPB_E_ARG, "gpb_chain_logpost: null pointer or negative size");
    int rc = chain_check(ctxs, E, "gpb_chain_logpost");
    if (rc) return rc;
    if (W == 0) return 0;
    GPB_HIP(hipSetDevice(ctx->device));
    return chain_rows(ctxs, E, Xs_dev, W, ll_dev, lo_dev, hi_dev, outside_value, inside_const);
}
