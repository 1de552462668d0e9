"""
Does the calibrated model describe the data, data set by data set: chi2 per emulator and per degree of freedom with the full
covariance the likelihood uses, over ALL samples of a chain on the device (gpb_gof_accumulate, gpb_chi2_sf, gpb_gof_influence;
DESIGN.md section 27).

The reference computes 1/2 dY^T C^-1 dY and sum ln L_ii in mvn_loglike (src/mcmc.py:23-65), adds them up over all emulators and
returns one number; examples/ClosureTest.ipynb judges the fit by eye from fifteen predictive curves, and the per-observable PIT of
Chain.posterior_predictive ignores every correlation (the PCA emulators' off-diagonal predictive covariance, the truncation term,
a coupled expdata_cov).  Here the two pieces are kept per row and emulator, with the whitened residuals z = L^-1 dY, the marginal
pulls, the closed-form posterior-predictive p-value Q(M / 2, chi2 / 2) and the importance weights of the posterior without one
data set.

No [S, nobs, nobs] or [S, nobs] array reaches the host: per slab and emulator the mean and the covariance are formed on the
device and reduced there; chi2 and ll stay on the device as [E, S].
"""
import numpy as np


class DataSetInfluence:
    """What the posterior would look like WITHOUT data set e, estimated by importance reweighting of the rows at hand with
    w_s = wt_s exp(-ll_e(s)) (gpb_gof_influence) — no second run:
      ess [E]            (sum w)^2 / sum w^2, in rows: the effective number of rows behind the estimate for data set e
      shift [E, ndim]    (mean without e - mean) / std, per parameter
      scale [E, ndim]    std without e / std
    mean and std are the weighted ones of the rows used (finite ll_e, non-zero weight).  The estimate is as good as its ess: a
    data set that dominates the likelihood leaves a handful of rows with all the weight, and shift and scale are then noise.  ess
    tells when that has happened; no threshold is applied here."""

    def __init__(self, ess, shift, scale, names=None):
        self.ess, self.shift, self.scale = ess, shift, scale
        self.names = None if names is None else list(names)

    def __repr__(self):
        return "DataSetInfluence(emulators=%d, ndim=%d, ess=%s)" % (self.shift.shape[0], self.shift.shape[1],
                                                                    np.array2string(self.ess, precision=1))


class GofTotal:
    """The chain's emulators taken together (GoodnessOfFit.total): n_bad, ndf, chi2_mean, chi2_quantiles [nq], chi2_min,
    chi2_min_index, chi2_min_params [ndim], ppp; joint: True when chi2 is that of the joint matrix of a coupled expdata_cov,
    False when it is the sum of the emulators' blocks."""

    def __init__(self, n_bad, ndf, chi2_mean, chi2_quantiles, chi2_min, chi2_min_index, chi2_min_params, ppp, joint):
        self.n_bad, self.ndf, self.chi2_mean, self.chi2_quantiles = int(n_bad), int(ndf), float(chi2_mean), chi2_quantiles
        self.chi2_min, self.chi2_min_index, self.chi2_min_params = float(chi2_min), int(chi2_min_index), chi2_min_params
        self.ppp, self.joint = float(ppp), bool(joint)


class GoodnessOfFit:
    """posterior_gof's result, E emulators (data sets), nobs observables in emuList order:
      n_samples            rows given;  n_bad [E]: rows whose covariance block had a non-positive pivot (left out of that emulator)
      ndf [E]              the NUMBER OF OBSERVABLES of the data set.  No fitted parameters are subtracted: the chi2 here is the
                           posterior's — one value per sample, with the emulator's predictive covariance inside C — not a
                           minimum, and under the model chi2 of a sample is chi2-distributed with M degrees of freedom
      quantiles [nq]       the levels;  chi2_quantiles [E, nq]: np.percentile's linear rule over the rows with a finite chi2,
                           UNWEIGHTED also when weights are given;  chi2_mean [E]: the weighted mean
      chi2_min [E], chi2_min_index [E], chi2_min_params [E, ndim]   the best row per data set
      ppp [E]              weighted mean over the rows of p = Q(M / 2, chi2 / 2): the posterior-predictive p-value of the chi2
                           discrepancy in closed form.  Near 0: the data set is not described; near 1: the covariance is too wide
      total                a GofTotal, or None with total_reason (a coupled chain with more than 2048 observables)
      resid_mean, resid_rms [nobs]   weighted mean and root mean square of the whitened sequential residuals z = L^-1 dY: z_m is
                           the residual of observable m given observables 0 .. m - 1 of its data set, N(0, 1) under the model
      pull_mean, pull_rms [nobs]     the same of the marginal pulls dY_m / sqrt(C_mm)
      influence            a DataSetInfluence, or None (not asked for, or a coupled expdata_cov: the blocks are then not
                           independent factors of the likelihood)
      rows                 with return_rows: dict of host arrays chi2 [S, E], loglike [S, E] (mvn_loglike's value per data set,
                           without the 2 pi constant), chi2_total [S], loglike_total [S]; NaN where a row was bad or had weight 0
    With a coupled expdata_cov the per-emulator entries are the valid MARGINAL checks of each data set (its own block of the
    covariance); total is then the chi2 of the joint matrix, not the sum of the blocks."""

    def __init__(self, n_samples, n_bad, ndf, quantiles, chi2_mean, chi2_quantiles, chi2_min, chi2_min_index, chi2_min_params,
                 ppp, total, total_reason, resid_mean, resid_rms, pull_mean, pull_rms, influence=None, rows=None, names=None):
        self.n_samples, self.n_bad, self.ndf = int(n_samples), np.asarray(n_bad, dtype=np.int64), np.asarray(ndf, dtype=np.int64)
        self.quantiles, self.chi2_mean, self.chi2_quantiles = quantiles, chi2_mean, chi2_quantiles
        self.chi2_min, self.chi2_min_index, self.chi2_min_params = chi2_min, chi2_min_index, chi2_min_params
        self.ppp, self.total, self.total_reason = ppp, total, total_reason
        self.resid_mean, self.resid_rms, self.pull_mean, self.pull_rms = resid_mean, resid_rms, pull_mean, pull_rms
        self.influence, self.rows = influence, rows
        self.names = None if names is None else list(names)

    def _band(self, quant, ndf):
        """(median, lo, hi) of chi2 / ndf from the levels 0.5, 0.16 and 0.84 where they are among the quantiles"""
        q = np.asarray(self.quantiles)
        out = []
        for lvl in (0.5, 0.16, 0.84):
            k = np.flatnonzero(np.abs(q - lvl) < 1e-12)
            out.append(float(quant[k[0]]) / ndf if k.size else float("nan"))
        return out

    def __repr__(self):
        E = len(self.ndf)
        lines = ["GoodnessOfFit(n_samples=%d, emulators=%d, nobs=%d, n_bad=%s)"
                 % (self.n_samples, E, int(self.ndf.sum()), self.n_bad.tolist()),
                 "  %-14s %5s  %-32s %s" % ("data set", "ndf", "chi2/ndf (median, 68 %)", "ppp")]
        for e in range(E):
            med, lo, hi = self._band(self.chi2_quantiles[e], float(self.ndf[e]))
            lines.append("  %-14s %5d  %7.3f  [%7.3f, %7.3f]         %.4f" % ("emulator %d" % e, self.ndf[e], med, lo, hi, self.ppp[e]))
        if self.total is not None:
            med, lo, hi = self._band(self.total.chi2_quantiles, float(self.total.ndf))
            lines.append("  %-14s %5d  %7.3f  [%7.3f, %7.3f]         %.4f"
                         % ("total (joint)" if self.total.joint else "total", self.total.ndf, med, lo, hi, self.total.ppp))
        else:
            lines.append("  total: none (%s)" % self.total_reason)
        return "\n".join(lines)


def slab_rows(chain, joint=0):
    """rows of one slab: from max_e 8 (P_e N_e + M_e^2 + 2 M_e) bytes per row — with a joint matrix of `joint` observables
    8 joint^2 more — by the rule of sensitivity.slab_rows (at most 2^15 rows), a multiple of 256; chain.gof_slab_rows overrides
    it (rounded down to a multiple of 256, at least 256)"""
    per_row = max(8 * (e._ngp * e._X_train.shape[0] + e.nobs * e.nobs + 2 * e.nobs) for e in chain.emuList) + 8 * joint * (joint + 1)
    slab = max(int(min(max((8 << 30) // per_row, 1024), 1 << 15)) // 256 * 256, 256)
    if getattr(chain, "gof_slab_rows", None) is not None:
        slab = max(int(chain.gof_slab_rows) // 256 * 256, 256)
    return slab


def _order_stats(e0, T, q):
    """per row of the device array T [R, S], over its finite entries: (mean [R], quantiles [R, nq] by np.percentile's linear
    rule, min [R], argmin [R] into the S columns, n_used [R]) — gpb_ppd_summary's moments and order statistics; rows with
    non-finite entries are compacted first"""
    import torch
    from .emulator import percentile_from_order
    R, S = int(T.shape[0]), int(T.shape[1])
    fin = torch.isfinite(T)
    mean, quant, n_used = np.full(R, np.nan), np.full((R, q.shape[0]), np.nan), np.zeros(R, dtype=np.int64)
    if bool(fin.all()):
        out = e0.ppd_summary(T, None, q)
        mean[:], quant[:], n_used[:] = out["moments"][:, 0], percentile_from_order(out["order"], q, S), S
    else:
        for r in range(R):
            v = T[r][fin[r]].contiguous()
            n_used[r] = int(v.shape[0])
            if n_used[r]:
                out = e0.ppd_summary(v[None, :], None, q)
                mean[r], quant[r] = out["moments"][0, 0], percentile_from_order(out["order"], q, n_used[r])[0]
    mn, arg = torch.where(fin, T, torch.full_like(T, float("inf"))).min(dim=1)
    return mean, quant, mn.cpu().numpy(), arg.cpu().numpy(), n_used


def posterior_gof(chain, X, weights=None, quantiles=(0.05, 0.16, 0.5, 0.84, 0.95), influence=True, return_rows=False, profile=None):
    """GoodnessOfFit of the rows X [S, ndim] (weights [S]: non-negative, not all zero) for the emulators and the experiment of
    `chain`.  Slab by slab (a multiple of 256 rows), emulator by emulator in emuList order: gpb_emu_predict (mean and covariance
    on the device; the rows mapped on the host for parameterTrafoPCA emulators, as Chain._ppd_arrays maps them), then
    gpb_gof_accumulate with that emulator's slice of expdata and its diagonal block of expdata_cov.  chi2 and ll stay on the
    device as [E, S]; their quantiles and means come from gpb_ppd_summary, the totals over the emulators from a loop in emuList
    order and gpb_chi2_sf, the influence of each data set from gpb_gof_influence.  Equal inputs give equal bits, whatever the slab
    size.  A coupled expdata_cov: the emulators' blocks as before (marginal checks), total from one gpb_gof_accumulate per slab on
    the joint [W, nobs, nobs] matrix with the full expdata_cov (nobs <= 2048, else total is None), influence None.
    profile: a dict that receives the milliseconds of the phases "predict", "accumulate" (events on the stream) and "summary".
    NotImplementedError for foreign emulators and a chain sharded over several ranks; ValueError for wrong shapes, non-finite
    rows, negative or all-zero weights, quantile levels outside [0, 1]."""
    import torch
    from .engine import GPEngine
    if not chain._native():
        raise NotImplementedError("goodness_of_fit needs every emulator of the chain to be this package's Emulator (foreign "
                                  "emulators expose no GP state to predict from on the device)")
    if chain.sharding is not None and getattr(chain.sharding, "world", 1) > 1:
        raise NotImplementedError("goodness_of_fit: a chain sharded over several ranks is not supported; call it on one rank "
                                  "(shard_over(None))")
    X = np.asarray(X, dtype=np.float64)
    if X.ndim != 2 or X.shape[1] != chain.ndim or X.shape[0] < 1:
        raise ValueError("goodness_of_fit: samples must be [S, %d], got %s" % (chain.ndim, X.shape))
    if not np.all(np.isfinite(X)):
        raise ValueError("goodness_of_fit: samples hold non-finite values")
    X = np.ascontiguousarray(X)
    S, d = X.shape
    w = None
    if weights is not None:
        w = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).reshape(-1))
        if w.shape[0] != S or not np.all(np.isfinite(w)) or np.any(w < 0.0) or not w.max() > 0.0:
            raise ValueError("goodness_of_fit: weights [%d] finite, non-negative, not all zero" % S)
    q = np.ascontiguousarray(np.atleast_1d(np.asarray(quantiles, dtype=np.float64)).reshape(-1))
    if q.shape[0] < 1 or q.shape[0] > GPEngine.PPD_MAX_LEVELS or not np.all((q >= 0.0) & (q <= 1.0)):
        raise ValueError("goodness_of_fit: 1 to %d quantile levels in [0, 1]" % GPEngine.PPD_MAX_LEVELS)
    if influence and d > GPEngine.GOF_MAX_D:
        raise ValueError("goodness_of_fit: influence takes at most %d parameters" % GPEngine.GOF_MAX_D)
    chain._prepare_blocks()
    coupled = bool(chain._coupled)
    dev = torch.device("cuda", chain.device or 0)
    engs = [e._engine_ready() for e in chain.emuList]
    for g in engs:
        g._need_data()
        g._track_stream()
    e0 = engs[0]
    E = len(engs)
    if influence and not coupled and E > GPEngine.GOF_MAX_E:
        raise ValueError("goodness_of_fit: influence takes at most %d emulators" % GPEngine.GOF_MAX_E)
    f64 = dict(dtype=torch.float64, device=dev)
    cov_exp = np.asarray(chain.expdata_cov, dtype=np.float64)
    yexp_all = np.ascontiguousarray(np.asarray(chain.expdata[0], dtype=np.float64).reshape(-1))
    Ms = [emu.nobs for emu in chain.emuList]
    MT = int(sum(Ms))
    if yexp_all.shape[0] != MT or cov_exp.shape != (MT, MT):
        raise ValueError("emulators provide %d observables, experiment has %d" % (MT, yexp_all.shape[0]))
    offs = np.concatenate([[0], np.cumsum(Ms)]).astype(int)
    yexp = [torch.as_tensor(np.ascontiguousarray(yexp_all[offs[k]:offs[k + 1]]), device=dev) for k in range(E)]
    Cadd = [torch.as_tensor(np.ascontiguousarray(cov_exp[offs[k]:offs[k + 1], offs[k]:offs[k + 1]]), device=dev) for k in range(E)]
    acc = [torch.zeros(GPEngine.gof_acc_doubles(M), **f64) for M in Ms]
    cnt = [torch.zeros(2, dtype=torch.int64, device=dev) for _ in Ms]
    chi2_T, ll_T = torch.empty((E, S), **f64), torch.empty((E, S), **f64)
    joint = coupled and MT <= GPEngine.GOF_MAX_M
    total_reason = None
    if coupled and not joint:
        total_reason = ("expdata_cov couples the emulators and their %d observables exceed the %d a joint factorisation takes"
                        % (MT, GPEngine.GOF_MAX_M))
    if joint:
        yexp_j, Cadd_j = torch.as_tensor(yexp_all, device=dev), torch.as_tensor(np.ascontiguousarray(cov_exp), device=dev)
        acc_j, cnt_j = torch.zeros(GPEngine.gof_acc_doubles(MT), **f64), torch.zeros(2, dtype=torch.int64, device=dev)
        chi2_j, ll_j = torch.empty((1, S), **f64), torch.empty((1, S), **f64)
    slab = slab_rows(chain, MT if joint else 0)
    ev = [] if profile is not None else None

    def mark():
        if ev is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record(torch.cuda.current_stream(dev))
            ev.append(e)
    for i0 in range(0, S, slab):
        i1 = min(i0 + slab, S)
        Xd = torch.as_tensor(X[i0:i1], device=dev)
        wd = None if w is None else torch.as_tensor(w[i0:i1], device=dev)
        if joint:
            yj, Cj = torch.empty((i1 - i0, MT), **f64), torch.zeros((i1 - i0, MT, MT), **f64)
        for k, (emu, g) in enumerate(zip(chain.emuList, engs)):
            Xg = Xd
            if getattr(emu, "parameterTrafoPCA_", False):
                Xg = torch.as_tensor(np.ascontiguousarray(emu._map_parameters(X[i0:i1])), device=dev)
            mark()
            y, C = g.emu_predict(Xg, return_cov=True)
            mark()
            if joint:                                # (before the call below destroys C)
                yj[:, offs[k]:offs[k + 1]] = y
                Cj[:, offs[k]:offs[k + 1], offs[k]:offs[k + 1]] = C
            g.gof_accumulate(y, C, yexp[k], Cadd[k], wd, chi2_T[k, i0:i1], ll_T[k, i0:i1], acc[k], cnt[k])
            mark()
            del y, C
        if joint:
            e0.gof_accumulate(yj, Cj, yexp_j, Cadd_j, wd, chi2_j[0, i0:i1], ll_j[0, i0:i1], acc_j, cnt_j)
            del yj, Cj
    if ev is not None:
        torch.cuda.synchronize(dev)
        profile["predict"] = float(sum(ev[i].elapsed_time(ev[i + 1]) for i in range(0, len(ev), 3)))
        profile["accumulate"] = float(sum(ev[i + 1].elapsed_time(ev[i + 2]) for i in range(0, len(ev), 3)))
        profile["slab_rows"] = slab
        import time
        t_sum = time.perf_counter()
    # ---- summaries: the emulators
    u = [e0.gof_unpack(acc[k], cnt[k], Ms[k]) for k in range(E)]
    mean_u, quant, cmin, carg, _ = _order_stats(e0, chi2_T, q)
    with np.errstate(all="ignore"):
        ws = np.array([v["wsum"] for v in u])
        chi2_mean = mean_u if w is None else np.array([v["z_sq"].sum() for v in u]) / ws
        ppp = np.array([v["p"] for v in u]) / ws
        resid_mean = np.concatenate([v["z"] / v["wsum"] for v in u])
        resid_rms = np.concatenate([np.sqrt(v["z_sq"] / v["wsum"]) for v in u])
        pull_mean = np.concatenate([v["pull"] / v["wsum"] for v in u])
        pull_rms = np.concatenate([np.sqrt(v["pull_sq"] / v["wsum"]) for v in u])
    n_bad = [v["n_bad"] for v in u]
    # ---- the total
    wd_all = None if w is None else torch.as_tensor(w, device=dev)
    if joint:
        tot_chi2, tot_ll = chi2_j, ll_j
    else:                                            # the blocks are independent factors: their sum, in emuList order
        tot_chi2, tot_ll = chi2_T[0:1].clone(), ll_T[0:1].clone()
        for k in range(1, E):
            tot_chi2 += chi2_T[k:k + 1]
            tot_ll += ll_T[k:k + 1]
    total = None
    if total_reason is None:
        t_mean, t_quant, t_min, t_arg, t_used = _order_stats(e0, tot_chi2, q)
        if joint:
            uj = e0.gof_unpack(acc_j, cnt_j, MT)
            with np.errstate(all="ignore"):
                t_ppp = uj["p"] / uj["wsum"]
                t_mean_w = uj["z_sq"].sum() / uj["wsum"]
            t_bad = uj["n_bad"]
        else:
            p_tot = e0.chi2_sf(tot_chi2[0], float(MT))
            fin = torch.isfinite(tot_chi2[0])
            wt_used = torch.ones(S, **f64) if wd_all is None else wd_all
            # weighted means as ratios of gpb_ppd_summary's means over the rows used: E (wt chi2) / E wt, E (wt p) / E wt
            st = torch.stack([wt_used * tot_chi2[0], wt_used * p_tot, wt_used])[:, fin].contiguous()
            if st.shape[1]:
                mom = e0.ppd_summary(st, None, q[:1], outputs=("moments",))["moments"][:, 0]
                t_mean_w, t_ppp = mom[0] / mom[2], mom[1] / mom[2]
            else:
                t_mean_w = t_ppp = float("nan")
            t_bad = int(torch.isnan(chi2_T).any(dim=0).sum().item()) - (0 if wd_all is None else int((wd_all == 0.0).sum().item()))
        total = GofTotal(t_bad, MT, t_mean[0] if w is None else t_mean_w, t_quant[0], t_min[0], t_arg[0],
                         X[int(t_arg[0])].copy(), t_ppp, joint)
    # ---- influence of each data set
    infl = None
    names = list(chain.pardict) if len(getattr(chain, "pardict", ())) == d else None
    if influence and not coupled:
        Xall = torch.as_tensor(X, device=dev)
        without = e0.gof_influence(ll_T, Xall, wd_all).cpu().numpy()
        # the same rows under their own weights: ll replaced by 0 where it is finite, NaN kept
        base = e0.gof_influence(torch.where(torch.isnan(ll_T), ll_T, torch.zeros_like(ll_T)), Xall, wd_all).cpu().numpy()
        with np.errstate(all="ignore"):
            def moments(o):
                m = o[:, 2:2 + d] / o[:, 0:1]
                return m, np.sqrt(np.maximum(o[:, 2 + d:2 + 2 * d] / o[:, 0:1] - m * m, 0.0))
            m1, s1 = moments(without)
            m0, s0 = moments(base)
            infl = DataSetInfluence(without[:, 0] ** 2 / without[:, 1], (m1 - m0) / s0, s1 / s0, names)
    rows = None
    if return_rows:
        rows = dict(chi2=np.ascontiguousarray(chi2_T.cpu().numpy().T), loglike=np.ascontiguousarray(ll_T.cpu().numpy().T))
        if total_reason is None:
            rows["chi2_total"], rows["loglike_total"] = tot_chi2[0].cpu().numpy(), tot_ll[0].cpu().numpy()
    if ev is not None:
        torch.cuda.synchronize(dev)
        profile["summary"] = 1e3 * (time.perf_counter() - t_sum)
    return GoodnessOfFit(S, n_bad, Ms, q, chi2_mean, quant, cmin, carg, X[carg].copy(), ppp, total, total_reason, resid_mean,
                         resid_rms, pull_mean, pull_rms, infl, rows, names)
