"""
Which of two calibrations predicts the data better: leave-one-out predictive accuracy by Pareto-smoothed importance sampling
(PSIS-LOO) with WAIC beside it, over ALL samples of a chain on the device (gpb_loo_pointwise, gpb_psis, gpb_psis_loo; DESIGN.md
section 33).

The reference has no model comparison.  The unit that is left out is one observable (its density given all other observables,
closed-form from the covariance the likelihood factorises: Buerkner, Gabry, Vehtari 2021) or one data set (an emulator's block of
the likelihood).  The importance weights 1 / p(y_unit | theta_s) are smoothed by a generalised Pareto fit to their tail (Vehtari,
Simpson, Gelman, Yao, Gabry 2024); the fitted shape khat says whether the estimate can be trusted: below 0.5 good, up to 0.7 usable,
above that the leave-one-out posterior is too far from the posterior for reweighting — the check that gof.DataSetInfluence, which
reweights by the raw exp(-ll_e), does not have: LooResult(unit="dataset").khat is the reliability of its rows.

No [S, nobs, nobs] array reaches the host: per slab and emulator the mean and the covariance are formed on the device and reduced
to the [nobs, S] pointwise arrays there.
"""
import warnings

import numpy as np

KHAT_GOOD, KHAT_OK = 0.5, 0.7


class PsisResult:
    """psis()'s result: khat [R] (the Pareto shape of the weights' tail; +inf where the tail had four values or fewer and nothing
    was smoothed), ess [R] = 1 / sum w^2 of the smoothed normalised weights, n_tail [R], log_weights [R, S] (logsumexp of a row
    is 0).  A one-dimensional input gives scalars and [S]."""

    def __init__(self, khat, ess, n_tail, log_weights):
        self.khat, self.ess, self.n_tail, self.log_weights = khat, ess, n_tail, log_weights

    def __repr__(self):
        return "PsisResult(khat=%s, ess=%s, n_tail=%s)" % (np.array2string(np.asarray(self.khat), precision=3),
                                                           np.array2string(np.asarray(self.ess), precision=1), self.n_tail)


def _engine(device=0):
    from .engine import GPEngine
    return GPEngine(device=device)


def psis(log_ratios, engine=None, device=0):
    """Pareto-smoothed importance sampling of log importance ratios [R, S] or [S] (numpy, finite): PsisResult.  The general tool:
    the weights of an SMC step, of a posterior without a data set (log ratios -ll_e), of any reweighting.  Runs on the device
    (gpb_psis); engine: a GPEngine to lend its device and stream (default: a new one on `device`)."""
    lr = np.asarray(log_ratios, dtype=np.float64)
    one = lr.ndim == 1
    if one:
        lr = lr[None, :]
    if lr.ndim != 2 or lr.shape[0] < 1 or lr.shape[1] < 1:
        raise ValueError("psis: log_ratios must be [R, S] or [S]")
    if not np.all(np.isfinite(lr)):
        raise ValueError("psis: log_ratios hold non-finite values")
    eng = engine if engine is not None else _engine(device)
    out = eng.psis(np.ascontiguousarray(lr))
    if one:
        return PsisResult(float(out["khat"][0]), float(out["ess"][0]), int(out["n_tail"][0]), out["log_weights"][0])
    return PsisResult(out["khat"], out["ess"], out["n_tail"], out["log_weights"])


class LooResult:
    """posterior_loo's result for n units (observables in emuList order, or data sets):
      unit, n_samples      "observable" or "dataset"; the samples used;  n_bad: samples left out because a covariance had a
                           non-positive pivot for some unit
      elpd_loo [n]         ln of the PSIS estimate of p(y_unit | y_-unit)
      p_loo [n]            lppd - elpd_loo, the effective number of parameters the unit fixes;  lppd [n] = ln mean_s p(y_unit | theta_s)
      elpd_waic, p_waic [n]   lppd - p_waic, and p_waic = the posterior variance of the pointwise log-likelihood (ddof 1)
      khat [n], ess [n], n_tail [n]   the Pareto shape of the importance ratios' tail, the effective sample size of the smoothed
                           weights, the tail's length.  khat <= 0.5: reliable; (0.5, 0.7]: usable; above 0.7: not to be trusted
                           (a warning is raised); above 1 the weights have no finite mean.  With unit="dataset" this is the
                           reliability check that gof.DataSetInfluence lacks
      loo_pit [n]          sum_s w_s Phi(zc_s): the CDF of the leave-one-out predictive distribution at the measurement, uniform
                           on (0, 1) for a calibrated model — the PIT of Chain.posterior_predictive without the measurement used
                           twice and with every correlation in; NaN for data sets and with pit=False
      elpd_loo_total, p_loo_total, elpd_waic_total, p_waic_total   sums over the units;  se_elpd_loo, se_elpd_waic:
                           sqrt(n var) of the pointwise values
      khat_counts          units with khat in (0.5, 0.7], (0.7, 1] and above 1
      pointwise            with return_pointwise: dict of host arrays ll [n, S] and, for observables, zc [n, S]"""

    def __init__(self, unit, n_samples, n_bad, cols, names=None, pointwise=None):
        self.unit, self.n_samples, self.n_bad = unit, int(n_samples), int(n_bad)
        self.elpd_loo, self.lppd, self.p_waic = cols[:, 0].copy(), cols[:, 1].copy(), cols[:, 2].copy()
        self.khat, self.ess, self.n_tail = cols[:, 3].copy(), cols[:, 4].copy(), cols[:, 5].astype(np.int64)
        self.loo_pit, self.min_ll = cols[:, 6].copy(), cols[:, 7].copy()
        self.p_loo = self.lppd - self.elpd_loo
        self.elpd_waic = self.lppd - self.p_waic
        n = cols.shape[0]
        self.n_units = n
        self.elpd_loo_total, self.p_loo_total = float(self.elpd_loo.sum()), float(self.p_loo.sum())
        self.elpd_waic_total, self.p_waic_total = float(self.elpd_waic.sum()), float(self.p_waic.sum())
        with np.errstate(all="ignore"):
            self.se_elpd_loo = float(np.sqrt(n * np.var(self.elpd_loo))) if n > 1 else float("nan")
            self.se_elpd_waic = float(np.sqrt(n * np.var(self.elpd_waic))) if n > 1 else float("nan")
        k = self.khat
        self.khat_counts = (int(((k > KHAT_GOOD) & (k <= KHAT_OK)).sum()), int(((k > KHAT_OK) & (k <= 1.0)).sum()), int((k > 1.0).sum()))
        self.names = None if names is None else list(names)
        self.pointwise = pointwise

    def __repr__(self):
        lines = ["LooResult(unit=%s, units=%d, n_samples=%d, n_bad=%d)" % (self.unit, self.n_units, self.n_samples, self.n_bad),
                 "  %-10s %12s %10s" % ("", "estimate", "se"),
                 "  %-10s %12.3f %10.3f" % ("elpd_loo", self.elpd_loo_total, self.se_elpd_loo),
                 "  %-10s %12.3f" % ("p_loo", self.p_loo_total),
                 "  %-10s %12.3f %10.3f" % ("elpd_waic", self.elpd_waic_total, self.se_elpd_waic),
                 "  %-10s %12.3f" % ("p_waic", self.p_waic_total),
                 "  khat: %d of %d units in (0.5, 0.7], %d in (0.7, 1], %d above 1; largest %.3f (unit %d), smallest ess %.1f"
                 % (self.khat_counts[0], self.n_units, self.khat_counts[1], self.khat_counts[2], float(np.max(self.khat)),
                    int(np.argmax(self.khat)), float(np.min(self.ess)))]
        return "\n".join(lines)


class LooComparison:
    """compare()'s result: elpd_diff = sum (a - b) of the pointwise elpd_loo (positive: a predicts better), se = sqrt(n var) of the
    pointwise differences, and the same for WAIC."""

    def __init__(self, elpd_diff, se, elpd_waic_diff, se_waic, n_units):
        self.elpd_diff, self.se, self.elpd_waic_diff, self.se_waic, self.n_units = elpd_diff, se, elpd_waic_diff, se_waic, n_units

    def __repr__(self):
        return "LooComparison(elpd_diff=%.3f, se=%.3f, elpd_waic_diff=%.3f, se_waic=%.3f, units=%d)" % (
            self.elpd_diff, self.se, self.elpd_waic_diff, self.se_waic, self.n_units)


def compare(a, b):
    """LooComparison of two LooResults of the same data: the units and their count must match (ValueError otherwise)."""
    if a.unit != b.unit or a.n_units != b.n_units:
        raise ValueError("compare: the results must have the same unit and the same number of units, got %s x %d and %s x %d"
                         % (a.unit, a.n_units, b.unit, b.n_units))
    n = a.n_units
    d, dw = a.elpd_loo - b.elpd_loo, a.elpd_waic - b.elpd_waic
    return LooComparison(float(d.sum()), float(np.sqrt(n * np.var(d))), float(dw.sum()), float(np.sqrt(n * np.var(dw))), n)


def posterior_loo(chain, X, unit="observable", pit=True, return_pointwise=False, profile=None, weights=None):
    """LooResult of the rows X [S, ndim] (unweighted posterior draws) for the emulators and the experiment of `chain`.  Slab by
    slab like gof.posterior_gof, emulator by emulator in emuList order: gpb_emu_predict (mean and covariance on the device), then
      unit="observable": gpb_loo_pointwise with that emulator's slice of expdata and its diagonal block of expdata_cov into its
        rows of one [nobs, S] array of conditional log densities (and of standardised conditional residuals with pit=True); a
        coupled expdata_cov makes the joint matrix the only correct one: one call per slab on [W, nobs, nobs], nobs <= 2048
        (NotImplementedError above);
      unit="dataset": gpb_gof_accumulate, whose ll per data set minus M / 2 ln 2 pi is the data set's log density; a coupled
        expdata_cov is refused (NotImplementedError): the blocks are then not factors of the likelihood.
    Samples whose flag is raised for any unit are compacted away and counted in n_bad; then one gpb_psis_loo over the units.
    Equal inputs give equal bits, whatever the slab size.  profile: a dict that receives the milliseconds of the phases "predict",
    "pointwise" and "psis".  weights: refused (ValueError) — PSIS is defined for unweighted draws; resample the particle set.
    NotImplementedError for foreign emulators and a chain sharded over several ranks; ValueError for wrong shapes, non-finite
    rows, fewer than two usable samples."""
    import torch
    from .engine import GPEngine
    from .gof import slab_rows
    if weights is not None:
        raise ValueError("loo: importance weights of weighted draws are out of scope; resample the particle set to equal weights")
    if unit not in ("observable", "dataset"):
        raise ValueError("loo: unit is 'observable' or 'dataset'")
    if not chain._native():
        raise NotImplementedError("loo needs every emulator of the chain to be this package's Emulator (foreign emulators expose "
                                  "no GP state to predict from on the device)")
    if chain.sharding is not None and getattr(chain.sharding, "world", 1) > 1:
        raise NotImplementedError("loo: a chain sharded over several ranks is not supported; call it on one rank (shard_over(None))")
    X = np.asarray(X, dtype=np.float64)
    if X.ndim != 2 or X.shape[1] != chain.ndim or X.shape[0] < 2:
        raise ValueError("loo: samples must be [S >= 2, %d], got %s" % (chain.ndim, X.shape))
    if not np.all(np.isfinite(X)):
        raise ValueError("loo: samples hold non-finite values")
    X = np.ascontiguousarray(X)
    S, d = X.shape
    if S > GPEngine.PSIS_MAX_S:
        raise ValueError("loo: at most 2^24 samples")
    chain._prepare_blocks()
    coupled = bool(chain._coupled)
    Ms = [emu.nobs for emu in chain.emuList]
    MT = int(sum(Ms))
    if coupled and unit == "dataset":
        raise NotImplementedError("loo: expdata_cov couples the emulators, so their blocks are not factors of the likelihood and a "
                                  "data set has no density of its own to leave out; use unit='observable'")
    if coupled and MT > GPEngine.GOF_MAX_M:
        raise NotImplementedError("loo: expdata_cov couples the emulators and their %d observables exceed the %d a joint "
                                  "factorisation takes" % (MT, GPEngine.GOF_MAX_M))
    dev = torch.device("cuda", chain.device or 0)
    engs = [e._engine_ready() for e in chain.emuList]
    for g in engs:
        g._need_data()
        g._track_stream()
    e0 = engs[0]
    E = len(engs)
    f64 = dict(dtype=torch.float64, device=dev)
    cov_exp = np.asarray(chain.expdata_cov, dtype=np.float64)
    yexp_all = np.ascontiguousarray(np.asarray(chain.expdata[0], dtype=np.float64).reshape(-1))
    if yexp_all.shape[0] != MT or cov_exp.shape != (MT, MT):
        raise ValueError("emulators provide %d observables, experiment has %d" % (MT, yexp_all.shape[0]))
    offs = np.concatenate([[0], np.cumsum(Ms)]).astype(int)
    yexp = [torch.as_tensor(np.ascontiguousarray(yexp_all[offs[k]:offs[k + 1]]), device=dev) for k in range(E)]
    Cadd = [torch.as_tensor(np.ascontiguousarray(cov_exp[offs[k]:offs[k + 1], offs[k]:offs[k + 1]]), device=dev) for k in range(E)]
    by_obs = unit == "observable"
    n_units = MT if by_obs else E
    ll_T = torch.empty((n_units, S), **f64)
    zc_T = torch.empty((n_units, S), **f64) if by_obs and pit else None
    bad = torch.zeros(S, dtype=torch.bool, device=dev)
    if by_obs:
        flag = torch.zeros(S, dtype=torch.uint8, device=dev)
    else:
        acc = [torch.zeros(GPEngine.gof_acc_doubles(M), **f64) for M in Ms]
        cnt = [torch.zeros(2, dtype=torch.int64, device=dev) for _ in Ms]
        chi2_T = torch.empty((E, S), **f64)
    if coupled:
        yexp_j, Cadd_j = torch.as_tensor(yexp_all, device=dev), torch.as_tensor(np.ascontiguousarray(cov_exp), device=dev)
    slab = slab_rows(chain, MT if coupled else 0)
    ev = [] if profile is not None else None

    def mark():
        if ev is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record(torch.cuda.current_stream(dev))
            ev.append(e)
    for i0 in range(0, S, slab):
        i1 = min(i0 + slab, S)
        Xd = torch.as_tensor(X[i0:i1], device=dev)
        if coupled:
            yj, Cj = torch.empty((i1 - i0, MT), **f64), torch.zeros((i1 - i0, MT, MT), **f64)
        for k, (emu, g) in enumerate(zip(chain.emuList, engs)):
            Xg = Xd
            if getattr(emu, "parameterTrafoPCA_", False):
                Xg = torch.as_tensor(np.ascontiguousarray(emu._map_parameters(X[i0:i1])), device=dev)
            mark()
            y, C = g.emu_predict(Xg, return_cov=True)
            mark()
            if coupled:
                yj[:, offs[k]:offs[k + 1]] = y
                Cj[:, offs[k]:offs[k + 1], offs[k]:offs[k + 1]] = C
            elif by_obs:
                g.loo_pointwise(y, C, yexp[k], Cadd[k], ll_T[offs[k]:offs[k + 1], i0:i1],
                                None if zc_T is None else zc_T[offs[k]:offs[k + 1], i0:i1], flag[i0:i1])
                bad[i0:i1] |= flag[i0:i1] != 0
            else:
                g.gof_accumulate(y, C, yexp[k], Cadd[k], None, chi2_T[k, i0:i1], ll_T[k, i0:i1], acc[k], cnt[k])
            mark()
            del y, C
        if coupled:
            e0.loo_pointwise(yj, Cj, yexp_j, Cadd_j, ll_T[:, i0:i1], None if zc_T is None else zc_T[:, i0:i1], flag[i0:i1])
            bad[i0:i1] |= flag[i0:i1] != 0
            del yj, Cj
    if not by_obs:                                     # mvn_loglike's value lacks the 2 pi constant; a bad row is NaN
        bad |= torch.isnan(ll_T).any(dim=0)
        ll_T -= torch.as_tensor(0.5 * np.log(2.0 * np.pi) * np.asarray(Ms, dtype=np.float64), device=dev)[:, None]
    if ev is not None:
        torch.cuda.synchronize(dev)
        profile["predict"] = float(sum(ev[i].elapsed_time(ev[i + 1]) for i in range(0, len(ev), 3)))
        profile["pointwise"] = float(sum(ev[i + 1].elapsed_time(ev[i + 2]) for i in range(0, len(ev), 3)))
        profile["slab_rows"] = slab
    n_bad = int(bad.sum().item())
    if n_bad:
        keep = ~bad
        ll_T = ll_T[:, keep].contiguous()
        zc_T = None if zc_T is None else zc_T[:, keep].contiguous()
    S_used = S - n_bad
    if S_used < 2:
        raise ValueError("loo: fewer than two samples have a positive-definite covariance")
    if not bool(torch.isfinite(ll_T).all()):
        raise ValueError("loo: the pointwise log-likelihood is not finite for some sample")
    mark()
    cols = e0.psis_loo(ll_T, zc_T)
    mark()
    if ev is not None:
        torch.cuda.synchronize(dev)
        profile["psis"] = float(ev[-2].elapsed_time(ev[-1]))
    cols = cols.cpu().numpy()
    pointwise = None
    if return_pointwise:
        pointwise = dict(ll=ll_T.cpu().numpy())
        if zc_T is not None:
            pointwise["zc"] = zc_T.cpu().numpy()
    res = LooResult(unit, S_used, n_bad, cols, None, pointwise)
    if np.any(res.khat > KHAT_OK):
        warnings.warn("loo: %d of %d units have a Pareto khat above 0.7 (largest %.2f): their leave-one-out estimates are not "
                      "reliable" % (res.khat_counts[1] + res.khat_counts[2], res.n_units, float(np.max(res.khat))), stacklevel=2)
    return res
