"""
History matching (Craig et al. 1997; Vernon, Goldstein & Bower 2010): how much of a parameter box the data already rule out, which
observable or data set does the ruling out, and where the next wave of model runs should go — the companion of GP-emulator
calibration that sits between design and sampling.  For a candidate x and an observable m the univariate implausibility is

    I_m(x) = |y_m - mu_m(x)| / sqrt(var_m(x) + V_m),      V_m = experimental variance + model discrepancy

with mu, var the emulator's mean and variance.  A candidate whose kth-largest I_m reaches the cutoff (3 by Pukelsheim's three-sigma
rule; kth = 2 forgives one badly emulated observable) is implausible; the others are not ruled out yet (NROY).  Everything per
candidate runs on the device (gpb_hm_uniform, gpb_emu_predict_diag, gpb_hm_implausibility, gpb_hm_maps) slab
by slab, with integer reductions only: the result does not depend on the slabs.

  implausibility        top-K, arg and group maxima for arrays the caller already has
  implausibility_maps   minimum-score and optical-depth maps of ANY per-row score
  history_match         Chain.history_match's implementation; HistoryMatch its result

The measure is the univariate one: correlations between observables (off-diagonal expdata_cov) are ignored.  A multivariate measure
goes through implausibility_maps with a score of the caller's, e.g. the per-row chi^2 of goodness_of_fit:

    g = chain.goodness_of_fit(X, return_rows=True)
    m = implausibility_maps(X, g.rows["chi2"].sum(axis=1), scipy.stats.chi2.ppf(0.995, chain.nobs), edges)
"""
import pickle
import warnings

import numpy as np


def _engine(engine, device):
    if engine is not None:
        return engine
    from .mcmc import _utility_engine
    return _utility_engine(device)


def _dev_f64(a, dev):
    import torch
    if hasattr(a, "data_ptr"):
        return a
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev)


def implausibility(mu_T, var_T, yexp, var_add=None, ranges=None, K=1, engine=None, device=0):
    """I = |yexp - mu| / sqrt(var + var_add) for observable-major arrays the caller already has: mu_T, var_T (or None) [M, S], numpy
    or torch cuda (e.g. what GPEngine.emu_predict_diag returns), yexp, var_add (None = 0; +inf masks an observable) [M].  Returns a
    dict of numpy arrays: "top" [K, S] the K <= 4 largest per sample, "arg" [S] the observable of the largest (the lowest on ties),
    "gmax" [G, S] the largest over each range [m0, m1) of `ranges` (when given), "bad": the number of samples with an undefined
    implausibility (a variance that is not positive under a non-zero residual, or a NaN) — those read +inf."""
    import torch
    eng = _engine(engine, device)
    dev = torch.device("cuda", eng.device)
    mu_T = _dev_f64(mu_T, dev)
    var_T = None if var_T is None else _dev_f64(var_T, dev)
    return eng.hm_implausibility(mu_T, var_T, yexp, var_add, ranges, K)


def implausibility_maps(X, score, cutoff, edges, pairs=None, engine=None, device=0):
    """The generic map builder: rows X [S, d] (numpy or torch cuda) with ANY per-row score [S] (no NaN).  Over edges [d, B + 1] (B <=
    64; a value is in bin b iff e[b] <= x < e[b + 1], the last bin closed) and pairs [npairs, 2] (default all i < j) returns a dict:
    "min1" [d, B], "min2" [npairs, B, B] the smallest score of the rows in the bin (+inf when empty: the minimum-implausibility
    maps), "cnt1", "cnt2" the rows in it, "nroy1", "nroy2" those with score < cutoff, and "depth1", "depth2" = nroy / cnt, the
    optical depth (NaN when empty)."""
    import torch
    eng = _engine(engine, device)
    dev = torch.device("cuda", eng.device)
    out = eng.hm_maps(_dev_f64(X, dev), _dev_f64(score, dev), cutoff, edges, pairs)
    return _with_depth(out)


def _with_depth(out):
    with np.errstate(invalid="ignore", divide="ignore"):
        for k in ("1", "2"):
            if "cnt" + k in out:
                out["depth" + k] = np.where(out["cnt" + k] > 0, out["nroy" + k] / np.maximum(out["cnt" + k], 1), np.nan)
    return out


class HistoryMatch:
    """Chain.history_match's result (d parameters, nobs observables, E emulators = data sets, B bins):
      n_samples, cutoff, kth      candidates judged; a candidate is NROY iff its kth-largest implausibility is < cutoff
      n_nroy, nroy_fraction       NROY candidates, their share of the box; nroy_fraction_se: its binomial standard error.  A fraction
                                  of 0 is a result, not an error: nothing survives — look at ruled_out_by and the discrepancy
      n_bad                       candidates with an undefined implausibility (they read +inf)
      ruled_out_by [nobs]         the candidates whose LARGEST implausibility is at observable m and is >= cutoff
      dataset_nroy_fraction [E]   the share of the box data set e ALONE leaves (its largest implausibility < cutoff)
      edges [d, B + 1], pairs [npairs, 2]
      min_implausibility_1d [d, B], min_implausibility_2d [npairs, B, B]    the smallest kth implausibility in the bin (+inf: empty)
      optical_depth_1d, optical_depth_2d                                      NROY candidates / candidates in the bin (NaN: empty)
      count_1d, count_2d, nroy_count_1d, nroy_count_2d                        the integers behind them
      nroy_box [d, 2]             the extent of the NROY candidates (NaN when there are none)
      nroy_samples [<= keep, d]   the first `keep` NROY candidates in row order: candidates for propose_design
      bounds [d, 2], names        the box that was sampled (None for X=), the parameters' names"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return ("HistoryMatch(n_samples=%d, cutoff=%g, kth=%d, nroy_fraction=%.4g +- %.2g, n_bad=%d)"
                % (self.n_samples, self.cutoff, self.kth, self.nroy_fraction, self.nroy_fraction_se, self.n_bad))

    def save(self, path):
        """pickle of the fields (numpy arrays and numbers)"""
        with open(path, "wb") as f:
            pickle.dump(dict(self.__dict__), f)

    @classmethod
    def load(cls, path):
        with open(path, "rb") as f:
            return cls(**pickle.load(f))

    def refocus(self, pad=0.0):
        """Bounds [d, 2] for the next wave: the NROY box widened by `pad` times its extent on either side, clipped to the box that
        was sampled.  ValueError when nothing survived."""
        if self.n_nroy < 1:
            raise ValueError("refocus: no candidate survived (nroy_fraction = 0): look at ruled_out_by and the discrepancy")
        lo, hi = self.nroy_box[:, 0], self.nroy_box[:, 1]
        w = (hi - lo) * float(pad)
        lo, hi = lo - w, hi + w
        if self.bounds is not None:
            lo, hi = np.maximum(lo, self.bounds[:, 0]), np.minimum(hi, self.bounds[:, 1])
        return np.stack([lo, hi], axis=1)


def _var_add(chain, discrepancy, rel_discrepancy, observable_mask):
    """[nobs]: diag(expdata_cov) + discrepancy + (rel_discrepancy expdata)^2, +inf where masked; and the mask (True = used)"""
    nobs = chain.nobs
    v = np.array(np.diagonal(np.atleast_2d(chain.expdata_cov)), dtype=np.float64)
    if discrepancy is not None:
        v = v + np.broadcast_to(np.asarray(discrepancy, dtype=np.float64), (nobs,))
    rel = np.broadcast_to(np.asarray(rel_discrepancy, dtype=np.float64), (nobs,))
    v = v + (rel * np.asarray(chain.expdata[0], dtype=np.float64)) ** 2
    used = np.ones(nobs, dtype=bool)
    if observable_mask is not None:
        used = np.asarray(observable_mask, dtype=bool).reshape(-1)
        if used.shape[0] != nobs:
            raise ValueError("observable_mask: expected %d entries" % nobs)
        v = np.where(used, v, np.inf)
    if np.any(np.isnan(v)) or np.any(v < 0.0):
        raise ValueError("the added variances (expdata_cov's diagonal + discrepancy) must not be negative or NaN")
    return np.ascontiguousarray(v), used


def _check_chain(chain, who):
    if not chain._native():
        raise NotImplementedError("%s needs every emulator of the chain to be this package's Emulator (foreign emulators expose no "
                                  "GP state to predict from on the device)" % who)
    if chain.sharding is not None and getattr(chain.sharding, "world", 1) > 1:
        raise NotImplementedError("%s: a chain sharded over several ranks is not supported; call it on one rank (shard_over(None))"
                                  % who)
    if sum(e.nobs for e in chain.emuList) != chain.nobs:
        raise ValueError("emulators provide %d observables, experiment has %d" % (sum(e.nobs for e in chain.emuList), chain.nobs))


def _engines(chain):
    engs = [e._engine_ready() for e in chain.emuList]
    for g in engs:
        g._need_data()
        g._track_stream()
    return engs


def _rows(chain, X, who):
    X = np.asarray(X, dtype=np.float64)
    if X.ndim == 3:
        X = X.reshape(-1, X.shape[-1])
    X = np.ascontiguousarray(np.atleast_2d(X))
    if X.ndim != 2 or X.shape[1] != chain.ndim or X.shape[0] < 1:
        raise ValueError("%s: X must be [S, %d], got %s" % (who, chain.ndim, X.shape))
    if not np.all(np.isfinite(X)):
        raise ValueError("%s: X holds non-finite values" % who)
    return X


def chain_implausibility(chain, X, kth=2, discrepancy=None, rel_discrepancy=0.0, observable_mask=None):
    """Chain.implausibility's implementation"""
    import torch
    _check_chain(chain, "implausibility")
    X = _rows(chain, X, "implausibility")
    vadd, used = _var_add(chain, discrepancy, rel_discrepancy, observable_mask)
    K = int(kth)
    if K < 1 or K > 4 or K > int(used.sum()):
        raise ValueError("kth = %d outside 1 .. min(4, %d unmasked observables)" % (K, int(used.sum())))
    engs = _engines(chain)
    e0 = engs[0]
    dev = torch.device("cuda", chain.device)
    S = X.shape[0]
    slab = min(chain._predict_slab_rows(chain.hm_slab_rows), S)
    mu_T = torch.empty((chain.nobs, slab), dtype=torch.float64, device=dev)
    var_T = torch.empty((chain.nobs, slab), dtype=torch.float64, device=dev)
    yexp = torch.as_tensor(np.ascontiguousarray(chain.expdata[0], dtype=np.float64), device=dev)
    vadd_d = torch.as_tensor(vadd, device=dev)
    ranges = _emu_ranges(chain)
    bad = torch.zeros((1,), dtype=torch.int64, device=dev)
    top, arg, gmax = np.empty((K, S)), np.empty(S, dtype=np.int32), np.empty((len(ranges), S))
    for i0 in range(0, S, slab):
        i1 = min(i0 + slab, S)
        Xd = torch.as_tensor(X[i0:i1], device=dev)
        esd = torch.zeros((i1 - i0,), dtype=torch.float64, device=dev)
        chain._predict_diag_slab(engs, X[i0:i1], Xd, esd, mu_T[:, :i1 - i0], var_T[:, :i1 - i0])
        r = e0.hm_implausibility(mu_T, var_T, yexp, vadd_d, ranges, K, S=i1 - i0, bad=bad, on_device=True)
        top[:, i0:i1], arg[i0:i1], gmax[:, i0:i1] = r["top"].cpu().numpy(), r["arg"].cpu().numpy(), r["gmax"].cpu().numpy()
    return {"top": top, "arg": arg, "gmax": gmax, "bad": int(bad.item())}


def _emu_ranges(chain):
    r, i0 = [], 0
    for e in chain.emuList:
        r.append((i0, i0 + e.nobs))
        i0 += e.nobs
    return np.asarray(r, dtype=np.int32)


def history_match(chain, n_samples=1 << 20, X=None, cutoff=3.0, kth=2, discrepancy=None, rel_discrepancy=0.0, observable_mask=None,
                  bins=20, bounds=None, pairs=None, keep=100000, seed=0):
    """Chain.history_match's implementation (its docstring has the meaning of the arguments)"""
    import torch
    _check_chain(chain, "history_match")
    d, nobs = chain.ndim, chain.nobs
    vadd, used = _var_add(chain, discrepancy, rel_discrepancy, observable_mask)
    kth = int(kth)
    if kth < 1 or kth > 4 or kth > int(used.sum()):
        raise ValueError("kth = %d outside 1 .. min(4, %d unmasked observables)" % (kth, int(used.sum())))
    cutoff = float(cutoff)
    if not np.isfinite(cutoff) or cutoff <= 0.0:
        raise ValueError("cutoff must be positive and finite")
    if X is not None:
        X = _rows(chain, X, "history_match")
        S = X.shape[0]
        box = None
        ext = np.stack([X.min(axis=0), X.max(axis=0)], axis=1)
        ext[:, 1] = np.where(ext[:, 1] > ext[:, 0], ext[:, 1], ext[:, 0] + 1.0)
    else:
        S = int(n_samples)
        if S < 1:
            raise ValueError("n_samples must be at least 1")
        box = np.stack([chain.min, chain.max], axis=1) if bounds is None else np.asarray(bounds, dtype=np.float64).reshape(d, 2)
        box = np.ascontiguousarray(box, dtype=np.float64)
        if not np.all(np.isfinite(box)) or not np.all(box[:, 1] > box[:, 0]):
            raise ValueError("bounds: [%d, 2] finite with hi > lo" % d)
        ext = box
    bins = int(bins)
    if not 1 <= bins <= 64:
        raise ValueError("bins outside 1 .. 64")
    edges = np.ascontiguousarray(np.stack([np.linspace(ext[j, 0], ext[j, 1], bins + 1) for j in range(d)]))
    if pairs is not None:
        pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
    engs = _engines(chain)
    e0 = engs[0]
    dev = torch.device("cuda", chain.device)
    slab = min(chain._predict_slab_rows(chain.hm_slab_rows), S)
    # the workspace: one slab of rows, predictions and scores — nothing grows with n_samples but the kept NROY rows (<= keep)
    Xd_buf = torch.empty((slab, d), dtype=torch.float64, device=dev)
    mu_T = torch.empty((nobs, slab), dtype=torch.float64, device=dev)
    var_T = torch.empty((nobs, slab), dtype=torch.float64, device=dev)
    esd_buf = torch.zeros((slab,), dtype=torch.float64, device=dev)
    yexp = torch.as_tensor(np.ascontiguousarray(chain.expdata[0], dtype=np.float64), device=dev)
    vadd_d = torch.as_tensor(vadd, device=dev)
    ranges = _emu_ranges(chain)
    E = len(ranges)
    bad = torch.zeros((1,), dtype=torch.int64, device=dev)
    ruled = torch.zeros((nobs,), dtype=torch.int64, device=dev)
    ds_nroy = torch.zeros((E,), dtype=torch.int64, device=dev)
    n_nroy = torch.zeros((), dtype=torch.int64, device=dev)
    box_lo = torch.full((d,), float("inf"), dtype=torch.float64, device=dev)
    box_hi = torch.full((d,), float("-inf"), dtype=torch.float64, device=dev)
    kept, n_kept, keep = [], 0, max(int(keep), 0)
    mapped = any(getattr(e, "parameterTrafoPCA_", False) for e in chain.emuList)
    maps = None
    for i0 in range(0, S, slab):
        n = min(slab, S - i0)
        Xd = Xd_buf[:n]
        if X is None:
            e0.hm_uniform(box[:, 0], box[:, 1], n, seed=seed, row0=i0, out=Xd)
        else:
            Xd.copy_(torch.as_tensor(X[i0:i0 + n]))
        X_host = X[i0:i0 + n] if X is not None else ((lambda t=Xd: t.cpu().numpy()) if mapped else None)
        chain._predict_diag_slab(engs, X_host, Xd, esd_buf[:n], mu_T[:, :n], var_T[:, :n])
        r = e0.hm_implausibility(mu_T, var_T, yexp, vadd_d, ranges, kth, S=n, bad=bad, on_device=True)
        score = r["top"][kth - 1]
        maps = e0.hm_maps(Xd, score, cutoff, edges, pairs, into=maps, on_device=True)
        # plumbing on the slab's results: integer counts, an extent and the first NROY rows
        nroy = score < cutoff
        out_by = r["top"][0] >= cutoff
        ruled += torch.bincount(r["arg"][out_by].to(torch.int64), minlength=nobs)
        ds_nroy += (r["gmax"] < cutoff).sum(dim=1)
        n_nroy += nroy.sum()
        idx = torch.nonzero(nroy).reshape(-1)
        if idx.numel():
            rows = Xd[idx]
            box_lo = torch.minimum(box_lo, rows.min(dim=0).values)
            box_hi = torch.maximum(box_hi, rows.max(dim=0).values)
            if n_kept < keep:
                rows = rows[:keep - n_kept]
                kept.append(rows.cpu().numpy())
                n_kept += rows.shape[0]
    n_nroy, n_bad = int(n_nroy.item()), int(bad.item())
    m = _with_depth({k: v.cpu().numpy() for k, v in maps.items()})
    if n_bad > 0:
        warnings.warn("history_match: %d of %d candidates have an undefined implausibility (a variance that is not positive, or a "
                      "NaN prediction); they count as implausible" % (n_bad, S), RuntimeWarning)
    f = n_nroy / S
    d2 = len(m["min2"]) if "min2" in m else 0
    return HistoryMatch(
        n_samples=S, cutoff=cutoff, kth=kth, n_nroy=n_nroy, nroy_fraction=f, nroy_fraction_se=float(np.sqrt(f * (1.0 - f) / S)),
        n_bad=n_bad, ruled_out_by=ruled.cpu().numpy(), dataset_nroy_fraction=ds_nroy.cpu().numpy() / S, edges=edges,
        pairs=(pairs if pairs is not None else np.array([(i, j) for i in range(d) for j in range(i + 1, d)], dtype=np.int32).reshape(-1, 2)),
        min_implausibility_1d=m["min1"], optical_depth_1d=m["depth1"], count_1d=m["cnt1"], nroy_count_1d=m["nroy1"],
        min_implausibility_2d=m["min2"] if d2 else np.zeros((0, bins, bins)), optical_depth_2d=m["depth2"] if d2 else np.zeros((0, bins, bins)),
        count_2d=m["cnt2"] if d2 else np.zeros((0, bins, bins), dtype=np.int64),
        nroy_count_2d=m["nroy2"] if d2 else np.zeros((0, bins, bins), dtype=np.int64),
        nroy_box=(np.stack([box_lo.cpu().numpy(), box_hi.cpu().numpy()], axis=1) if n_nroy else np.full((d, 2), np.nan)),
        nroy_samples=(np.concatenate(kept, axis=0) if kept else np.zeros((0, d))), bounds=box, names=list(chain.pardict))
