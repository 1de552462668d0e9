"""float64 numpy model of the history-matching kernels (csrc/gpb_hm.hip: gpb_hm_uniform, gpb_hm_implausibility, gpb_hm_maps) and of
their rules in include/gpbayes.h (a helper module, not a test file).  Arrays are observable-major where the device's are.

  uniform_rows     the candidate rows of gpb_hm_uniform restated through oracle.stretch_oracle's Philox (tag 16, keyed by the
                   absolute row): x = lo + (hi - lo) u with the product and the sum rounded separately
  implausibility   I = |yexp - mu| / sqrt(var + vadd) with numpy's abs, +, sqrt and / under the rules for v <= 0, NaN and +inf; the K
                   largest per sample by a stable argsort of -I (the lowest observable first among equals), the maximum per range
  maps             per bin and bin pair the count, the count of rows with score < cutoff and the minimum score, from np.searchsorted
                   with gpb_chain_marginals' last-bin-closed rule, np.add.at and np.minimum.at
  history_match    what Chain.history_match derives from those on the host
Every operation is a correctly rounded IEEE operation, the minima are exact and the rest are integers: the device equals this model
bit for bit."""
import numpy as np

from oracle.stretch_oracle import philox4x32_10, u01

TAG_HM = 16


def uniform_rows(lo, hi, row0, S, seed):
    """X [S, d]: row r is the absolute row R = row0 + r, element j from philox(seed, (R lo, R hi, j, 16))"""
    lo, hi = np.asarray(lo, dtype=np.float64).reshape(-1), np.asarray(hi, dtype=np.float64).reshape(-1)
    d = lo.shape[0]
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    R = np.uint64(int(row0)) + np.arange(S, dtype=np.uint64)[:, None]
    j = np.arange(d, dtype=np.uint64)[None, :]
    x, y, _, _ = philox4x32_10((seed & 0xFFFFFFFF, seed >> 32), (R & np.uint64(0xFFFFFFFF), R >> np.uint64(32), j, TAG_HM))
    u = u01(x, y)
    t = (hi - lo)[None, :] * u
    return lo[None, :] + t


def implausibility_matrix(mu_T, var_T, yexp, vadd):
    """(I [M, S], bad [S]): bad marks the samples with an observable whose I is +inf by the `otherwise` rule"""
    mu_T = np.asarray(mu_T, dtype=np.float64)
    M, S = mu_T.shape
    var_T = np.zeros((M, S)) if var_T is None else np.asarray(var_T, dtype=np.float64)
    vadd = np.zeros(M) if vadd is None else np.asarray(vadd, dtype=np.float64)
    with np.errstate(all="ignore"):
        r = np.abs(np.asarray(yexp, dtype=np.float64)[:, None] - mu_T)
        v = var_T + vadd[:, None]
        ok = (v > 0.0) & ~np.isnan(r)
        q = r / np.sqrt(np.where(ok, v, 1.0))
        q = np.where(np.isnan(q), 0.0, q)                        # inf / inf: a non-finite mean under vadd = +inf
        other = np.where(r == 0.0, 0.0, np.inf)
    I = np.where(ok, q, other)
    bad = np.any(~ok & (other == np.inf), axis=0)
    return I, bad


def implausibility(mu_T, var_T, yexp, vadd, ranges, K):
    """dict: top [K, S], arg [S] (int32), gmax [G, S], n_bad"""
    I, bad = implausibility_matrix(mu_T, var_T, yexp, vadd)
    order = np.argsort(-I, axis=0, kind="stable")
    top = np.take_along_axis(I, order[:K], axis=0)
    ranges = np.zeros((0, 2), dtype=np.int64) if ranges is None else np.asarray(ranges, dtype=np.int64).reshape(-1, 2)
    gmax = np.stack([I[m0:m1].max(axis=0) for m0, m1 in ranges]) if len(ranges) else np.zeros((0, I.shape[1]))
    return {"top": top, "arg": order[0].astype(np.int32), "gmax": gmax, "n_bad": int(np.count_nonzero(bad)), "I": I}


def bin_codes(X, edges):
    """codes [S, d]: the bin of every value, -1 outside (NaN included); the last bin is closed"""
    X, edges = np.asarray(X, dtype=np.float64), np.asarray(edges, dtype=np.float64)
    S, d = X.shape
    B = edges.shape[1] - 1
    codes = np.full((S, d), -1, dtype=np.int64)
    for j in range(d):
        e, v = edges[j], X[:, j]
        b = np.searchsorted(e, v, side="right") - 1
        b[v == e[B]] = B - 1
        inside = (v >= e[0]) & (v <= e[B])
        codes[inside, j] = b[inside]
    return codes


def all_pairs(d):
    return np.array([(i, j) for i in range(d) for j in range(i + 1, d)], dtype=np.int32).reshape(-1, 2)


def maps(X, score, cutoff, edges, pairs=None, into=None):
    """dict min1, cnt1, nroy1 [d, B] and min2, cnt2, nroy2 [npairs, B, B]; into: an earlier result to accumulate onto (init = 0)"""
    X, score = np.asarray(X, dtype=np.float64), np.asarray(score, dtype=np.float64)
    S, d = X.shape
    B = np.asarray(edges).shape[1] - 1
    pairs = all_pairs(d) if pairs is None else np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if into is None:
        out = {"min1": np.full((d, B), np.inf), "cnt1": np.zeros((d, B), dtype=np.int64), "nroy1": np.zeros((d, B), dtype=np.int64),
               "min2": np.full((len(pairs), B, B), np.inf), "cnt2": np.zeros((len(pairs), B, B), dtype=np.int64),
               "nroy2": np.zeros((len(pairs), B, B), dtype=np.int64)}
    else:
        out = {k: np.array(v) for k, v in into.items()}
    codes = bin_codes(X, edges)
    nroy = (score < cutoff).astype(np.int64)
    for j in range(d):
        k = codes[:, j] >= 0
        np.add.at(out["cnt1"][j], codes[k, j], 1)
        np.add.at(out["nroy1"][j], codes[k, j], nroy[k])
        np.minimum.at(out["min1"][j], codes[k, j], score[k])
    for p, (i, j) in enumerate(pairs):
        k = (codes[:, i] >= 0) & (codes[:, j] >= 0)
        idx = (codes[k, i], codes[k, j])
        np.add.at(out["cnt2"][p], idx, 1)
        np.add.at(out["nroy2"][p], idx, nroy[k])
        np.minimum.at(out["min2"][p], idx, score[k])
    return out


def history_match(X, mu_T, var_T, yexp, vadd, ranges, kth, cutoff, edges, pairs=None, keep=100000):
    """the fields of history.HistoryMatch from the rows X and the predictions at them"""
    r = implausibility(mu_T, var_T, yexp, vadd, ranges, kth)
    score = r["top"][kth - 1]
    nroy = score < cutoff
    S, M = X.shape[0], np.asarray(mu_T).shape[0]
    out = maps(X, score, cutoff, edges, pairs)
    out["n_samples"], out["n_nroy"], out["n_bad"] = S, int(np.count_nonzero(nroy)), r["n_bad"]
    out["ruled_out_by"] = np.bincount(r["arg"][r["top"][0] >= cutoff], minlength=M).astype(np.int64)
    out["dataset_nroy_fraction"] = np.count_nonzero(r["gmax"] < cutoff, axis=1) / S
    Xn = X[nroy]
    out["nroy_samples"] = Xn[:keep]
    out["nroy_box"] = (np.stack([Xn.min(axis=0), Xn.max(axis=0)], axis=1) if len(Xn) else np.full((X.shape[1], 2), np.nan))
    return out
