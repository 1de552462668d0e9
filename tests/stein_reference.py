"""Host model of gpb_stein_thin and gpb_stein_ksd (include/gpbayes.h) in numpy, fp64: the rule of the header
followed literally — whole pair matrices, one numpy operation per rounding (numpy fuses nothing), np.argmin for the pick, the
header's summation order for the full discrepancy.  tests/test_gpu_stein.py compares idx, ksd, obj, row_sum, ksd2 and n_skipped
with np.array_equal, nothing excluded; tests/test_stein_reference.py pins the model's kp to torch.autograd derivatives of the
base kernel and the running-sum ksd to the pair-matrix sum of the picks."""
import numpy as np

CHUNK = 1024            # GPB_STEIN_CHUNK
ROW_CHUNK = 256


def prepare(x, g, ginv):
    """(X, B, G, valid, tr): b = Ginv x (acc = acc + Ginv[j][l] * x[l], l ascending), rows with a non-finite entry in x, g or b
    NaN throughout; tr summed ascending from 0"""
    x, g, ginv = (np.array(a, dtype=np.float64) for a in (x, g, ginv))
    n, d = x.shape
    b = np.zeros((n, d))
    with np.errstate(all="ignore"):
        for j in range(d):
            acc = np.zeros(n)
            for l in range(d):
                acc = acc + ginv[j, l] * x[:, l]
            b[:, j] = acc
    valid = np.isfinite(x).all(axis=1) & np.isfinite(g).all(axis=1) & np.isfinite(b).all(axis=1)
    X, B, G = x.copy(), b, g.copy()
    X[~valid], B[~valid], G[~valid] = np.nan, np.nan, np.nan
    tr = 0.0
    for j in range(d):
        tr = tr + ginv[j, j]
    return X, B, G, valid, tr


def kp_matrix(Xi, Bi, Gi, Xj, Bj, Gj, tr):
    """kp(i, j) [ni, nj] of the rows i against the rows j"""
    ni, nj, d = Xi.shape[0], Xj.shape[0], Xi.shape[1]
    q = np.ones((ni, nj))
    t1, t3, t4 = np.zeros((ni, nj)), np.zeros((ni, nj)), np.zeros((ni, nj))
    with np.errstate(all="ignore"):
        for l in range(d):
            r = Xi[:, l][:, None] - Xj[:, l][None, :]
            h = Bi[:, l][:, None] - Bj[:, l][None, :]
            q = q + r * h
            t1 = t1 + h * h
            t3 = t3 + (Gi[:, l][:, None] - Gj[:, l][None, :]) * h
            t4 = t4 + Gi[:, l][:, None] * Gj[:, l][None, :]
        s = np.sqrt(q)
        i1 = 1.0 / s
        i2 = 1.0 / q
        i3 = i1 * i2
        i5 = i3 * i2
        return (-3.0 * t1) * i5 + (tr + t3) * i3 + t4 * i1


def kp_diag(X, B, G, tr):
    """kp(i, i) [n], by the same formula (r = x - x and so on)"""
    n, d = X.shape
    q = np.ones(n)
    t1, t3, t4 = np.zeros(n), np.zeros(n), np.zeros(n)
    with np.errstate(all="ignore"):
        for l in range(d):
            r = X[:, l] - X[:, l]
            h = B[:, l] - B[:, l]
            q = q + r * h
            t1 = t1 + h * h
            t3 = t3 + (G[:, l] - G[:, l]) * h
            t4 = t4 + G[:, l] * G[:, l]
        s = np.sqrt(q)
        i1 = 1.0 / s
        i2 = 1.0 / q
        i3 = i1 * i2
        i5 = i3 * i2
        return (-3.0 * t1) * i5 + (tr + t3) * i3 + t4 * i1


def thin(x, g, ginv, m, return_ties=False):
    """dict idx [m] int32, ksd [m], obj [n] (after the last update), n_skipped; with return_ties also ties [m]: how many rows
    sat at the minimum when pick t was made"""
    X, B, G, valid, tr = prepare(x, g, ginv)
    n = X.shape[0]
    obj = kp_diag(X, B, G, tr)
    idx, ksd, ties = np.empty(m, dtype=np.int32), np.empty(m), np.zeros(m, dtype=np.int64)
    S = 0.0
    for t in range(1, m + 1):
        cand = np.flatnonzero(valid & ~np.isnan(obj))
        if cand.size == 0:
            idx[t - 1], ksd[t - 1], S = -1, np.nan, np.nan
            continue
        pick = int(cand[np.argmin(obj[cand])])                 # (np.argmin: the first of equal minima, the lowest row)
        ties[t - 1] = int(np.sum(obj[cand] == obj[pick]))
        S = S + obj[pick]
        with np.errstate(all="ignore"):
            ksd[t - 1] = np.sqrt(S) / t
        idx[t - 1] = pick
        k = kp_matrix(X, B, G, X[pick:pick + 1], B[pick:pick + 1], G[pick:pick + 1], tr)[:, 0]
        with np.errstate(all="ignore"):
            obj = obj + 2.0 * k
    out = dict(idx=idx, ksd=ksd, obj=obj, n_skipped=int(n - valid.sum()))
    if return_ties:
        out["ties"] = ties
    return out


def row_sums(x, g, ginv, rows=None, block=256):
    """row_sum of the rows `rows` (default all): per chunk of CHUNK columns a partial from 0 in ascending j (a skipped j adds
    +0), the chunk partials from 0 in ascending order; NaN for a skipped row"""
    X, B, G, valid, tr = prepare(x, g, ginv)
    n = X.shape[0]
    rows = np.arange(n) if rows is None else np.asarray(rows)
    out = np.zeros(rows.shape[0])
    for r0 in range(0, rows.shape[0], block):
        ii = rows[r0:r0 + block]
        a = np.zeros(ii.shape[0])
        for j0 in range(0, n, CHUNK):
            jj = slice(j0, min(n, j0 + CHUNK))
            k = kp_matrix(X[ii], B[ii], G[ii], X[jj], B[jj], G[jj], tr)
            k = np.where(np.isnan(k), 0.0, k)
            a = a + np.cumsum(k, axis=1)[:, -1]                # (np.cumsum adds strictly left to right; 0 + k_0 = k_0)
        out[r0:r0 + block] = a
    out[~valid[rows]] = np.nan
    return out


def tree_total(row_sum, valid):
    """sum_i row_sum_i in the header's order: chunks of 256 rows (skipped rows and the rows behind n count +0), four groups of 64
    by the butterfly v[l] = v[l] + v[l ^ o], o = 32 .. 1, then (w0 + w1) + (w2 + w3); the chunk sums from 0 in ascending order"""
    n = row_sum.shape[0]
    nc = (n + ROW_CHUNK - 1) // ROW_CHUNK
    v = np.zeros(nc * ROW_CHUNK)
    v[:n] = np.where(valid, row_sum, 0.0)
    v = v.reshape(nc, 4, 64)
    lane = np.arange(64)
    o = 32
    while o >= 1:
        v = v + v[:, :, lane ^ o]
        o >>= 1
    w = v[:, :, 0]
    cs = (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])
    tot = 0.0
    for c in range(nc):
        tot = tot + cs[c]
    return tot


def ksd_full(x, g, ginv, row_sum=None):
    """dict row_sum [n], ksd2, n_skipped; row_sum given (the device's, where the model's would take minutes): only the total"""
    X, B, G, valid, tr = prepare(x, g, ginv)
    rs = row_sums(x, g, ginv) if row_sum is None else np.asarray(row_sum)
    nv = float(int(valid.sum()))
    with np.errstate(all="ignore"):
        ksd2 = np.float64(tree_total(rs, valid)) / np.float64(nv * nv)
    return dict(row_sum=rs, ksd2=float(ksd2), n_skipped=int(X.shape[0] - valid.sum()))


def ksd_of(x, g, ginv):
    """sqrt of the plain pair-matrix mean of the rows given (np.sum: another order than the device's) — the independent check"""
    X, B, G, valid, tr = prepare(x, g, ginv)
    k = kp_matrix(X[valid], B[valid], G[valid], X[valid], B[valid], G[valid], tr)
    return float(np.sqrt(k.sum()) / valid.sum())
