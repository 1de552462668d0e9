"""Host model of gpb_chain_kmeans (include/gpbayes.h) in numpy, fp64: the weighted moments, the k-means++
seeding driven by uniforms, Lloyd's iteration with sklearn's loop and stopping rule, the empty-cluster rule (the centre stays)
and the best restart.  tests/test_kmeans_reference.py pins the Lloyd part to scikit-learn; tests/test_gpu_kmeans.py compares the
library with it.  A helper module, not a test file.

The model also reports how far its decisions are from turning on rounding: min_gap, over all iterations and restarts the
smallest (d2 - d1) / d2 between a row's two nearest centres, and seed_margin, the smallest distance of a seeding target from
a running-sum boundary relative to the total."""
import functools

import numpy as np

# (nsteps, nwalkers, d, k, R), weighted: a row count below one workgroup | several rows of walkers, the 20 parameters of the
# reference's analyses | several ranges in the seeding scan, weights | odd everything, d = 24 | every limit of d, k and R | k = 1
CASES = (((257, 1, 3, 2, 1), False), ((50, 20, 20, 10, 3), False), ((4099, 1, 20, 10, 10), True), ((33, 31, 24, 7, 2), False),
         ((600, 5, 64, 32, 16), False), ((40, 1, 5, 1, 1), False))
SEEDS = (11, 12, 13, 11, 15, 11)           # chosen so that min_gap >= 1e-6 and seed_margin >= 1e-9 hold (the CPU tier asserts it)
MAX_ITER, TOL = 300, 1e-4
DISCARD, THIN = 3, 2


def chain(n, nw, d, k, seed):
    """[n, nw, d]: max(k, 2) Gaussian blobs, every column with its own offset and scale (so that standardising matters and no
    mean is close to 0)"""
    rng = np.random.default_rng(seed)
    nb = max(k, 2)
    cen = 2.5 * rng.standard_normal((nb, d))
    z = cen[rng.integers(0, nb, n * nw)] + rng.standard_normal((n * nw, d))
    scale = np.exp(rng.uniform(-2.0, 2.0, d))
    off = scale * rng.choice([-1.0, 1.0], d) * rng.uniform(4.0, 9.0, d)
    return (z * scale + off).reshape(n, nw, d)


@functools.lru_cache(maxsize=None)
def case(i):
    """(x [n, nw, d], w [n] or None, init [R, k, d] in the chain's units, u [R, k]) of CASES[i]"""
    (n, nw, d, k, R), weighted = CASES[i]
    rng = np.random.default_rng(1000 + SEEDS[i])
    x = chain(n, nw, d, k, SEEDS[i])
    w = rng.exponential(1.0, n) if weighted else None
    flat = x.reshape(-1, d)
    init = np.stack([flat[rng.choice(n * nw, k, replace=False)] for _ in range(R)])
    init = init + 0.05 * flat.std(axis=0) * rng.standard_normal(init.shape)         # (not rows of the chain: no zero distances)
    u = rng.random((R, k))
    for a in (x, init, u) + (() if w is None else (w,)):
        a.setflags(write=False)
    return x, w, init, u


def embed(x):
    """an array whose [DISCARD::THIN] view is x (other values in between)"""
    big = np.random.default_rng(5).standard_normal((DISCARD + x.shape[0] * THIN,) + x.shape[1:]) * 50.0
    big[DISCARD::THIN] = x
    return big


def sqdist(z, C):
    """[S, k]: |z_i - C_c|^2 as a sum of squared differences"""
    out = np.empty((z.shape[0], C.shape[0]))
    for c in range(C.shape[0]):
        t = z - C[c]
        out[:, c] = np.einsum("ij,ij->i", t, t)
    return out


def moments(X, w=None, standardize=True):
    """X [S, d] -> (mean, scale, var_z, weff, n_skipped): the weighted mean and population standard deviation of the rows that
    are finite (the others get weight 0); a column that is constant over the rows of positive weight, or whose standard
    deviation is 0, has scale 1; standardize=False: mean 0, scale 1.  var_z: the weighted variance of the columns of z."""
    X = np.asarray(X, dtype=np.float64)
    fin = np.all(np.isfinite(X), axis=1)
    weff = np.where(fin, 1.0 if w is None else np.asarray(w, dtype=np.float64), 0.0)
    pos = weff > 0
    Xp, wp = X[pos], weff[pos]
    W = wp.sum()
    mu = (wp[:, None] * Xp).sum(axis=0) / W
    const = Xp.min(axis=0) == Xp.max(axis=0)
    mu = np.where(const, Xp[0], mu)
    var = np.where(const, 0.0, (wp[:, None] * (Xp - mu) ** 2).sum(axis=0) / W)
    sc = np.sqrt(var)
    sc[sc == 0.0] = 1.0
    if not standardize:
        return np.zeros_like(mu), np.ones_like(sc), var, weff, int((~fin).sum())
    return mu, sc, var / sc ** 2, weff, int((~fin).sum())


def _gap(D):
    if D.shape[1] < 2 or D.shape[0] == 0:
        return np.inf
    p = np.partition(D, 1, axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        g = (p[:, 1] - p[:, 0]) / p[:, 1]
    return float(np.nanmin(g))


def seed_rows(z, weff, u_r):
    """the k-means++ rows of one restart, u_r [k]: (indices [k], the smallest margin)"""
    k = u_r.shape[0]
    idx = np.empty(k, dtype=np.int64)
    margin, D = np.inf, None
    for c in range(k):
        v = weff if c == 0 else weff * D
        cum = np.cumsum(v)
        tot = cum[-1]
        if not tot > 0.0:
            idx[c] = idx[c - 1]
            continue
        t = u_r[c] * tot
        i = int(np.searchsorted(cum, t, side="right"))
        idx[c] = i
        margin = min(margin, (cum[i] - t) / tot, (t - (cum[i - 1] if i else 0.0)) / tot)
        Dn = sqdist(z, z[i][None])[:, 0]
        D = Dn if D is None else np.minimum(D, Dn)
    return idx, margin


def lloyd(z, weff, C, max_iter, tolabs, valid=None):
    """sklearn's _kmeans_single_lloyd restated: (centres, labels, inertia, n_iter, converged, size, wsum, min_gap).  Rows of
    weight 0 are labelled but decide nothing; `valid` rows (default all) enter min_gap and get labels, the others -1."""
    valid = np.ones(z.shape[0], bool) if valid is None else valid
    pos = weff > 0
    k = C.shape[0]
    C = C.copy()
    old, gap, conv, n_iter = None, np.inf, False, 0
    for it in range(max_iter):
        D = sqdist(z, C)
        gap = min(gap, _gap(D[valid]))
        lab = D.argmin(axis=1)
        hot = (lab[pos][:, None] == np.arange(k)).astype(np.float64)              # [rows, k]
        ws, sums = hot.T @ weff[pos], hot.T @ (weff[pos][:, None] * z[pos])
        Cn = np.where((ws > 0.0)[:, None], sums / np.where(ws > 0.0, ws, 1.0)[:, None], C)
        shift = ((Cn - C) ** 2).sum()
        C, n_iter = Cn, it + 1
        if old is not None and np.array_equal(lab[pos], old[pos]):
            conv = True
            break
        if shift <= tolabs:
            conv = True
            break
        old = lab
    D = sqdist(z, C)
    gap = min(gap, _gap(D[valid]))
    lab = D.argmin(axis=1)
    inertia = float((weff[pos] * D[pos].min(axis=1)).sum())
    size = np.bincount(lab[pos], minlength=k).astype(np.int64)
    wsum = np.bincount(lab[pos], weights=weff[pos], minlength=k)
    return C, np.where(valid, lab, -1).astype(np.int32), inertia, n_iter, conv, size, wsum, gap


def kmeans(X, w, k, R, init=None, u=None, max_iter=MAX_ITER, tol=TOL, standardize=True):
    """the whole of gpb_chain_kmeans for the rows X [S, d] in their order: a dict with the library's outputs (labels [R, S]
    of every restart) plus min_gap and seed_margin"""
    X = np.asarray(X, dtype=np.float64)
    mu, sc, var_z, weff, nskip = moments(X, w, standardize)
    fin = np.all(np.isfinite(X), axis=1)
    z = np.where(fin[:, None], (np.where(fin[:, None], X, 0.0) - mu) / sc, 0.0)
    tolabs = tol * var_z.mean()
    seed_index = np.full((R, k), -1, dtype=np.int64)
    margin = np.inf
    if init is not None:
        C0 = (np.asarray(init, dtype=np.float64) - mu) / sc
    else:
        C0 = np.empty((R, k, X.shape[1]))
        for r in range(R):
            seed_index[r], m = seed_rows(z, weff, np.asarray(u)[r])
            C0[r] = z[seed_index[r]]
            margin = min(margin, m)
    keys = ("centers_z", "labels", "inertia", "n_iter", "converged", "size", "wsum", "gap")
    runs = [dict(zip(keys, lloyd(z, weff, C0[r], max_iter, tolabs, valid=fin))) for r in range(R)]
    out = {key: np.array([q[key] for q in runs]) for key in keys}
    out["centers"] = out["centers_z"] * sc + mu
    low = np.sort(out["inertia"])
    out["best_margin"] = float((low[1] - low[0]) / low[0]) if R > 1 and low[0] > 0.0 else np.inf       # how clear the best restart is
    out.update(mean=mu, scale=sc, seed_index=seed_index, n_skipped=nskip, best=int(np.argmin(out["inertia"])),
               min_gap=float(out.pop("gap").min()), seed_margin=float(margin), tolabs=tolabs, z=z, weff=weff)
    return out


def order_of(i, layout):
    """the rows of CASES[i] in the order the library counts them for a layout: steps (and the thinned view): step-major;
    walkers: walker-major"""
    x = case(i)[0]
    return (x if layout == "steps" else x.transpose(1, 0, 2)).reshape(-1, x.shape[2])


@functools.lru_cache(maxsize=None)
def model(i, how, layout="steps"):
    """the model's answer for CASES[i], how = "init" or "u", computed once"""
    (n, nw, d, k, R), _ = CASES[i]
    x, w, init, u = case(i)
    return kmeans(order_of(i, layout), w, k, R, init=init if how == "init" else None, u=u if how == "u" else None)


def runs():
    """every (case, how, layout) the model is run for: the walkers order is another run only where the seeding sees another order"""
    out = []
    for i, ((n, nw, d, k, R), _) in enumerate(CASES):
        for how in ("init", "u"):
            out.append((i, how, "steps"))
            if how == "u" and nw > 1 and n > 1:        # (from given centres the order of the rows decides nothing)
                out.append((i, how, "walkers"))
    return out
