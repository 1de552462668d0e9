"""The numpy model of gpb_psis / gpb_psis_loo / gpb_loo_pointwise (include/gpbayes.h has the specification): Pareto-smoothed
importance sampling of Vehtari, Simpson, Gelman, Yao, Gabry (JMLR 2024) step for step as ArviZ's _psislw / _gpdfit / _gpinv compute
it, in plain float64 or, by the dtype argument, in np.longdouble; the leave-one-out conditionals of a Gaussian from np.linalg.inv;
and the input sets that the host tier and the GPU tier share."""
import numpy as np
import scipy.special

LOO_COLS = ("elpd_loo", "lppd", "p_waic", "khat", "ess", "n_tail", "loo_pit", "min_ll")
MIN_TAIL = 5


def tail_max(S):
    """M = min(S // 5, ceil(3 sqrt(S)))"""
    return int(min(S // 5, int(np.ceil(3.0 * np.sqrt(float(S))))))


def gpd_fit(t, dtype=np.float64, details=None):
    """(khat, sigma) of the ascending excesses t [n], n >= 5 — ArviZ's _gpdfit.  details: a dict that receives the candidates "b", their
    weights "w" before the threshold, and "m_est"."""
    t = np.asarray(t, dtype=dtype)
    n = t.shape[0]
    m_est = 30 + int(np.sqrt(float(n)))
    b = 1 - np.sqrt(dtype(m_est) / (np.arange(1, m_est + 1, dtype=dtype) - dtype(0.5)))
    b = b / (3 * t[int(n / 4 + 0.5) - 1])
    b = b + 1 / t[-1]
    k = np.log1p(-b[:, None] * t).mean(axis=1)
    L = n * (np.log(-(b / k)) - k - 1)
    w = 1 / np.exp(L - L[:, None]).sum(axis=1)
    if details is not None:
        details.update(b=b.copy(), w=w.copy(), m_est=m_est)
    keep = w >= 10 * np.finfo(np.float64).eps
    w, b = w[keep], b[keep]
    w = w / w.sum()
    bh = np.sum(b * w)
    kk = np.log1p(-bh * t).mean()
    sigma = -kk / bh
    return (n * kk + 5) / (n + 10), sigma


def gpd_quantile(p, khat, sigma):
    """ArviZ's _gpinv for 0 < p < 1 and sigma > 0; the khat == 0 branch is the exponential's"""
    if khat == 0:
        return -sigma * np.log1p(-p)
    return np.expm1(-khat * np.log1p(-p)) / khat * sigma


def psis_row(lr, dtype=np.float64, details=None):
    """(lw [S], khat, n_tail, ess) of one row of log ratios.  details: a dict that receives "tail" (the sample indices of the
    tail in ascending order of x, ties by index), "smoothed" (bool), "x" (the shifted ratios), "fit" (gpd_fit's details)."""
    lr = np.asarray(lr, dtype=dtype)
    S = lr.shape[0]
    x = lr - lr.max()
    M = tail_max(S)
    order = np.argsort(x, kind="stable")
    cutoff = max(x[order[S - M - 1]], np.log(dtype(np.finfo(np.float64).tiny)))
    ecut = np.exp(cutoff)
    tail = np.flatnonzero(x > cutoff)
    n = tail.shape[0]
    khat, smoothed = dtype(np.inf), False
    fit = {}
    tail_sorted = tail[np.argsort(x[tail], kind="stable")]
    x0 = x.copy()
    if n >= MIN_TAIL:
        t = np.exp(x[tail_sorted]) - ecut
        khat, sigma = gpd_fit(t, dtype, fit)
        if np.isfinite(khat):
            p = (np.arange(n, dtype=dtype) + dtype(0.5)) / n
            x = x.copy()
            x[tail_sorted] = np.log(gpd_quantile(p, khat, sigma) + ecut)
            x[x > 0] = 0
            smoothed = True
    lse = _lse(x)
    lw = x - lse
    ess = 1 / np.sum(np.exp(2 * lw))
    if details is not None:
        details.update(tail=tail_sorted, smoothed=smoothed, x=x0, fit=fit, cutoff=cutoff)
    return lw, khat, n, ess


def _lse(a):
    m = a.max()
    return m + np.log(np.sum(np.exp(a - m)))


def psis(lr_T, dtype=np.float64):
    """rows of lr_T [R, S]: dict of lw [R, S], khat, n_tail, ess [R]"""
    lr_T = np.atleast_2d(np.asarray(lr_T))
    rows = [psis_row(r, dtype) for r in lr_T]
    return dict(lw=np.array([r[0] for r in rows]), khat=np.array([r[1] for r in rows]), n_tail=np.array([r[2] for r in rows]),
                ess=np.array([r[3] for r in rows]))


def psis_loo(ll_T, zc_T=None, dtype=np.float64):
    """[R, 8] in the order of LOO_COLS, from the pointwise log-likelihoods ll_T [R, S]"""
    ll_T = np.atleast_2d(np.asarray(ll_T, dtype=dtype))
    out = np.full((ll_T.shape[0], len(LOO_COLS)), np.nan, dtype=dtype)
    for r, ll in enumerate(ll_T):
        S = ll.shape[0]
        lw, khat, n, ess = psis_row(-ll, dtype)
        out[r, 0] = _lse(lw + ll)
        out[r, 1] = _lse(ll) - np.log(dtype(S))
        out[r, 2] = np.var(ll, ddof=1) if S > 1 else np.nan
        out[r, 3:6] = khat, ess, n
        if zc_T is not None:
            zc = np.asarray(zc_T[r])
            out[r, 6] = np.sum(np.exp(lw) * scipy.special.ndtr(zc.astype(np.float64)).astype(dtype))
        out[r, 7] = ll.min()
    return out


def loo_pointwise(y, C, yexp, Cadd=None):
    """(ll_T [M, W], zc_T [M, W]) from np.linalg.inv: ll = -1/2 ln(2 pi / P_mm) - 1/2 g_m^2 / P_mm, zc = g_m / sqrt(P_mm) with
    P = (C[w] + Cadd)^-1, g = P (y[w] - yexp)"""
    y, C = np.asarray(y, dtype=np.float64), np.asarray(C, dtype=np.float64)
    W, M = y.shape
    ll, zc = np.empty((M, W)), np.empty((M, W))
    for w in range(W):
        P = np.linalg.inv(C[w] if Cadd is None else C[w] + Cadd)
        g = P @ (y[w] - yexp)
        d = np.diag(P)
        ll[:, w] = -0.5 * np.log(2 * np.pi / d) - 0.5 * g * g / d
        zc[:, w] = g / np.sqrt(d)
    return ll, zc


def loo_by_deletion(y, Cw, yexp, m):
    """(ll, zc) of observable m by conditioning the Gaussian N(0, Cw) of dY on all other observables: the Schur complement of row
    and column m — not the precision matrix"""
    dY = np.asarray(y, dtype=np.float64) - yexp
    M = dY.shape[0]
    o = np.array([i for i in range(M) if i != m], dtype=int)
    if o.size:
        sol = np.linalg.solve(Cw[np.ix_(o, o)], np.column_stack([dY[o], Cw[o, m]]))
        mean = Cw[m, o] @ sol[:, 0]
        var = Cw[m, m] - Cw[m, o] @ sol[:, 1]
    else:
        mean, var = 0.0, Cw[m, m]
    r = dY[m] - mean
    return -0.5 * np.log(2 * np.pi * var) - 0.5 * r * r / var, r / np.sqrt(var)


def change_of_weights(lr, lw):
    """per sample |(lw_s - lw_ref) - (x_s - x_ref)|, ref the smallest sample (which no tail holds): what smoothing did to the sample's
    weight relative to the body's, free of the normalisation.  0 up to rounding for a sample that was not smoothed — and for a
    tail's largest value when its smoothed value is truncated to 0, where it was"""
    lr = np.asarray(lr, dtype=np.float64)
    x = lr - lr.max()
    ref = int(np.argmin(x))
    return np.abs((lw - lw[ref]) - (x - x[ref]))


def changed_set(lr, lw):
    """the samples whose weight smoothing changed by more than 1e-8 (test_psis_reference.py: on the shared sets every change is
    either below 1e-12 or above 1e-7)"""
    return np.flatnonzero(change_of_weights(lr, np.asarray(lw, dtype=np.float64)) > 1e-8)


# ---- the input sets both tiers use ------------------------------------------------------------------------------------------------
SCALES = (0.1, 0.3, 0.6, 0.9, 1.3)
SIZES = (100, 640, 4096, 20000)
EDGE_SIZES = (20, 25, 26, 225, 226, 4096, 4097, 20000)


def chi2_ratios(a, S, seed=0):
    """lr = a z^2 / 2, z standard normal: the ratios' tail is Pareto with shape a, so khat ~ a"""
    z = np.random.default_rng(1000 * seed + S).standard_normal(S)
    return a * z * z / 2


def tied_ratios(S=4096, seed=3):
    """half of the values tied in pairs: every value of the upper half appears twice"""
    v = chi2_ratios(0.6, S // 2, seed)
    return np.random.default_rng(seed).permutation(np.concatenate([v, v]))


def all_equal(S=640):
    return np.full(S, -3.25)


def wide_range(S=640, seed=5):
    """a row whose range exceeds 745: most of its shifted values lie below ln DBL_MIN, and so does the (M + 1)-th largest"""
    r = np.random.default_rng(seed)
    lr = -800.0 - 100.0 * r.random(S)
    lr[r.choice(S, 40, replace=False)] = -3.0 * r.random(40)
    return lr


def cutoff_ties(S=640, seed=7):
    """the (M + 1)-th largest value appears five times, some of them among what would be the tail: n_tail < M"""
    lr = chi2_ratios(0.5, S, seed)
    order = np.argsort(lr)
    M = tail_max(S)
    lr[order[S - M - 1:S - M + 3]] = lr[order[S - M - 2]]
    return lr


def named_sets():
    """name -> lr [S] of every input set of the GPU tier"""
    sets = {}
    for a in SCALES:
        for S in SIZES:
            sets["chi2_a%g_S%d" % (a, S)] = chi2_ratios(a, S)
    for S in EDGE_SIZES:
        sets["edge_S%d" % S] = chi2_ratios(0.7, S, seed=11)
    sets["tied"] = tied_ratios()
    sets["all_equal"] = all_equal()
    sets["wide_range"] = wide_range()
    sets["cutoff_ties"] = cutoff_ties()
    return sets


def row_block(n_rows, S=640):
    """[n_rows, S]: the rows of the GPU tier's many-row cases"""
    return np.stack([chi2_ratios(SCALES[r % 5], S, seed=20 + r) for r in range(n_rows)])


def all_gpu_sets():
    """named_sets() and the 65 rows of row_block: everything the GPU tier feeds gpb_psis"""
    sets = named_sets()
    for r, row in enumerate(row_block(65)):
        sets["row_%d" % r] = row
    return sets


# sets whose n_tail is meant to sit at or below the "<= 4" boundary
SHORT_TAIL_SETS = ("edge_S20", "all_equal")


def well_conditioned_cov(W, M, seed=0, with_add=False):
    """(y [W, M], C [W, M, M], yexp [M], Cadd [M, M] or None): C[w] = Q diag(lambda) Q^T with lambda in [1, 100] (condition number
    <= 100) and a random orthogonal Q"""
    r = np.random.default_rng(seed + 17 * M + W)
    C = np.empty((W, M, M))
    for w in range(W):
        Q, _ = np.linalg.qr(r.standard_normal((M, M)))
        lam = np.exp(r.uniform(0.0, np.log(100.0), M))
        lam[0], lam[-1] = 1.0, 100.0 if M > 1 else 1.0
        A = (Q * lam) @ Q.T
        C[w] = 0.5 * (A + A.T)
    Cadd = None
    if with_add:
        B = r.standard_normal((M, M))
        Cadd = B @ B.T / M + np.eye(M)
    yexp = r.standard_normal(M)
    y = yexp + 3.0 * r.standard_normal((W, M))
    return y, C, yexp, Cadd
