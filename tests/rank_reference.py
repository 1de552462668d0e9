"""Host model of the rank-normalised diagnostics (a helper module, not a test file): rank-normalised split-R-hat (bulk and folded)
and bulk / tail / mean / quantile effective sample sizes of Vehtari, Gelman, Simpson, Carpenter and Buerkner (2021), restated in
numpy / scipy exactly as include/gpbayes.h specifies gpb_chain_rank_diag — scipy's rankdata and ndtri, numpy's median and
quantile, FFT autocovariances (with a long-double direct-sum twin), Stan's rho-hat and Geyer's two loops — and the MH-like AR(1)
chains the tests run on.  arviz and posterior are not needed."""
import functools

import numpy as np
import scipy.special
import scipy.stats

NO_BAND = 1 << 30                         # GPB_RANK_NO_BAND: the first loop needed a lag beyond max_lag

# (nsteps, nwalkers, ndim) of the GPU tests: one 64 x 64 tile of Y and one sort block; odd nsteps (the dropped middle step); two
# walkers; a few blocks; 23 800 keys = six sort blocks and a band of six block diagonals
SHAPES = ((64, 16, 1), (65, 17, 2), (130, 2, 3), (300, 6, 3), (700, 34, 3))
PHIS = (0.5, 0.8, 0.3)
SEEDS = {SHAPES[0]: 0, SHAPES[1]: 0, SHAPES[2]: 0, SHAPES[3]: 0, SHAPES[4]: 0}      # chosen by test_rank_reference.py's margin test
BAND_LAGS = (0, 63, 64, 65, 349)          # max_lag for the last shape: h - 1 = 349
# a slowly mixing chain whose series stop far beyond the first block diagonal of the band: phi = 0.97 and 0.95, six walkers; the
# indicator of the 0.05 level of parameter 0 stops at lag 133 (it reads lags up to 135), every other series at 345 (up to 347 =
# h - 3): lags on block diagonals 0 ... 5 reach the results
LONG_SHAPE, LONG_PHIS, LONG_SEED = (700, 6, 2), (0.97, 0.95), 1
LONG_BAND_LAGS = (127, 128, 134, 135, 192, 346, 347, 349)      # just below and at what the two kinds of series read, and block edges
PROBS = (0.05, 0.95)
MARGIN = 1e-9                             # every pair the first loop examines has |re + ro| >= this on the tests' inputs


# ---------------------------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def mh_chain(n_t, n_w, n_d, seed=None, phis=PHIS):
    """[n_t, n_w, n_d]: stationary AR(1) series of unit variance (parameter j: coefficient phis[j % len]) in which every step
    repeats the previous value with probability 1/2, as a rejected Metropolis proposal does: half the values are ties.  Parameter
    1 carries an offset of 1e3.  Read-only (shared)."""
    seed = SEEDS.get((n_t, n_w, n_d), 0) if seed is None else seed
    rng = np.random.default_rng([seed, n_t, n_w, n_d, 7])
    x = np.empty((n_t, n_w, n_d))
    for j in range(n_d):
        phi = phis[j % len(phis)]
        e = rng.standard_normal((n_t, n_w))
        stay = rng.random((n_t, n_w)) < 0.5
        x[0, :, j] = e[0]
        for t in range(1, n_t):
            x[t, :, j] = np.where(stay[t], x[t - 1, :, j], phi * x[t - 1, :, j] + np.sqrt(1.0 - phi * phi) * e[t])
    if n_d > 1:
        x[:, :, 1] += 1e3
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def sort_case():
    """[520, 20, 4] = 10 400 kept keys per parameter, three sort blocks of 4096.  Parameter 0: values over 600 binades and both
    signs, with +-0.0 and denormals sprinkled in; parameter 1: a run of 5000 equal values (longer than a sort block) and a run of
    300 equal values laid across the boundary between the second and the third block of the sorted order, the rest distinct;
    parameter 2: never varies; parameter 3: an MH-like AR(1) series.  Read-only."""
    n_t, n_w = 520, 20
    n = n_t * n_w
    rng = np.random.default_rng(20211)
    x = np.empty((n_t, n_w, 4))
    a = rng.standard_normal(n) * np.exp2(rng.integers(-300, 300, n).astype(np.float64))
    a[rng.choice(n, 40, replace=False)] = 0.0
    a[rng.choice(n, 40, replace=False)] = -0.0
    a[rng.choice(n, 40, replace=False)] = 5e-324 * rng.integers(-9, 10, 40)
    a[rng.choice(n, 20, replace=False)] = 2.2250738585072014e-308 * rng.choice([-1.0, 1.0, 0.5, -0.5], 20)
    x[:, :, 0] = a.reshape(n_t, n_w)
    b = np.sort(rng.standard_normal(n))
    b[:5000] = b[4999]                      # sorted positions 0 .. 4999: one run across the first block boundary
    b[8192 - 150:8192 + 150] = b[8192]      # a run across the boundary at 8192
    x[:, :, 1] = rng.permutation(b).reshape(n_t, n_w)
    x[:, :, 2] = 0.3
    x[:, :, 3] = mh_chain(n_t, n_w, 1, seed=3)[:, :, 0]
    x.setflags(write=False)
    return x


# ---------------------------------------------------------------------------------------------------------------- pieces
def kept(x):
    """x [n_t, n_w] -> the kept draws [2 h, n_w] in (step, walker) order: steps t < h and t >= n_t - h, -0.0 as +0.0"""
    n_t = x.shape[0]
    h = n_t // 2
    return np.concatenate([x[:h], x[n_t - h:]], axis=0) + 0.0


def split(v, n_w):
    """kept values [2 h, n_w] (or flat) -> split chains [m = 2 n_w, h]: chain w = first half of walker w, n_w + w = its second"""
    v = np.asarray(v).reshape(-1, n_w)
    h = v.shape[0] // 2
    return np.concatenate([v[:h].T, v[h:].T], axis=0)


def rank2(v):
    """2 x the average rank (1-based) of every value among all of v, int64, in v's own order"""
    r = scipy.stats.rankdata(np.asarray(v).reshape(-1), method="average")
    r2 = np.rint(2.0 * r).astype(np.int64)
    assert np.array_equal(r2 * 0.5, r)
    return r2


def z_of(r2, n):
    return scipy.special.ndtri((r2 * 0.5 - 0.375) / (n + 0.25))


def moments(a):
    """split chains a [m, h] -> (W, var of the chain means (ddof 1)) in long double"""
    a = np.asarray(a, dtype=np.longdouble)
    return a.var(axis=1, ddof=1).mean(), a.mean(axis=1).var(ddof=1)


def rhat_of(a):
    h = a.shape[1]
    W, vm = moments(a)
    B = h * vm
    vp = (h - 1) / np.longdouble(h) * W + B / h
    if vp == 0:
        return np.nan
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.sqrt(vp / W))


def acov_fft(a):
    """A(t), t < h: the mean over the split chains of the biased autocovariance (1 / h) sum_s y(s) y(s + t), y centred by the
    chain's own mean; FFT zero-padded to twice the next power of two (no wrap-around)"""
    m, h = a.shape
    ld = np.asarray(a, dtype=np.longdouble)
    y = np.asarray(ld - ld.mean(axis=1, keepdims=True), dtype=np.float64)      # (centred in long double: an offset costs nothing)
    nfft = 2
    while nfft < 2 * h:
        nfft *= 2
    f = np.fft.rfft(y, n=nfft, axis=1)
    ac = np.fft.irfft(f * np.conjugate(f), n=nfft, axis=1)[:, :h] / h
    return ac.mean(axis=0)


def acov_direct(a):
    """the same by direct lag sums in long double"""
    a = np.asarray(a, dtype=np.longdouble)
    m, h = a.shape
    y = a - a.mean(axis=1, keepdims=True)
    return np.array([np.sum(y[:, :h - t] * y[:, t:]) for t in range(h)], dtype=np.longdouble) / h / m


def ess_of(a, max_lag=None, acov=acov_fft):
    """Stan's effective sample size of the series a [m, h] -> (ess, stop, margin): stop = max_t, or max_lag | NO_BAND when the
    first loop needs a lag beyond max_lag (then ess = NaN), or -1 for a series that never varies (ess = NaN); margin = the least
    |re + ro| the first loop examined (inf when it examined none)."""
    m, h = a.shape
    n = m * h
    L = h - 1 if max_lag is None else int(max_lag)
    A = np.asarray(acov(a), dtype=np.float64)
    mean_var = A[0] * h / (h - 1.0)
    if np.all(a == a.flat[0]):
        return np.nan, -1, np.inf
    var_plus = mean_var * (h - 1.0) / h + float(np.asarray(a, dtype=np.longdouble).mean(axis=1).var(ddof=1))
    if var_plus == 0.0:
        return np.nan, -1, np.inf
    rho = 1.0 - (mean_var - A) / var_plus
    rho[0] = 1.0
    if L < 1:
        return np.nan, L | NO_BAND, np.inf
    R = np.zeros(h + 2)
    re, ro = 1.0, rho[1]
    R[0], R[1] = re, ro
    t = 1
    margin = abs(re + ro)
    while t < h - 3 and re + ro > 0.0:
        if t + 2 > L:
            return np.nan, L | NO_BAND, margin
        re, ro = rho[t + 1], rho[t + 2]
        margin = min(margin, abs(re + ro))
        if re + ro >= 0.0:
            R[t + 1], R[t + 2] = re, ro
        t += 2
    max_t = t - 2
    if re > 0.0:
        R[max_t + 1] = re
    t = 1
    while t <= max_t - 2:
        if R[t + 1] + R[t + 2] > R[t - 1] + R[t]:
            R[t + 1] = R[t + 2] = (R[t - 1] + R[t]) / 2.0
        t += 2
    s = 0.0
    for k in range(max_t + 1):
        s += R[k]
    tau = -1.0 + 2.0 * s + R[max_t + 1]
    tau = max(tau, 1.0 / np.log10(n))
    return n / tau, max_t, margin


def var_plus_of(a):
    """var_plus of the series a [m, h] in long double: A(0) + var(chain means, ddof 1), A(0) = mean_var (h - 1) / h"""
    a = np.asarray(a, dtype=np.longdouble)
    if np.all(a == a.flat[0]):
        return 0.0
    y = a - a.mean(axis=1, keepdims=True)
    return float(np.mean(y * y) + a.mean(axis=1).var(ddof=1))


# ---------------------------------------------------------------------------------------------------------------- the statistic
def rank_diag(x, probs=PROBS, max_lag=None):
    """gpb_chain_rank_diag of x [n_t, n_w, n_d] -> dict(rank2 [d, n] int64, median [d], quant [d, nq], rhat [d, 2], ess [d, K],
    stop [d, K] int32, sd [d], margin: the least |re + ro| of any series)"""
    x = np.asarray(x, dtype=np.float64)
    n_t, n_w, d = x.shape
    h = n_t // 2
    n = 2 * h * n_w
    nq = len(probs)
    K = 2 + nq
    out = dict(rank2=np.empty((d, n), dtype=np.int64), median=np.empty(d), quant=np.empty((d, nq)), rhat=np.empty((d, 2)),
               ess=np.empty((d, K)), stop=np.empty((d, K), dtype=np.int32), sd=np.empty(d), margin=np.inf)
    for j in range(d):
        v = kept(x[:, :, j])
        flat = v.reshape(-1)
        r2 = rank2(flat)
        med = np.median(flat)
        q = np.array([np.quantile(flat, p) for p in probs])
        series = [split(z_of(r2, n), n_w), split(v, n_w)] + [split((v <= qp).astype(np.float64), n_w) for qp in q]
        folded = split(z_of(rank2(np.abs(flat - med)), n), n_w)
        out["rank2"][j], out["median"][j], out["quant"][j] = r2, med, q
        out["rhat"][j] = rhat_of(series[0]), rhat_of(folded)
        for k, a in enumerate(series):
            out["ess"][j, k], out["stop"][j, k], mg = ess_of(a, max_lag)
            out["margin"] = min(out["margin"], mg)
        with np.errstate(invalid="ignore"):
            out["sd"][j] = np.sqrt(var_plus_of(series[1]))
    return out


@functools.lru_cache(maxsize=None)
def reference(shape, max_lag=None, probs=PROBS):
    """the model's answer for mh_chain(*shape), computed once"""
    return rank_diag(mh_chain(*shape), probs, max_lag)


def classic_split_rhat(x):
    """section 18's split-R-hat of x [n_t, n_w, n_d], per parameter"""
    return np.array([rhat_of(split(kept(x[:, :, j]), x.shape[1])) for j in range(x.shape[2])])


def long_chain():
    return mh_chain(*LONG_SHAPE, seed=LONG_SEED, phis=LONG_PHIS)


@functools.lru_cache(maxsize=None)
def long_reference(max_lag=None):
    return rank_diag(long_chain(), PROBS, max_lag)


def gpu_inputs():
    """(label, array, max_lag) of every input the GPU tests compare against the model"""
    cases = [("%dx%dx%d" % s, mh_chain(*s), None) for s in SHAPES]
    cases += [("band %d" % L, mh_chain(*SHAPES[-1]), L) for L in BAND_LAGS]
    cases += [("long", long_chain(), None)] + [("long band %d" % L, long_chain(), L) for L in LONG_BAND_LAGS]
    cases += [("sort case", sort_case(), None), ("thinned", mh_chain(*SHAPES[-1])[100::3], None)]
    return cases
