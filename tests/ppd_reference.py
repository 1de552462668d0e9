"""Host model of the posterior-predictive summaries (a helper module, not a test file): what gpb_ppd_summary computes per
observable row, restated with exact tools — np.sort for the order statistics, math.fsum of 0.5 * scipy.special.erfc for the
mixture CDF, math.fsum moments, and the 64-halving search as include/gpbayes.h states it.  Also the error bars the CPU and the
GPU tests share, and the rows they are run on."""
import math

import numpy as np
from scipy.special import erfc

SQRT2 = math.sqrt(2.0)
U53, U52 = 2.0 ** -53, 2.0 ** -52
LEVELS_ORDER = (0.0, 0.05, 0.5, 0.95, 1.0)
LEVELS_16 = tuple(np.linspace(0.0, 1.0, 16))
LEVELS_MIX = (0.0013, 0.05, 0.16, 0.5, 0.84, 0.95, 0.9987)


def clog2(S):
    return int(math.ceil(math.log2(S))) if S > 1 else 0


# ---------------------------------------------------------------------------- order statistics and the band
def ranks(q, S):
    """k = floor(q (S - 1)) and min(k + 1, S - 1): the neighbours of numpy's virtual index (n - 1) q"""
    k = np.floor(np.asarray(q, dtype=np.float64) * (S - 1)).astype(np.int64)
    return k, np.minimum(k + 1, S - 1)


def order_stats(row, q):
    """[nq, 2]: np.sort(row)[k], np.sort(row)[min(k + 1, S - 1)]"""
    s = np.sort(np.asarray(row, dtype=np.float64))
    k, k1 = ranks(q, s.shape[0])
    return np.stack([s[k], s[k1]], axis=-1)


def band(row, q):
    """np.percentile(row, 100 q) from the two order statistics by numpy's rule: lo + (hi - lo) g for g < 1/2, else
    hi - (hi - lo) (1 - g), g = q (S - 1) - k"""
    q = np.asarray(q, dtype=np.float64)
    S = np.asarray(row).shape[0]
    o = order_stats(row, q)
    virt = q * (S - 1)
    g = virt - np.floor(virt)
    lo, hi = o[:, 0], o[:, 1]
    return np.where(g >= 0.5, hi - (hi - lo) * (1.0 - g), lo + (hi - lo) * g)


# ---------------------------------------------------------------------------- moments
def _fsum(x):
    try:
        return math.fsum(x)
    except OverflowError:                    # (a row of 1e300s: the squares are not representable)
        return math.inf


def moments(mu, var=None, mean=None):
    """(E mu, E var, E (mu - m)^2) by math.fsum; m = E mu, or `mean` (the device's own first moment: the summand of ITS third
    moment is (mu - m_dev)^2, and m_dev is held to its own bar)"""
    mu = np.asarray(mu, dtype=np.float64)
    S = mu.shape[0]
    m1 = _fsum(mu) / S
    m = m1 if mean is None else float(mean)
    with np.errstate(over="ignore"):
        d2 = (mu - m) ** 2
    return m1, (0.0 if var is None else _fsum(np.asarray(var, dtype=np.float64)) / S), _fsum(d2) / S


def moment_bar(S, terms):
    """(ceil(log2 S) + 4) 2^-53 E|term|: a compensated partial sum per thread, at most ceil(log2 S) levels of a pairwise tree,
    the division by S and the model's own rounding"""
    with np.errstate(over="ignore"):
        return (clog2(S) + 4) * U53 * (_fsum(np.abs(terms)) / S)


# ---------------------------------------------------------------------------- predictive mixture
def tau_of(var, vadd, S):
    v = np.zeros(S) if var is None else np.asarray(var, dtype=np.float64)
    return np.sqrt(np.maximum(v + (0.0 if vadd is None else vadd), 0.0))


def mix_cdf(y, mu, tau):
    """F(y) = 1/S sum_s Phi((y - mu_s) / tau_s) as 0.5 erfc((mu_s - y) / (tau_s sqrt2)), summed exactly; tau_s = 0: the step
    y >= mu_s"""
    mu, tau = np.asarray(mu, dtype=np.float64), np.asarray(tau, dtype=np.float64)
    pos = tau > 0.0
    t = np.where(y >= mu, 1.0, 0.0)
    t[pos] = 0.5 * erfc((mu[pos] - y) / (tau[pos] * SQRT2))
    return math.fsum(t) / mu.shape[0]


def bracket(mu, tau):
    return float(np.min(mu - 9.0 * tau)), float(np.max(mu + 9.0 * tau))


def mix_quantile(q, mu, tau, cdf=mix_cdf):
    """exactly 64 halvings of the bracket: mid = (a + b) / 2, F(mid) < q moves a, otherwise b; early only when mid is no longer
    strictly between a and b; the result is b.  q = 0: -inf, q = 1: +inf."""
    if q <= 0.0:
        return -math.inf
    if q >= 1.0:
        return math.inf
    a, b = bracket(mu, tau)
    for _ in range(64):
        mid = 0.5 * (a + b)
        if not (a < mid < b):
            break
        if cdf(mid, mu, tau) < q:
            a = mid
        else:
            b = mid
    return b


def cdf_bar(mu, tau):
    """(bar, second term) on |F_fsum(y_dev) - q|: k 2^-53 + f 2^-52 max(|a0|, |b0|, b0 - a0) with k = 16 (the OpenCL bound on
    erfc, in ulp) + 8 (the rounding of its argument) + ceil(log2 S) (the summation tree) + 8 (the model's own rounding), f =
    mean_s 1 / (sqrt(2 pi) tau_s) the bound on the mixture's density, [a0, b0] the starting bracket: the second term is what
    one ulp of y can move F"""
    S = np.asarray(mu).shape[0]
    k = 16 + 8 + clog2(S) + 8
    a0, b0 = bracket(mu, tau)
    f = float(np.mean(1.0 / (math.sqrt(2.0 * math.pi) * np.asarray(tau, dtype=np.float64))))
    second = f * U52 * max(abs(a0), abs(b0), b0 - a0)
    return k * U53 + second, second


# ---------------------------------------------------------------------------- the rows of the tests
ORDER_SIZES = (1, 2, 255, 256, 257, 1000)
ROW_KINDS = ("normal", "constant", "half_tied", "wide")


def make_rows(kind, S, M=3, seed=0):
    """[M, S] rows of one kind: "normal" draws of both signs; "constant" one repeated value; "half_tied" half the entries one
    value; "wide" magnitudes 1e-300 .. 1e300 of both signs with +0.0 and -0.0 among them"""
    rng = np.random.default_rng([seed, S, ROW_KINDS.index(kind)])
    if kind == "normal":
        return rng.standard_normal((M, S))
    if kind == "constant":
        return np.repeat(rng.standard_normal((M, 1)) * 3.0, S, axis=1)
    if kind == "half_tied":
        x = rng.standard_normal((M, S))
        for m in range(M):
            x[m, rng.permutation(S)[:S // 2]] = x[m, 0]
        return x
    x = 10.0 ** rng.uniform(-300.0, 300.0, (M, S)) * rng.choice([-1.0, 1.0], (M, S))
    x[:, 0] = 0.0
    if S > 1:
        x[:, S // 2] = -0.0
    return x


# (S, centre of mu, spread of mu, tau: a number, or "loguniform" = exp(U(-8, 1)) per sample)
MIX_CASES = {
    "one": (1, 5.0, 1.0, 0.3),
    "two": (2, 0.0, 1.0, 0.3),
    "thousand": (1000, 0.0, 1.0, 0.2),
    "narrow_tau": (257, 0.0, 1.0, 1e-6),
    "mixed_tau": (513, 0.0, 5.0, "loguniform"),
    "offset": (300, 100.0, 1e-3, 1e-4),
}


def make_mix(name, seed=0):
    """(mu [S], var [S]) of a mixture case; var = tau^2"""
    S, centre, spread, tau = MIX_CASES[name]
    rng = np.random.default_rng([seed, 77, list(MIX_CASES).index(name)])
    mu = centre + spread * rng.standard_normal(S)
    t = np.exp(rng.uniform(-8.0, 1.0, S)) if tau == "loguniform" else np.full(S, float(tau))
    return mu, t * t
