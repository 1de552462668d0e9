"""Host model of gpb_chain_knn (include/gpbayes.h) in numpy, fp64, and of the estimators that
gpbayestools_hic_amd/divergence.py builds on it.  The model follows the header's rule literally — every coordinate scaled
once, acc = acc + t * t over the coordinates in order on whole pair matrices (numpy rounds the product and the sum separately:
no fused multiply-add), np.lexsort on (row number, distance), the skip rules — so that the library's r2, idx, zeros and
n_skipped are compared with np.array_equal, nothing excluded.  tests/test_knn_reference.py pins the model to
scipy.spatial.cKDTree and the estimators to closed forms."""
import math

import numpy as np

KMAX = 16
DISCARD, THIN = 5, 3


def scaled(X, inv_scale):
    """(Z, bad): z = x * inv_scale, one rounding; bad: the rows with a scaled coordinate that is not finite"""
    X = np.asarray(X, dtype=np.float64)
    with np.errstate(all="ignore"):
        Z = X * np.asarray(inv_scale, dtype=np.float64)[None, :]
    return Z, ~np.all(np.isfinite(Z), axis=1)


def pair_r2(ZA, ZB):
    """[nA, nB]: acc = 0; for j: t = za_j - zb_j; acc = acc + t * t"""
    acc = np.zeros((ZA.shape[0], ZB.shape[0]))
    with np.errstate(all="ignore"):
        for j in range(ZA.shape[1]):
            t = ZA[:, j, None] - ZB[None, :, j]
            acc = acc + t * t
    return acc


def knn(A, B=None, inv_scale=None, kmax=8, skip_zero=True):
    """the whole of gpb_chain_knn for the rows A [nA, d] (and B [nB, d], or None: self mode) in their order: a dict with r2
    [nA, kmax], idx [nA, kmax] (int32), zeros [nA] (int32), n_skipped (a pair)"""
    A = np.asarray(A, dtype=np.float64)
    d = A.shape[1]
    inv = np.ones(d) if inv_scale is None else np.asarray(inv_scale, dtype=np.float64)
    ZA, badA = scaled(A, inv)
    self_mode = B is None
    ZB, badB = (ZA, badA) if self_mode else scaled(B, inv)
    nA, nB = ZA.shape[0], ZB.shape[0]
    D = pair_r2(ZA, ZB)
    cand = np.broadcast_to(~badB[None, :], (nA, nB)).copy()
    if self_mode:
        cand[np.arange(nA), np.arange(nA)] = False
    cand[badA] = False
    zero = cand & (D == 0.0)
    zeros = zero.sum(axis=1).astype(np.int32)
    if skip_zero:
        cand &= ~zero
    D = np.where(cand, D, np.inf)
    cols = np.broadcast_to(np.arange(nB)[None, :], (nA, nB))
    order = np.lexsort((cols, D), axis=1)[:, :kmax]                       # ascending distance, equal distances by row number
    r2 = np.take_along_axis(D, order, axis=1)
    idx = np.where(np.isfinite(r2), order, -1).astype(np.int32)
    if nB < kmax:
        r2 = np.concatenate([r2, np.full((nA, kmax - nB), np.inf)], axis=1)
        idx = np.concatenate([idx, np.full((nA, kmax - nB), -1, dtype=np.int32)], axis=1)
    return {"r2": r2, "idx": idx, "zeros": zeros, "n_skipped": (int(badA.sum()), 0 if self_mode else int(badB.sum()))}


# ---------------------------------------------------------------------------------------------------------------- estimators
def digamma_int(n):
    """psi(n) for an integer n >= 1: -gamma + sum_{m < n} 1 / m, the asymptotic series from 64 on"""
    n = int(n)
    if n < 64:
        return -np.euler_gamma + float(np.sum(1.0 / np.arange(1, n)))
    x = float(n)
    return math.log(x) - 0.5 / x - 1.0 / (12 * x ** 2) + 1.0 / (120 * x ** 4) - 1.0 / (252 * x ** 6)


def log_unit_ball(d):
    """ln c_d, c_d = pi^(d/2) / Gamma(d/2 + 1)"""
    return 0.5 * d * math.log(math.pi) - math.lgamma(0.5 * d + 1.0)


def kl_entropy(r2, d, keep=None):
    """Kozachenko-Leonenko, [kmax]: psi(n) - psi(k) + ln c_d + (d / n) sum_i ln rho_k(i), rho = sqrt(r2[:, k - 1]) over the n
    rows of keep (default all); nan for a k whose distances are not all finite and positive"""
    r2 = np.asarray(r2)[slice(None) if keep is None else keep]
    n, kmax = r2.shape
    out = np.full(kmax, np.nan)
    for k in range(1, kmax + 1):
        col = r2[:, k - 1]
        if n and np.all(np.isfinite(col)) and np.all(col > 0.0):
            out[k - 1] = digamma_int(n) - digamma_int(k) + log_unit_ball(d) + (d / n) * np.sum(np.log(np.sqrt(col)))
    return out


def wkv_divergence(r2_aa, r2_ab, d, m, keep=None):
    """Wang-Kulkarni-Verdu D(A || B), [kmax]: (d / n) sum_i ln(nu_k(i) / rho_k(i)) + ln(m / (n - 1)), rho within A, nu from A
    to the m rows of B"""
    sel = slice(None) if keep is None else keep
    rho2, nu2 = np.asarray(r2_aa)[sel], np.asarray(r2_ab)[sel]
    n, kmax = rho2.shape
    out = np.full(kmax, np.nan)
    for k in range(1, kmax + 1):
        a, b = rho2[:, k - 1], nu2[:, k - 1]
        if n > 1 and m > 0 and np.all(np.isfinite(a)) and np.all(np.isfinite(b)) and np.all(a > 0.0) and np.all(b > 0.0):
            out[k - 1] = (d / n) * np.sum(np.log(np.sqrt(b) / np.sqrt(a))) + math.log(m / (n - 1.0))
    return out


# ---------------------------------------------------------------------------------------------------------------- test data
def points(n, d, seed, spread=1.0):
    return spread * np.random.default_rng(seed).standard_normal((n, d))


def embed(x):
    """a longer [DISCARD + THIN n, nw, d] array whose [DISCARD::THIN] view is x (the other rows hold other values)"""
    n, nw, d = x.shape
    big = np.random.default_rng(99).standard_normal((DISCARD + THIN * n, nw, d))
    big[DISCARD::THIN] = x
    return big
