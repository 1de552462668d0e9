"""Host model of gpb_gof_accumulate, gpb_chi2_sf and gpb_gof_influence (csrc/gpb_gof.hip): per row w, with dY = y[w] - yexp and
Cw = C[w] + Cadd = L L^T,
    z = L^-1 dY      chi2 = z^T z      logdet = 2 sum ln L_ii      ll = -chi2 / 2 - sum ln L_ii      p = Q(M / 2, chi2 / 2)
    pull_m = dY_m / sqrt(Cw_mm)
twice: in np.longdouble with sens_reference's Cholesky and forward substitution (the reference the errors are measured against) and
in plain fp64 through scipy.linalg.cho_factor / cho_solve and scipy.special.gammaincc (the route a user would take on the host: its
error sets the bar, sens_reference.f_bar).  Q itself through mpmath at 50 digits."""
import math

import numpy as np
import scipy.linalg
import scipy.special

import sens_reference as SR
from sens_reference import EPS, CHUNK, f_bar, spd_case  # noqa: F401  (the tests take them from here)


def chi2_sf(x, ndf):
    """Q(ndf / 2, x / 2) as an mpmath number at 50 digits (NaN for a NaN x, 1 for x <= 0)"""
    import mpmath
    with mpmath.workdps(50):
        if x != x:
            return mpmath.nan
        if x <= 0:
            return mpmath.mpf(1)
        return +mpmath.gammainc(mpmath.mpf(ndf) / 2, mpmath.mpf(float(x)) / 2, mpmath.inf, regularized=True)


def sf_relerr(q, x, ndf):
    """(relative error of q against mpmath, the true Q as a float)"""
    import mpmath
    with mpmath.workdps(50):
        t = chi2_sf(x, ndf)
        if t == 0:
            return (0.0 if q == 0.0 else math.inf), 0.0
        return float(abs(mpmath.mpf(float(q)) - t) / t), float(t)


def sf_bar(err_scipy):
    """the bar on the relative error of Q wherever the true Q >= 1e-290: sens_reference.f_bar's factor and floor"""
    return max(8.0 * err_scipy, 64.0 * EPS)


_host_bar = []


def host_sf_bar():
    """the bar of tests/test_chi2_sf_host.py as a number: sf_bar of scipy gammaincc's worst relative error over sf_grid()
    (wherever the true Q >= 1e-290) — the bar every p of the device is held to, whatever its own inputs"""
    if not _host_bar:
        worst = 0.0
        for ndf, x in sf_grid():
            e, true = sf_relerr(float(scipy.special.gammaincc(ndf / 2.0, x / 2.0)), x, ndf)
            if true >= 1e-290:
                worst = max(worst, e)
        _host_bar.append(sf_bar(worst))
    return _host_bar[0]


def rows(y, C, yexp, Cadd=None):
    """dict of the per-row quantities.  np.longdouble: z [W, M], chi2, logdet, ll [W]; fp64: pull [W, M], p [W] (scipy's gammaincc
    at the long-double chi2 rounded); the scipy route: z64, chi2_64, logdet64, ll64; bad, bad64 [W].  Bad rows hold NaN."""
    y, C = np.asarray(y, dtype=np.float64), np.asarray(C, dtype=np.float64)
    Cw = SR._cw(C, Cadd)
    W, M = y.shape
    dY = y - np.asarray(yexp, dtype=np.float64)[None, :]
    ld = np.longdouble
    out = dict(z=np.full((W, M), np.nan, dtype=ld), chi2=np.full(W, np.nan, dtype=ld), logdet=np.full(W, np.nan, dtype=ld),
               ll=np.full(W, np.nan, dtype=ld), z64=np.full((W, M), np.nan), chi2_64=np.full(W, np.nan),
               logdet64=np.full(W, np.nan), ll64=np.full(W, np.nan), p=np.full(W, np.nan),
               bad=np.zeros(W, dtype=bool), bad64=np.zeros(W, dtype=bool))
    with np.errstate(all="ignore"):
        out["pull"] = dY / np.sqrt(np.diagonal(Cw, axis1=1, axis2=2))
    for w in range(W):
        L = SR._cholesky_ld(Cw[w]) if np.all(np.isfinite(Cw[w])) else None
        if L is None:
            out["bad"][w] = True
        else:
            z = SR._forward_ld(L, dY[w].astype(ld))
            sld = np.sum(np.log(np.diagonal(L)))
            out["z"][w], out["chi2"][w], out["logdet"][w] = z, z @ z, 2 * sld
            out["ll"][w] = -out["chi2"][w] / 2 - sld
            out["p"][w] = scipy.special.gammaincc(M / 2.0, float(out["chi2"][w]) / 2.0)
        try:
            cf = scipy.linalg.cho_factor(Cw[w], lower=True)
        except (np.linalg.LinAlgError, ValueError):
            out["bad64"][w] = True
            continue
        L64 = np.tril(cf[0])
        out["z64"][w] = scipy.linalg.solve_triangular(L64, dY[w], lower=True)
        out["chi2_64"][w] = dY[w] @ scipy.linalg.cho_solve(cf, dY[w])
        s64 = np.sum(np.log(np.diagonal(L64)))
        out["logdet64"][w] = 2.0 * s64
        out["ll64"][w] = -0.5 * out["chi2_64"][w] - s64
    return out


def err(a, ref):
    """max |a - ref| / max |ref| against the long-double values (sens_reference.err's measure)"""
    ref = np.asarray(ref, dtype=np.longdouble)
    scale = np.max(np.abs(ref))
    d = np.max(np.abs(np.asarray(a, dtype=np.longdouble) - ref))
    return float(d / scale) if scale > 0 else float(d)


def sums(r, wt=None):
    """the weighted sums over the rows in np.longdouble, bad and weight-0 rows left out as the kernel leaves them out: wsum, p, z,
    z_sq, pull, pull_sq, and abs_* = sum wt |term| for the bars; n_bad counts the bad rows with a non-zero weight (a weightless
    row is not evaluated)"""
    W = r["z"].shape[0]
    wt = np.ones(W) if wt is None else np.asarray(wt, dtype=np.float64)
    use = (~r["bad"]) & (wt != 0.0)
    wl = wt[use].astype(np.longdouble)
    out = dict(wsum=wl.sum(), n_bad=int((r["bad"] & (wt != 0.0)).sum()))
    z, pull = r["z"][use], r["pull"][use].astype(np.longdouble)
    for k, v in (("p", r["p"][use].astype(np.longdouble)), ("z", z), ("z_sq", z * z), ("pull", pull), ("pull_sq", pull * pull)):
        out[k] = np.tensordot(wl, v, axes=(0, 0))
        out["abs_" + k] = np.tensordot(wl, np.abs(v), axes=(0, 0))
    return out


def sum_bar(abs_sum):
    """|device sum - exact sum| <= 1e-13 sum wt |term|: a tree of depth at most 16 + 16 + 3 additions plus the rounding of each
    term, about 4e-15, with a margin of 25"""
    return 1e-13 * np.asarray(abs_sum, dtype=np.float64)


def influence(ll_T, x, wt=None):
    """gpb_gof_influence's output [E, 2 + 2 d] with math.fsum, and the matching sum w |term| [E, 2 + 2 d] for the bars: per
    emulator w_s = wt_s exp(-(ll_T[e, s] - min)) over the rows with a finite ll and a non-zero weight"""
    ll_T, x = np.asarray(ll_T, dtype=np.float64), np.asarray(x, dtype=np.float64)
    E, S = ll_T.shape
    d = x.shape[1]
    wt = np.ones(S) if wt is None else np.asarray(wt, dtype=np.float64)
    out, ab = np.zeros((E, 2 + 2 * d)), np.zeros((E, 2 + 2 * d))
    for e in range(E):
        use = (~np.isnan(ll_T[e])) & (wt != 0.0)
        if not use.any():
            continue
        w = wt[use] * np.exp(-(ll_T[e, use] - ll_T[e, use].min()))
        xs = x[use]
        out[e, 0], out[e, 1] = math.fsum(w), math.fsum(w * w)
        ab[e, 0], ab[e, 1] = out[e, 0], out[e, 1]
        for j in range(d):
            out[e, 2 + j], out[e, 2 + d + j] = math.fsum(w * xs[:, j]), math.fsum(w * (xs[:, j] * xs[:, j]))
            ab[e, 2 + j], ab[e, 2 + d + j] = math.fsum(w * np.abs(xs[:, j])), out[e, 2 + d + j]
    return out, ab


def mvn_loglike_restated(dy, cov):
    """the reference's mvn_loglike (src/mcmc.py:23-65) restated: -1/2 dy^T C^-1 dy - sum ln L_ii through scipy's Cholesky"""
    L, lower = scipy.linalg.cho_factor(cov, lower=False)
    alpha = scipy.linalg.cho_solve((L, lower), dy)
    return -0.5 * float(np.dot(dy, alpha)) - float(np.log(L.diagonal()).sum())


def sf_grid():
    """the (ndf, x) grid of tests/host/chi2_sf_check.cpp, as it forms it"""
    out = []
    for ndf in (1.0, 2.0, 3.0, 16.0, 55.0, 64.0, 540.0, 2048.0):
        xs = [r * ndf for r in (0.0, 1e-3, 0.3, 0.9, 1.0, 1.1, 2.0, 5.0, 40.0)]
        sw = ndf + 2.0
        xs += [np.nextafter(sw, -np.inf), sw, np.nextafter(sw, np.inf)]
        out += [(ndf, float(x)) for x in xs]
    return out
