"""Host model of gpb_sens_accumulate (csrc/gpb_sens.hip): per row w, with Cw = C[w] + Cadd = L L^T,
    F_w = J^T Cw^-1 J = (L^-1 J)^T (L^-1 J)      R_w[m, j] = (x_j J_mj) / y_m      I_w[m, j] = (J_mj J_mj) / Cw_mm
F twice: in np.longdouble with its own Cholesky and forward substitution (the reference the errors are measured against) and in
plain fp64 through scipy.linalg.cho_factor / cho_solve (the route a user would take on the host: its error sets the bar).  R and I
in fp64 with the parenthesisation above, which the kernel follows operation by operation."""
import numpy as np
import scipy.linalg

EPS = 2.0 ** -53
CHUNK = 256


def _cholesky_ld(A):
    """lower Cholesky factor of A in np.longdouble, None at a non-positive pivot"""
    A = np.array(A, dtype=np.longdouble)
    M = A.shape[0]
    L = np.zeros((M, M), dtype=np.longdouble)
    for j in range(M):
        s = A[j, j] - np.dot(L[j, :j], L[j, :j])
        if not s > 0:
            return None
        L[j, j] = np.sqrt(s)
        if j + 1 < M:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def _forward_ld(L, B):
    """L^-1 B by forward substitution in np.longdouble"""
    U = np.array(B, dtype=np.longdouble)
    for k in range(L.shape[0]):
        U[k] = (U[k] - L[k, :k] @ U[:k]) / L[k, k]
    return U


def _cw(C, Cadd):
    C = np.asarray(C, dtype=np.float64)
    return C if Cadd is None else C + np.asarray(Cadd, dtype=np.float64)[None]


def fisher_longdouble(J, C, Cadd=None):
    """(F [W, d, d] np.longdouble, bad [W] bool): bad rows hold zeros"""
    Cw = _cw(C, Cadd)
    W, M, d = J.shape
    F = np.zeros((W, d, d), dtype=np.longdouble)
    bad = np.zeros(W, dtype=bool)
    for w in range(W):
        L = _cholesky_ld(Cw[w])
        if L is None:
            bad[w] = True
            continue
        U = _forward_ld(L, J[w])
        F[w] = U.T @ U
    return F, bad


def fisher_scipy(J, C, Cadd=None):
    """(F [W, d, d] float64, bad [W] bool) through cho_factor / cho_solve"""
    Cw = _cw(C, Cadd)
    W, M, d = J.shape
    F = np.zeros((W, d, d))
    bad = np.zeros(W, dtype=bool)
    for w in range(W):
        try:
            cf = scipy.linalg.cho_factor(Cw[w], lower=True)
        except np.linalg.LinAlgError:
            bad[w] = True
            continue
        F[w] = J[w].T @ scipy.linalg.cho_solve(cf, J[w])
    return F, bad


def response(J, y, x):
    """R [W, M, d] = (x_j J_mj) / y_m in fp64"""
    with np.errstate(all="ignore"):
        return (x[:, None, :] * J) / y[:, :, None]


def information(J, C, Cadd=None):
    """I [W, M, d] = (J_mj J_mj) / Cw_mm in fp64"""
    dg = np.diagonal(_cw(C, Cadd), axis1=1, axis2=2)
    with np.errstate(all="ignore"):
        return (J * J) / dg[:, :, None]


def rows(J, y, C, Cadd, x):
    """dict of the per-row quantities: F (np.longdouble), F64 (the scipy route), R, I (fp64), bad"""
    F, bad = fisher_longdouble(J, C, Cadd)
    F64, bad64 = fisher_scipy(J, C, Cadd)
    return dict(F=F, F64=F64, R=response(J, y, x), I=information(J, C, Cadd), bad=bad, bad64=bad64)


def err(A, F):
    """max |A - F| / max |F| against the long-double F"""
    F = np.asarray(F, dtype=np.longdouble)
    return float(np.max(np.abs(np.asarray(A, dtype=np.longdouble) - F)) / np.max(np.abs(F)))


def f_bar(err_scipy):
    """the bar on err(device): both routes are backward-stable Cholesky solves whose error scales with cond(C); the factor 8
    covers another elimination order and fma contraction, the floor 64 ulp a case where scipy happens to be exact"""
    return max(8.0 * err_scipy, 64.0 * EPS)


def sums(r, wt=None):
    """the weighted sums over the rows in np.longdouble (bad and weight-0 rows left out as the kernel leaves them out), and
    sum wt |term| for the bars of the R / I sums: dict wsum, fisher, fisher64, response, response_sq, obs_information, abs_*"""
    W = r["R"].shape[0]
    wt = np.ones(W) if wt is None else np.asarray(wt, dtype=np.float64)
    use = (~r["bad"]) & (wt != 0.0)
    wl = wt[use].astype(np.longdouble)
    out = dict(wsum=wl.sum(), n_bad=int(r["bad"].sum()))
    out["fisher"] = np.tensordot(wl, r["F"][use], axes=(0, 0))
    out["fisher64"] = np.tensordot(wt[use], r["F64"][use], axes=(0, 0))
    R, I = r["R"][use].astype(np.longdouble), r["I"][use].astype(np.longdouble)
    R2 = (r["R"][use] * r["R"][use]).astype(np.longdouble)
    for k, v in (("response", R), ("response_sq", R2), ("obs_information", I)):
        out[k] = np.tensordot(wl, v, axes=(0, 0))
        out["abs_" + k] = np.tensordot(wl, np.abs(v), axes=(0, 0))
    return out


def sum_bar(abs_sum):
    """|device sum - exact sum| <= 256 2^-53 sum wt |term|: a chunk's tree is 16 + 16 additions deep, the chunks add one
    addition each and wt * term one rounding — 34 + W / 256 roundings on any path, far inside 256 for the sizes tested"""
    return 256.0 * EPS * np.asarray(abs_sum, dtype=np.float64)


def spd_case(W, M, d, seed, jitter=1e-6):
    """the tests' inputs: C = B B^T + jitter tr / M I per row, random J and x, y bounded away from 0"""
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((W, M, M))
    C = B @ np.swapaxes(B, 1, 2)
    tr = np.trace(C, axis1=1, axis2=2)
    C = C + (jitter * tr / M)[:, None, None] * np.eye(M)[None]
    C = 0.5 * (C + np.swapaxes(C, 1, 2))
    J = rng.standard_normal((W, M, d))
    y = rng.uniform(0.5, 2.0, (W, M)) * rng.choice([-1.0, 1.0], (W, M))
    x = rng.uniform(0.1, 1.0, (W, d))
    return (np.ascontiguousarray(a) for a in (J, y, C, x))


def notebook_response(predict, x0, h):
    """examples/SensitivityAnalysis.ipynb's matrix [nobs, ndim] at the point x0 with the relative step h: for every parameter j,
    (Y+ - Y-) / (2 s) * x0_j / ((Y+ + Y-) / 2) with the step s = h x0_j and Y+- = predict(x0 with x0_j +- s).  (The notebook
    takes h = 0.1.)"""
    x0 = np.asarray(x0, dtype=np.float64)
    cols = []
    for j in range(x0.shape[0]):
        s = h * x0[j]
        xp, xm = x0.copy(), x0.copy()
        xp[j] = x0[j] + s
        xm[j] = x0[j] - s
        Yp, Ym = predict(xp), predict(xm)
        cols.append((Yp - Ym) / (2.0 * s) * x0[j] / ((Yp + Ym) / 2.0))
    return np.stack(cols, axis=1)
