"""Stochastic-kriging reference for the tests (a helper module, not a test file): numpy restatements of everything that reads the
per-point training noise t_i = alpha + s_i.  cv_reference.py and design_reference.py apply ONE scalar alpha to every fold and
every candidate; here the fold's covariance loses diag(t_F), the refit keeps t[keep], and candidate c is observed with its own
tau[p][c].

    projection     s[k, i] = sum_m (E[i, m] / scale[m])^2 comp[k, m]^2 / ev[k]       (whitened PC k; no PCA: (E / scale)^2)
    CV             G = (Ky^-1)_FF, mean = z_F - G^-1 alpha_F, cov = G^-1 - diag(t_F), Ky = K + sigma_n^2 I + diag(t)
    design         J(c) = sum_p g_p [sum_r w_r s_p(r, c)^2] / (s_p(c, c) + tau[p][c]),  tau[p][c] = sigma_n^2 + (alpha + s_c[p][c])

The GP algebra itself is the oracle's (oracle.gp_oracle: kernel_train does K[diag] += alpha, which broadcasts a vector)."""
import numpy as np
from scipy.linalg import cho_factor, cho_solve, cholesky, solve_triangular

import design_reference as D
from oracle import gp_oracle as O

ALPHA = 0.1
KINDS = {"RBF": O.KIND_RBF, "Matern": O.KIND_MATERN15, "Matern25": O.KIND_MATERN25}


def noise_rows(P, N, seed, lo=1e-4, hi=0.3):
    """s [P, N] log-uniform in [lo, hi], different per GP"""
    rng = np.random.default_rng(seed)
    return np.exp(rng.uniform(np.log(lo), np.log(hi), size=(P, N)))


# ---------------------------------------------------------------------------- projection
def projection(E, scale, comp=None, ev=None, npc=None):
    """s [ngp, n] from errors E [n, nobs], written as loops over (GP, event, observable)"""
    E, scale = np.asarray(E, dtype=np.float64), np.asarray(scale, dtype=np.float64)
    n, nobs = E.shape
    if comp is None:
        return np.array([[(E[i, m] / scale[m]) ** 2 for i in range(n)] for m in range(nobs)])
    s = np.zeros((npc, n))
    for k in range(npc):
        for i in range(n):
            for m in range(nobs):
                s[k, i] += (E[i, m] / scale[m]) ** 2 * comp[k, m] ** 2 / ev[k]
    return s


# ---------------------------------------------------------------------------- cross-validation
def cv_closed_form(X, z, theta, kind, t, folds):
    """[(mean [k], cov [k, k]) per fold] from one factorisation of the full design with the vector t on its diagonal (alpha_
    refined twice in long double, as cv_reference.closed_form does and for its reason)"""
    t = np.asarray(t, dtype=np.float64)
    L, a = O.gp_factor(X, z, theta, kind, t)
    Ky = O.kernel_train(X, theta, kind, t).astype(np.longdouble)
    for _ in range(2):
        r = (z.astype(np.longdouble) - Ky @ a.astype(np.longdouble)).astype(np.float64)
        a = a + cho_solve((L, True), r, check_finite=False)
    Linv = solve_triangular(L, np.eye(L.shape[0]), lower=True, check_finite=False)
    out = []
    for F in folds:
        F = np.asarray(F)
        V = Linv[:, F]
        cf = cho_factor(V.T @ V, lower=True, check_finite=False)
        mean = z[F] - cho_solve(cf, a[F], check_finite=False)
        cov = cho_solve(cf, np.eye(len(F)), check_finite=False) - np.diag(t[F])
        out.append((mean, cov))
    return out


def cv_brute_force(X, z, theta, kind, t, folds):
    """[(mean [k], cov [k, k]) per fold]: the GP refitted on the remaining rows with THEIR noise t[keep], predicted at the fold"""
    t = np.asarray(t, dtype=np.float64)
    out = []
    for F in folds:
        F = np.asarray(F)
        keep = np.setdiff1d(np.arange(X.shape[0]), F)
        L, a = O.gp_factor(X[keep], z[keep], theta, kind, t[keep])
        out.append(O.gp_predict_cov(X[F], X[keep], theta, L, a, kind))
    return out


# ---------------------------------------------------------------------------- design
def _posterior_cov(X, theta_p, kind, t, A, B):
    """s(A, B) of one GP whose training diagonal carries sigma_n^2 + t (t a vector over the design)"""
    c, ell, nz = D.unpack(theta_p, X.shape[1])
    L = cholesky(c * D.kern(X, X, ell, kind) + np.diag(nz + np.asarray(t, dtype=np.float64)), lower=True)
    vA = solve_triangular(L, c * D.kern(X, A, ell, kind), lower=True)
    vB = vA if B is A else solve_triangular(L, c * D.kern(X, B, ell, kind), lower=True)
    return c * D.kern(A, B, ell, kind) - vA.T @ vB


def averaged_variance(X, theta, kind, t, Xr, w, g):
    """sum_p g_p sum_r w_r s_p(r, r); t [P, N]"""
    return float(sum(g[p] * (w @ np.diag(_posterior_cov(X, theta[p], kind, t[p], Xr, Xr))) for p in range(theta.shape[0])))


def design_greedy(X, theta, kind, t, Xc, Xr, w, g, T, t_c):
    """The greedy loop by the rank-one formulas with the training noise t [P, N] (= alpha + s) and the candidates' t_c [P, C]
    (= alpha + s_c): candidate c is observed with tau[p][c] = sigma_n^2 + t_c[p][c].  Returns dict(picks, gain, scores [T, C],
    gaps [T] = (best - second best) / best of each step, variance0)."""
    P, C = theta.shape[0], Xc.shape[0]
    nz = np.exp(theta[:, -1])
    tau = nz[:, None] + np.asarray(t_c, dtype=np.float64)
    S_rc = [_posterior_cov(X, theta[p], kind, t[p], Xr, Xc) for p in range(P)]
    S_cc = [_posterior_cov(X, theta[p], kind, t[p], Xc, Xc) for p in range(P)]
    el = np.ones(C, dtype=bool)
    picks, gain, scores, gaps = np.empty(T, dtype=np.int64), np.empty(T), np.empty((T, C)), np.empty(T)
    for step in range(T):
        J = np.zeros(C)
        for p in range(P):
            J += g[p] * ((w @ S_rc[p] ** 2) / (np.diag(S_cc[p]) + tau[p]))
        row = np.where(el, J, -np.inf)
        scores[step] = row
        order = np.sort(row[el])[::-1]
        gaps[step] = (order[0] - order[1]) / order[0] if order.shape[0] > 1 else np.inf
        b = int(np.argmax(row))
        picks[step], gain[step] = b, row[b]
        el[b] = False
        for p in range(P):
            den = S_cc[p][b, b] + tau[p][b]
            S_rc[p] = S_rc[p] - np.outer(S_rc[p][:, b], S_cc[p][b, :]) / den
            S_cc[p] = S_cc[p] - np.outer(S_cc[p][:, b], S_cc[p][b, :]) / den
    return dict(picks=picks, gain=gain, scores=scores, gaps=gaps, variance0=averaged_variance(X, theta, kind, t, Xr, w, g))


def design_refit_scores(X, theta, kind, t, Xc, Xr, w, g, t_c, chosen):
    """Brute force: (J [C], base): base the averaged variance of the design X + Xc[chosen] (the chosen candidates on the diagonal
    with their own t_c), J[c] = base - that of the design with candidate c appended as well, a fresh Cholesky each"""
    chosen = list(chosen)
    Xd = np.concatenate([X, Xc[chosen]], axis=0)
    td = np.concatenate([t, t_c[:, chosen]], axis=1)
    base = averaged_variance(Xd, theta, kind, td, Xr, w, g)
    J = np.array([base - averaged_variance(np.concatenate([Xd, Xc[c:c + 1]], axis=0), theta, kind,
                                           np.concatenate([td, t_c[:, c:c + 1]], axis=1), Xr, w, g) for c in range(Xc.shape[0])])
    return J, base


def design_case(N=70, d=5, P=3, C=40, R=30, seed=3, kernel="RBF"):
    """design_reference.make_case plus training noise s [P, N] (log-uniform in [1e-4, 0.3]) and candidate noise s_c [P, C]
    spanning two decades (log-uniform in [3e-3, 0.3])"""
    c = D.make_case(N, d, P, C, R, seed, kernel)
    c["s"] = noise_rows(P, N, seed + 50)
    c["s_c"] = noise_rows(P, C, seed + 60, 3e-3, 0.3)
    return c
