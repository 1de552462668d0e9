"""Cross-validation reference for the tests (a helper module, not a test file): the closed-form hold-out predictions of a
fitted GP in numpy on the oracle's own Cholesky factor, and the brute-force refits they must equal.

With Ky = K + (sigma_n^2 + alpha) I = L L^T (oracle.gp_oracle.gp_factor) and a fold F (Rasmussen & Williams 5.4.2, for blocks):
    G = (Ky^-1)_FF = (L^-1[:, F])^T (L^-1[:, F]),   mean = z_F - G^-1 alpha_F,   cov = G^-1 - alpha I
is what GPR(kernel at the same theta, alpha).fit(X without F, z without F).predict(X_F, return_cov=True) returns (sklearn's
predictive prior carries the White noise but not alpha: gp_oracle.prior_var, gp_predict_cov).  Also here: the shapes, data and
hyper-parameters the CPU and the GPU tests share."""
import numpy as np
from scipy.linalg import cho_factor, cho_solve, solve_triangular

from gpbayestools_hic_amd import synth
from oracle import gp_oracle as O

ALPHA = 0.1
KINDS = {"RBF": O.KIND_RBF, "Matern": O.KIND_MATERN15, "Matern25": O.KIND_MATERN25}


def closed_form(X, z, theta, kind, alpha, folds):
    """[(mean [k], cov [k, k]) per fold] from ONE factorisation of the full design.  alpha_ = Ky^-1 z is refined twice with
    the residual in long double: at the "hard" theta of N = 1000 (cond Ky ~ 1e5) the plain cho_solve leaves ~7e-13 in the
    means, as much as the brute-force refits carry themselves, and the two would be compared at the sum of their noise"""
    L, a = O.gp_factor(X, z, theta, kind, alpha)
    Ky = O.kernel_train(X, theta, kind, alpha).astype(np.longdouble)
    for _ in range(2):
        r = (z.astype(np.longdouble) - Ky @ a.astype(np.longdouble)).astype(np.float64)
        a = a + cho_solve((L, True), r, check_finite=False)
    Linv = solve_triangular(L, np.eye(L.shape[0]), lower=True, check_finite=False)
    out = []
    for F in folds:
        F = np.asarray(F)
        V = Linv[:, F]
        G = V.T @ V
        cf = cho_factor(G, lower=True, check_finite=False)
        mean = z[F] - cho_solve(cf, a[F], check_finite=False)
        cov = cho_solve(cf, np.eye(len(F)), check_finite=False) - alpha * np.eye(len(F))
        out.append((mean, cov))
    return out


def brute_force(X, z, theta, kind, alpha, folds):
    """[(mean [k], cov [k, k]) per fold]: the GP refitted on the remaining rows (same theta), predicted at the fold"""
    out = []
    for F in folds:
        F = np.asarray(F)
        keep = np.setdiff1d(np.arange(X.shape[0]), F)
        L, a = O.gp_factor(X[keep], z[keep], theta, kind, alpha)
        out.append(O.gp_predict_cov(X[F], X[keep], theta, L, a, kind))
    return out


def flatten(res):
    """per-fold results -> (mean [n_idx], var [n_idx]) in the order of the concatenated folds"""
    return np.concatenate([m for m, _ in res]), np.concatenate([np.diag(c) for _, c in res])


# ---------------------------------------------------------------------------- data and hyper-parameters of the tests
def make_data(N, d, P, seed):
    """X = lhs(N, d, seed), z_p = sin(X w_p) + 0.1 eps with seeded w_p ~ N(0, I): Z [P, N]"""
    X = synth.lhs(N, d, seed)
    rng = np.random.default_rng(seed + 1000)
    Wt = rng.standard_normal((d, P))
    Z = np.sin(X @ Wt) + 0.1 * rng.standard_normal((N, P))
    return X, np.ascontiguousarray(Z.T)


def theta_of(name, d):
    """ "mid": c = 1, l = 1.5, sigma_n^2 = 0.05; "hard": c = 10, l = 3, sigma_n^2 = 0.01; "aniso": c = 3, l from 0.5 to 2 over
    the dimensions, sigma_n^2 = 0.2 — all inside the search box of Emulator._theta0_bounds for a unit design"""
    if name == "mid":
        c, ls, nz = 1.0, np.full(d, 1.5), 0.05
    elif name == "hard":
        c, ls, nz = 10.0, np.full(d, 3.0), 0.01
    else:
        c, ls, nz = 3.0, np.linspace(0.5, 2.0, d), 0.2
    return np.concatenate([[np.log(c)], np.log(ls), [np.log(nz)]])


def thetas_of(names, d):
    return np.array([theta_of(n, d) for n in names])


def contiguous_folds(N, k):
    return [np.arange(i, min(i + k, N)) for i in range(0, N, k)]


def shuffled_folds(N, k, seed):
    perm = np.random.default_rng(seed).permutation(N)
    return [perm[i:i + k] for i in range(0, N, k)]


def kfold(N, nfolds, seed):
    """sklearn KFold(nfolds, shuffle=True) sizes over a seeded permutation"""
    perm = np.random.default_rng(seed).permutation(N)
    sizes = np.full(nfolds, N // nfolds)
    sizes[:N % nfolds] += 1
    return np.split(perm, np.cumsum(sizes)[:-1])


def mean_err(got, ref, z):
    """max |got - ref| / max(|z|, 1)"""
    return float(np.max(np.abs(np.asarray(got) - np.asarray(ref)) / np.maximum(np.abs(z), 1.0)))
