"""Gradient reference for the tests (a helper module, not a test file): a float64 torch restatement of the oracle's
log-posterior — kernels, L-solve, the four observable-transform modes, the block multivariate normal, the prior box
(oracle/gp_oracle.py: kernel_cross, gp_predict, emulator_predict, mvn_loglike_batched, log_prob) — whose derivative comes
from CPU torch.autograd, derived independently of the hand-written HIP kernels.  The GP factorisation is the oracle's own
(gp_factor: scipy Cholesky of K + alpha I)."""
import math

import numpy as np
import torch

from oracle import gp_oracle as O

T = torch.float64


def _t(a):
    return torch.as_tensor(np.asarray(a, dtype=np.float64), dtype=T)


def state_from_oracle(emu):
    """the state of an oracle.gp_oracle.OracleEmulator (fitted): design, hyper-parameters, factors, transform"""
    return dict(X=_t(emu.X), thetas=_t(emu.thetas), L=[_t(L) for L in emu.L], a=[_t(a) for a in emu.a], kind=emu.kind,
                mode=emu.mode, A=None if emu.A is None else _t(emu.A), mu=_t(emu.mu),
                cov_trunc=None if emu.cov_trunc is None else _t(emu.cov_trunc), scale=_t(emu.scale))


def state_from_emulator(emu):
    """the same state for a trained gpbayestools_hic_amd.Emulator, factorised by the oracle (scipy) from its design, its GP
    targets and its hyper-parameters — nothing is read back from the device.  A stochastic-kriging emulator
    (simulation_error=True) carries its per-point noise point_noise_ [P, N]: GP p is factored with the vector
    emu.alpha + point_noise_[p] on its training diagonal."""
    X = np.asarray(emu._X_train, float)
    Z = np.asarray(emu._Z_train, float)
    kind = O.KIND_NAMES[emu.kernel_type_]
    noise = getattr(emu, "point_noise_", None)
    L, a = [], []
    for p in range(Z.shape[0]):
        Lp, ap = O.gp_factor(X, Z[p], emu.thetas_[p], kind, emu.alpha if noise is None else emu.alpha + np.asarray(noise[p], float))
        L.append(_t(Lp)); a.append(_t(ap))
    no_pca = emu.perform_no_PCA_
    return dict(X=_t(X), thetas=_t(emu.thetas_), L=L, a=a, kind=kind, mode=int(emu._mode),
                A=None if no_pca else _t(emu._A), mu=_t(emu.scaler.mean_),
                cov_trunc=None if no_pca else _t(emu._cov_trunc), scale=_t(emu.scaler.scale_))


def kernel_cross(Xs, X, theta, kind):
    """c k(|(x* - x) / l|) from the differences; the square root is kept off zero so that autograd sees a query point on a
    training point as the ordinary case it is (the value moves by < 1e-150)"""
    d = X.shape[1]
    c, ls = torch.exp(theta[0]), torch.exp(theta[1:1 + d])
    D = (Xs[:, None, :] - X[None, :, :]) / ls
    r2 = (D * D).sum(-1)
    if kind == O.KIND_RBF:
        return c * torch.exp(-0.5 * r2)
    r = torch.sqrt(r2 + 1e-300)
    if kind == O.KIND_MATERN15:
        t = r * math.sqrt(3.0)
        return c * (1.0 + t) * torch.exp(-t)
    t = r * math.sqrt(5.0)
    return c * (1.0 + t + t * t / 3.0) * torch.exp(-t)


def gp_mean_var(st, Xs):
    """per-GP mean, variance [W, P] (oracle.gp_predict)"""
    d = st["X"].shape[1]
    ms, vs = [], []
    for p in range(st["thetas"].shape[0]):
        th = st["thetas"][p]
        Ks = kernel_cross(Xs, st["X"], th, st["kind"])
        ms.append(Ks @ st["a"][p])
        V = torch.linalg.solve_triangular(st["L"][p], Ks.T, upper=False)
        vs.append(torch.exp(th[0]) + torch.exp(th[d + 1]) - (V * V).sum(0))
    return torch.stack(ms, 1), torch.stack(vs, 1)


def emulator_mean_cov(st, Xs):
    """Emulator.predict(X, return_cov=True, extra_std=0) (oracle.emulator_predict)"""
    m, v = gp_mean_var(st, Xs)
    mode = st["mode"]
    no_pca = mode in (O.MODE_NO_PCA, O.MODE_NO_PCA_EXPDIAG)
    expdiag = mode in (O.MODE_EXPDIAG, O.MODE_NO_PCA_EXPDIAG)
    if no_pca:
        mean = m * st["scale"] + st["mu"]
        cov = torch.diag_embed(v)
    else:
        A = st["A"]
        mean = m @ A + st["mu"]
        cov = torch.einsum("wk,ki,kj->wij", v, A, A) + st["cov_trunc"]
    if expdiag:
        mean = torch.exp(mean)
        cov = torch.diag_embed(torch.diagonal(cov, dim1=1, dim2=2) * mean * mean)
    return mean, cov


def block_loglike(st, Xs, yexp, cov_exp):
    mean, cov = emulator_mean_cov(st, Xs)
    dY = mean - yexp
    Lc = torch.linalg.cholesky(cov + cov_exp)
    z = torch.linalg.solve_triangular(Lc, dY[..., None], upper=False)[..., 0]
    return -0.5 * (z * z).sum(-1) - torch.log(torch.diagonal(Lc, dim1=1, dim2=2)).sum(-1)


def log_posterior(states, X, lo, hi, yexp, cov_exp, outside=-np.inf):
    """oracle.log_prob for a chain of emulators (block-diagonal covariance, emuList order); X is a torch tensor"""
    lo, hi = _t(lo), _t(hi)
    inside = ((X > lo) & (X < hi)).all(1)
    yexp, cov_exp = _t(yexp).reshape(-1), _t(cov_exp)
    ll = torch.zeros(X.shape[0], dtype=T)
    i0 = 0
    for st in states:
        M = st["mu"].shape[0]
        ll = ll + block_loglike(st, X, yexp[i0:i0 + M], cov_exp[i0:i0 + M, i0:i0 + M])
        i0 += M
    return torch.where(inside, ll + O.EXTRA_STD_CONST, torch.full_like(ll, outside))


def value_and_grad(fn, X):
    """fn(torch X) -> [W] values; returns (values, d values / d X) as numpy"""
    Xt = _t(X).clone().requires_grad_(True)
    v = fn(Xt)
    (g,) = torch.autograd.grad(v.sum(), Xt)
    return v.detach().numpy(), g.numpy()


def jacobian_rows(fn, X):
    """fn(torch X[W, d]) -> [W, K] row-wise outputs; returns J [W, K, d] (rows independent)"""
    Xt = _t(X)
    out = []
    for w in range(Xt.shape[0]):
        out.append(torch.autograd.functional.jacobian(lambda x: fn(x[None, :])[0], Xt[w]).numpy())
    return np.stack(out)
