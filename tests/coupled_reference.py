"""Reference of the coupled chain likelihood for the tests (a helper module, not a test file): the float64 torch restatement
of tests/grad_reference.py with an experimental covariance that may couple the emulators — the joint mean and the
block-diagonal model covariance of all emulators (grad_reference.emulator_mean_cov), plus the FULL cov_exp, one Cholesky per
row (oracle.log_prob with chain_predict; the reference's src/mcmc.py:288-293).  Its derivative comes from CPU torch.autograd.
Also the covariances the coupled tests use."""
import numpy as np
import torch

import grad_reference as R
from oracle import gp_oracle as O


def log_posterior(states, X, lo, hi, yexp, cov_exp, outside=-np.inf):
    """oracle.log_prob for a chain of emulators under a full experimental covariance; X is a torch tensor"""
    lo, hi = R._t(lo), R._t(hi)
    inside = ((X > lo) & (X < hi)).all(1)
    yexp, cov_exp = R._t(yexp).reshape(-1), R._t(cov_exp)
    MT = yexp.shape[0]
    means, cov = [], torch.zeros((X.shape[0], MT, MT), dtype=R.T)
    i0 = 0
    for st in states:
        m, c = R.emulator_mean_cov(st, X)
        k = m.shape[1]
        means.append(m)
        cov[:, i0:i0 + k, i0:i0 + k] = c
        i0 += k
    assert i0 == MT
    dY = torch.cat(means, 1) - yexp
    Lc = torch.linalg.cholesky(cov + cov_exp)
    z = torch.linalg.solve_triangular(Lc, dY[..., None], upper=False)[..., 0]
    ll = -0.5 * (z * z).sum(-1) - torch.log(torch.diagonal(Lc, dim1=1, dim2=2)).sum(-1)
    return torch.where(inside, ll + O.EXTRA_STD_CONST, torch.full_like(ll, outside))


def sources_a(yexp, lo_frac=0.25, hi_frac=0.75):
    """the two fully correlated sources of covariance (a): 0.03 |y_exp| over all observables, 0.05 |y_exp| over the index
    range [lo_frac, hi_frac) of them (the callers choose one that straddles two emulators)"""
    y = np.abs(np.asarray(yexp, dtype=np.float64))
    n = y.shape[0]
    s2 = np.zeros(n)
    s2[int(lo_frac * n):int(hi_frac * n)] = 0.05 * y[int(lo_frac * n):int(hi_frac * n)]
    return np.stack([0.03 * y, s2])


def cov_a(yexp, sigma, **kw):
    """(a): diag(sigma^2) + two rank-one sources, summed as Chain.set_systematics sums them"""
    cov = np.zeros((len(sigma), len(sigma)))
    np.fill_diagonal(cov, np.asarray(sigma, dtype=np.float64) ** 2)
    for s in sources_a(yexp, **kw):
        cov += np.outer(s, s)
    return cov


def cov_b(sigma):
    """(b): sigma_i sigma_j exp(-|i - j| / 5) over the whole index range: couples at full rank"""
    s = np.asarray(sigma, dtype=np.float64)
    i = np.arange(len(s))
    return np.outer(s, s) * np.exp(-np.abs(i[:, None] - i[None, :]) / 5.0)
