"""CPU tier: the host model of the closed-form Sobol indices (tests/sobol_reference.py) against Gauss-Legendre quadrature of the
same integrands, and the properties any Sobol decomposition has.  The GPU tests compare the device with this model."""
import numpy as np
import pytest

import sobol_reference as R


def _gl(n, lo, hi):
    x, w = np.polynomial.legendre.leggauss(n)
    return 0.5 * (hi - lo) * x + 0.5 * (hi + lo), 0.5 * (hi - lo) * w


def test_one_dimensional_pieces_against_quadrature():
    """I and Q are box averages of one and of a product of two Gaussian factors: 200-node Gauss-Legendre, 1e-13 relative"""
    rng = np.random.default_rng(0)
    x, w = _gl(200, R.LO, R.HI)
    width = R.HI - R.LO
    worst = 0.0
    for _ in range(50):
        a, b = rng.uniform(0.0, 1.0, 2)
        ell, ellp = rng.uniform(0.5, 3.0, 2) * width
        i_ref = (w * np.exp(-(x - a) ** 2 / (2 * ell ** 2))).sum() / width
        q_ref = (w * np.exp(-(x - a) ** 2 / (2 * ell ** 2) - (x - b) ** 2 / (2 * ellp ** 2))).sum() / width
        worst = max(worst, abs(R.I1(a, ell, R.LO, R.HI) / i_ref - 1.0), abs(R.Q1(a, b, ell, ellp, R.LO, R.HI) / q_ref - 1.0))
    assert worst < 1e-13, worst


def _model(N, d, P, seed, A=None):
    X, Z, theta, lo, hi = R.make_case(N, d, P, seed)
    alpha = R.host_alpha(X, Z, theta)
    amp, ell = np.exp(theta[:, 0]), np.exp(theta[:, 1:d + 1])
    e, H, Ue, UH = R.gp_integrals(X, alpha, amp, ell, lo, hi)
    rng = np.random.default_rng(seed + 7)
    A = rng.standard_normal((P, 3)) if A is None else A
    mu = rng.standard_normal(A.shape[1])
    mean, V, UV = R.observables(e, H, Ue, UH, A, mu)
    return dict(X=X, alpha=alpha, amp=amp, ell=ell, lo=lo, hi=hi, A=A, mu=mu, mean=mean, V=V, UV=UV, e=e, H=H)


def test_two_dimensions_against_tensor_quadrature():
    """d = 2, N = 40, P = 2: mean, variance and both first-order indices against a 64 x 64 tensor Gauss-Legendre quadrature of the
    model's own GP mean, 1e-10 relative"""
    m = _model(40, 2, 2, 3)
    x, w = _gl(64, R.LO, R.HI)
    w = w / (R.HI - R.LO)
    g0, g1 = np.meshgrid(x, x, indexing="ij")
    f = (R.gp_mean(np.stack([g0.ravel(), g1.ravel()], axis=1), m["X"], m["alpha"], m["amp"], m["ell"]) @ m["A"] + m["mu"])
    f = f.reshape(64, 64, -1)
    mean = np.einsum("i,j,ijm->m", w, w, f)
    var = np.einsum("i,j,ijm->m", w, w, f ** 2) - mean ** 2
    v0 = np.einsum("i,im->m", w, np.einsum("j,ijm->im", w, f) ** 2) - mean ** 2
    v1 = np.einsum("j,jm->m", w, np.einsum("i,ijm->jm", w, f) ** 2) - mean ** 2
    first, _ = R.indices(m["V"])
    assert np.max(np.abs(m["mean"] / mean - 1.0)) < 1e-10
    assert np.max(np.abs(m["V"][:, 4] / var - 1.0)) < 1e-10
    assert np.max(np.abs(first[:, 0] / (v0 / var) - 1.0)) < 1e-10 and np.max(np.abs(first[:, 1] / (v1 / var) - 1.0)) < 1e-10
    # the main-effect curve is the quadrature's conditional mean
    curve = R.main_effect(m["X"], m["alpha"], m["amp"], m["ell"], m["lo"], m["hi"], 0, x, m["A"], m["mu"])
    assert np.max(np.abs(curve - np.einsum("j,ijm->im", w, f))) < 1e-12 * max(1.0, np.abs(f).max())


def test_additive_target_has_no_interactions():
    """GP p varies with input p alone (every other length scale 1e9 widths: that factor is 1 in fp64), so f is additive and
    first = total within the model's own bar"""
    N, d, P = 48, 3, 3
    X, Z, theta, lo, hi = R.make_case(N, d, P, 5)
    for p in range(P):
        for l in range(d):
            if l != p:
                theta[p, 1 + l] = np.log(1e9 * (R.HI - R.LO))
    alpha = R.host_alpha(X, Z, theta)
    amp, ell = np.exp(theta[:, 0]), np.exp(theta[:, 1:d + 1])
    e, H, Ue, UH = R.gp_integrals(X, alpha, amp, ell, lo, hi)
    A = np.random.default_rng(1).standard_normal((P, 2))
    _, V, UV = R.observables(e, H, Ue, UH, A, np.zeros(2))
    first, total = R.indices(V)
    bf, bt = R.index_bars(V, R.bar_factor(N, d) * UV)
    assert np.all(np.abs(first - total) <= bf + bt), (np.abs(first - total).max(), (bf + bt).min())
    assert np.all(np.abs(first.sum(axis=1) - 1.0) <= bf.sum(axis=1))


def test_one_dimension():
    """d = 1: {j} is all and all \\ {j} is empty (V_empty = e^2 - e^2 up to rounding): first = 1 exactly, total = 1 within the bar"""
    m = _model(64, 1, 1, 2, A=np.array([[1.3, -0.4]]))
    first, total = R.indices(m["V"])
    _, bt = R.index_bars(m["V"], R.bar_factor(64, 1) * m["UV"])
    assert np.array_equal(first, np.ones_like(first))
    assert np.all(np.abs(total - 1.0) <= bt)


@pytest.mark.parametrize("N,d,P,seed", [(64, 3, 2, 1), (100, 3, 3, 11), (150, 5, 3, 12), (65, 9, 2, 4)])
def test_ordering(N, d, P, seed):
    """first <= total and sum_j first <= 1 (within the bar), the cap on U_S / V the GPU tests rely on"""
    m = _model(N, d, P, seed)
    first, total = R.indices(m["V"])
    bf, bt = R.index_bars(m["V"], R.bar_factor(N, d) * m["UV"])
    assert np.all(m["V"][:, 2 * d] > 0)
    assert np.all(first <= total + bf + bt)
    assert np.all(first.sum(axis=1) <= 1.0 + bf.sum(axis=1))
    assert np.all(first >= -bf)
    ratio = (m["UV"] / m["V"][:, 2 * d:]).max()
    print("U_S / V: %.3g" % ratio)
    assert ratio <= R.CAP
