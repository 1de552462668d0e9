"""CPU tier: the stochastic-kriging reference (tests/sk_reference.py) against independent statements of the same quantities.
  * the oracle with a VECTOR alpha is sklearn's GPR(alpha=<array>) (L_, alpha_, LML and its gradient), <= 1e-13;
  * the cross-validation closed form with diag(t_F) equals the refit with t[keep], at tests/test_cv_reference.py's bars;
  * the design score with tau[p][c] equals the refit drop, as tests/test_design_reference.py checks the scalar model;
  * the projection s is the variance of transform(S + noise) — algebraically: unit errors on one observable at a time;
  * the GPU design case of tests/test_gpu_point_noise.py has a top-two gap far above that test's bar at every step."""
import numpy as np
import pytest

import cv_reference as CV
import sk_reference as SK
from conftest import maxrel, relerr
from oracle import gp_oracle as O

MEAN_BAR, VAR_BAR = 1e-12, 1e-11          # tests/test_cv_reference.py


@pytest.mark.parametrize("kernel", ["RBF", "Matern", "Matern25"])
def test_oracle_with_vector_alpha_is_sklearn(kernel):
    pytest.importorskip("sklearn")
    from sklearn.gaussian_process import GaussianProcessRegressor as GPR
    from sklearn.gaussian_process.kernels import RBF, ConstantKernel, Matern, WhiteKernel
    N, d = 70, 5
    X, Z = CV.make_data(N, d, 1, seed=21)
    z, th = Z[0], CV.theta_of("aniso", d)
    t = SK.ALPHA + SK.noise_rows(1, N, seed=22)[0]
    ell = np.exp(th[1:d + 1])
    inner = RBF(ell) if kernel == "RBF" else Matern(ell, nu=1.5 if kernel == "Matern" else 2.5)
    gp = GPR(ConstantKernel(np.exp(th[0])) * inner + WhiteKernel(np.exp(th[-1])), alpha=t, optimizer=None).fit(X, z)
    assert np.allclose(gp.kernel_.theta, th, rtol=0, atol=1e-15)
    L, a = O.gp_factor(X, z, th, SK.KINDS[kernel], t)
    v, g = O.lml(th, X, z, SK.KINDS[kernel], t, eval_gradient=True)
    vs, gs = gp.log_marginal_likelihood(gp.kernel_.theta, eval_gradient=True)
    eL, ea = maxrel(L, gp.L_), maxrel(a, gp.alpha_)
    ev, eg = abs(v - vs) / abs(vs), maxrel(g, gs)
    print("vector alpha, oracle against sklearn: L %.2g, alpha_ %.2g, LML %.2g, gradient %.2g" % (eL, ea, ev, eg))
    assert eL <= 1e-13 and ea <= 1e-13 and ev <= 1e-13 and eg <= 1e-13


def _cv_agree(X, z, theta, kind, t, folds):
    cf = SK.cv_closed_form(X, z, theta, kind, t, folds)
    bf = SK.cv_brute_force(X, z, theta, kind, t, folds)
    for F, (mc, cc), (mb, cb) in zip(folds, cf, bf):
        em = CV.mean_err(mc, mb, z[np.asarray(F)])
        ev, ec = relerr(np.diag(cc), np.diag(cb)), maxrel(cc, cb)
        assert em < MEAN_BAR and ev < VAR_BAR and ec < VAR_BAR, (em, ev, ec)


@pytest.mark.parametrize("kernel", ["RBF", "Matern", "Matern25"])
def test_cv_closed_form_is_the_refit(kernel):
    for N in (70, 128):
        d = 5
        X, Z = CV.make_data(N, d, 3, seed=12)
        s = SK.noise_rows(3, N, seed=31)
        all_folds = [[[i] for i in range(N)]] + [CV.contiguous_folds(N, k) for k in (2, 7, 64)] + [CV.shuffled_folds(N, 7, seed=5)]
        for folds in all_folds:
            for p, name in enumerate(("mid", "hard", "aniso")):
                _cv_agree(X, Z[p], CV.theta_of(name, d), SK.KINDS[kernel], SK.ALPHA + s[p], folds)


def test_cv_scalar_noise_is_the_scalar_reference():
    """a uniform t is cv_reference's scalar alpha: the two helper modules state one model"""
    N, d = 70, 5
    X, Z = CV.make_data(N, d, 1, seed=12)
    th, folds = CV.theta_of("mid", d), CV.contiguous_folds(N, 7)
    a = CV.closed_form(X, Z[0], th, O.KIND_RBF, 0.15, folds)
    b = SK.cv_closed_form(X, Z[0], th, O.KIND_RBF, np.full(N, 0.15), folds)
    for (ma, ca), (mb, cb) in zip(a, b):
        assert np.array_equal(ma, mb) and np.array_equal(ca, cb)


@pytest.mark.parametrize("kernel,seed", [("RBF", 2), ("Matern", 4), ("Matern25", 5)])
def test_design_scores_are_the_refit_drop(kernel, seed):
    c = SK.design_case(N=40, d=3, P=2, C=20, R=25, seed=seed, kernel=kernel)
    T, C = 4, 20
    t, t_c = SK.ALPHA + c["s"], SK.ALPHA + c["s_c"]
    args = (c["X"], c["theta"], kernel, t, c["Xc"], c["Xr"], c["w"], c["g"])
    m = SK.design_greedy(*args, T, t_c)
    assert np.all(m["gain"] >= 0.0)
    chosen, el = [], np.ones(C, dtype=bool)
    for step in range(T):
        J, base = SK.design_refit_scores(*args, t_c, chosen)
        if step == 0:
            assert abs(base - m["variance0"]) <= 1e-12 * m["variance0"]
        top = J[el].max()
        assert np.all(np.abs(m["scores"][step][el] - J[el]) <= 1e-11 * top)
        b = int(np.argmax(np.where(el, J, -np.inf)))
        assert b == m["picks"][step] and m["gain"][step] == m["scores"][step][b]
        chosen.append(b)
        el[b] = False
    final = SK.design_refit_scores(*args, t_c, chosen)[1]
    assert abs((m["variance0"] - m["gain"].sum()) - final) <= 1e-11 * m["variance0"]


def test_design_noise_matters_and_reduces_to_the_scalar_model():
    import design_reference as D
    c = SK.design_case()
    N, C = c["X"].shape[0], c["Xc"].shape[0]
    P = c["theta"].shape[0]
    args = (c["X"], c["theta"], "RBF")
    rest = (c["Xc"], c["Xr"], c["w"], c["g"], 5)
    scalar = D.greedy(*args, *rest, alpha_reg=SK.ALPHA)
    same = SK.design_greedy(*args, np.full((P, N), SK.ALPHA), *rest, np.full((P, C), SK.ALPHA))
    assert np.array_equal(scalar["picks"], same["picks"]) and np.allclose(scalar["gain"], same["gain"], rtol=1e-12, atol=0)
    noisy = SK.design_greedy(*args, np.full((P, N), SK.ALPHA), *rest, SK.ALPHA + c["s_c"])
    assert not np.array_equal(noisy["scores"][0], same["scores"][0])
    assert np.all(noisy["scores"][0] < same["scores"][0])            # a noisier observation teaches less, at every candidate


def test_gpu_design_case_has_clear_winners():
    """the case tests/test_gpu_point_noise.py runs (C = 40, R = 30, T = 5): the device must reproduce the picks, so at every step
    the best score leads the second best by far more than that test's bar of 1e-9 max J"""
    c = SK.design_case()
    m = SK.design_greedy(c["X"], c["theta"], "RBF", SK.ALPHA + c["s"], c["Xc"], c["Xr"], c["w"], c["g"], 5, SK.ALPHA + c["s_c"])
    print("top-two gaps of the GPU design case:", m["gaps"])
    assert np.all(m["gaps"] >= 1e-6)
    assert c["s_c"].max() / c["s_c"].min() >= 30.0                   # the candidates' noise does span about two decades


def test_projection_is_the_variance_of_the_transformed_noise():
    """transform is linear: a unit error on observable m alone moves whitened PC k by comp[k, m] / (scale[m] sqrt(ev[k])).
    Independent errors add in variance, so s[k, i] must be sum_m E[i, m]^2 x (that response)^2: push the unit vectors through
    the package's own Standardizer / WhitenedPCA and compare"""
    from gpbayestools_hic_amd.emulator import project_errors
    from gpbayestools_hic_amd.preprocess import Standardizer, WhitenedPCA
    rng = np.random.default_rng(7)
    n, nobs, npc = 40, 6, 4
    Y = rng.standard_normal((n, nobs)) @ rng.standard_normal((nobs, nobs)) + rng.standard_normal(nobs)
    E = rng.uniform(0.01, 0.1, size=(n, nobs))
    sc, pc = Standardizer(), WhitenedPCA()
    Z0 = pc.fit_transform(sc.fit_transform(Y))
    resp = np.empty((nobs, npc))                                      # d z_k / d y_m, from the transform itself
    for m in range(nobs):
        e = np.zeros(nobs); e[m] = 1.0
        resp[m] = (pc.transform(sc.transform(Y[:1] + e)) - Z0[:1])[0, :npc]
    want = (E ** 2 @ resp ** 2).T                                     # [npc, n]
    got = project_errors(E, sc.scale_, pc.components_, pc.explained_variance_, npc)
    ref = SK.projection(E, sc.scale_, pc.components_, pc.explained_variance_, npc)
    assert got.shape == (npc, n)
    assert relerr(got, ref) < 1e-14 and relerr(got, want) < 1e-10     # (the finite response carries the transform's rounding)
    # without the PCA: one GP per observable
    got0, ref0 = project_errors(E, sc.scale_), SK.projection(E, sc.scale_)
    assert got0.shape == (nobs, n) and relerr(got0, ref0) < 1e-15
    resp0 = np.array([(sc.transform(Y[:1] + np.eye(nobs)[m]) - sc.transform(Y[:1]))[0, m] for m in range(nobs)])
    assert relerr(got0, (E * resp0).T ** 2) < 1e-10
