"""GPU tier of the gradient path: gpb_gp_predict_grad, gpb_emu_predict_jac and gpb_chain_logpost_grad (through GPEngine,
Emulator.predict_jacobian, Chain.log_posterior / log_likelihood(return_grad=True) and Chain.find_map) against the autograd
gradient of the torch restatement in tests/grad_reference.py.  Bars are row-wise: |g - g_ref|_inf <= 1e-9 max(|g_ref|_inf, 1),
the bar of the LML gradient, unless a test states another and why."""
import os

import numpy as np
import pytest

import grad_reference as R

pytestmark = pytest.mark.gpu

BAR = 1e-9


def _rowerr(g, ref):
    g, ref = np.asarray(g).reshape(len(g), -1), np.asarray(ref).reshape(len(ref), -1)
    return np.abs(g - ref).max(1) / np.maximum(np.abs(ref).max(1), 1.0)


def _emulator(tmp, N, d, M, P, kernel="RBF", no_pca=False, expdiag=False, ell=1.5, seed=0, mapped=False, yerr=0.01,
              simulation_error=False):
    """an Emulator trained at fixed hyper-parameters on synthetic data, plus a Chain over it whose experiment is the noiseless
    prediction at the truth point (5 % errors).  yerr: the training events' statistical errors, a number or a callable of the
    observables Y -> [N, M]; simulation_error: stochastic kriging, those errors on the GPs' training diagonals"""
    from gpbayestools_hic_amd import synth
    from gpbayestools_hic_amd.emulator import Emulator
    from gpbayestools_hic_amd.mcmc import Chain
    os.makedirs(tmp, exist_ok=True)
    lo, hi = np.zeros(d), np.ones(d)
    X = synth.lhs(N, d, seed=synth.SEED + seed)
    Y = synth.observables(X, M, seed=synth.SEED + 1 + seed)
    tp, pf, ep = (os.path.join(tmp, n) for n in ("train.pkl", "par.txt", "exp.pkl"))
    synth.write_training_pickle(tp, X, Y, yerr(Y) if callable(yerr) else yerr)
    synth.write_parameter_file(pf, lo, hi)
    emu = Emulator(training_set_path=tp, parameter_file=pf, npc=P, device=0, perform_no_PCA=no_pca,
                   logTrafo=expdiag, exp_and_cov_diagonal=expdiag, parameterTrafoPCA=mapped, simulation_error=simulation_error)
    ktype = {"RBF": "RBF", "Matern15": "Matern", "Matern25": "Matern25"}[kernel]
    ngp = M if no_pca else P
    if mapped:
        ext = np.ptp(emu.PCA_new_design_points, axis=0)
        th = synth.fixed_theta(len(ext), ngp, ell=ell)
        th[:, 1:-1] += np.log(ext)[None, :]
    else:
        th = synth.fixed_theta(d, ngp, ell=ell)
    emu.trainEmulator([True] * emu.nev, kernel_type=ktype, thetas=th)
    xstar = synth.truth_point(d)
    yexp = emu.predict(xstar[None, :], return_cov=False)[0]
    synth.write_experiment_pickle(ep, yexp, 0.05 * np.abs(yexp))
    chain = Chain(mcmc_path=os.path.join(tmp, "mcmc", "chain.pkl"), expdata_path=ep, model_parafile=pf, device=0)
    chain.emuList = [emu]
    return chain, emu, xstar


def _ref_logpost(chain, states, outside=-np.inf):
    return lambda x: R.log_posterior(states, x, chain.min, chain.max, chain.expdata[0], chain.expdata_cov, outside=outside)


def _rows(d, seed, n=12):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.05, 0.95, (n, d))


# ------------------------------------------------------------------ 1. per-GP derivatives
@pytest.mark.parametrize("kernel", ["RBF", "Matern15", "Matern25"])
@pytest.mark.parametrize("d", [8, 20])
def test_predict_grad_matches_autograd(tmp_path, kernel, d):
    _, emu, _ = _emulator(str(tmp_path), 160, d, 6, 3, kernel)
    eng = emu._engine_ready()
    X = _rows(d, 1)
    X[0] = emu._X_train[7]                                    # exactly on a training point
    X[1] = 0.0
    X[2] = 1.0                                                # the box corners
    X[3, ::2] = 0.0
    st = R.state_from_emulator(emu)
    dm, dv = eng.predict_grad(X)
    jm = R.jacobian_rows(lambda x: R.gp_mean_var(st, x)[0], X)
    jv = R.jacobian_rows(lambda x: R.gp_mean_var(st, x)[1], X)
    assert dm.shape == dv.shape == (len(X), 3, d)
    assert np.all(_rowerr(dm, jm) <= BAR), _rowerr(dm, jm)
    assert np.all(_rowerr(dv, jv) <= BAR), _rowerr(dv, jv)
    assert np.array_equal(eng.predict_grad(X, return_var=False), dm)


def test_predict_grad_difference_form(tmp_path):
    """length scales far below the design's extent: the GPs are built in the difference form (GPB_GET_FORM)"""
    _, emu, _ = _emulator(str(tmp_path), 128, 8, 6, 3, "Matern15", ell=0.03)
    eng = emu._engine_ready()
    assert np.all(eng.get("form") == 1)
    X = np.concatenate([emu._X_train[:4] + 1e-3, _rows(8, 2, 4)])
    st = R.state_from_emulator(emu)
    dm, dv = eng.predict_grad(X)
    assert np.all(_rowerr(dm, R.jacobian_rows(lambda x: R.gp_mean_var(st, x)[0], X)) <= BAR)
    assert np.all(_rowerr(dv, R.jacobian_rows(lambda x: R.gp_mean_var(st, x)[1], X)) <= BAR)


# ------------------------------------------------------------------ 2. observable-space Jacobian
@pytest.mark.parametrize("mode", ["pca", "no_pca", "expdiag", "no_pca_expdiag"])
def test_predict_jacobian_modes(tmp_path, mode):
    _, emu, _ = _emulator(str(tmp_path), 128, 8, 8, 4, no_pca="no_pca" in mode, expdiag="expdiag" in mode)
    X = _rows(8, 3)
    st = R.state_from_emulator(emu)
    J = emu.predict_jacobian(X)
    ref = R.jacobian_rows(lambda x: R.emulator_mean_cov(st, x)[0], X)
    assert J.shape == (len(X), emu.nobs, 8)
    assert np.all(_rowerr(J, ref) <= BAR), _rowerr(J, ref)


def test_predict_jacobian_parameter_map(tmp_path):
    """parameterTrafoPCA: against central differences of Emulator.predict (step 1e-6).  Bar 1e-6: the differences carry
    ~eps |y| / h ~ 1e-9 of rounding and h^2 |y'''| of truncation per entry, far above 1e-9 but far below a wrong chain rule."""
    _, emu, _ = _emulator(str(tmp_path), 160, 20, 6, 3, mapped=True)
    X = _rows(20, 4, 6)
    J = emu.predict_jacobian(X)
    h = 1e-6
    fd = np.empty_like(J)
    for q in range(20):
        e = np.zeros(20); e[q] = h
        fd[:, :, q] = (emu.predict(X + e, return_cov=False) - emu.predict(X - e, return_cov=False)) / (2 * h)
    assert np.all(_rowerr(J, fd) <= 1e-6), _rowerr(J, fd)


# ------------------------------------------------------------------ 3. log-posterior gradients
def _check_chain(chain, states, X, finite=False):
    outside = -1e300 if finite else -np.inf
    plain = chain.log_likelihood(X, finite=True) if finite else chain.log_posterior(X)
    lp, g = chain.log_likelihood(X, finite=True, return_grad=True) if finite else chain.log_posterior(X, return_grad=True)
    assert np.array_equal(lp, plain)
    inside = np.all((X > chain.min) & (X < chain.max), axis=1)
    assert np.all(g[~inside] == 0.0) and np.all(lp[~inside] == outside)
    v, gref = R.value_and_grad(_ref_logpost(chain, states, outside), X)
    assert np.all(_rowerr(g[inside], gref[inside]) <= BAR), _rowerr(g[inside], gref[inside])
    return lp, g


@pytest.mark.parametrize("finite", [False, True])
def test_log_posterior_grad_single_emulator(tmp_path, finite):
    chain, emu, xstar = _emulator(str(tmp_path), 128, 8, 4, 4)
    X = _rows(8, 5, 40)
    X[3, 2] = 1.2
    X[9, 0] = 0.0                                             # on the boundary: outside (open box)
    X[20:] = xstar + 0.02 * np.random.default_rng(6).standard_normal((20, 8))
    _check_chain(chain, [R.state_from_emulator(emu)], X, finite)


@pytest.mark.parametrize("mode", ["no_pca", "expdiag", "no_pca_expdiag"])
def test_log_posterior_grad_modes(tmp_path, mode):
    chain, emu, xstar = _emulator(str(tmp_path), 128, 8, 8, 4, no_pca="no_pca" in mode, expdiag="expdiag" in mode)
    X = xstar + 0.05 * np.random.default_rng(7).standard_normal((24, 8))
    _check_chain(chain, [R.state_from_emulator(emu)], X)


def test_log_posterior_grad_cfg3_lowrank_and_dense(tmp_path):
    """cfg 3 (N 1024, d 15, M 32, npc 10: the low-rank block likelihood) at 512 rows, and npc 20 > 16 (the dense block)"""
    from gpbayestools_hic_amd import synth
    for npc, sub in ((10, "a"), (20, "b")):
        chain, emu, xstar = _emulator(str(tmp_path / sub), 1024, 15, 32, npc)
        X = synth.walkers_ball(512, xstar, radius=0.05, seed=8)
        X[::37, 4] = 1.5
        _check_chain(chain, [R.state_from_emulator(emu)], X)


def test_log_posterior_grad_nine_emulators(tmp_path):
    from gpbayestools_hic_amd.workload import build_multi_chain
    from test_gpu_multi_emulator import SPECS, D
    chain, emus, info = build_multi_chain(SPECS, D, workdir=str(tmp_path))
    X = info["xstar"] + 0.03 * np.random.default_rng(9).standard_normal((32, D))
    X[5, 1] = 1.1
    _check_chain(chain, [R.state_from_emulator(e) for e in emus], X)


def test_log_posterior_grad_nine_mapped_emulators(tmp_path):
    """parameterTrafoPCA on every emulator (d = 20): against central differences of the log-posterior (step 1e-6).  Bar
    1e-5 relative to max(|g|_inf, 1): rounding of lp (~1e-13 |lp| / h) and truncation, not the 1e-9 of the unmapped chains."""
    from gpbayestools_hic_amd.workload import build_multi_chain
    from test_gpu_multi_emulator import SPECS
    chain, emus, info = build_multi_chain(SPECS, 20, workdir=str(tmp_path), mapped=True)
    X = np.clip(info["xstar"] + 0.02 * np.random.default_rng(10).standard_normal((4, 20)), 0.01, 0.99)
    lp, g = chain.log_posterior(X, return_grad=True)
    assert np.array_equal(lp, chain.log_posterior(X))
    h = 1e-6
    fd = np.empty_like(g)
    for q in range(20):
        e = np.zeros(20); e[q] = h
        fd[:, q] = (chain.log_posterior(X + e) - chain.log_posterior(X - e)) / (2 * h)
    assert np.all(_rowerr(g, fd) <= 1e-5), _rowerr(g, fd)


# ------------------------------------------------------------------ 4. batch invariance
def test_gradient_rows_do_not_depend_on_the_batch(tmp_path):
    chain, emu, _ = _emulator(str(tmp_path), 256, 8, 6, 4)
    X = np.random.default_rng(11).uniform(0.0, 1.0, (2048, 8))
    lp, g = chain.log_posterior(X, return_grad=True)
    chain.grad_slab_rows = 1024                               # two slabs: rows 1023 | 1024 on either side of the cut
    lp2, g2 = chain.log_posterior(X, return_grad=True)
    assert np.array_equal(lp, lp2) and np.array_equal(g, g2)
    for w in (0, 1023, 1024, 2047):
        lw, gw = chain.log_posterior(X[w:w + 1], return_grad=True)
        assert np.array_equal(lw, lp[w:w + 1]) and np.array_equal(gw, g[w:w + 1])
    J = emu.predict_jacobian(X)
    assert np.array_equal(emu.predict_jacobian(X[1000:1100]), J[1000:1100])


# ------------------------------------------------------------------ 5. MAP search
def test_find_map_closure(tmp_path):
    import scipy.optimize
    chain, emu, xstar = _emulator(str(tmp_path), 128, 6, 4, 4, ell=0.8)
    lp_star = chain.log_posterior(xstar[None, :])[0]
    Xo, lpo = chain.find_map(nstarts=8, seed=3)
    assert Xo.shape == (8, 6) and np.all(np.diff(lpo) <= 0.0)
    assert lpo[0] >= lp_star - 1e-8, (lpo[0], lp_star)
    lpb, gb = chain.log_posterior(Xo[:1], return_grad=True)
    eps = 1e-9 * (chain.max - chain.min)
    lo, hi = chain.min + eps, chain.max - eps
    pg = np.where((Xo[0] <= lo) & (gb[0] < 0), 0.0, np.where((Xo[0] >= hi) & (gb[0] > 0), 0.0, gb[0]))
    # 1e-4, not 1e-5: scipy's L-BFGS-B stops on its relative-decrease test (factr 1e7: 2.2e-9 |lp|, |lp| ~ 1e2 here) before its
    # projected-gradient test; measured worst component 2.8e-5 at the first run of this test
    assert np.max(np.abs(pg)) <= 1e-4, pg
    draws = np.random.default_rng(12).uniform(chain.min, chain.max, (4096, 6))
    assert lpo[0] >= np.max(chain.log_posterior(draws))
    # one start, driven by scipy's own minimize on the same device function: the same point bit for bit
    X0 = np.random.default_rng(13).uniform(chain.min, chain.max, (3, 6))
    Xl, _ = chain.find_map(X0=X0)

    def f(x):
        v, g = chain.log_posterior(x[None, :], return_grad=True)
        return -v[0], -g[0]
    res = scipy.optimize.minimize(f, X0[1], method="L-BFGS-B", jac=True, bounds=np.stack([lo, hi], 1))
    assert any(np.array_equal(res.x, x) for x in Xl)


# ------------------------------------------------------------------ 6. protocol
def test_protocol(tmp_path):
    chain, emu, _ = _emulator(str(tmp_path), 96, 5, 4, 3)
    X = _rows(5, 14, 7)
    out = chain.log_posterior(X)
    assert isinstance(out, np.ndarray) and out.shape == (7,)
    lp, g = chain.log_posterior(X, return_grad=True)
    assert lp.shape == (7,) and g.shape == (7, 5)
    lp1, g1 = chain.log_likelihood(X[0], return_grad=True)
    assert lp1.shape == (1,) and g1.shape == (1, 5)
    assert isinstance(chain.log_likelihood(X, return_grad=False), np.ndarray)

    class Foreign:                                            # the reference's predict protocol, host-side
        def __init__(self, e):
            self.e, self.nobs = e, e.nobs

        def predict(self, X, return_cov=True, extra_std=0.0):
            return self.e.predict(X, return_cov=return_cov, extra_std=extra_std)
    chain.emuList = [Foreign(emu)]
    assert chain.log_posterior(X).shape == (7,)
    with pytest.raises(NotImplementedError):
        chain.log_posterior(X, return_grad=True)
