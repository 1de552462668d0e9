"""GPU tier: Emulator(simulation_error=True) — stochastic kriging through the public classes.  The training
pickle is written in tmp_path: 96 events x 6 observables over 3 parameters; the statistical errors vary over events and
observables and stay below 10 % relative, so no event is dropped.  References: tests/sk_reference.py's projection, the numpy
oracle with vector alphas (sklearn's GPR(alpha=<array>), tests/test_sk_reference.py), and the engine-level entry points."""
import types

import numpy as np
import pytest

import sk_reference as SK
from conftest import maxrel, relerr
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

NEV, D_IN, NOBS, NPC = 96, 3, 6, 3


def _training_data(seed=0):
    from gpbayestools_hic_amd import synth
    X = synth.lhs(NEV, D_IN, seed=100 + seed)
    Y = synth.observables(X, NOBS, seed=200 + seed)                  # 2 + sin + cos / 2 + noise: in [0.4, 3.6]
    rel = np.random.default_rng(300 + seed).uniform(0.005, 0.08, size=Y.shape)
    return X, Y, np.abs(Y) * rel


def _emulator(tmp_path, X, Y, E, tag="e", **kw):
    from gpbayestools_hic_amd import Emulator, synth
    tp, pf = str(tmp_path / (tag + "_train.pkl")), str(tmp_path / (tag + "_par.txt"))
    synth.write_training_pickle(tp, X, Y, E)
    synth.write_parameter_file(pf, np.zeros(D_IN), np.ones(D_IN))
    kw.setdefault("simulation_error", True)
    emu = Emulator(training_set_path=tp, parameter_file=pf, npc=NPC, **kw)
    assert emu.nev == X.shape[0]                                      # nothing dropped
    return emu


def _thetas(P):
    from gpbayestools_hic_amd import synth
    th = synth.fixed_theta(D_IN, P, c=1.0, ell=0.9, noise=0.02)
    th[:, 0] += np.linspace(0.0, 0.5, P)
    th[:, 1] += np.linspace(-0.3, 0.3, P)
    return th


ALL = [True] * NEV


def _oracle_sk(X, Y, E, thetas, alpha, mode=O.MODE_PCA):
    """the oracle emulator with the vector alpha + s on every GP's diagonal"""
    emu = O.OracleEmulator(X, Y, np.zeros(D_IN), np.ones(D_IN), NPC, O.KIND_RBF, mode, alpha)
    if mode == O.MODE_PCA:
        s = SK.projection(E, emu.scale, emu.components, emu.explained_variance, NPC)
    else:
        s = SK.projection(E, emu.scale)
    emu.thetas, emu.L, emu.a = np.asarray(thetas, dtype=np.float64), [], []
    for p in range(emu.npc):
        L, a = O.gp_factor(emu.X, np.ascontiguousarray(emu.Z[:, p]), emu.thetas[p], O.KIND_RBF, alpha + s[p])
        emu.L.append(L); emu.a.append(a)
    return emu, s


@pytest.mark.parametrize("no_pca", [False, True])
def test_projection_and_predict_at_fixed_theta(tmp_path, no_pca):
    X, Y, E = _training_data()
    emu = _emulator(tmp_path, X, Y, E, perform_no_PCA=no_pca)
    P = NOBS if no_pca else NPC
    th = _thetas(P)
    emu.trainEmulator(ALL, thetas=th)
    if no_pca:
        want = SK.projection(E, emu.scaler.scale_)
    else:
        want = SK.projection(E, emu.scaler.scale_, emu.pca.components_, emu.pca.explained_variance_, NPC)
    assert emu.point_noise_.shape == (P, NEV) and relerr(emu.point_noise_, want) < 1e-14
    assert emu.point_noise_.min() > 0.0 and emu.point_noise_.max() / emu.point_noise_.min() > 10.0      # it does vary
    ora, s = _oracle_sk(X, Y, E, th, emu.alpha, O.MODE_NO_PCA if no_pca else O.MODE_PCA)
    assert relerr(emu.point_noise_, s) < 1e-10                        # (the oracle's own scaler and PCA)
    Xs = np.random.default_rng(5).uniform(size=(33, D_IN))
    es = np.linspace(0.0, 0.2, 33)
    mean, cov = emu.predict(Xs, return_cov=True, extra_std=es)
    mo, co = ora.predict(Xs, True, es)
    em, ec = relerr(mean, mo), maxrel(cov, co)
    print("predict against the vector-alpha oracle: mean %.2g, cov %.2g" % (em, ec))
    assert em < 1e-11 and ec < 1e-10
    # and the noise reaches the fit: the same emulator without it predicts something else
    plain = _emulator(tmp_path, X, Y, E, tag="p", perform_no_PCA=no_pca, simulation_error=False)
    plain.trainEmulator(ALL, thetas=th)
    assert plain.point_noise_ is None and relerr(plain.predict(Xs, return_cov=False), mo) > 1e-6


def test_search_against_oracle(tmp_path):
    """the full hyper-parameter search against gp_oracle.gp_fit_theta with the vector alpha, from the same start: LML* within
    1e-7 relative and theta* within atol = 5e-3 (tests/test_gpu_dropin.py's two numbers against sklearn's search)"""
    X, Y, E = _training_data()
    emu = _emulator(tmp_path, X, Y, E)
    emu.trainEmulator(ALL)
    th0, bnd = emu._theta0_bounds("RBF")
    for p in range(NPC):
        tho, vo = O.gp_fit_theta(emu._X_train, emu._Z_train[p], th0, bnd, O.KIND_RBF, emu.alpha + emu.point_noise_[p])
        print("GP %d: LML* %.10g (oracle %.10g), |dtheta| %.2g" % (p, emu.lml_[p], vo, np.max(np.abs(emu.thetas_[p] - tho))))
        assert abs(emu.lml_[p] - vo) < 1e-7 * abs(vo)
        assert np.allclose(emu.thetas_[p], tho, atol=5e-3)


def test_train_emulators_together_and_masked_training(tmp_path):
    from gpbayestools_hic_amd.emulator import train_emulators
    Xa, Ya, Ea = _training_data(0)
    Xb, Yb, Eb = _training_data(1)
    alone = [_emulator(tmp_path, Xa, Ya, Ea, "a1"), _emulator(tmp_path, Xb, Yb, Eb, "b1", simulation_error=False)]
    for e in alone:
        e.trainEmulator(ALL)
    both = [_emulator(tmp_path, Xa, Ya, Ea, "a2"), _emulator(tmp_path, Xb, Yb, Eb, "b2", simulation_error=False)]
    train_emulators(both)                                            # one batch: a with its rows, b with zero rows
    for e1, e2 in zip(alone, both):
        assert np.array_equal(e1.thetas_, e2.thetas_) and np.array_equal(e1.lml_, e2.lml_)
    # a masked training uses the masked rows: the bits of an emulator built from the reduced pickle
    mask = np.ones(NEV, dtype=bool)
    mask[[3, 40, 41, 95]] = False
    th = _thetas(NPC)
    full = both[0]
    full.trainEmulator(mask, thetas=th)
    red = _emulator(tmp_path, Xa[mask], Ya[mask], Ea[mask], "r")
    red.trainEmulator([True] * red.nev, thetas=th)
    assert np.array_equal(full.point_noise_, red.point_noise_) and full.point_noise_.shape == (NPC, NEV - 4)
    Xs = np.random.default_rng(6).uniform(size=(20, D_IN))
    for a, b in zip(full.predict(Xs), red.predict(Xs)):
        assert np.array_equal(a, b)
    # the hold-out helper retrains on a subset: its noise is the subset's
    full.testEmulatorErrors(nTestPoints=8, thetas=th)
    assert full.point_noise_.shape == (NPC, NEV - 8)


def test_digest_pickle_and_cross_validate(tmp_path):
    import dill
    X, Y, E = _training_data()
    th = _thetas(NPC)
    emu = _emulator(tmp_path, X, Y, E)
    emu.trainEmulator(ALL, thetas=th)
    E2 = E.copy()
    E2[17, 2] *= 1.01
    other = _emulator(tmp_path, X, Y, E2, "o")
    other.trainEmulator(ALL, thetas=th)
    plain = _emulator(tmp_path, X, Y, E, "p", simulation_error=False)
    plain.trainEmulator(ALL, thetas=th)
    again = _emulator(tmp_path, X, Y, E, "s")
    again.trainEmulator(ALL, thetas=th)
    assert emu.state_digest() == again.state_digest()
    assert emu.state_digest() != other.state_digest() and emu.state_digest() != plain.state_digest()
    # pickle round trip: the same bits
    Xs = np.random.default_rng(7).uniform(size=(20, D_IN))
    back = dill.loads(dill.dumps(emu))
    assert back.simulation_error_ and np.array_equal(back.point_noise_, emu.point_noise_)
    assert back.state_digest() == emu.state_digest()
    for a, b in zip(emu.predict(Xs), back.predict(Xs)):
        assert np.array_equal(a, b)
    # a state pickled before the feature existed has neither attribute: it loads, as an emulator without the noise
    st = plain.__getstate__()
    st.pop("simulation_error_"); st.pop("point_noise_")
    old = type(plain).__new__(type(plain))
    old.__setstate__(st)
    assert old.simulation_error_ is False and old.point_noise_ is None and old.state_digest() == plain.state_digest()
    assert np.array_equal(old.predict(Xs, return_cov=False), plain.predict(Xs, return_cov=False))
    # cross_validate = the engine-level CV of the GPs through the observable transform
    folds = [np.arange(i, NEV, 16) for i in range(16)]               # 16 folds of 6 events
    pred, perr, truth, terr = emu.cross_validate(folds)
    gm, gv = emu._engine_ready().cross_validate(folds)
    mo, co = O.emulator_predict(gm, gv, np.zeros(gm.shape[0]), mode=O.MODE_PCA, A=emu._A, mu=emu.scaler.mean_, cov_trunc=emu._cov_trunc)
    flat = np.concatenate(folds)
    assert relerr(pred, mo) < 1e-11 and relerr(perr ** 2, np.diagonal(co, axis1=1, axis2=2)) < 1e-10
    assert np.array_equal(truth, Y[flat]) and np.array_equal(terr, E[flat])
    # ... which is the refit without the fold, with the remaining events' noise (sk_reference's brute force), GP by GP
    for p in range(NPC):
        bf = SK.cv_brute_force(emu._X_train, emu._Z_train[p], th[p], O.KIND_RBF, emu.alpha + emu.point_noise_[p], folds[:3])
        q = 0
        for (mb, cb) in bf:
            k = mb.shape[0]
            assert maxrel(gm[q:q + k, p], mb) < 1e-11 and relerr(gv[q:q + k, p], np.diag(cb)) < 1e-10
            q += k


def test_propose_design_with_candidate_error(tmp_path):
    X, Y, E = _training_data()
    th = _thetas(NPC)
    emu = _emulator(tmp_path, X, Y, E)
    emu.trainEmulator(ALL, thetas=th)
    rng = np.random.default_rng(8)
    cand = rng.uniform(size=(40, D_IN))
    ce = 2.0 * np.abs(rng.uniform(0.005, 0.5, size=(40, NOBS)))
    g = emu._design_gp_weights(None)
    w = np.full(40, 1.0 / 40)
    s_c = SK.projection(ce, emu.scaler.scale_, emu.pca.components_, emu.pca.explained_variance_, NPC)
    t = emu.alpha + emu.point_noise_
    model = SK.design_greedy(emu._X_train, th, "RBF", t, cand, cand, w, g, 4, emu.alpha + s_c)
    assert np.all(model["gaps"] > 1e-6)
    got = emu.propose_design(4, cand, candidate_error=ce, return_scores=True)
    assert np.array_equal(got.indices, model["picks"])
    top = np.array([row[np.isfinite(row)].max() for row in model["scores"]])
    assert np.all(np.abs(got.gain - model["gain"]) < 1e-9 * top)
    # None on a simulation_error emulator: every GP's mean training noise at every candidate
    mean_noise = np.repeat(emu.point_noise_.mean(axis=1)[:, None], 40, axis=1)
    m2 = SK.design_greedy(emu._X_train, th, "RBF", t, cand, cand, w, g, 4, emu.alpha + mean_noise)
    got2 = emu.propose_design(4, cand, return_scores=True)
    assert np.all(m2["gaps"] > 1e-6) and np.array_equal(got2.indices, m2["picks"])
    assert np.all(np.abs(got2.gain - m2["gain"]) < 1e-9 * np.array([row[np.isfinite(row)].max() for row in m2["scores"]]))
    with pytest.raises(ValueError):
        emu.propose_design(4, cand, candidate_error=ce[:, :-1])
    with pytest.raises(ValueError):
        emu.propose_design(4, cand, candidate_error=-ce)
    # the chain splits the columns per emulator
    from gpbayestools_hic_amd import Chain, synth
    ep = str(tmp_path / "exp.pkl")
    yexp = emu.predict(np.full((1, D_IN), 0.5), return_cov=False)[0]
    synth.write_experiment_pickle(ep, np.concatenate([yexp, yexp]), 0.05 * np.abs(np.concatenate([yexp, yexp])))
    emu_b = _emulator(tmp_path, X, Y, E, "b", simulation_error=False)
    emu_b.trainEmulator(ALL, thetas=th)
    chain = Chain(mcmc_path=str(tmp_path / "mcmc" / "chain.pkl"), expdata_path=ep, model_parafile=str(tmp_path / "e_par.txt"))
    chain.emuList = [emu, emu_b]
    ce2 = np.concatenate([ce, 0.5 * ce], axis=1)
    u = 1.0 / np.diag(chain.expdata_cov)
    got3 = chain.propose_design(3, cand, candidate_error=ce2, return_scores=True)
    Ja = SK.design_greedy(emu._X_train, th, "RBF", t, cand, cand, w, emu._design_gp_weights(u[:NOBS]), 1, emu.alpha + s_c)
    sb = SK.projection(0.5 * ce, emu_b.scaler.scale_, emu_b.pca.components_, emu_b.pca.explained_variance_, NPC)
    Jb = SK.design_greedy(emu_b._X_train, th, "RBF", np.full_like(t, emu_b.alpha), cand, cand, w, emu_b._design_gp_weights(u[NOBS:]),
                          1, emu_b.alpha + sb)
    J0 = Ja["scores"][0] + Jb["scores"][0]
    assert np.max(np.abs(got3.scores[0] - J0)) < 1e-9 * J0.max()
    with pytest.raises(ValueError):
        chain.propose_design(3, cand, candidate_error=ce)


def test_from_reference_with_array_alphas(tmp_path):
    pytest.importorskip("sklearn")
    from sklearn.gaussian_process import GaussianProcessRegressor as GPR
    from sklearn.gaussian_process.kernels import RBF, ConstantKernel, WhiteKernel
    from gpbayestools_hic_amd import Emulator
    X, Y, E = _training_data()
    th = _thetas(NPC)
    mu, scale, var = O.standardize_fit(Y)
    Zfull, comps, ev, pmean = O.pca_whiten_fit((Y - mu) / scale)
    s = SK.projection(E, scale, comps, ev, NPC)
    gps = []
    for p in range(NPC):
        k = ConstantKernel(np.exp(th[p, 0])) * RBF(np.exp(th[p, 1:1 + D_IN])) + WhiteKernel(np.exp(th[p, -1]))
        gps.append(GPR(k, alpha=0.03 * (p + 1) + s[p], optimizer=None).fit(X, Zfull[:, p]))      # another array per GP
    ns = types.SimpleNamespace
    ref = ns(logTrafo_=False, parameterTrafoPCA_=False, exp_and_cov_diagonal_=False, perform_no_PCA_=False, npc=NPC, nrestarts=0,
             pardict=None, gps=gps, design_points=X, model_data=Y, model_data_err=E, design_min=np.zeros(D_IN), design_max=np.ones(D_IN),
             scaler=ns(mean_=mu, scale_=scale, var_=var),
             pca=ns(n_components_=NOBS, mean_=pmean, components_=comps, explained_variance_=ev, explained_variance_ratio_=ev / ev.sum()))
    with pytest.raises(ValueError, match="simulation_error=True"):    # not without being asked: the call of before refuses as before
        Emulator.from_reference(ref)
    emu = Emulator.from_reference(ref, simulation_error=True)
    assert emu.alpha == 0.0 and emu.simulation_error_
    assert np.array_equal(emu.point_noise_, np.array([g.alpha for g in gps]))
    # the sklearn emulator's arithmetic, restated: per-GP predict, then the observable transform
    Xs = np.random.default_rng(9).uniform(size=(25, D_IN))
    pm, pv = [], []
    for g in gps:
        m, sd = g.predict(Xs, return_std=True)
        pm.append(m); pv.append(sd ** 2)
    T, _, cov_trunc = O.emulator_transforms(comps, ev, scale, var, NPC)
    mo, co = O.emulator_predict(np.stack(pm, 1), np.stack(pv, 1), np.zeros(25), mode=O.MODE_PCA, A=T[:NPC], mu=mu, cov_trunc=cov_trunc)
    mean, cov = emu.predict(Xs, return_cov=True)
    em, ec = relerr(mean, mo), maxrel(cov, co)
    print("adopted vector-alpha emulator against sklearn's arithmetic: mean %.2g, cov %.2g" % (em, ec))
    assert em < 1e-10 and ec < 1e-10
    # wrong length, and a scalar among the arrays: refused
    gps[1].alpha = gps[1].alpha[:-1]
    with pytest.raises(ValueError, match="one entry per training point"):
        Emulator.from_reference(ref, simulation_error=True)
    gps[1].alpha = 0.1
    with pytest.raises(ValueError, match="mix"):
        Emulator.from_reference(ref, simulation_error=True)


def test_zero_errors_give_the_plain_emulators_bits(tmp_path):
    """alpha + 0 is formed first: an emulator whose events carry no error searches, predicts and draws its learning curves
    exactly as one without the option; with the errors the learning curves' fits take the folds' own rows and move"""
    X, Y, E = _training_data()
    zero = _emulator(tmp_path, X, Y, np.zeros_like(E), "z")
    plain = _emulator(tmp_path, X, Y, E, "p", simulation_error=False)
    zero.trainEmulator(ALL)
    plain.trainEmulator(ALL)
    assert np.all(zero.point_noise_ == 0.0) and plain.point_noise_ is None
    assert np.array_equal(zero.thetas_, plain.thetas_) and np.array_equal(zero.lml_, plain.lml_)
    Xs = np.random.default_rng(11).uniform(size=(10, D_IN))
    for a, b in zip(zero.predict(Xs), plain.predict(Xs)):
        assert np.array_equal(a, b)
    cz, cp = zero.print_learning_curve(), plain.print_learning_curve()
    assert len(cz) == NPC and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(cz, cp))
    noisy = _emulator(tmp_path, X, Y, E, "n")
    cn = noisy.print_learning_curve()
    assert all(a.shape == b.shape for a, b in zip(cn, cp))
    assert any(not np.array_equal(a, b, equal_nan=True) for a, b in zip(cn, cp))
