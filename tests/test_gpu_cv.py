"""GPU tier: closed-form leave-one-out / leave-k-out cross-validation on the device (gpb_gp_cv, gpb_emu_cv,
GPEngine.cross_validate / emu_cross_validate, Emulator.cross_validate) against brute-force refits on the host
(tests/cv_reference.brute_force: oracle gp_factor on the remaining rows + gp_predict_cov).
Bars: mean 1e-11 x max(|z|, 1); variance relerr 1e-10; fold covariance maxrel 1e-10.
Measured on an MI355X over all cases here: mean 7.9e-13, variance 3.1e-12, fold covariance 1.9e-12 (the largest at N = 1000, "hard"
theta, where the host references themselves carry ~6e-13)."""
import functools

import numpy as np
import pytest

import cv_reference as R
from conftest import maxrel, relerr
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

MEAN_BAR, VAR_BAR = 1e-11, 1e-10
KERNELS = ["RBF", "Matern", "Matern25"]
THREE = ("mid", "hard", "aniso")


def _engine(X, Z, kernel, thetas):
    from gpbayestools_hic_amd import GPEngine
    eng = GPEngine(0)
    eng.set_data(X, Z, kernel, R.ALPHA)
    eng.set_theta(thetas)
    eng.factor()
    return eng


@functools.lru_cache(maxsize=None)
def _case(N, d, P, seed, names):
    X, Z = R.make_data(N, d, P, seed)
    return X, Z, R.thetas_of(names, d)


def _check(got, folds, X, Z, thetas, kernel, host=None, which=None):
    """device (mean [n, P], var [n, P], cov [P, nf, kmax, kmax] or None) against brute-force refits — or against host[p][f],
    per-GP results computed before — fold by fold (which: a subset of the folds)"""
    mean, var, cov = got
    kind = R.KINDS[kernel]
    worst = [0.0, 0.0, 0.0]
    off = np.concatenate([[0], np.cumsum([len(f) for f in folds])])
    for p in range(Z.shape[0]):
        sel = range(len(folds)) if which is None else which
        res = [host[p][f] for f in sel] if host else R.brute_force(X, Z[p], thetas[p], kind, R.ALPHA, [folds[f] for f in sel])
        for f, (mr, cr) in zip(sel, res):
            F, sl, k = np.asarray(folds[f]), slice(off[f], off[f + 1]), len(folds[f])
            worst[0] = max(worst[0], R.mean_err(mean[sl, p], mr, Z[p][F]))
            worst[1] = max(worst[1], relerr(var[sl, p], np.diag(cr)))
            if cov is not None:
                worst[2] = max(worst[2], maxrel(cov[p, f, :k, :k], cr))
                pad = cov[p, f].copy()
                pad[:k, :k] = 0.0
                assert not pad.any()
    print("cv errors (mean, var, cov): %.2e %.2e %.2e" % tuple(worst))
    assert worst[0] < MEAN_BAR and worst[1] < VAR_BAR and worst[2] < VAR_BAR, worst


# ---------------------------------------------------------------------------- 1. leave-one-out
@pytest.mark.parametrize("kernel", KERNELS)
def test_leave_one_out(kernel):
    """N = 100, d = 3 (Np = 128: 16 pad rows in front, 12 behind), three theta; idx = None and every point its own fold"""
    N = 100
    X, Z, th = _case(N, 3, 3, 11, THREE)
    eng = _engine(X, Z, kernel, th)
    folds = [[i] for i in range(N)]
    m0, v0 = eng.cross_validate()
    _check((m0, v0, None), folds, X, Z, th, kernel)
    m1, v1, c1 = eng.cross_validate(folds, return_cov=True)
    assert np.array_equal(m0, m1) and np.array_equal(v0, v1)
    assert c1.shape == (3, N, 1, 1) and np.array_equal(c1[:, :, 0, 0].T, v1)
    perm = np.random.default_rng(3).permutation(N)[:40]
    m2, v2 = eng.cross_validate([[i] for i in perm])
    assert np.array_equal(m2, m0[perm]) and np.array_equal(v2, v0[perm])
    eng.close()


# ---------------------------------------------------------------------------- 2. folds
def _folds_150():
    N = 150
    return {"seven": R.contiguous_folds(N, 7), "sixtyfour": R.contiguous_folds(N, 64), "shuffled37": R.shuffled_folds(N, 37, seed=5)}


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("shape", ["seven", "sixtyfour", "shuffled37"])
def test_folds(kernel, shape):
    """N = 150, d = 5 (Np = 192: 32 pad rows in front, 10 behind)"""
    X, Z, th = _case(150, 5, 3, 12, THREE)
    folds = _folds_150()[shape]
    if shape == "sixtyfour":
        assert [len(f) for f in folds] == [64, 64, 22]
    if shape == "shuffled37":
        assert len(folds[-1]) == 2
    eng = _engine(X, Z, kernel, th)
    got = eng.cross_validate(folds, return_cov=True)
    _check(got, folds, X, Z, th, kernel)
    m, v = eng.cross_validate(folds)                     # the variance does not depend on whether the blocks are asked for
    assert np.array_equal(m, got[0]) and np.array_equal(v, got[1])
    eng.close()


@pytest.mark.parametrize("kernel", KERNELS)
def test_general_path_agrees_with_fast_path(kernel):
    """folds of one point through the fold kernel (a fold of two added: the call leaves the leave-one-out path)"""
    N = 150
    X, Z, th = _case(N, 5, 3, 12, THREE)
    eng = _engine(X, Z, kernel, th)
    m0, v0 = eng.cross_validate()
    folds = [[i] for i in range(N - 2)] + [[N - 2, N - 1]]
    m1, v1 = eng.cross_validate(folds)
    n = N - 2
    assert not np.array_equal(v0[:n], v1[:n])            # (another order of the same sums)
    assert relerr(m1[:n], m0[:n]) < 1e-13 and relerr(v1[:n], v0[:n]) < 1e-13
    eng.close()


# ---------------------------------------------------------------------------- 3. edges
@pytest.mark.parametrize("N,d", [(64, 1), (64, 8), (65, 1), (65, 8)])
def test_edges(N, d):
    """no padding (N = 64) and the most (N = 65: 48 pad rows in front, 15 behind); a fold with the first and the last point;
    one fold alone; points in no fold"""
    X, Z, th = _case(N, d, 2, 13, ("mid", "hard"))
    rest = np.setdiff1d(np.arange(N), [0, N - 1, 7])
    folds = [np.array([N - 1, 0])] + [rest[i:i + 9] for i in range(0, 36, 9)]
    assert sum(len(f) for f in folds) < N
    for kernel in ("RBF", "Matern25"):
        eng = _engine(X, Z, kernel, th)
        _check(eng.cross_validate(folds, return_cov=True), folds, X, Z, th, kernel)
        _check(eng.cross_validate(folds[:1], return_cov=True), folds[:1], X, Z, th, kernel)          # nf = 1
        _check(eng.cross_validate([[N - 1]], return_cov=True), [[N - 1]], X, Z, th, kernel)
        m, v = eng.cross_validate()
        _check((m, v, None), [[i] for i in range(N)], X, Z, th, kernel)
        eng.close()


# ---------------------------------------------------------------------------- 4. bitwise independence
def test_bits_do_not_depend_on_company():
    N = 150
    X, Z, th = _case(N, 5, 3, 12, THREE)
    folds = R.shuffled_folds(N, 37, seed=5)
    off = np.concatenate([[0], np.cumsum([len(f) for f in folds])])
    eng = _engine(X, Z, "Matern25", th)
    mA, vA, cA = eng.cross_validate(folds, return_cov=True)
    pick = [0, 2, len(folds) - 1]                        # the last one is the ragged fold of 2
    mB, vB, cB = eng.cross_validate([folds[f] for f in pick], return_cov=True)
    rows = np.concatenate([np.arange(off[f], off[f + 1]) for f in pick])
    assert np.array_equal(mB, mA[rows]) and np.array_equal(vB, vA[rows])
    assert np.array_equal(cB, cA[:, pick])
    loo = eng.cross_validate()
    eng1 = _engine(X, Z[:1], "Matern25", th[:1])
    m1, v1, c1 = eng1.cross_validate(folds, return_cov=True)
    assert np.array_equal(m1[:, 0], mA[:, 0]) and np.array_equal(v1[:, 0], vA[:, 0]) and np.array_equal(c1[0], cA[0])
    loo1 = eng1.cross_validate()
    assert np.array_equal(loo1[0][:, 0], loo[0][:, 0]) and np.array_equal(loo1[1][:, 0], loo[1][:, 0])
    eng.close(); eng1.close()


# ---------------------------------------------------------------------------- 5. state
def test_state_is_untouched():
    from gpbayestools_hic_amd.engine import MODE_PCA
    N, d, P, M = 150, 5, 3, 4
    X, Z, th = _case(N, d, P, 12, THREE)
    rng = np.random.default_rng(8)
    eng = _engine(X, Z, "RBF", th)
    eng.set_transform(MODE_PCA, rng.standard_normal(M), A=rng.standard_normal((P, M)), cov_trunc=0.01 * np.eye(M))
    eng.set_likelihood(rng.standard_normal(M), 0.05 * np.eye(M))
    Xs = rng.random((70, d))
    before = (eng.predict(Xs), eng.loglike(Xs), eng.get("alpha"), eng.get("Linv"))
    folds = R.shuffled_folds(N, 37, seed=5)
    for call in (lambda: eng.cross_validate(), lambda: eng.cross_validate(folds, return_cov=True),
                 lambda: eng.emu_cross_validate(), lambda: eng.emu_cross_validate(folds)):
        call()
        after = (eng.predict(Xs), eng.loglike(Xs), eng.get("alpha"), eng.get("Linv"))
        assert np.array_equal(before[0][0], after[0][0]) and np.array_equal(before[0][1], after[0][1])
        assert all(np.array_equal(b, a) for b, a in zip(before[1:], after[1:]))
    eng.close()


# ---------------------------------------------------------------------------- 6. one larger shape
@functools.lru_cache(maxsize=None)
def _large_host(kernel):
    N = 1000
    X, Z, th = _case(N, 8, 4, 14, ("mid", "hard", "mid", "hard"))
    kf = R.kfold(N, 16, seed=6)
    everything = [[i] for i in range(N)] + kf
    return kf, [R.closed_form(X, Z[p], th[p], R.KINDS[kernel], R.ALPHA, everything) for p in range(4)]


@pytest.mark.parametrize("kernel", ["RBF", "Matern25"])
def test_larger_shape(kernel):
    """N = 1000, d = 8, P = 4 (Np = 1024: 16 pad rows in front, 8 behind): all of it against the closed form on the host, five
    leave-one-out points and three of the 16 shuffled folds (sizes 63 / 62) against brute-force refits"""
    N = 1000
    X, Z, th = _case(N, 8, 4, 14, ("mid", "hard", "mid", "hard"))
    kf, host = _large_host(kernel)
    assert sorted({len(f) for f in kf}) == [62, 63]
    eng = _engine(X, Z, kernel, th)
    loo_folds = [[i] for i in range(N)]
    m, v = eng.cross_validate()
    got = eng.cross_validate(kf, return_cov=True)
    eng.close()
    _check((m, v, None), loo_folds, X, Z, th, kernel, host=[h[:N] for h in host])
    _check(got, kf, X, Z, th, kernel, host=[h[N:] for h in host])
    _check((m, v, None), loo_folds, X, Z, th, kernel, which=[0, 1, 499, 998, 999])
    _check(got, kf, X, Z, th, kernel, which=[0, 7, 15])


# ---------------------------------------------------------------------------- 7. emulator level
MODES = {"pca": {}, "nopca": dict(perform_no_PCA=True), "logexp": dict(logTrafo=True, exp_and_cov_diagonal=True),
         "nopca_logexp": dict(perform_no_PCA=True, logTrafo=True, exp_and_cov_diagonal=True)}


def _emulator(tmp_path, kw):
    from gpbayestools_hic_amd import Emulator, synth
    N, d, nobs = 100, 4, 6
    X = synth.lhs(N, d, 21)
    Y = synth.observables(X, nobs, seed=22)
    tp, pf = str(tmp_path / "train.pkl"), str(tmp_path / "par.txt")
    synth.write_training_pickle(tp, X, Y, 0.02 * Y)
    synth.write_parameter_file(pf, np.zeros(d), np.ones(d))
    emu = Emulator(training_set_path=tp, parameter_file=pf, npc=3, **kw)
    P = nobs if kw.get("perform_no_PCA") else 3
    emu.trainEmulator([True] * emu.nev, kernel_type="RBF", thetas=R.thetas_of((THREE * 2)[:P], d))
    return emu


def _emulator_reference(emu, folds):
    """oracle.emulator_predict on the brute-force per-GP hold-out means / variances, and the four arrays of
    Emulator.cross_validate rebuilt from it, model_data and model_data_err"""
    X, Z, P = emu._X_train, emu._Z_train, emu._ngp
    flat = np.concatenate([np.asarray(f) for f in folds])
    gm, gv = np.empty((len(flat), P)), np.empty((len(flat), P))
    for p in range(P):
        gm[:, p], gv[:, p] = R.flatten(R.brute_force(X, Z[p], emu.thetas_[p], O.KIND_RBF, emu.alpha, folds))
    mean, cov = O.emulator_predict(gm, gv, 0.0, mode=emu._mode, A=emu._A, mu=emu.scaler.mean_, cov_trunc=emu._cov_trunc,
                                   scale=emu.scaler.scale_)
    pred, perr = mean, np.sqrt(np.diagonal(cov, axis1=1, axis2=2))
    if emu.logTrafo_ and not emu.exp_and_cov_diagonal_:
        pred, perr = np.exp(pred), perr * np.exp(pred)
    truth, terr = emu.model_data[flat], emu.model_data_err[flat]
    if emu.logTrafo_:
        truth = np.exp(truth)
        terr = terr * truth
    return mean, cov, (pred, perr, truth, terr)


def _check_four(got, want):
    assert relerr(got[0], want[0]) < 1e-11 and relerr(got[1], want[1]) < 1e-10
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])


@pytest.mark.parametrize("mode", list(MODES))
def test_emulator_cross_validate(tmp_path, mode):
    emu = _emulator(tmp_path, MODES[mode])
    N = emu.nev
    loo = [[i] for i in range(N)]
    mean, cov, four = _emulator_reference(emu, loo)
    gm, gc = emu._engine_ready().emu_cross_validate()
    assert relerr(gm, mean) < 1e-11 and maxrel(gc, cov) < 1e-10
    assert relerr(emu._engine_ready().emu_cross_validate(return_cov=False), mean) < 1e-11
    got = emu.cross_validate()
    assert all(a.shape == (N, emu.nobs) for a in got)
    _check_four(got, four)
    import dill
    emu2 = dill.loads(dill.dumps(emu))
    assert all(np.array_equal(a, b) for a, b in zip(emu2.cross_validate(), got))
    # k folds in order, and shuffled as sklearn's KFold(shuffle=True, random_state=3) orders them
    ten = R.contiguous_folds(N, 10)
    _check_four(emu.cross_validate(folds=10), _emulator_reference(emu, ten)[2])
    order = np.arange(N)
    np.random.RandomState(3).shuffle(order)
    shuffled = [order[i:i + 10] for i in range(0, N, 10)]
    _check_four(emu.cross_validate(folds=10, shuffle=True, random_state=3), _emulator_reference(emu, shuffled)[2])
    _check_four(emu.cross_validate(folds=shuffled), _emulator_reference(emu, shuffled)[2])
    # 5 folds of 20 events are inside the limit of 64 events per fold; one fold of all 100 events is not
    _check_four(emu.cross_validate(folds=5), _emulator_reference(emu, R.contiguous_folds(N, 20))[2])
    with pytest.raises(ValueError, match="64"):
        emu.cross_validate(folds=1)
    with pytest.raises(ValueError, match="64"):
        emu.cross_validate(folds=[np.arange(65)])


def test_validation_summaries():
    from gpbayestools_hic_amd import honesty, rms_relative_error
    rng = np.random.default_rng(9)
    n, nobs = 17, 5
    truth = 1.0 + rng.random((n, nobs))
    pred = truth + 0.1 * rng.standard_normal((n, nobs))
    perr = 0.05 + 0.1 * rng.random((n, nobs))
    rel, hon = np.zeros(nobs), np.zeros(nobs)
    for j in range(nobs):
        for i in range(n):
            rel[j] += ((pred[i, j] - truth[i, j]) / truth[i, j]) ** 2
            hon[j] += ((pred[i, j] - truth[i, j]) / perr[i, j]) ** 2
    assert relerr(rms_relative_error(pred, truth), np.sqrt(rel / n)) < 1e-14
    assert relerr(honesty(pred, perr, truth), np.sqrt(hon / n)) < 1e-14


# ---------------------------------------------------------------------------- 8. errors
def test_errors_leave_the_context_usable():
    from gpbayestools_hic_amd import GPEngine
    from gpbayestools_hic_amd._native import GPBError, ptr
    N, d, P = 100, 3, 3
    X, Z, th = _case(N, d, P, 11, THREE)
    E_ARG, E_STATE = -1, -2
    eng = GPEngine(0)
    eng.set_data(X, Z, "RBF", R.ALPHA)
    eng.set_theta(th)
    out, out2 = np.empty((N, P)), np.empty((N, P))

    def raw(idx, fptr, e=eng):
        idx = None if idx is None else np.ascontiguousarray(idx, dtype=np.int32)
        fptr = None if fptr is None else np.ascontiguousarray(fptr, dtype=np.int32)
        n = N if idx is None else len(idx)
        nf = n if fptr is None else len(fptr) - 1
        return e.lib.gpb_gp_cv(e.h, ptr(idx), n, ptr(fptr), nf, 0, ptr(out), ptr(out2), None)

    assert raw(None, None) == E_STATE                    # no factorisation
    with pytest.raises(GPBError, match="gpb_gp_factor"):
        eng.cross_validate()
    eng.factor()
    assert raw(np.arange(65), [0, 65]) == E_ARG          # fold of 65
    assert raw(np.arange(10), [0, 5, 5, 10]) == E_ARG    # empty fold
    assert raw([1, 2, 2, 3], [0, 2, 4]) == E_ARG         # duplicate index
    assert raw([1, N], [0, 2]) == E_ARG                  # index = N
    assert raw([1, 2, 3], [0, 2, 4]) == E_ARG            # fold_ptr does not end at n_idx
    assert raw([1, 2, 3], [1, 2, 3]) == E_ARG            # ... or start at 0
    for bad in ([np.arange(65)], [[1, 2], []], [[1, 2], [2, 3]], [[1, N]], [[-1]]):
        with pytest.raises(ValueError):
            eng.cross_validate(bad)
    with pytest.raises(ValueError, match="64"):
        eng.cross_validate([np.arange(65)])
    mean = np.empty((N, 1))
    assert eng.lib.gpb_emu_cv(eng.h, None, N, None, N, 0, ptr(mean), None) == E_STATE      # no transform
    with pytest.raises(GPBError, match="gpb_emu_set_transform"):
        eng.emu_cross_validate()
    Xs = np.random.default_rng(2).random((33, d))
    m, v = eng.predict(Xs)
    for p in range(P):
        mo, vo = O.gp_predict(Xs, X, th[p], *O.gp_factor(X, Z[p], th[p], O.KIND_RBF, R.ALPHA), O.KIND_RBF)
        assert relerr(m[:, p], mo) < 1e-11 and relerr(v[:, p], vo) < 1e-10
    _check(eng.cross_validate([[3, 4], [5]], return_cov=True), [[3, 4], [5]], X, Z, th, "RBF")
    eng.close()
    multi = GPEngine(0)
    multi.set_data_multi([X, X[:90]], [Z[0], Z[1][:90]], "RBF", R.ALPHA)
    multi.set_theta(th[:2])
    multi.factor()
    assert raw(None, None, multi) == E_STATE
    with pytest.raises(GPBError, match="fit-only"):
        multi.cross_validate()
    multi.close()
