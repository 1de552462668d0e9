"""GPU tier: per-point simulation noise on the GPs' training diagonal (gpb_gp_set_point_noise, gpb_design_set_noise; DESIGN.md
section 16) through every kernel that reads that diagonal: the K assembly in both distance forms, the closed-form
cross-validation, the design score.  The reference is the numpy oracle called with the VECTOR alpha + s (oracle.gp_oracle:
sklearn's GPR(alpha=<array>) bit for bit, tests/test_sk_reference.py) and tests/sk_reference.py.

Shapes: d = 5, P = 3; N = 70 pads to 128 (48 rows in front, 10 behind), N = 128 has no padding; all three kernel families;
alpha = 0.1; s log-uniform in [1e-4, 0.3], different per GP.  Tolerances are the project's own for the same quantities
(tests/test_gpu_engine.py, test_gpu_cv.py, test_gpu_design.py)."""
import functools

import numpy as np
import pytest

import cv_reference as CV
import sk_reference as SK
from conftest import maxrel, relerr
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

ALPHA = SK.ALPHA
D_IN, P_GP = 5, 3
KERNELS = ["RBF", "Matern", "Matern25"]
E_ARG, E_STATE = -1, -2


@functools.lru_cache(maxsize=None)
def _data(N):
    """X, Z [P, N], thetas [P, d + 2] and s [P, N], shared and read-only.  GP 1 has a length scale of 0.02: S = sum_k (extent_k /
    l_k)^2 ~ 1.2e4 > 1024, so choose_forms sends it to the difference form (k_kmat) while GPs 0 and 2 take k_kmat_mfma"""
    X, Z = CV.make_data(N, D_IN, P_GP, seed=40 + N)
    th = CV.thetas_of(("mid", "hard", "aniso"), D_IN)
    th[1, 1:1 + D_IN] = np.log(0.02)
    return X, Z, th, SK.noise_rows(P_GP, N, seed=N)


def _engine(X, Z, kernel, alpha=ALPHA, s=None):
    from gpbayestools_hic_amd import GPEngine
    eng = GPEngine(0)
    eng.set_data(X, Z, kernel, alpha, point_noise=s)
    return eng


def _fit_bits(eng, th):
    """everything the training diagonal reaches: LML and gradient, then L and alpha_ of the factorisation at th"""
    v, g = eng.lml(th)
    eng.set_theta(th)
    eng.factor()
    return v, g, eng.get("L"), eng.get("alpha")


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------------------- 1. fit
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("N", [70, 128])
def test_fit_against_oracle(N, kernel):
    X, Z, th, s = _data(N)
    eng = _engine(X, Z, kernel, ALPHA, s)
    v, g, L, a = _fit_bits(eng, th)
    assert list(eng.get("form")) == [0, 1, 0]                        # both K kernels in one context
    Xs = np.random.default_rng(3).uniform(size=(37, D_IN))
    m, var = eng.predict(Xs)
    eng.close()
    kind = SK.KINDS[kernel]
    for p in range(P_GP):
        t = ALPHA + s[p]
        Lo, ao = O.gp_factor(X, Z[p], th[p], kind, t)
        vo, go = O.lml(th[p], X, Z[p], kind, t, eval_gradient=True)
        mo, varo = O.gp_predict(Xs, X, th[p], Lo, ao, kind)
        errs = (maxrel(L[p], Lo), maxrel(a[p], ao), abs(v[p] - vo) / abs(vo), maxrel(g[p], go), maxrel(m[:, p], mo),
                relerr(var[:, p], varo))
        print("N %d %s GP %d: L %.2g alpha_ %.2g LML %.2g grad %.2g mean %.2g var %.2g" % ((N, kernel, p) + errs))
        assert errs[0] < 1e-11 and errs[1] < 1e-10 and errs[2] < 1e-10 and errs[3] < 1e-9 and errs[4] < 1e-11 and errs[5] < 1e-10
    # the noise is not a no-op: the scalar fit differs visibly
    Lo0, _ = O.gp_factor(X, Z[0], th[0], kind, ALPHA)
    assert maxrel(L[0], Lo0) > 1e-4


# ---------------------------------------------------------------------------- 2. bits
@pytest.mark.parametrize("N", [70, 128])
def test_bits(N):
    X, Z, th, s = _data(N)
    plain = _engine(X, Z, "RBF")
    ref = _fit_bits(plain, th)
    plain.close()
    # no call == a zero array: alpha + 0 is formed first
    e = _engine(X, Z, "RBF", ALPHA, np.zeros_like(s))
    assert _same(_fit_bits(e, th), ref)
    # a set followed by a reset with NULL == never set
    e.set_point_noise(s)
    assert not _same(_fit_bits(e, th), ref)
    e.set_point_noise(None)
    assert _same(_fit_bits(e, th), ref)
    e.close()
    # uniform s0 with alpha == the scalar fl(alpha + s0)
    s0 = 0.0371
    a = _engine(X, Z, "RBF", ALPHA, np.full_like(s, s0))
    b = _engine(X, Z, "RBF", ALPHA + s0)
    assert _same(_fit_bits(a, th), _fit_bits(b, th))
    a.close(); b.close()


# ---------------------------------------------------------------------------- 3. batches
def test_multi_subset_and_restart_copies():
    from gpbayestools_hic_amd import GPEngine
    Ns = [70, 100, 70]
    th = CV.thetas_of(("mid", "hard", "aniso"), D_IN)
    th[1, 1:1 + D_IN] = np.log(0.02)                                 # one GP in the difference form here too
    Xs, Zs, Ss = [], [], []
    for p, n in enumerate(Ns):
        X, Z = CV.make_data(n, D_IN, 1, seed=70 + p)
        Xs.append(X); Zs.append(Z[0]); Ss.append(SK.noise_rows(1, n, seed=80 + p)[0])
    alone = []
    for p in range(3):
        e = GPEngine(0)
        e.set_data_multi([Xs[p]], [Zs[p]], "RBF", ALPHA, [Ss[p]])
        alone.append(e.lml_subset([0], th[p:p + 1]))
        e.close()
    multi = GPEngine(0)
    multi.set_data_multi(Xs, Zs, "RBF", ALPHA, Ss)
    for idx in ([0, 1, 2], [2, 0], [1]):
        v, g = multi.lml_subset(idx, th[idx])
        for a, p in enumerate(idx):
            assert v[a] == alone[p][0][0] and np.array_equal(g[a], alone[p][1][0]), (idx, p)
    multi.close()
    # noise matters, per GP: GP 0 with GP 2's row is another number
    e = GPEngine(0)
    e.set_data_multi([Xs[0]], [Zs[0]], "RBF", ALPHA, [Ss[2]])
    assert e.lml_subset([0], th[:1])[0][0] != alone[0][0][0]
    e.close()
    # a restart batch: copies = 3 of the three GPs, every copy the bits of copy 0 at equal theta
    from gpbayestools_hic_amd.emulator import _SearchEngine
    se = _SearchEngine(0, Xs, Zs, "RBF", ALPHA, 3, Ss)
    v, g = se.lml(np.tile(th, (3, 1)))
    for c in range(3):
        assert np.array_equal(v[3 * c:3 * c + 3], v[:3]) and np.array_equal(g[3 * c:3 * c + 3], g[:3])
    assert np.array_equal(v[:3], [a[0][0] for a in alone])
    v2, _ = se.lml_active(np.array([4, 8]), th[[1, 2]])
    assert np.array_equal(v2, v[[1, 2]])
    se.close()


# ---------------------------------------------------------------------------- 4. cross-validation
def _cv_check(res, folds, X, Z, th, s, kernel):
    """device (mean, var, cov) against the brute-force refits with t[keep]: means within 1e-11, covariances within 1e-10"""
    mean, var, cov = res
    q = 0
    for f, F in enumerate(folds):
        k = len(F)
        for p in range(P_GP):
            (mb, cb), = SK.cv_brute_force(X, Z[p], th[p], SK.KINDS[kernel], ALPHA + s[p], [F])
            em = CV.mean_err(mean[q:q + k, p], mb, Z[p][np.asarray(F)])
            ev = relerr(var[q:q + k, p], np.diag(cb))
            ec = maxrel(cov[p, f, :k, :k], cb)
            assert em < 1e-11 and ev < 1e-10 and ec < 1e-10, (f, p, em, ev, ec)
            assert np.all(cov[p, f, k:, :] == 0.0) and np.all(cov[p, f, :, k:] == 0.0)
        q += k


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("N", [70, 128])
def test_cv_against_refits(N, kernel):
    X, Z, th, s = _data(N)
    th = CV.thetas_of(("mid", "hard", "aniso"), D_IN)                # (the refit of a near-diagonal K checks little)
    eng = _engine(X, Z, kernel, ALPHA, s)
    eng.set_theta(th)
    eng.factor()
    loo = [[i] for i in range(N)]
    m, v, c = eng.cross_validate(None, return_cov=True)
    _cv_check((m, v, c), loo, X, Z, th, s, kernel)
    # folds of 1, 2, 7 and (where 74 points exist: N = 128) 64 points in one call, scattered over the design; N = 70 takes its
    # fold of 64 in test_cv_fold_of_64
    perm = np.random.default_rng(9).permutation(N)
    folds = [perm[0:1], perm[1:3], perm[3:10]] + ([perm[10:74]] if N >= 74 else [])
    _cv_check(eng.cross_validate(folds, return_cov=True), folds, X, Z, th, s, kernel)
    eng.close()


@pytest.mark.parametrize("N", [70, 128])
def test_cv_fold_of_64(N):
    """the largest fold the closed form takes, alone"""
    X, Z, _, s = _data(N)
    th = CV.thetas_of(("mid", "hard", "aniso"), D_IN)
    eng = _engine(X, Z, "RBF", ALPHA, s)
    eng.set_theta(th)
    eng.factor()
    folds = [np.random.default_rng(10).permutation(N)[:64]]
    _cv_check(eng.cross_validate(folds, return_cov=True), folds, X, Z, th, s, "RBF")
    eng.close()


@pytest.mark.parametrize("kernel", KERNELS)
def test_cv_general_path_agrees_with_fast_path(kernel):
    N = 70
    X, Z, _, s = _data(N)
    th = CV.thetas_of(("mid", "hard", "aniso"), D_IN)
    eng = _engine(X, Z, kernel, ALPHA, s)
    eng.set_theta(th)
    eng.factor()
    m0, v0 = eng.cross_validate()
    m1, v1 = eng.cross_validate([[i] for i in range(N - 2)] + [[N - 2, N - 1]])
    n = N - 2
    assert relerr(m1[:n], m0[:n]) < 1e-13 and relerr(v1[:n], v0[:n]) < 1e-13
    eng.close()


# ---------------------------------------------------------------------------- 5. design
BAR = 1e-9          # tests/test_gpu_design.py: every score and gain within 1e-9 max_c J_t(c) of its step


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda:0")


def _design_run(eng, c, T, s_c):
    eng.design_begin(_dev(c["Xc"]), _dev(c["Xr"]), _dev(c["w"]), c["g"], candidate_noise=s_c)
    try:
        return eng.design_run(T, None, return_scores=True)
    finally:
        eng.design_end()


def test_design_with_candidate_noise():
    c = SK.design_case()                                             # N = 70, d = 5, P = 3, C = 40, R = 30
    T = 5
    model = SK.design_greedy(c["X"], c["theta"], "RBF", ALPHA + c["s"], c["Xc"], c["Xr"], c["w"], c["g"], T, ALPHA + c["s_c"])
    assert np.all(model["gaps"] >= 1e-6)                             # (tests/test_sk_reference.py prints them)
    eng = _engine(c["X"], c["Z"], "RBF", ALPHA, c["s"])
    eng.set_theta(c["theta"])
    eng.factor()
    picks, gain, scores = _design_run(eng, c, T, c["s_c"])
    assert np.array_equal(picks, model["picks"])
    for t in range(T):
        el = np.isfinite(model["scores"][t])
        top = model["scores"][t][el].max()
        es, eg = np.abs(scores[t][el] - model["scores"][t][el]).max() / top, abs(gain[t] - model["gain"][t]) / top
        print("design step %d: scores %.2g, gain %.2g of max J" % (t, es, eg))
        assert es < BAR and eg < BAR
        assert np.all(np.isneginf(scores[t][~el]))
    # torch input gives the numpy input's bits; a zero array gives the bits of no call; None takes it away again
    again = _design_run(eng, c, T, _dev(c["s_c"]))
    assert _same(again, (picks, gain, scores))
    none = _design_run(eng, c, T, None)
    zero = _design_run(eng, c, T, np.zeros_like(c["s_c"]))
    assert _same(none, zero) and not np.array_equal(none[2], scores)
    eng.design_begin(_dev(c["Xc"]), _dev(c["Xr"]), _dev(c["w"]), c["g"], candidate_noise=c["s_c"])
    eng.design_set_noise(None)
    off = eng.design_run(T, None, return_scores=True)
    eng.design_end()
    assert _same(off, none)
    eng.close()


# ---------------------------------------------------------------------------- 6. errors
def test_errors_leave_the_context_usable():
    from gpbayestools_hic_amd._native import GPBError
    X, Z, th, s = _data(70)
    eng = _engine(X, Z, "RBF", ALPHA, s)
    ref = _fit_bits(eng, th)
    for bad_value in (-1e-3, np.nan, np.inf):
        bad = s.copy()
        bad[1, 17] = bad_value
        with pytest.raises(GPBError, match=r"code %d" % E_ARG):
            eng.set_point_noise(bad)
        assert _same(_fit_bits(eng, th), ref)                        # still the noise installed before
    with pytest.raises(ValueError):
        eng.set_point_noise(s[:, :-1])
    with pytest.raises(ValueError):
        eng.set_point_noise(s[:2])
    # design noise before begin
    eng.set_theta(th)
    eng.factor()
    with pytest.raises(GPBError, match=r"code %d" % E_STATE):
        eng.design_set_noise(np.zeros((P_GP, 8)))
    c = SK.design_case()
    eng.design_begin(_dev(c["Xc"]), _dev(c["Xr"]), _dev(c["w"]), c["g"])
    with pytest.raises(ValueError):
        eng.design_set_noise(np.zeros((P_GP, 39)))
    with pytest.raises(ValueError):
        eng.design_set_noise(-np.ones((P_GP, 40)))
    eng.design_run(2)
    with pytest.raises(GPBError, match=r"code %d" % E_STATE):        # the run consumed the workspace
        eng.design_set_noise(np.zeros((P_GP, 40)))
    eng.design_end()
    assert _same(_fit_bits(eng, th), ref)
    eng.close()
    # a new set_data resets the context to "none"
    e2 = _engine(X, Z, "RBF", ALPHA, s)
    e2.set_data(X, Z, "RBF", ALPHA)
    plain = _engine(X, Z, "RBF")
    assert _same(_fit_bits(e2, th), _fit_bits(plain, th))
    e2.close(); plain.close()
