"""GPU tier: the two output routes of every entry point that takes on_device.  With on_device = 0 the results are formed in a
staging buffer on the device and copied to host memory; with on_device = 1 they go to the caller's device pointers.  Both routes
run the same kernels, so they must give the same bits: doubles are compared with np.array_equal(..., equal_nan=True), integers
exactly.  Entry points with optional outputs are asked for all of them and with each one left out in turn.

One context throughout: N = 70, d = 3, P = 2, RBF (Np = 128: 48 rows of padding in front and 10 behind), a PCA transform with
M = 4 and a likelihood block.  The batches on it are W = 5, then 300, then 5 again: the stage grows while it is held, then is
larger than needed."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, D, P, M = 70, 3, 2, 4
BATCHES = (5, 300, 5)


def _same(a, b):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    b = b.cpu().numpy() if hasattr(b, "cpu") else np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind == "f":
        return np.array_equal(a, b, equal_nan=True)
    return np.array_equal(a, b)


@pytest.fixture(scope="module")
def ctx():
    import torch
    from gpbayestools_hic_amd import GPEngine, synth
    rng = np.random.default_rng(4170)
    X = synth.lhs(N, D, seed=synth.SEED + N)
    Z = np.ascontiguousarray(synth.observables(X, P, seed=synth.SEED + N + 1).T) - 2.0
    theta = synth.fixed_theta(D, P) + 0.05 * rng.standard_normal((P, D + 2))
    A = rng.standard_normal((P, M))
    mu = 2.0 + rng.standard_normal(M)
    c0 = 0.01 * rng.standard_normal((M, M))
    yexp = mu + 0.1 * rng.standard_normal(M)
    eng = GPEngine(0)
    eng.set_data(X, Z, kernel="RBF")
    eng.set_theta(theta)
    eng.factor()
    eng.set_transform(0, mu, A=A, cov_trunc=c0 @ c0.T + 1e-3 * np.eye(M))
    eng.set_likelihood(yexp, np.diag((0.05 * np.abs(yexp)) ** 2))
    dev = torch.device("cuda", 0)
    Xq = synth.walkers(max(BATCHES), D, seed=synth.SEED + N + 2)
    yield dict(eng=eng, dev=dev, Xq=Xq, rng=rng)
    eng.close()


def _dev(ctx, a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device=ctx["dev"])


def _empty(ctx, shape, dtype=None):
    import torch
    return torch.empty(shape, dtype=dtype or torch.float64, device=ctx["dev"])


def _batches(ctx):
    for W in BATCHES:
        Xh = np.ascontiguousarray(ctx["Xq"][:W])
        yield W, Xh, _dev(ctx, Xh)


def test_gp_predict(ctx):
    eng = ctx["eng"]
    for W, Xh, Xd in _batches(ctx):
        mh, vh = eng.predict(Xh)
        md, vd = eng.predict(Xd)
        assert _same(mh, md) and _same(vh, vd), W
        assert _same(eng.predict(Xh, return_var=False), eng.predict(Xd, return_var=False)), W
        assert _same(eng.predict(Xh, return_var=False), mh), W


def test_gp_predict_cov(ctx):
    from gpbayestools_hic_amd import _native as nat
    eng = ctx["eng"]
    for W, Xh, Xd in _batches(ctx):
        mh, ch = eng.predict_cov(Xh)
        md, cd = _empty(ctx, (W, P)), _empty(ctx, (P, W, W))
        eng._ck(eng.lib.gpb_gp_predict_cov(eng.h, nat.ptr(Xd), W, 1, nat.ptr(md), nat.ptr(cd)))
        assert _same(mh, md) and _same(ch, cd), W


def test_gp_predict_grad(ctx):
    eng = ctx["eng"]
    for W, Xh, Xd in _batches(ctx):
        mh, vh = eng.predict_grad(Xh)
        md, vd = eng.predict_grad(Xd)
        assert _same(mh, md) and _same(vh, vd), W
        assert _same(eng.predict_grad(Xh, return_var=False), eng.predict_grad(Xd, return_var=False)), W


def test_emu_predict(ctx):
    eng = ctx["eng"]
    for W, Xh, Xd in _batches(ctx):
        es = 0.01 + 0.001 * np.arange(W)
        for extra in (None, es):
            mh, ch = eng.emu_predict(Xh, extra_std=extra)
            md, cd = eng.emu_predict(Xd, extra_std=extra)
            assert _same(mh, md) and _same(ch, cd), W
            assert _same(eng.emu_predict(Xh, return_cov=False, extra_std=extra), eng.emu_predict(Xd, return_cov=False, extra_std=extra)), W


def test_emu_predict_diag(ctx):
    """and on the device route with ld = W + 3 into sentinel-filled arrays: the columns at and beyond W keep the sentinel"""
    from gpbayestools_hic_amd import _native as nat
    eng = ctx["eng"]
    sentinel = -12345.678
    for W, Xh, Xd in _batches(ctx):
        mh, vh = eng.emu_predict_diag(Xh)
        md, vd = eng.emu_predict_diag(Xd)
        assert _same(mh, md) and _same(vh, vd), W
        big = (_empty(ctx, (M, W + 3)).fill_(sentinel), _empty(ctx, (M, W + 3)).fill_(sentinel))
        eng.emu_predict_diag(Xd, out=(big[0][:, :W], big[1][:, :W]))
        for host, wide in zip((mh, vh), big):
            wide = wide.cpu().numpy()
            assert _same(host, np.ascontiguousarray(wide[:, :W])), W
            assert np.all(wide[:, W:] == sentinel), W
        # the variance left out, both routes through the C ABI
        m1 = np.empty((M, W))
        eng._ck(eng.lib.gpb_emu_predict_diag(eng.h, nat.ptr(Xh), W, 0, None, nat.ptr(m1), None, W))
        m2 = _empty(ctx, (M, W + 3)).fill_(sentinel)
        eng._ck(eng.lib.gpb_emu_predict_diag(eng.h, nat.ptr(Xd), W, 1, None, nat.ptr(m2), None, W + 3))
        m2 = m2.cpu().numpy()
        assert _same(m1, mh) and _same(m1, np.ascontiguousarray(m2[:, :W])) and np.all(m2[:, W:] == sentinel), W


def test_emu_predict_jac(ctx):
    from gpbayestools_hic_amd import _native as nat
    eng = ctx["eng"]
    for W, Xh, Xd in _batches(ctx):
        jh = eng.emu_predict_jac(Xh)
        jd = _empty(ctx, (W, M, D))
        eng._ck(eng.lib.gpb_emu_predict_jac(eng.h, nat.ptr(Xd), W, 1, nat.ptr(jd)))
        assert _same(jh, jd), W


def test_loglike(ctx):
    import torch
    eng = ctx["eng"]
    for W, Xh, Xd in _batches(ctx):
        lh = eng.loglike(Xh)
        ld = eng.loglike(Xd)
        assert _same(lh, ld), W
        start = np.linspace(-3.0, 2.0, W)
        ah = eng.loglike(Xh, out=start.copy(), accumulate=True)
        ad = eng.loglike(Xd, out=_dev(ctx, start), accumulate=True)
        assert _same(ah, ad), W
        assert not _same(ah, lh), W
        # without the not-positive-definite count: the device route stays asynchronous
        nh = eng.loglike(Xh, check=False)
        nd = eng.loglike(Xd, check=False)
        torch.cuda.synchronize()
        assert _same(nh, nd) and _same(nh, lh), W


def test_mvn_loglike(ctx):
    eng, rng = ctx["eng"], np.random.default_rng(7)
    W = 3
    dY = rng.standard_normal((W, M))
    G = rng.standard_normal((W, M, M))
    cov = G @ np.transpose(G, (0, 2, 1)) + 0.5 * np.eye(M)
    assert _same(eng.mvn_loglike(dY, cov), eng.mvn_loglike(_dev(ctx, dY), _dev(ctx, cov)))


@pytest.mark.parametrize("folds", [None, [[4], [9, 2, 31]]], ids=["loo", "folds_1_3"])
def test_cross_validation(ctx, folds):
    """gpb_gp_cv and gpb_emu_cv: all outputs, and each optional one left out in turn"""
    from gpbayestools_hic_amd import _native as nat
    eng = ctx["eng"]
    idx, fptr, n, nf, kmax = eng._cv_folds(folds)
    for want_var, want_cov in ((True, True), (False, True), (True, False), (False, False)):
        host = [np.empty((n, P)), np.empty((n, P)) if want_var else None, np.empty((P, nf, kmax, kmax)) if want_cov else None]
        devs = [_empty(ctx, (n, P)), _empty(ctx, (n, P)) if want_var else None, _empty(ctx, (P, nf, kmax, kmax)) if want_cov else None]
        eng._ck(eng.lib.gpb_gp_cv(eng.h, nat.ptr(idx), n, nat.ptr(fptr), nf, 0, *[nat.ptr(o) for o in host]))
        eng._ck(eng.lib.gpb_gp_cv(eng.h, nat.ptr(idx), n, nat.ptr(fptr), nf, 1, *[nat.ptr(o) for o in devs]))
        for h, d in zip(host, devs):
            assert (h is None and d is None) or _same(h, d), (want_var, want_cov)
    for want_cov in (True, False):
        host = [np.empty((n, M)), np.empty((n, M, M)) if want_cov else None]
        devs = [_empty(ctx, (n, M)), _empty(ctx, (n, M, M)) if want_cov else None]
        eng._ck(eng.lib.gpb_emu_cv(eng.h, nat.ptr(idx), n, nat.ptr(fptr), nf, 0, *[nat.ptr(o) for o in host]))
        eng._ck(eng.lib.gpb_emu_cv(eng.h, nat.ptr(idx), n, nat.ptr(fptr), nf, 1, *[nat.ptr(o) for o in devs]))
        for h, d in zip(host, devs):
            assert (h is None and d is None) or _same(h, d), want_cov


def test_sobol(ctx):
    """gpb_gp_sobol, gpb_emu_sobol and gpb_emu_main_effect over the box [0, 1]^3"""
    from gpbayestools_hic_amd import _native as nat
    eng = ctx["eng"]
    lo, hi = np.zeros(D), np.ones(D)
    for h, d in zip(eng.sobol(lo, hi), eng.sobol(lo, hi, on_device=True)):
        assert _same(h, d)
    for h, d in zip(eng.emu_sobol(lo, hi), eng.emu_sobol(lo, hi, on_device=True)):
        assert _same(h, d)
    G = 7
    t = np.linspace(0.05, 0.95, G)
    for j in range(D):
        ch = eng.emu_main_effect(lo, hi, j, t)
        cd = _empty(ctx, (G, M))
        eng._ck(eng.lib.gpb_emu_main_effect(eng.h, nat.ptr(lo), nat.ptr(hi), j, nat.ptr(_dev(ctx, t)), G, 1, nat.ptr(cd)))
        assert _same(ch, cd), j


def test_ppd_summary(ctx):
    eng, rng = ctx["eng"], np.random.default_rng(11)
    S = 33
    mu_T = _dev(ctx, rng.standard_normal((M, S)))
    var_T = _dev(ctx, 0.1 + rng.random((M, S)))
    yobs = rng.standard_normal(M)
    q = [0.16, 0.5, 0.84]
    names = ("moments", "order", "mixq", "pit")
    for outputs in (names,) + tuple(tuple(k for k in names if k != left) for left in names):
        h = eng.ppd_summary(mu_T, var_T, q, yobs=yobs, outputs=outputs)
        d = eng.ppd_summary(mu_T, var_T, q, yobs=yobs, outputs=outputs, on_device=True)
        assert set(h) == set(d) == set(outputs)
        for k in outputs:
            assert _same(h[k], d[k]), (outputs, k)


@pytest.mark.parametrize("layout", ["steps", "walkers"])
def test_mcmc_diag(ctx, layout):
    eng, rng = ctx["eng"], np.random.default_rng(13)
    x = np.cumsum(rng.standard_normal((16, 4, 3)), axis=0)
    x_dev = _dev(ctx, x if layout == "steps" else np.transpose(x, (1, 0, 2)))
    names = ("rho", "tau", "window", "moments", "rhat", "nconst")
    for outputs in (names,) + tuple(tuple(k for k in names if k != left) for left in names):
        h = eng.mcmc_diag(x_dev, layout=layout, max_lag=5, outputs=outputs)
        d = eng.mcmc_diag(x_dev, layout=layout, max_lag=5, outputs=outputs, on_device=True)
        assert set(h) == set(d) == set(outputs)
        for k in outputs:
            assert _same(h[k], d[k]), (outputs, k)


@pytest.mark.parametrize("weighted", [False, True])
def test_chain_marginals(ctx, weighted):
    eng, rng = ctx["eng"], np.random.default_rng(17)
    x = rng.random((16, 4, 3))
    weights = None
    if weighted:                                  # (weights go with a flat particle set: one walker)
        x = x.reshape(64, 1, 3)
        weights = 0.1 + rng.random(64)
    x_dev = _dev(ctx, x)
    edges = np.tile(np.linspace(0.05, 0.95, 5), (3, 1))          # B = 4; some samples fall outside
    names = ("h1", "h2", "outside")
    for outputs in (names,) + tuple(tuple(k for k in names if k != left) for left in names):
        h = eng.chain_marginals(x_dev, edges=edges, weights=weights, outputs=outputs)
        d = eng.chain_marginals(x_dev, edges=edges, weights=weights, outputs=outputs, on_device=True)
        assert set(h) == set(d) == set(outputs)
        for k in outputs:
            assert h[k].dtype == np.int64 and _same(h[k], d[k]), (outputs, k)
