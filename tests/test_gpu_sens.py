"""GPU tier: response matrix and Fisher information on the device — gpb_sens_accumulate (GPEngine.sens_accumulate / sens_unpack),
the device path of GPEngine.emu_predict_jac and Chain.sensitivity — against the host model of tests/sens_reference.py.

Bars.  F: err(A) = max |A - F_longdouble| / max |F_longdouble| with err(device) <= max(8 err(scipy fp64 route), 64 2^-53) — both
routes are backward-stable Cholesky solves whose error scales with cond(C); the factor 8 covers another elimination order and fma
contraction, not another error class.  Sums of R, R^2 and I: 256 2^-53 sum wt |term|.  R and I of one row, the triangles of F,
slabs against one call, a bad row against a weightless one: bit equality.

What the F bar can and cannot tell.  At cond(C) ~ 1e6 two eliminations of the same error class land anywhere from 0.001 to 11
times each other's error on a given seed (a plain right-looking fp64 Cholesky gave 11 x scipy's at (33, 20) and 0.6 x at
(17, 5)): a factor of 8 on five rows is partly a lottery on the seeds, and a pass does not by itself show the better algorithm.
The kernel carries its dot products in two doubles, which takes the per-term roundings out of L and U; the measured ratios are in
profiles/sens_accuracy.txt, and the figures in test_fisher_accuracy's docstring are copied from there."""
import functools
import os

import numpy as np
import pytest

import cv_reference as CV
import sens_reference as R

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -2


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _util():
    from gpbayestools_hic_amd import GPEngine
    return GPEngine(0)


def _dev(a):
    torch, dev = _torch()
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), device=dev)


def _run(J, y, C, Cadd, x, wt=None, splits=None):
    """the unpacked sums of the rows, accumulated in the slabs `splits` (row counts; default one call)"""
    torch, dev = _torch()
    eng = _util()
    W, M, d = J.shape
    acc = torch.zeros(eng.sens_acc_doubles(M, d), dtype=torch.float64, device=dev)
    cnt = torch.zeros(2, dtype=torch.int64, device=dev)
    Cd = _dev(Cadd)
    i0 = 0
    for n in splits or [W]:
        i1 = i0 + n
        eng.sens_accumulate(_dev(J[i0:i1]), _dev(y[i0:i1]), _dev(C[i0:i1]), Cd, _dev(x[i0:i1]),
                            None if wt is None else _dev(wt[i0:i1]), acc, cnt)
        i0 = i1
    assert i0 == W
    return eng.sens_unpack(acc, cnt, M, d), acc.cpu().numpy(), cnt.cpu().numpy()


def _lds_edge(d):
    from gpbayestools_hic_amd import GPEngine
    return max(m for m in range(1, 400) if GPEngine.sens_path(m, d) == "lds")


# ---------------------------------------------------------------------------- 1. accuracy of F
def _shapes():
    Me = _lds_edge(20)
    return [(1, 1), (3, 2), (17, 5), (33, 20), (64, 20), (Me, 20), (Me + 1, 20), (130, 20), (5, 64)]


@pytest.mark.parametrize("idx", range(9))
def test_fisher_accuracy(idx):
    """W = 5 rows of C = B B^T + 1e-6 tr / M I; every row's F on its own (one call per row, so that no sum enters), the five
    matrices of a case against the long-double model's as one array, at the bar above.
    Worst ratio err(device) / err(scipy) measured: 4.26 at (80, 20), 4.16 at (33, 20); 0.12 to 1.53 at the other seven."""
    from gpbayestools_hic_amd import GPEngine
    M, d = _shapes()[idx]
    if idx in (5, 6):
        assert GPEngine.sens_path(M, d) == ("lds" if idx == 5 else "global")
    J, y, C, x = R.spd_case(5, M, d, seed=1000 + idx)
    r = R.rows(J, y, C, None, x)
    assert not r["bad"].any()
    Fd = np.zeros((5, d, d))
    for w in range(5):
        u, _, cnt = _run(J[w:w + 1], y[w:w + 1], C[w:w + 1], None, x[w:w + 1])
        assert cnt.tolist() == [1, 0] and u["wsum"] == 1.0
        Fd[w] = u["fisher"]
    # one error per case: the largest deviation over the five rows against the largest entry of the five long-double matrices
    e_dev, e_ref = R.err(Fd, r["F"]), R.err(r["F64"], r["F"])
    lines = ["M=%d d=%d path=%s err_device=%.3e err_scipy=%.3e ratio=%.2f"
             % (M, d, GPEngine.sens_path(M, d), e_dev, e_ref, e_dev / e_ref if e_ref > 0 else float("inf"))]
    print(lines[-1])
    assert e_dev <= R.f_bar(e_ref), lines[-1]
    out = os.environ.get("GPB_SENS_ACCURACY_OUT")           # (the record in profiles/sens_accuracy.txt is made this way)
    if out:
        with open(out, "a") as f:
            f.write("\n".join(lines) + "\n")


# ---------------------------------------------------------------------------- 2. per-row values
@pytest.mark.parametrize("M,d", [(3, 2), (17, 5), (64, 20), (130, 20)])
@pytest.mark.parametrize("with_cadd", [False, True])
def test_one_row_is_the_host_formulas_bit_for_bit(M, d, with_cadd):
    J, y, C, x = R.spd_case(1, M, d, seed=M + d)
    Cadd = np.diag(np.random.default_rng(2).uniform(0.1, 1.0, M)) if with_cadd else None
    u, _, cnt = _run(J, y, C, Cadd, x)
    assert u["wsum"] == 1.0 and cnt.tolist() == [1, 0]
    Rm, Im = R.response(J, y, x)[0], R.information(J, C, Cadd)[0]
    assert np.array_equal(u["response"], Rm) and np.array_equal(u["obs_information"], Im)
    assert np.array_equal(u["response_sq"], Rm * Rm)
    assert np.array_equal(u["fisher"], u["fisher"].T)


def test_a_zero_mean_stays_in_its_own_entries():
    J, y, C, x = R.spd_case(1, 4, 3, seed=9)
    y[0, 2] = 0.0
    u, _, _ = _run(J, y, C, None, x)
    assert not np.isfinite(u["response"][2]).any()
    keep = [0, 1, 3]
    assert np.array_equal(u["response"][keep], R.response(J, y, x)[0][keep])
    assert np.isfinite(u["fisher"]).all() and np.isfinite(u["obs_information"]).all()


# ---------------------------------------------------------------------------- 3. slab independence
def test_slabs_give_the_bits_of_one_call():
    torch, dev = _torch()
    eng = _util()
    J, y, C, x = R.spd_case(600, 17, 5, seed=11)
    wt = np.random.default_rng(12).uniform(0.0, 2.0, 600)
    for weights in (None, wt):
        _, a1, c1 = _run(J, y, C, None, x, weights)
        for splits in ((256, 256, 88), (512, 88)):
            _, a, c = _run(J, y, C, None, x, weights, splits)
            assert np.array_equal(a, a1) and np.array_equal(c, c1), splits
        assert c1.tolist() == [600, 0]
    # after a ragged slab the next call is refused and nothing is written
    acc = torch.zeros(eng.sens_acc_doubles(17, 5), dtype=torch.float64, device=dev)
    cnt = torch.zeros(2, dtype=torch.int64, device=dev)
    eng.sens_accumulate(_dev(J[:88]), _dev(y[:88]), _dev(C[:88]), None, _dev(x[:88]), None, acc, cnt)
    a0, c0 = acc.cpu().numpy(), cnt.cpu().numpy()
    from gpbayestools_hic_amd import _native as nat
    Cd = _dev(C[88:344])
    rc = eng.lib.gpb_sens_accumulate(eng.h, 256, 17, 5, nat.ptr(_dev(J[88:344])), nat.ptr(_dev(y[88:344])), nat.ptr(Cd), None,
                                     nat.ptr(_dev(x[88:344])), None, nat.ptr(acc), nat.ptr(cnt))
    assert rc == E_STATE
    assert np.array_equal(acc.cpu().numpy(), a0) and np.array_equal(cnt.cpu().numpy(), c0) and c0.tolist() == [88, 0]
    assert np.array_equal(Cd.cpu().numpy(), C[88:344])
    with pytest.raises(nat.GPBError, match="256"):
        eng.sens_accumulate(_dev(J[88:344]), _dev(y[88:344]), Cd, None, _dev(x[88:344]), None, acc, cnt)


# ---------------------------------------------------------------------------- 4. weights and bad rows
@pytest.mark.parametrize("M,d", [(17, 5), (90, 7)])
def test_weighted_sums_against_the_model(M, d):
    W = 300
    J, y, C, x = R.spd_case(W, M, d, seed=21)
    rng = np.random.default_rng(22)
    wt = rng.uniform(0.0, 3.0, W)
    wt[rng.choice(W, 40, replace=False)] = 0.0
    Cadd = np.diag(rng.uniform(0.1, 1.0, M))
    u, _, cnt = _run(J, y, C, Cadd, x, wt)
    s = R.sums(R.rows(J, y, C, Cadd, x), wt)
    assert cnt.tolist() == [W, 0]
    assert abs(u["wsum"] - float(s["wsum"])) <= 256 * R.EPS * float(s["wsum"])
    e_dev, e_ref = R.err(u["fisher"], s["fisher"]), R.err(s["fisher64"], s["fisher"])
    print("weighted F: err_device=%.3e err_scipy=%.3e" % (e_dev, e_ref))
    assert e_dev <= R.f_bar(e_ref)
    for k in ("response", "response_sq", "obs_information"):
        diff = np.abs(u[k].astype(np.longdouble) - s[k]).astype(np.float64)
        bar = R.sum_bar(s["abs_" + k])
        print("%s: worst ratio to the bar %.3f" % (k, float(np.max(diff / bar))))
        assert np.all(diff <= bar), k


@pytest.mark.parametrize("M,d", [(6, 3), (90, 4)])
def test_a_bad_row_is_a_weightless_row(M, d):
    """seven rows, row 3 indefinite (one eigenvalue flipped): counted once, and the sums are those of the call with row 3 valid
    and weight 0; a NaN in a weight-0 row changes nothing"""
    J, y, C, x = R.spd_case(7, M, d, seed=31)
    ev, V = np.linalg.eigh(C[3])
    ev[M // 2] = -ev[M // 2]
    Cb = C.copy()
    Cb[3] = (V * ev) @ V.T
    Cb[3] = 0.5 * (Cb[3] + Cb[3].T)
    wt = np.array([1.0, 0.5, 2.0, 1.5, 0.0, 1.0, 0.25])
    _, a_bad, c_bad = _run(J, y, Cb, None, x, wt)
    w0 = wt.copy()
    w0[3] = 0.0
    _, a_0, c_0 = _run(J, y, C, None, x, w0)
    assert c_bad.tolist() == [7, 1] and c_0.tolist() == [7, 0]
    assert np.isfinite(a_bad).all() and np.array_equal(a_bad, a_0)
    Jn, yn, Cn, xn = J.copy(), y.copy(), C.copy(), x.copy()
    Jn[4, 0, 0] = yn[4, 1] = Cn[4, 0, 0] = xn[4, 0] = np.nan
    _, a_n, c_n = _run(Jn, yn, Cn, None, xn, w0)
    assert np.array_equal(a_n, a_0) and np.array_equal(c_n, c_0)
    # without weights the bad row is left out just the same
    _, a_u, c_u = _run(J, y, Cb, None, x)
    keep = [0, 1, 2, 4, 5, 6]
    _, a_k, _ = _run(J[keep], y[keep], C[keep], None, x[keep])
    assert c_u.tolist() == [7, 1] and a_u[0] == 6.0 and np.isfinite(a_u).all()
    assert np.allclose(a_u, a_k, rtol=1e-13, atol=0)


# ---------------------------------------------------------------------------- 5. argument errors
def test_argument_errors_write_nothing():
    torch, dev = _torch()
    from gpbayestools_hic_amd import _native as nat
    eng = _util()
    W, M, d = 4, 3, 2
    J, y, C, x = R.spd_case(W, M, d, seed=41)
    big = 5000
    t = dict(J=_dev(J), y=_dev(y), C=_dev(C), x=_dev(x), acc=torch.full((big,), 7.0, dtype=torch.float64, device=dev),
             cnt=torch.zeros(2, dtype=torch.int64, device=dev))

    def call(W=W, M=M, d=d, ctx=True, **null):
        p = {k: (None if null.get(k) else nat.ptr(v)) for k, v in t.items()}
        return eng.lib.gpb_sens_accumulate(eng.h if ctx else None, W, M, d, p["J"], p["y"], p["C"], None, p["x"], None, p["acc"],
                                           p["cnt"])
    assert call(ctx=False) == E_ARG
    for name in ("J", "y", "C", "x", "acc", "cnt"):
        assert call(**{name: True}) == E_ARG, name
    assert call(W=-1) == E_ARG and call(M=0) == E_ARG and call(d=0) == E_ARG
    assert call(M=2049) == E_ARG and call(d=65) == E_ARG
    assert call(W=0) == 0                                  # a no-op
    assert (t["acc"] == 7.0).all().item() and t["cnt"].tolist() == [0, 0]
    assert np.array_equal(t["C"].cpu().numpy(), C)
    acc = torch.zeros(eng.sens_acc_doubles(M, d), dtype=torch.float64, device=dev)
    with pytest.raises(ValueError):
        eng.sens_accumulate(t["J"], t["y"][:, :2], t["C"], None, t["x"], None, acc, t["cnt"])
    with pytest.raises(ValueError):
        eng.sens_accumulate(t["J"], t["y"], t["C"], None, t["x"], None, acc[:-1], t["cnt"])
    with pytest.raises(ValueError):
        eng.sens_accumulate(t["J"], t["y"], t["C"], None, t["x"], None, acc, t["cnt"].to(torch.int32))
    with pytest.raises(ValueError):
        eng.sens_accumulate(t["J"].cpu(), t["y"], t["C"], None, t["x"], None, acc, t["cnt"])


# ---------------------------------------------------------------------------- 6. emu_predict_jac on the device
MODES = {"pca": 0, "no_pca": 1, "expdiag": 2, "no_pca_expdiag": 3}


@functools.lru_cache(maxsize=None)
def _mode_engine(mode):
    """the small engine of tests/test_gpu_ppd.py: N = 100, d = 3; PCA modes P = 3, M = 5, no-PCA modes P = M = 5"""
    from gpbayestools_hic_amd import GPEngine
    no_pca = mode in ("no_pca", "no_pca_expdiag")
    P, M = (5, 5) if no_pca else (3, 5)
    X, Z = CV.make_data(100, 3, P, 21)
    eng = GPEngine(0)
    eng.set_data(X, 0.3 * Z, "RBF", CV.ALPHA)
    eng.set_theta(CV.thetas_of(("mid", "hard", "aniso", "mid", "aniso")[:P], 3))
    eng.factor()
    rng = np.random.default_rng(4)
    mu = 0.2 * rng.standard_normal(M)
    if no_pca:
        eng.set_transform(MODES[mode], mu, scale=rng.uniform(0.5, 1.5, M))
    else:
        B = rng.standard_normal((M, M))
        eng.set_transform(MODES[mode], mu, A=0.5 * rng.standard_normal((P, M)), cov_trunc=0.01 * B @ B.T)
    return eng, M


@pytest.mark.parametrize("mode", list(MODES))
def test_predict_jac_on_the_device(mode):
    torch, dev = _torch()
    from gpbayestools_hic_amd import synth
    eng, M = _mode_engine(mode)
    Xs = synth.walkers(130, 3, seed=8)
    want = eng.emu_predict_jac(Xs)
    assert isinstance(want, np.ndarray) and want.shape == (130, M, 3)
    Xd = torch.as_tensor(Xs, device=dev)
    got = eng.emu_predict_jac(Xd)
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), want)
    out = torch.full((130, M, 3), float("nan"), dtype=torch.float64, device=dev)
    assert eng.emu_predict_jac(Xd, out=out) is out and np.array_equal(out.cpu().numpy(), want)
    with pytest.raises(ValueError):
        eng.emu_predict_jac(Xd, out=out[:100])
    with pytest.raises(ValueError):
        eng.emu_predict_jac(Xs, out=out)


# ---------------------------------------------------------------------------- 7. Chain.sensitivity
SPECS = [(100, 5, 3, "RBF"), (130, 4, 2, "Matern25")]
FIELDS = ("n_bad", "response_mean", "response_std", "obs_information", "fisher", "fisher_total", "information", "param_mean",
          "param_cov")


@functools.lru_cache(maxsize=None)
def _chain(mapped):
    import tempfile
    from gpbayestools_hic_amd import synth, workload
    chain, emus, info = workload.build_multi_chain(SPECS, 20, workdir=tempfile.mkdtemp(prefix="gpb_sens_"), mapped=mapped)
    X = synth.walkers(300, 20, seed=31)
    return chain, X, chain.sensitivity(X)


@pytest.mark.parametrize("mapped", [False, True])
def test_chain_sensitivity(mapped):
    chain, X, res = _chain(mapped)
    S, d = X.shape
    width = chain.max - chain.min
    assert res.n_samples == S and res.n_bad.tolist() == [0, 0] and res.names == list(chain.pardict)
    assert res.fisher.shape == (2, d, d) and res.response_mean.shape == (chain.nobs, d)
    r0 = 0
    for k, emu in enumerate(chain.emuList):
        M = emu.nobs
        J = emu.predict_jacobian(X)
        y, C = emu.predict(X, return_cov=True)
        Cadd = chain.expdata_cov[r0:r0 + M, r0:r0 + M]
        s = R.sums(R.rows(J, y, C, Cadd, X))
        assert float(s["wsum"]) == S and s["n_bad"] == 0
        e_dev, e_ref = R.err(res.fisher[k] * S, s["fisher"]), R.err(s["fisher64"], s["fisher"])
        print("mapped=%s emulator %d: F err_device=%.3e err_scipy=%.3e bar=%.3e" % (mapped, k, e_dev, e_ref, R.f_bar(e_ref)))
        # (the division by S and the multiplication back are two more roundings: inside the bar's floor)
        assert e_dev <= R.f_bar(e_ref)
        rows = slice(r0, r0 + M)
        worst = 0.0
        for got, key in ((res.response_mean[rows] * S, "response"), (res.obs_information[rows] / (width * width) * S, "obs_information")):
            diff = np.abs(got.astype(np.longdouble) - s[key]).astype(np.float64)
            bar = R.sum_bar(s["abs_" + key])
            worst = max(worst, float(np.max(diff / bar)))
            assert np.all(diff <= bar), key
        m1 = (s["response"] / S).astype(np.float64)
        var = (s["response_sq"] / S).astype(np.float64) - m1 * m1
        bar = R.sum_bar(s["abs_response_sq"]) / S + 2 * np.abs(m1) * R.sum_bar(s["abs_response"]) / S + 8 * R.EPS * np.abs(m1 * m1)
        assert np.all(np.abs(res.response_std[rows] ** 2 - np.maximum(var, 0.0)) <= bar + 4 * R.EPS * np.abs(var))
        print("mapped=%s emulator %d: sums' worst ratio to the bar %.3f" % (mapped, k, worst))
        r0 += M
    assert np.array_equal(res.information, np.stack([np.diag(f) for f in res.fisher]) * (width * width)[None, :])
    assert np.array_equal(res.fisher_total, res.fisher.sum(0))
    assert np.allclose(res.param_mean, X.mean(0), rtol=1e-13) and np.allclose(res.param_cov, np.cov(X.T, bias=True), rtol=1e-10)
    ev, _ = res.stiff_directions()
    assert ev.shape == (d,) and ev[0] > 0
    # slabs, unit weights, a stored [nwalkers, nsteps, ndim] chain: the same bits
    chain.sens_slab_rows = 256
    try:
        r_slab = chain.sensitivity(X)
    finally:
        chain.sens_slab_rows = None
    r_ones = chain.sensitivity(X, weights=np.ones(S))
    r_3d = chain.sensitivity(X.reshape(3, 100, d).transpose(1, 0, 2))      # [nwalkers = 100, nsteps = 3]: another row order
    for f in FIELDS:
        assert np.array_equal(getattr(r_slab, f), getattr(res, f)), f
        assert np.array_equal(getattr(r_ones, f), getattr(res, f)), f
    assert r_3d.n_samples == S and np.allclose(r_3d.fisher, res.fisher, rtol=1e-10)
    half = chain.sensitivity(X.reshape(3, 100, d), discard=50)
    assert half.n_samples == 150


def test_sampler_sensitivity_is_the_chains_on_the_stored_rows():
    """StretchSampler.sensitivity(discard, thin): the stored [nsteps, nwalkers, ndim] view, flattened and copied to the host, gives
    what Chain.sensitivity gives on those rows (same rows, same order: the same bits)"""
    from gpbayestools_hic_amd import StretchSampler, synth
    chain, _, _ = _chain(False)
    s = StretchSampler(chain, 40, seed=5)
    with pytest.raises(AttributeError):
        s.sensitivity()
    s.run(synth.walkers_ball(40, np.full(20, 0.5), 0.02, seed=6), 12)
    for discard, thin in ((0, 1), (3, 2)):
        a = s.sensitivity(discard=discard, thin=thin)
        rows = s._chain_dev[discard::thin].reshape(-1, 20).cpu().numpy()
        b = chain.sensitivity(rows)
        assert a.n_samples == rows.shape[0] == 40 * len(range(discard, 12, thin))
        for f in FIELDS:
            assert np.array_equal(getattr(a, f), getattr(b, f)), f
    with pytest.raises(ValueError):
        s.sensitivity(thin=0)


# ---------------------------------------------------------------------------- 8. the notebook's matrix
def test_response_is_the_notebooks_matrix():
    """three rows, one at a time: R from the device against examples/SensitivityAnalysis.ipynb's central differences of
    chain._predict at relative steps h = 1e-4 and 2e-4: |R - FD(h)| <= |FD(2h) - FD(h)| + 1e-9 max(1, |R|) — three times the
    Richardson estimate of FD(h)'s truncation error, plus FD's rounding 2^-53 |y| / h"""
    chain, X, _ = _chain(False)

    def predict(x):
        return chain._predict(x[None, :])[0][0]
    for i in (0, 7, 123):
        Rd = chain.sensitivity(X[i:i + 1]).response_mean
        f1, f2 = R.notebook_response(predict, X[i], 1e-4), R.notebook_response(predict, X[i], 2e-4)
        bar = np.abs(f2 - f1) + 1e-9 * np.maximum(1.0, np.abs(Rd))
        assert np.all(np.abs(Rd - f1) <= bar), (i, float(np.max(np.abs(Rd - f1) / bar)))


# ---------------------------------------------------------------------------- 9. refusals
def test_chain_sensitivity_refusals():
    chain, X, _ = _chain(False)

    class Foreign:
        nobs = 4

        def predict(self, X, return_cov=True, extra_std=0):
            return np.zeros((X.shape[0], 4)), np.zeros((X.shape[0], 4, 4))

    class TwoRanks:
        world, rank = 2, 0

    keep, cov = list(chain.emuList), chain.expdata_cov
    try:
        chain.emuList = [keep[0], Foreign()]
        with pytest.raises(NotImplementedError, match="foreign"):
            chain.sensitivity(X)
        chain.emuList = keep
        chain.sharding = TwoRanks()
        with pytest.raises(NotImplementedError, match="sharded"):
            chain.sensitivity(X)
        chain.sharding = None
        chain.set_systematics(0.03 * chain.expdata[0][None, :])           # one normalisation source shared by all observables
        with pytest.raises(NotImplementedError, match="couples"):
            chain.sensitivity(X)
    finally:
        chain.emuList, chain.sharding, chain.expdata_cov = keep, None, cov
    for bad in (X[:, :19], X.reshape(2, 3, 50, 20), np.zeros((0, 20))):
        with pytest.raises(ValueError):
            chain.sensitivity(bad)
    Xn = X.copy()
    Xn[5, 2] = np.inf
    with pytest.raises(ValueError):
        chain.sensitivity(Xn)
    for w in (-np.ones(300), np.zeros(300), np.ones(299)):
        with pytest.raises(ValueError):
            chain.sensitivity(X, weights=w)
    with pytest.raises(ValueError):
        chain.sensitivity(X.reshape(3, 100, 20), weights=np.ones(300))
    assert np.array_equal(chain.sensitivity(X).fisher, _chain(False)[2].fisher)         # the chain is as it was
