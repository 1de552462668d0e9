"""GPU tier: the pointwise leave-one-out conditionals on the device — gpb_loo_pointwise (GPEngine.loo_pointwise) — against the
numpy model of tests/psis_reference.py, and posterior_loo / Chain.loo / sampler.loo end to end on the synthetic chain of
tests/test_gpu_gof.py.

Bar of the conditionals: 1e-10 relative (to 1 + |value|), the project's parity standard, on covariances Q diag(lambda) Q^T with
lambda in [1, 100] (condition number <= 100, plus a positive definite Cadd): np.linalg.inv is then good to ~1e-14 and a fair
reference.  A bad row against the run without it, a slab against one call, a result against itself: bit equality."""
import functools
import warnings

import numpy as np
import pytest
import scipy.special

import psis_reference as R

pytestmark = pytest.mark.gpu

REL_BAR = 1e-10
E_ARG = -1


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _eng():
    from gpbayestools_hic_amd import GPEngine
    return GPEngine(0)


def _dev(a):
    torch, dev = _torch()
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), device=dev)


def _run(y, C, yexp, Cadd, with_zc=True, ld=None):
    torch, dev = _torch()
    W, M = y.shape
    ld = W if ld is None else ld
    ll = torch.full((M, ld), 7.0, dtype=torch.float64, device=dev)
    zc = torch.full((M, ld), 7.0, dtype=torch.float64, device=dev) if with_zc else None
    flag = torch.full((W,), 9, dtype=torch.uint8, device=dev)
    _eng().loo_pointwise(_dev(y), _dev(C), _dev(yexp), _dev(Cadd), ll[:, :W], None if zc is None else zc[:, :W], flag)
    return ll.cpu().numpy(), None if zc is None else zc.cpu().numpy(), flag.cpu().numpy()


@pytest.mark.parametrize("M", [1, 2, 63, 64, 65, 89, 90, 130])
@pytest.mark.parametrize("with_add", [False, True])
def test_conditionals_against_the_model(M, with_add):
    """M on both sides of the LDS rule (89 | 90) and of a wave, W = 3 rows.  Measured: worst 9.0e-15 (M = 89), far below 1/16 of the bar."""
    eng = _eng()
    assert eng.gof_path(M) == ("lds" if M <= 89 else "global")
    y, C, yexp, Cadd = R.well_conditioned_cov(3, M, seed=1, with_add=with_add)
    want_ll, want_zc = R.loo_pointwise(y, C, yexp, Cadd)
    ll, zc, flag = _run(y, C, yexp, Cadd)
    e1 = float((np.abs(ll - want_ll) / (1 + np.abs(want_ll))).max())
    e2 = float((np.abs(zc - want_zc) / (1 + np.abs(want_zc))).max())
    print("loo_pointwise M=%d Cadd=%s: ll %.1e  zc %.1e" % (M, with_add, e1, e2))
    assert not flag.any() and e1 <= REL_BAR and e2 <= REL_BAR
    ll2, none, _ = _run(y, C, yexp, Cadd, with_zc=False)
    assert none is None and np.array_equal(ll2, ll)


@pytest.mark.parametrize("W", [1, 255, 257])
@pytest.mark.parametrize("M", [5, 90])
def test_rows_strides_and_a_bad_row(W, M):
    """W in {1, 255, 257} rows on both paths, written into the first W columns of a wider array: against the model, the columns
    beyond W untouched; then the middle row's covariance made indefinite: NaN in that column only, its flag alone raised, the
    neighbours bit for bit what they were"""
    y, C, yexp, Cadd = R.well_conditioned_cov(W, M, seed=2, with_add=True)
    want_ll, want_zc = R.loo_pointwise(y, C, yexp, Cadd)
    ll, zc, flag = _run(y, C, yexp, Cadd, ld=W + 3)
    assert np.all(ll[:, W:] == 7.0) and np.all(zc[:, W:] == 7.0) and not flag.any()
    e = max(float((np.abs(ll[:, :W] - want_ll) / (1 + np.abs(want_ll))).max()), float((np.abs(zc[:, :W] - want_zc) / (1 + np.abs(want_zc))).max()))
    print("loo_pointwise W=%d M=%d: %.1e" % (W, M, e))
    assert e <= REL_BAR
    b = W // 2
    Cb = C.copy()
    Cb[b, M - 1, M - 1] = -1e3                                   # the last pivot turns negative
    ll_b, zc_b, flag_b = _run(y, Cb, yexp, Cadd, ld=W + 3)
    assert flag_b[b] == 1 and flag_b.sum() == 1
    assert np.isnan(ll_b[:, b]).all() and np.isnan(zc_b[:, b]).all()
    keep = np.arange(W + 3) != b
    assert np.array_equal(ll_b[:, keep], ll[:, keep]) and np.array_equal(zc_b[:, keep], zc[:, keep])


def test_argument_errors():
    torch, dev = _torch()
    eng = _eng()
    from gpbayestools_hic_amd import _native as nat
    y, C, yexp, _ = R.well_conditioned_cov(4, 3, seed=3)
    t = dict(y=_dev(y), C=_dev(C), yexp=_dev(yexp), ll=torch.zeros((3, 4), dtype=torch.float64, device=dev),
             flag=torch.zeros(4, dtype=torch.uint8, device=dev))
    p = {k: nat.ptr(v) for k, v in t.items()}
    call = eng.lib.gpb_loo_pointwise
    assert call(eng.h, 4, 0, p["y"], p["C"], p["yexp"], None, p["ll"], None, 4, p["flag"]) == E_ARG
    assert call(eng.h, 4, 2049, p["y"], p["C"], p["yexp"], None, p["ll"], None, 4, p["flag"]) == E_ARG
    assert call(eng.h, 4, 3, p["y"], p["C"], p["yexp"], None, p["ll"], None, 3, p["flag"]) == E_ARG
    assert call(eng.h, 4, 3, p["y"], p["C"], p["yexp"], None, None, None, 4, p["flag"]) == E_ARG
    assert call(eng.h, 4, 3, p["y"], p["C"], p["yexp"], None, p["ll"], None, 4, None) == E_ARG
    assert call(eng.h, 0, 3, p["y"], p["C"], p["yexp"], None, p["ll"], None, 4, p["flag"]) == 0
    assert float(t["ll"].abs().sum()) == 0.0
    with pytest.raises(ValueError):
        eng.loo_pointwise(t["y"], t["C"], t["yexp"], None, t["ll"][:, :3], None, t["flag"])
    with pytest.raises(ValueError):
        eng.loo_pointwise(t["y"], t["C"], t["yexp"], None, t["ll"], None, t["flag"].to(torch.int32))
    with pytest.raises(ValueError):
        eng.loo_pointwise(t["y"], t["C"], t["yexp"], None, t["ll"].t().contiguous().t(), None, t["flag"])


# ---------------------------------------------------------------------------- the chain
SPECS = [(100, 5, 3, "RBF"), (130, 4, 2, "Matern25"), (90, 6, 3, "RBF")]
FIELDS = ("elpd_loo", "p_loo", "lppd", "elpd_waic", "p_waic", "khat", "ess", "n_tail", "loo_pit", "min_ll")


@functools.lru_cache(maxsize=None)
def _chain():
    import tempfile
    from gpbayestools_hic_amd import synth, workload
    chain, emus, info = workload.build_multi_chain(SPECS, 20, workdir=tempfile.mkdtemp(prefix="gpb_loo_"), mapped=False)
    X = synth.walkers_ball(600, info["xstar"], 0.01, seed=31)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = {u: chain.loo(X, unit=u, return_pointwise=True) for u in ("observable", "dataset")}
    return chain, X, res, info


def _same(a, b):
    for f in FIELDS:
        assert np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True), f
    assert a.n_samples == b.n_samples and a.n_bad == b.n_bad and a.khat_counts == b.khat_counts


def test_chain_loo_per_observable():
    """Chain.loo on the three-emulator chain of the goodness-of-fit tests, 600 rows around the point the data were made at: the
    pointwise arrays against the model on the emulators' own predictions (1e-9: the device's and the host's predictions differ),
    the result against the model on the returned pointwise arrays (the bars of tests/test_gpu_psis.py), the derived fields, the
    slab size, compare(), the repr"""
    from gpbayestools_hic_amd import loo
    chain, X, res, _ = _chain()
    r = res["observable"]
    S = X.shape[0]
    assert r.unit == "observable" and r.n_units == 15 and r.n_samples == S and r.n_bad == 0
    ll, zc = r.pointwise["ll"], r.pointwise["zc"]
    assert ll.shape == (15, S) and zc.shape == (15, S)
    r0 = 0
    for emu in chain.emuList:
        M = emu.nobs
        y, C = emu.predict(X, return_cov=True)
        w_ll, w_zc = R.loo_pointwise(y, C, chain.expdata[0][r0:r0 + M], chain.expdata_cov[r0:r0 + M, r0:r0 + M])
        assert np.allclose(ll[r0:r0 + M], w_ll, rtol=1e-9, atol=1e-9) and np.allclose(zc[r0:r0 + M], w_zc, rtol=1e-9, atol=1e-9)
        r0 += M
    want = R.psis_loo(ll, zc)
    assert np.abs(r.elpd_loo - want[:, 0]).max() <= 1e-11 and np.abs(r.khat - want[:, 3]).max() <= 1e-12
    assert np.array_equal(r.n_tail, want[:, 5].astype(np.int64)) and np.array_equal(r.min_ll, ll.min(axis=1))
    for got, c in ((r.lppd, 1), (r.p_waic, 2), (r.ess, 4), (r.loo_pit, 6)):
        assert np.allclose(got, want[:, c], rtol=1e-12, atol=0)
    assert np.array_equal(r.p_loo, r.lppd - r.elpd_loo) and np.array_equal(r.elpd_waic, r.lppd - r.p_waic)
    assert r.elpd_loo_total == float(r.elpd_loo.sum()) and abs(r.se_elpd_loo - np.sqrt(15 * np.var(r.elpd_loo))) <= 1e-12
    assert np.all(r.p_loo > 0) and np.all((r.loo_pit > 0) & (r.loo_pit < 1))
    k = r.khat
    assert r.khat_counts == (int(((k > 0.5) & (k <= 0.7)).sum()), int(((k > 0.7) & (k <= 1)).sum()), int((k > 1).sum()))
    assert "elpd_loo" in repr(r) and "khat" in repr(r)
    chain.gof_slab_rows = 256
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            r_slab = chain.loo(X)
            no_pit = chain.loo(X, pit=False)
    finally:
        chain.gof_slab_rows = None
    _same(r_slab, r)
    assert r_slab.pointwise is None and np.isnan(no_pit.loo_pit).all() and np.array_equal(no_pit.elpd_loo, r.elpd_loo)
    c = loo.compare(r, r_slab)
    assert c.elpd_diff == 0.0 and c.se == 0.0 and c.elpd_waic_diff == 0.0 and c.n_units == 15 and "elpd_diff" in repr(c)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        half = chain.loo(X.reshape(3, 200, 20), discard=100)
    assert half.n_samples == 300


def test_chain_loo_per_data_set():
    """unit="dataset": lppd is logsumexp of goodness_of_fit(return_rows=True)'s loglike minus M / 2 ln 2 pi minus ln S (1e-12
    relative); the result against the model on the returned rows; no PIT; slabs give the same bits"""
    chain, X, res, _ = _chain()
    r = res["dataset"]
    S = X.shape[0]
    assert r.unit == "dataset" and r.n_units == 3 and r.n_bad == 0 and np.isnan(r.loo_pit).all() and "zc" not in r.pointwise
    gof = chain.goodness_of_fit(X, return_rows=True, influence=False)
    Ms = np.array([5, 4, 6])
    lppd = scipy.special.logsumexp(gof.rows["loglike"], axis=0) - 0.5 * Ms * np.log(2 * np.pi) - np.log(S)
    print("loo per data set: lppd against goodness_of_fit's rows, worst %.1e relative" % np.max(np.abs(r.lppd - lppd) / np.abs(lppd)))
    assert np.allclose(r.lppd, lppd, rtol=1e-12, atol=0)
    want = R.psis_loo(r.pointwise["ll"])
    assert np.abs(r.elpd_loo - want[:, 0]).max() <= 1e-11
    fin = np.isfinite(want[:, 3])
    assert np.abs(r.khat[fin] - want[fin, 3]).max() <= 1e-12 and np.array_equal(r.n_tail, want[:, 5].astype(np.int64))
    chain.gof_slab_rows = 256
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _same(chain.loo(X, unit="dataset"), r)
    finally:
        chain.gof_slab_rows = None


def test_a_shifted_observable_stands_out():
    """pseudo-data from the chain's own predictive distribution at x0 with one observable moved by 5 sigma of its conditional
    distribution: among the fifteen it has the largest khat and the lowest elpd_loo — first for the model on the emulators' own
    predictions (the seed is judged by the reference alone), then on the device"""
    from gpbayestools_hic_amd import synth
    chain, _, _, info = _chain()
    x0 = info["xstar"]
    X = synth.walkers_ball(600, x0, 0.05, seed=77)
    rng = np.random.default_rng(78)
    keep = chain.expdata
    target = 7                                                   # observable 2 of emulator 1
    pseudo, ref_ll, r0 = [], [], 0
    for k, emu in enumerate(chain.emuList):
        M = emu.nobs
        mu, C = emu.predict(x0[None, :], return_cov=True)
        Ce = chain.expdata_cov[r0:r0 + M, r0:r0 + M]
        yk = mu[0] + np.linalg.cholesky(C[0] + Ce) @ rng.standard_normal(M)
        if r0 <= target < r0 + M:
            m = target - r0
            yk[m] += 5.0 / np.sqrt(np.linalg.inv(C[0] + Ce)[m, m])
        pseudo.append(yk)
        y, Cx = emu.predict(X, return_cov=True)
        ref_ll.append(R.loo_pointwise(y, Cx, yk, Ce)[0])
        r0 += M
    ref = R.psis_loo(np.concatenate(ref_ll))
    print("shifted observable: reference khat %s\n  elpd_loo %s" % (np.round(ref[:, 3], 3).tolist(), np.round(ref[:, 0], 2).tolist()))
    assert np.argmax(ref[:, 3]) == target and np.argmin(ref[:, 0]) == target
    try:
        chain.expdata = np.concatenate(pseudo)[None, :]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            res = chain.loo(X)
    finally:
        chain.expdata = keep
    print("shifted observable: device khat %s" % np.round(res.khat, 3).tolist())
    assert int(np.argmax(res.khat)) == target and int(np.argmin(res.elpd_loo)) == target
    assert np.allclose(res.elpd_loo, ref[:, 0], rtol=1e-7, atol=1e-7)


def test_khat_warning():
    from gpbayestools_hic_amd import loo
    cols = np.zeros((4, 8))
    cols[:, 3] = [0.2, 0.6, 0.8, 1.4]
    r = loo.LooResult("observable", 10, 0, cols)
    assert r.khat_counts == (1, 1, 1)
    chain, X, res, _ = _chain()
    r = res["dataset"]
    if np.any(r.khat > 0.7):
        with pytest.warns(UserWarning, match="khat above 0.7"):
            chain.loo(X, unit="dataset")


def test_refusals_and_the_coupled_chain(tmp_path):
    from gpbayestools_hic_amd import loo, synth
    from gpbayestools_hic_amd.workload import build_multi_chain
    chain, X, res, _ = _chain()
    with pytest.raises(ValueError, match="resample"):
        chain.loo(X, weights=np.ones(X.shape[0]))
    with pytest.raises(ValueError):
        chain.loo(X, unit="emulator")
    for bad in (X[:, :19], X[:1], np.zeros((2, 3, 4, 20))):
        with pytest.raises(ValueError):
            chain.loo(bad)
    with pytest.raises(ValueError, match="same unit"):
        loo.compare(res["observable"], res["dataset"])
    short = loo.LooResult("observable", 10, 0, np.zeros((14, 8)))
    with pytest.raises(ValueError):
        loo.compare(res["observable"], short)

    class TwoRanks:
        world, rank = 2, 0
    try:
        chain.sharding = TwoRanks()
        with pytest.raises(NotImplementedError, match="sharded"):
            chain.loo(X)
    finally:
        chain.sharding = None
    # a coupled expdata_cov: the joint matrix per observable, no data sets
    cch, _, _ = build_multi_chain([(48, 12, 3, "RBF"), (64, 20, 5, "Matern25")], 5, workdir=str(tmp_path))
    Xc = synth.walkers(300, 5, seed=5)
    cch.set_systematics(0.03 * cch.expdata[0][None, :])
    with pytest.raises(NotImplementedError, match="not factors"):
        cch.loo(Xc, unit="dataset")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rc = cch.loo(Xc, return_pointwise=True)
    assert cch._coupled and rc.n_units == 32 and rc.n_bad == 0
    ys, Cs = zip(*[e.predict(Xc, return_cov=True) for e in cch.emuList])
    Cj = np.zeros((300, 32, 32))
    Cj[:, :12, :12], Cj[:, 12:, 12:] = Cs
    w_ll, w_zc = R.loo_pointwise(np.concatenate(ys, axis=1), Cj, cch.expdata[0], cch.expdata_cov)
    assert np.allclose(rc.pointwise["ll"], w_ll, rtol=1e-8, atol=1e-8) and np.allclose(rc.pointwise["zc"], w_zc, rtol=1e-8, atol=1e-8)


def test_sampler_loo_is_the_chains_on_the_stored_rows():
    from gpbayestools_hic_amd import StretchSampler, synth
    chain, _, _, _ = _chain()
    s = StretchSampler(chain, 40, seed=5)
    s.run(synth.walkers_ball(40, np.full(20, 0.5), 0.02, seed=6), 12)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a = s.loo(discard=3, thin=2)
        rows = s._chain_dev[3::2].reshape(-1, 20).cpu().numpy()
        b = chain.loo(rows)
    assert a.n_samples == rows.shape[0] == 40 * len(range(3, 12, 2))
    _same(a, b)
