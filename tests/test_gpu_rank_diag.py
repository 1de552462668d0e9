"""GPU tier: rank-normalised diagnostics of a resident chain — gpb_chain_rank_diag (GPEngine.rank_diag), diagnostics.rank_diagnose,
sampler.rank_diagnostics and Chain.rank_convergence — against the host model of tests/rank_reference.py (scipy's rankdata and
ndtri, numpy's median and quantile, FFT autocovariances, Stan's estimator) on the MH-like AR(1) chains of that module, in which half
the values are ties, and on a case made for the sort.  tests/test_rank_reference.py shows every decision of the estimator's first
loop on these inputs to be at least 5.9e-4 away from flipping.

Exact (array_equal): rank2, median, quant, stop.  Bars, starting from tests/test_gpu_diag.py's for the same kinds of quantity:
R-hat and sd 1e-12 relative (MOM_BAR), ESS 2 (stop + 2) RHO_BAR relative with RHO_BAR = 6e-14 per lag; these series also carry
the deviation of the device's Phi^-1 from scipy's.  Measured on an MI355X over the cases of sections 1 and 2: R-hat within 2.2e-16
relative, sd within 1.9e-14 (shape 130 x 2 x 3, the parameter with the offset of 1e3), ESS within 8.3e-14 relative = 0.011 of
its bar (the same shape and parameter, stop 61; on the slowly mixing chain, stop 345: 8.4e-14 = 0.002 of its bar) — every one
below 1/16 of its starting bar, so the bars stay.  Layouts, parameters
alone, thinned views, on_device, subsets of the outputs, the band, the parameter groups and a second call: bit equality.  Every
case prints its figures with -s.  DESIGN.md section 32."""
import functools
import pickle

import numpy as np
import pytest

import acf_reference as A
import cv_reference as CV
import rank_reference as M

pytestmark = pytest.mark.gpu

E_ARG = -1
RHO_BAR = 6e-14
MOM_BAR = 1e-12
KEYS = ("rank2", "median", "quant", "rhat", "ess", "stop", "sd")
EXACT = ("rank2", "median", "quant", "stop")


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _eng():
    from gpbayestools_hic_amd import GPEngine
    return GPEngine(0)


@functools.lru_cache(maxsize=None)
def _dev_chain(shape, layout="steps"):
    torch, dev = _torch()
    x = torch.as_tensor(np.array(M.mh_chain(*shape)), device=dev)
    return x if layout == "steps" else x.permute(1, 0, 2).contiguous()


@functools.lru_cache(maxsize=None)
def _full(shape):
    """the device's answer with the whole band, steps layout, host outputs, every output: computed once, compared by many"""
    return _eng().rank_diag(_dev_chain(shape), "steps", M.PROBS, None, outputs=KEYS)


def _same(a, b, keys=KEYS):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True) for k in keys)


def _against_model(out, ref, label):
    for k in EXACT:
        if k in out:
            assert out[k].dtype == ref[k].dtype and np.array_equal(out[k], ref[k]), (label, k)
    nan = np.isnan(ref["ess"])
    assert np.array_equal(np.isnan(out["ess"]), nan) and np.array_equal(np.isnan(out["rhat"]), np.isnan(ref["rhat"]))
    with np.errstate(invalid="ignore", divide="ignore"):
        err_rhat = np.abs(out["rhat"] - ref["rhat"]) / np.abs(ref["rhat"])
        err_sd = np.where(ref["sd"] == 0.0, np.abs(out["sd"]), np.abs(out["sd"] - ref["sd"]) / ref["sd"])
        err_ess = np.abs(out["ess"] - ref["ess"]) / np.abs(ref["ess"])
    bar_ess = 2.0 * (ref["stop"] + 2.0) * RHO_BAR
    e_rhat = float(np.nanmax(err_rhat)) if not np.all(np.isnan(err_rhat)) else 0.0
    units = float(np.max(np.where(nan, 0.0, err_ess / bar_ess)))
    print("%s: rhat %.3g rel, sd %.3g rel, ess %.3g rel = %.3g of its bar (stop %s)"
          % (label, e_rhat, float(np.max(err_sd)), float(np.max(np.where(nan, 0.0, err_ess))), units, ref["stop"].tolist()))
    assert e_rhat <= MOM_BAR and float(np.max(err_sd)) <= MOM_BAR
    assert np.all(err_ess[~nan] <= bar_ess[~nan])


# ---------------------------------------------------------------------------- 1. against the host model
@pytest.mark.parametrize("shape", M.SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_rank_diag_matches_the_model(shape):
    out = _full(shape)
    h = shape[0] // 2
    assert out["rank2"].shape == (shape[2], 2 * h * shape[1]) and out["rank2"].dtype == np.int64 and out["stop"].dtype == np.int32
    _against_model(out, M.reference(shape), "shape %s" % (shape,))


@pytest.mark.parametrize("max_lag", M.BAND_LAGS)
def test_band_edges(max_lag):
    """h = 350 = 6 block rows; max_lag 0, 63 (block diagonals 0 and 1), 64, 65 (0 .. 2), 349 (all): against the model, and wherever
    the estimator stayed inside the band bit for bit the answer of the full band; else stop = max_lag | NO_BAND and ess = NaN"""
    shape = M.SHAPES[-1]
    out = _eng().rank_diag(_dev_chain(shape), "steps", M.PROBS, max_lag, outputs=KEYS)
    ref = M.reference(shape, max_lag)
    _against_model(out, ref, "max_lag %d" % max_lag)
    full = _full(shape)
    assert _same(out, full, ("rank2", "median", "quant", "rhat", "sd"))
    inside = out["stop"] < M.NO_BAND
    assert np.array_equal(out["stop"][inside], full["stop"][inside]) and np.array_equal(out["ess"][inside], full["ess"][inside])
    assert M.NO_BAND == _eng().RANK_NO_BAND
    assert np.all(out["stop"][~inside] == (max_lag | M.NO_BAND)) and np.all(np.isnan(out["ess"][~inside]))
    assert np.all(full["stop"][~inside] + 2 > max_lag)                 # flagged only where the first loop read beyond the band
    if max_lag == 0:
        assert not inside.any()
    if max_lag >= 63:
        assert inside.all()


@functools.lru_cache(maxsize=None)
def _long(max_lag=None):
    torch, dev = _torch()
    return _eng().rank_diag(torch.as_tensor(np.array(M.long_chain()), device=dev), "steps", M.PROBS, max_lag, outputs=KEYS)


def test_a_slowly_mixing_chain_reads_every_block_diagonal():
    """phi = 0.97 and 0.95, 700 x 6: one series stops at lag 133, the others at 345 and read rho-hat up to lag 347 — lags of all six
    block diagonals of the band reach ess, against the model; both layouts the same bits"""
    torch, dev = _torch()
    ref = M.long_reference()
    assert sorted(set(ref["stop"].reshape(-1).tolist())) == [133, 345]
    out = _long()
    _against_model(out, ref, "long chain")
    xw = torch.as_tensor(np.ascontiguousarray(np.array(M.long_chain()).transpose(1, 0, 2)), device=dev)
    assert _same(_eng().rank_diag(xw, "walkers", M.PROBS, None, outputs=KEYS), out)


@pytest.mark.parametrize("max_lag", M.LONG_BAND_LAGS)
def test_band_edges_beyond_the_first_block_diagonal(max_lag):
    """the slowly mixing chain with bands that end just below and at what its series read (134 / 135 for the one that stops at
    133, 346 / 347 for those that stop at 345) and at block edges between: against the model; flagged exactly where the first
    loop read beyond the band, and bit for bit the full band's answer everywhere else"""
    out, full, ref = _long(max_lag), _long(), M.long_reference(max_lag)
    _against_model(out, ref, "long chain, max_lag %d" % max_lag)
    assert _same(out, full, ("rank2", "median", "quant", "rhat", "sd"))
    flagged = full["stop"] + 2 > max_lag
    assert np.array_equal(out["stop"] >= M.NO_BAND, flagged)
    assert np.array_equal(out["stop"][~flagged], full["stop"][~flagged]) and np.array_equal(out["ess"][~flagged], full["ess"][~flagged])
    assert np.all(out["stop"][flagged] == (max_lag | M.NO_BAND)) and np.all(np.isnan(out["ess"][flagged]))
    assert flagged.any() == (max_lag < 347) and (~flagged).any() == (max_lag >= 135)


def test_the_sort_case():
    """keys over 600 binades and both signs with +-0.0 and denormals; a run of equal values longer than a sort block and one
    across a block boundary; a parameter that never varies; an ordinary one: 10 400 keys = three sort blocks"""
    torch, dev = _torch()
    x = M.sort_case()
    ref = M.rank_diag(x)
    for layout, xd in (("steps", x), ("walkers", np.ascontiguousarray(x.transpose(1, 0, 2)))):
        out = _eng().rank_diag(torch.as_tensor(np.array(xd), device=dev), layout, M.PROBS, None, outputs=KEYS)
        _against_model(out, ref, "sort case, %s" % layout)
        assert np.all(out["stop"][2] == -1) and np.all(np.isnan(out["ess"][2])) and np.all(np.isnan(out["rhat"][2]))
        assert out["sd"][2] == 0.0 and out["median"][2] == 0.3 and np.all(out["rank2"][2] == x.shape[0] * x.shape[1] + 1)
    assert np.max(np.bincount(ref["rank2"][1])) == 5000


# ---------------------------------------------------------------------------- 2. bit equality
@pytest.mark.parametrize("shape", M.SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_layouts_on_device_outputs_alone_and_second_call(shape):
    eng = _eng()
    full = _full(shape)
    assert _same(eng.rank_diag(_dev_chain(shape), "steps", M.PROBS, None, outputs=KEYS), full)                     # a second call
    assert _same(eng.rank_diag(_dev_chain(shape, "walkers"), "walkers", M.PROBS, None, outputs=KEYS), full)        # the pickles' layout
    dev_out = eng.rank_diag(_dev_chain(shape), "steps", M.PROBS, None, on_device=True, outputs=KEYS)
    assert all(v.is_cuda for v in dev_out.values())
    assert _same({k: v.cpu().numpy() for k, v in dev_out.items()}, full)
    for k in KEYS:
        one = eng.rank_diag(_dev_chain(shape), "steps", M.PROBS, None, outputs=(k,))
        assert list(one) == [k] and _same(one, full, (k,))
    assert list(eng.rank_diag(_dev_chain(shape), "steps")) == list(KEYS[1:])                                      # the default: no rank2


@pytest.mark.parametrize("shape", M.SHAPES[2:], ids=lambda s: "%dx%dx%d" % s)
def test_a_parameter_alone_and_a_level_alone(shape):
    """d = 3 against each parameter alone: as a strided view of the same array (no copy) and as an array of its own; and the
    0.95 level alone against its column of the call with both levels"""
    eng = _eng()
    full = _full(shape)
    x = _dev_chain(shape)
    for j in range(shape[2]):
        for view in (x[:, :, j:j + 1], x[:, :, j:j + 1].contiguous()):
            one = eng.rank_diag(view, "steps", M.PROBS, None, outputs=KEYS)
            assert _same(one, {k: full[k][j:j + 1] for k in KEYS})
    one = eng.rank_diag(x, "steps", M.PROBS[1:], None, outputs=KEYS)
    assert _same(one, full, ("rank2", "median", "rhat", "sd"))
    assert np.array_equal(one["quant"][:, 0], full["quant"][:, 1])
    for k in ("ess", "stop"):
        assert np.array_equal(one[k], full[k][:, [0, 1, 3]])


def test_thinned_view_is_the_thinned_copy():
    eng = _eng()
    view = _dev_chain(M.SHAPES[-1])[100::3]
    assert not view.is_contiguous()
    a = eng.rank_diag(view, "steps", M.PROBS, None, outputs=KEYS)
    assert _same(a, eng.rank_diag(view.contiguous(), "steps", M.PROBS, None, outputs=KEYS))
    _against_model(a, M.rank_diag(M.mh_chain(*M.SHAPES[-1])[100::3]), "thinned view")


def test_parameter_groups():
    """the debug library takes a workspace cap (option key 53; the product library refuses it): one parameter per group against
    the single group of the default"""
    from conftest import debug_engine
    with pytest.raises(Exception):
        _eng().tune("rank_ws_bytes", 1000)
    dbg = debug_engine()
    dbg.tune("rank_ws_bytes", 1000)
    try:
        for shape in M.SHAPES[3:]:
            assert _same(dbg.rank_diag(_dev_chain(shape), "steps", M.PROBS, None, outputs=KEYS), _full(shape))
    finally:
        dbg.tune("rank_ws_bytes", 0)
    assert _same(dbg.rank_diag(_dev_chain(M.SHAPES[3]), "steps", M.PROBS, None, outputs=KEYS), _full(M.SHAPES[3]))


def test_mcmc_diag_and_predict_are_untouched():
    """a context with a factorised GP: predict and gpb_mcmc_diag, the rank diagnostics on the same context, both again — the
    same bits"""
    from gpbayestools_hic_amd import GPEngine
    X, Z = CV.make_data(100, 3, 3, 21)
    eng = GPEngine(0)
    eng.set_data(X, 0.3 * Z, "RBF", CV.ALPHA)
    eng.set_theta(CV.thetas_of(("mid", "hard", "aniso"), 3))
    eng.factor()
    Xs = np.random.default_rng(8).uniform(0.0, 1.0, (130, 3))
    shape = M.SHAPES[3]
    before = eng.predict(Xs, return_var=True)
    diag = eng.mcmc_diag(_dev_chain(shape), "steps", None, A.C)
    out = eng.rank_diag(_dev_chain(shape), "steps", M.PROBS, None, outputs=KEYS)
    assert _same(out, _full(shape))
    after = eng.predict(Xs, return_var=True)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    again = eng.mcmc_diag(_dev_chain(shape), "steps", None, A.C)
    assert all(np.array_equal(diag[k], again[k], equal_nan=True) for k in diag)


# ---------------------------------------------------------------------------- 3. errors
def test_argument_errors():
    from gpbayestools_hic_amd import _native as nat
    torch, dev = _torch()
    eng = _eng()
    n, nw, d = 20, 4, 3
    x = torch.zeros((n, nw, d), dtype=torch.float64, device=dev)
    sd = np.full(d, -7.0)
    big = 1 << 31

    def rc(n=n, nw=nw, d=d, ss=nw * d, ws=d, probs=(0.05, 0.95), nq=None, max_lag=None):
        p = np.array(probs, dtype=np.float64)
        return eng.lib.gpb_chain_rank_diag(eng.h, nat.ptr(x), n, nw, d, ss, ws, nat.ptr(p), len(p) if nq is None else nq,
                                           n // 2 - 1 if max_lag is None else max_lag, 0, None, None, None, None, None, None,
                                           nat.ptr(sd))

    assert rc() == 0 and np.all(sd == 0.0)                      # (the valid call: a chain of zeros never varies)
    sd[:] = -7.0
    # (arguments, what the message must name): every entry passes all the checks but the one it is listed under
    bad = [(dict(n=3, max_lag=0), "nsteps >= 4"),
           (dict(n=big, max_lag=0), "steps, walkers or parameters"), (dict(nw=big, ss=big * d), "steps, walkers or parameters"),
           (dict(d=big, ws=big, ss=nw * big), "steps, walkers or parameters"),
           (dict(nw=0), "nwalkers >= 1"), (dict(d=0), "d >= 1"),
           (dict(n=1 << 20, nw=1 << 11, ss=(1 << 11) * d, max_lag=0), "kept draws"),
           (dict(nq=0), "nq <= 8"), (dict(probs=(0.1,) * 9), "nq <= 8"),
           (dict(probs=(0.0, 0.5)), "level outside"), (dict(probs=(0.5, 1.0)), "level outside"), (dict(probs=(float("nan"),)), "level outside"),
           (dict(max_lag=-1), "max_lag outside"), (dict(max_lag=n // 2), "max_lag outside"),
           (dict(ws=d - 1), "stride below d"), (dict(ss=d - 1, ws=n * d), "stride below d"), (dict(ws=-d), "stride below d"),
           (dict(ss=nw * d - 1), "neither stride spans"), (dict(ss=d, ws=n * d - 1), "neither stride spans")]
    for kw, what in bad:
        assert rc(**kw) == E_ARG, kw
        msg = eng.lib.gpb_last_error(eng.h).decode()
        assert "gpb_chain_rank_diag" in msg and what in msg, (kw, msg)
    assert np.all(sd == -7.0)                                   # nothing was written
    assert rc(ss=d, ws=n * d) == 0                              # the other layout's strides are fine
    with pytest.raises(ValueError):
        eng.rank_diag(x, "rows")
    with pytest.raises(ValueError):
        eng.rank_diag(x.cpu(), "steps")
    with pytest.raises(ValueError):
        eng.rank_diag(x, "steps", outputs=("tau",))


# ---------------------------------------------------------------------------- 4. Python
@functools.lru_cache(maxsize=None)
def _sampler():
    """LoggingEnsembleSampler over a host Gaussian log-probability: 8 walkers, 2 parameters, 400 steps"""
    from gpbayestools_hic_amd import LoggingEnsembleSampler
    s = LoggingEnsembleSampler(8, 2, lambda X: -0.5 * np.sum((X / np.array([1.0, 3.0])) ** 2, axis=1), seed=11)
    s.run_mcmc(np.random.default_rng(2).standard_normal((8, 2)), 400)
    return s


def _check_python(r, x_steps, probs=M.PROBS):
    """a RankDiagnostics against the model of x_steps [n_t, n_w, n_d] (a device-made input: its margins are checked here)"""
    levels = list(probs) + [p for p in M.PROBS if p not in probs]
    ref = M.rank_diag(x_steps, levels)
    assert ref["margin"] >= M.MARGIN
    nq = len(probs)
    assert np.array_equal(r.median, ref["median"]) and np.array_equal(r.quantiles, ref["quant"][:, :nq])
    bar = 2.0 * (ref["stop"] + 2.0) * RHO_BAR
    tail = [2 + levels.index(p) for p in M.PROBS]
    for got, want, b in ((r.ess_bulk, ref["ess"][:, 0], bar[:, 0]), (r.ess_mean, ref["ess"][:, 1], bar[:, 1]),
                         (r.ess_tail, ref["ess"][:, tail].min(axis=1), bar[:, tail].max(axis=1))):
        assert np.all(np.abs(got - want) <= b * want)
    assert np.all(np.abs(r.ess_quantile - ref["ess"][:, 2:2 + nq]) <= bar[:, 2:2 + nq] * ref["ess"][:, 2:2 + nq])
    assert np.allclose(r.rhat_bulk, ref["rhat"][:, 0], rtol=MOM_BAR, atol=0) and np.allclose(r.rhat_folded, ref["rhat"][:, 1], rtol=MOM_BAR, atol=0)
    assert np.array_equal(r.rhat, np.maximum(r.rhat_bulk, r.rhat_folded))
    assert np.allclose(r.sd, ref["sd"], rtol=MOM_BAR, atol=0) and np.array_equal(r.mcse_mean, r.sd / np.sqrt(r.ess_mean))
    ok = (r.rhat < r.rhat_max) & (np.minimum(r.ess_bulk, r.ess_tail) >= r.min_ess)
    assert np.array_equal(r.converged_per_parameter, ok) and r.converged == bool(ok.all())


def test_rank_diagnose_and_the_sampler_accessor():
    from gpbayestools_hic_amd.diagnostics import rank_diagnose
    import gpbayestools_hic_amd.diagnostics as D
    s = _sampler()
    chain = s.chain.transpose(1, 0, 2)                                  # emcee's [nwalkers, nsteps, ndim] -> [n_t, n_w, n_d]
    r = rank_diagnose(chain)
    _check_python(r, chain)
    assert r.n_steps == 400 and r.n_walkers == 8 and r.n_draws == 3200 and "RankDiagnostics(" in repr(r) and "ess_tail" in repr(r)
    for discard, thin in ((0, 1), (100, 1), (50, 3)):
        d = s.rank_diagnostics(discard=discard, thin=thin)
        _check_python(d, chain[discard::thin])
        print("discard %d thin %d:\n%r" % (discard, thin, d))
    d = s.rank_diagnostics(discard=100, probs=(0.5,), min_ess=1e9)
    _check_python(d, chain[100:], probs=(0.5,))
    assert d.ess_quantile.shape == (2, 1) and not d.converged and "NO" in repr(d)
    assert s.rank_diagnostics(discard=100, min_ess=0, rhat_max=np.inf).converged is True
    # the starting band is a choice: a search that starts at 2 lags and doubles finds the same bits
    start, D.START_MAX_LAG = D.START_MAX_LAG, 2
    try:
        r2 = rank_diagnose(chain)
    finally:
        D.START_MAX_LAG = start
    for k in ("rhat", "ess_bulk", "ess_tail", "ess_mean", "ess_quantile", "sd", "median"):
        assert np.array_equal(getattr(r2, k), getattr(r, k)), k
    # and on the slowly mixing chain the search has to double beyond lag 64 and 128: the same bits as the full band at once
    long = np.array(M.long_chain())
    D.START_MAX_LAG = 40
    try:
        r3 = rank_diagnose(long)
    finally:
        D.START_MAX_LAG = start
    full = _long()
    assert np.array_equal(r3.ess_bulk, full["ess"][:, 0]) and np.array_equal(r3.ess_mean, full["ess"][:, 1])
    assert np.array_equal(r3.ess_quantile, full["ess"][:, 2:]) and np.array_equal(r3.ess_tail, full["ess"][:, 2:].min(axis=1))
    assert r3.thin == 1 and s.rank_diagnostics(discard=50, thin=3).thin == 3
    with pytest.raises(ValueError, match="weighted"):
        rank_diagnose(chain, weights=np.ones(400))
    with pytest.raises(ValueError, match="particle set"):
        rank_diagnose(chain[:, 0, :])
    with pytest.raises(ValueError):
        rank_diagnose(chain, probs=(0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7))   # with 0.05 and 0.95: nine levels


def test_chain_rank_convergence_is_sampler_rank_diagnostics(tmp_path):
    from gpbayestools_hic_amd import synth
    from gpbayestools_hic_amd.mcmc import Chain
    s = _sampler()
    d = s.rank_diagnostics(discard=100, thin=2)
    pf, ep = str(tmp_path / "par.txt"), str(tmp_path / "exp.pkl")
    synth.write_parameter_file(pf, -10.0 * np.ones(2), 10.0 * np.ones(2))
    with open(ep, "wb") as f:
        pickle.dump({"0": {"obs": np.array([[1.0], [0.1]])}}, f)
    ch = Chain(mcmc_path=str(tmp_path / "mcmc" / "c.pkl"), expdata_path=ep, model_parafile=pf)
    c = ch.rank_convergence(s.chain, discard=100, thin=2)                    # [nwalkers, nsteps, ndim], as the pickles hold it
    for k in ("rhat", "rhat_bulk", "rhat_folded", "ess_bulk", "ess_tail", "ess_mean", "ess_quantile", "mcse_mean", "median",
              "quantiles", "sd", "converged_per_parameter"):
        assert np.array_equal(getattr(c, k), getattr(d, k)), k
    assert c.names == list(ch.pardict) and c.n_steps == 150
    ch.chain = s.chain
    assert np.array_equal(ch.rank_convergence(discard=100, thin=2).ess_bulk, d.ess_bulk)
    with pytest.raises(ValueError, match="weighted"):
        ch.rank_convergence(s.chain, weights=np.ones(8))
    with pytest.raises(ValueError, match="particle set"):
        ch.rank_convergence(s.chain.reshape(-1, 2))
