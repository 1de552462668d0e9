"""GPU tier: convergence diagnostics of a resident chain — gpb_mcmc_diag (GPEngine.mcmc_diag), diagnostics.integrated_time,
StretchSampler.get_autocorr_time / diagnostics and Chain.convergence — against the host model of tests/acf_reference.py (emcee's
FFT form restated in numpy, split-R-hat in long double) on the AR(1) chains of that module, whose window decisions
tests/test_acf_reference.py shows to be at least 0.019 away from flipping.

Bars.  rho: absolute (rho is normalised to rho[0] = 1); the project's fp64 parity bar is 1e-10, the largest deviation measured on
an MI355X over the cases of sections 1 and 2 is 3.68e-15 (shape 300 x 6 x 3; the model's own FFT is within 8.3e-15 of long-double
direct sums there), four orders below it, so the bar is tightened to 16 x the measured value: RHO_BAR = 6e-14 (the stuck-walker
case added later measures 4.4e-15; the bar stays).  window: equal; tau:
2 (window + 1) RHO_BAR (measured at most 3.9e-14, shape 65 x 17 x 2, window 21); moments and R-hat: 1e-12 relative against the
long-double model (measured at most 8.0e-14 and 3.0e-14, shape 130 x 2 x 3).  Layouts, parameters alone, on_device, subsets of the
outputs, the band (max_lag) and a second call: bit equality.  Every case prints its figures with -s.  DESIGN.md section 18."""
import functools
import pickle

import numpy as np
import pytest

import acf_reference as R
import cv_reference as CV

pytestmark = pytest.mark.gpu

E_ARG = -1
RHO_BAR = 6e-14
MOM_BAR = 1e-12
KEYS = ("rho", "tau", "window", "moments", "rhat", "nconst")


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
    x = torch.as_tensor(np.array(R.ar1_chain(*shape)), device=dev)               # (a copy: the shared array is read-only)
    return x if layout == "steps" else x.permute(1, 0, 2).contiguous()


@functools.lru_cache(maxsize=None)
def _full(shape):
    """the device's answer at max_lag = nsteps - 1, steps layout, host outputs: computed once, compared by many"""
    return _eng().mcmc_diag(_dev_chain(shape), "steps", shape[0] - 1, R.C)


def _same(a, b, keys=KEYS):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True) for k in keys)


def _against_model(out, ref, label):
    err_rho = float(np.max(np.abs(out["rho"] - ref["rho"])))
    win = out["window"].astype(np.int64)
    w = win & ~R.NO_WINDOW
    err_tau = np.abs(out["tau"] - ref["tau"])
    mom = np.asarray(ref["moments"], dtype=np.float64)
    err_mom = float(np.max(np.abs(out["moments"] - ref["moments"]) / np.abs(ref["moments"])))
    err_rhat = float(np.max(np.abs(out["rhat"] - ref["rhat"]) / np.abs(ref["rhat"])))
    print("%s: rho %.3g, tau %.3g (window %s), moments %.3g rel, rhat %.3g rel" % (label, err_rho, err_tau.max(), list(win), err_mom,
                                                                                 err_rhat))
    assert mom.shape == out["moments"].shape
    assert err_rho <= RHO_BAR
    assert np.array_equal(win, ref["window"])
    assert np.all(err_tau <= 2.0 * (w + 1) * RHO_BAR)
    assert err_mom <= MOM_BAR and err_rhat <= MOM_BAR
    assert np.array_equal(out["nconst"], ref["nconst"])


# ---------------------------------------------------------------------------- 1. against the host model
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_diag_matches_the_model(shape):
    out = _full(shape)
    assert out["rho"].shape == (shape[2], shape[0]) and out["window"].dtype == np.int32
    _against_model(out, R.reference(*shape), "shape %s" % (shape,))


@pytest.mark.parametrize("max_lag", R.BAND_LAGS)
def test_band_edges(max_lag):
    """700 steps = 11 block rows; max_lag 0, 63 (block diagonals 0 and 1), 64, 65, 127 (0 .. 2), 699 (all): against the model, and the
    leading lags bit for bit those of the full band; tau / window too whenever the window is inside the smaller band"""
    shape = R.SHAPES[-1]
    out = _eng().mcmc_diag(_dev_chain(shape), "steps", max_lag, R.C)
    _against_model(out, R.reference(*shape, max_lag=max_lag), "max_lag %d" % max_lag)
    full = _full(shape)
    assert np.array_equal(out["rho"], full["rho"][:, :max_lag + 1])
    assert _same(out, full, ("moments", "rhat", "nconst"))
    for j in range(shape[2]):
        if full["window"][j] <= max_lag:
            assert out["window"][j] == full["window"][j] and out["tau"][j] == full["tau"][j]
        else:
            assert out["window"][j] == (max_lag | R.NO_WINDOW)


def test_no_window_inside_max_lag():
    """parameter 1 (tau ~ 9) has no window within 5 lags: the flag bit is set and tau = taus[max_lag], which is the sequential scan
    of the device's own rho, bit for bit"""
    shape = R.SHAPES[3]
    out = _eng().mcmc_diag(_dev_chain(shape), "steps", 5, R.C)
    assert out["window"][1] == (5 | R.NO_WINDOW) == (5 | _eng().DIAG_NO_WINDOW)
    taus = 2.0 * np.cumsum(out["rho"], axis=1) - 1.0
    for j in range(shape[2]):
        w = int(out["window"][j]) & ~R.NO_WINDOW
        assert out["tau"][j] == taus[j, w]
        assert np.all(np.arange(w) < R.C * taus[j, :w])                      # no earlier lag qualified
        assert (w >= R.C * taus[j, w]) == (out["window"][j] < R.NO_WINDOW)
    _against_model(out, R.reference(*shape, max_lag=5), "max_lag 5")


# ---------------------------------------------------------------------------- 2. bit equality
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_layouts_on_device_and_second_call(shape):
    eng = _eng()
    full = _full(shape)
    L = shape[0] - 1
    assert _same(eng.mcmc_diag(_dev_chain(shape), "steps", L, R.C), full)                        # a second call
    assert _same(eng.mcmc_diag(_dev_chain(shape, "walkers"), "walkers", L, R.C), full)           # the pickles' layout
    dev_out = eng.mcmc_diag(_dev_chain(shape), "steps", L, R.C, on_device=True)
    assert all(v.is_cuda for v in dev_out.values())
    assert _same({k: v.cpu().numpy() for k, v in dev_out.items()}, full)
    for k in KEYS:
        one = eng.mcmc_diag(_dev_chain(shape), "steps", L, R.C, outputs=(k,))
        assert list(one) == [k] and _same(one, full, (k,))


@pytest.mark.parametrize("shape", R.SHAPES[2:], ids=lambda s: "%dx%dx%d" % s)
def test_a_parameter_alone(shape):
    """d = 3 against each parameter alone: as a strided view of the same array (no copy) and as an array of its own"""
    eng = _eng()
    full = _full(shape)
    x = _dev_chain(shape)
    for j in range(shape[2]):
        for view in (x[:, :, j:j + 1], x[:, :, j:j + 1].contiguous()):
            one = eng.mcmc_diag(view, "steps", shape[0] - 1, R.C)
            assert _same(one, {k: full[k][j:j + 1] for k in KEYS})


def test_thinned_view_is_the_thinned_copy():
    """chain[discard::thin] through its strides against a contiguous copy of the same draws"""
    eng = _eng()
    x = _dev_chain(R.SHAPES[-1])
    view = x[100::3]
    assert not view.is_contiguous()
    a = eng.mcmc_diag(view, "steps", None, R.C)
    assert _same(a, eng.mcmc_diag(view.contiguous(), "steps", None, R.C))
    thinned = R.ar1_chain(*R.SHAPES[-1])[100::3]
    ref = R.integrated_time(thinned, R.C)
    ref["moments"], ref["rhat"] = R.split_rhat(thinned)
    assert min(R.window_margin(ref["taus"][j], ref["window"][j] & ~R.NO_WINDOW, R.C) for j in range(3)) > 1e-6
    _against_model(a, ref, "thinned view")


# ---------------------------------------------------------------------------- 3. edge cases
def test_constant_walkers():
    torch, dev = _torch()
    eng = _eng()
    shape = R.SHAPES[3]
    x = np.array(R.ar1_chain(*shape))
    x[:, 2, 0] = 0.25
    out = eng.mcmc_diag(torch.as_tensor(x, device=dev), "steps", None, R.C)
    ref = R.integrated_time(x, R.C)
    ref["moments"], ref["rhat"] = R.split_rhat(x)
    assert list(out["nconst"]) == [1, 0, 0]
    _against_model(out, ref, "one constant walker")
    for k in ("rho", "tau", "window"):                                          # the other parameters: untouched
        assert np.array_equal(out[k][1:], _full(shape)[k][1:])
    x[:, :, 0] = 0.25
    out = eng.mcmc_diag(torch.as_tensor(x, device=dev), "steps", None, R.C)
    assert out["nconst"][0] == shape[1] and out["window"][0] == -1
    assert np.isnan(out["rho"][0]).all() and np.isnan(out["tau"][0]) and np.isnan(out["rhat"][0])
    assert out["moments"][0, 0] == 0.25 and out["moments"][0, 1] == 0.0 and out["moments"][0, 2] == 0.0
    for k in KEYS:
        assert np.array_equal(out[k][1:], _full(shape)[k][1:])


def _kahan_mean(v, n):
    """the mean of n copies of v as a compensated sum in sequence computes it (IEEE doubles: Python floats)"""
    s = c = 0.0
    for _ in range(n):
        y = v - c
        t = s + y
        c = (t - s) - y
        s = t
    return s / n


@pytest.mark.parametrize("shape", R.SHAPES[3:], ids=lambda s: "%dx%dx%d" % s)
def test_stuck_walkers_at_arbitrary_values(shape):
    """walkers stuck at values whose rounded mean is not the value (standard normal draws, parameter 1: 1e3 + one, kept when the
    compensated sequential mean over n copies differs from the value): every one is left out and counted, as the model — which
    compares the values — does; n = 300 and 700"""
    torch, dev = _torch()
    n, nw, d = shape
    x = np.array(R.ar1_chain(*shape))
    rng = np.random.default_rng(17)

    def inexact_value(offset):
        """a draw whose compensated sequential mean over n steps is NOT the value: centred on that mean the series has c0 > 0"""
        while True:
            v = rng.standard_normal() + offset
            if _kahan_mean(v, n) != v:
                return v
    stuck = {0: [0, 3], 1: [1, 2, 4], 2: [5]}
    for j, ws in stuck.items():
        for w in ws:
            x[:, w, j] = inexact_value(1e3 if j == 1 else 0.0)
    ref = R.integrated_time(x, R.C)
    ref["moments"], ref["rhat"] = R.split_rhat(x)
    assert list(ref["nconst"]) == [2, 3, 1]
    assert min(R.window_margin(ref["taus"][j], ref["window"][j] & ~R.NO_WINDOW, R.C) for j in range(d)) > 1e-6
    for layout, xd in (("steps", x), ("walkers", np.ascontiguousarray(x.transpose(1, 0, 2)))):
        out = _eng().mcmc_diag(torch.as_tensor(xd, device=dev), layout, None, R.C)
        assert list(out["nconst"]) == [2, 3, 1]
        _against_model(out, ref, "stuck walkers, %s" % layout)
    # the same parameter without its stuck walkers: the same bits when the padded walker count is the same
    keep = [w for w in range(nw) if w not in stuck[2]]
    if (len(keep) + 15) // 16 == (nw + 15) // 16:
        rest = _eng().mcmc_diag(torch.as_tensor(np.ascontiguousarray(x[:, keep, 2:3]), device=dev), "steps", None, R.C)
        assert rest["tau"][0] == out["tau"][2] and rest["window"][0] == out["window"][2]


def test_argument_errors():
    from gpbayestools_hic_amd import _native as nat
    torch, dev = _torch()
    eng = _eng()
    n, nw, d = 20, 4, 3
    x = torch.zeros((n, nw, d), dtype=torch.float64, device=dev)
    tau = np.full(d, -7.0)
    big = 1 << 31

    def rc(n=n, nw=nw, d=d, ss=nw * d, ws=d, max_lag=n - 1, c=5.0):
        return eng.lib.gpb_mcmc_diag(eng.h, nat.ptr(x), n, nw, d, ss, ws, max_lag, c, 0, None, nat.ptr(tau), None, None, None, None)

    assert rc() == 0 and np.all(np.isnan(tau))               # (the valid call: a chain of zeros never moved)
    tau[:] = -7.0
    # (arguments, what the message must name): every entry passes all the checks but the one it is listed under
    bad = [(dict(n=3, max_lag=2), "nsteps >= 4"),
           (dict(n=big), "2^31 - 1"), (dict(nw=big, ss=big * d), "2^31 - 1"), (dict(d=big, ws=big, ss=nw * big), "2^31 - 1"),
           (dict(nw=0), "nwalkers >= 1"), (dict(d=0), "d >= 1"),
           (dict(max_lag=-1), "max_lag outside"), (dict(max_lag=n), "max_lag outside"),
           (dict(c=0.0), "c must be"), (dict(c=-1.0), "c must be"), (dict(c=float("inf")), "c must be"), (dict(c=float("nan")), "c must be"),
           (dict(ws=d - 1), "stride below d"), (dict(ss=d - 1, ws=n * d), "stride below d"), (dict(ws=-d), "stride below d"),
           (dict(ss=-nw * d), "stride below d"),
           (dict(ss=nw * d - 1), "neither stride spans"), (dict(ss=d, ws=n * d - 1), "neither stride spans")]
    for kw, what in bad:
        assert rc(**kw) == E_ARG, kw
        msg = eng.lib.gpb_last_error(eng.h).decode()
        assert "gpb_mcmc_diag" in msg and what in msg, (kw, msg)
    assert np.all(tau == -7.0)                                 # nothing was written
    assert rc(ss=d, ws=n * d) == 0                            # the other layout's strides are fine
    with pytest.raises(ValueError):
        eng.mcmc_diag(x, "rows")
    with pytest.raises(ValueError):
        eng.mcmc_diag(x.cpu(), "steps")
    with pytest.raises(ValueError):
        eng.mcmc_diag(x.permute(0, 2, 1), "steps")             # the parameters must have unit stride


def test_predict_is_untouched():
    """a context with a factorised GP: predict, diagnostics on the same context, predict again — the same bits"""
    from gpbayestools_hic_amd import GPEngine
    X, Z = CV.make_data(100, 3, 3, 21)
    eng = GPEngine(0)
    eng.set_data(X, 0.3 * Z, "RBF", CV.ALPHA)
    eng.set_theta(CV.thetas_of(("mid", "hard", "aniso"), 3))
    eng.factor()
    Xs = np.random.default_rng(8).uniform(0.0, 1.0, (130, 3))
    before = eng.predict(Xs, return_var=True)
    out = eng.mcmc_diag(_dev_chain(R.SHAPES[3]), "steps", None, R.C)
    assert _same(out, _full(R.SHAPES[3]))
    after = eng.predict(Xs, return_var=True)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))


# ---------------------------------------------------------------------------- 4. Python
def test_integrated_time_shape_rules():
    from gpbayestools_hic_amd.diagnostics import integrated_time
    torch, dev = _torch()
    shape = R.SHAPES[3]
    x = R.ar1_chain(*shape)
    full = _full(shape)
    assert np.array_equal(integrated_time(x, quiet=True), full["tau"])                                   # [n_t, n_w, n_d]
    assert np.array_equal(integrated_time(_dev_chain(shape), quiet=True), full["tau"])                   # a device tensor
    assert np.array_equal(integrated_time(x[:, :, 0], quiet=True), full["tau"][:1])                      # [n_t, n_w]
    one = integrated_time(x[:, 0, :], quiet=True, has_walkers=False)                                     # [n_t, n_d]
    assert one.shape == (3,)
    assert np.array_equal(integrated_time(x[:, 0, 0], quiet=True), one[:1])                              # [n_t]
    assert np.array_equal(integrated_time(x[:, :1, 0], quiet=True), one[:1])
    with pytest.raises(ValueError):
        integrated_time(np.zeros((8, 2, 2, 2)))
    # the starting band is a choice: a search that starts at 8 lags and doubles finds the same bits
    import gpbayestools_hic_amd.diagnostics as D
    start, D.START_MAX_LAG = D.START_MAX_LAG, 8
    try:
        assert np.array_equal(integrated_time(x, quiet=True), full["tau"])
    finally:
        D.START_MAX_LAG = start


@functools.lru_cache(maxsize=None)
def _sampler():
    """LoggingEnsembleSampler over a host Gaussian log-probability: 8 walkers, 2 parameters, 400 steps"""
    from gpbayestools_hic_amd import LoggingEnsembleSampler
    s = LoggingEnsembleSampler(8, 2, lambda X: -0.5 * np.sum((X / np.array([1.0, 3.0])) ** 2, axis=1), seed=11)
    s.run_mcmc(np.random.default_rng(2).standard_normal((8, 2)), 400)
    return s


def _model_tau(x_steps, c=R.C):
    """model tau of a [n_t, n_w, n_d] array, with the margin check of tests/test_acf_reference.py for this (device-made) input"""
    ref = R.integrated_time(x_steps, c)
    for j in range(x_steps.shape[2]):
        assert R.window_margin(ref["taus"][j], int(ref["window"][j]) & ~R.NO_WINDOW, c) > 1e-6
    return ref


def test_sampler_get_autocorr_time():
    from gpbayestools_hic_amd.diagnostics import AutocorrError
    s = _sampler()
    chain = s.chain.transpose(1, 0, 2)                                  # emcee's [nwalkers, nsteps, ndim] -> [n_t, n_w, n_d]
    for discard, thin in ((0, 1), (100, 1), (0, 2), (50, 3)):
        ref = _model_tau(chain[discard::thin])
        tau = s.get_autocorr_time(discard=discard, thin=thin, quiet=True)
        w = ref["window"] & ~R.NO_WINDOW
        print("discard %d thin %d: tau %s, model %s, window %s" % (discard, thin, tau, thin * ref["tau"], list(w)))
        assert np.all(np.abs(tau - thin * ref["tau"]) <= thin * 2.0 * (w + 1) * RHO_BAR)
    tau = s.get_autocorr_time(quiet=True)
    tol = 2.0 * 400 / tau.min()                                         # tol tau > n for every parameter ...
    with pytest.raises(AutocorrError) as e:
        s.get_autocorr_time(tol=tol)
    assert np.array_equal(e.value.tau, tau)
    assert np.array_equal(s.get_autocorr_time(tol=tol, quiet=True), tau)
    assert np.array_equal(s.get_autocorr_time(tol=0), tau)              # ... and tol tau <= n with tol = 0: no error


def test_chain_convergence_is_sampler_diagnostics(tmp_path):
    from gpbayestools_hic_amd import synth
    from gpbayestools_hic_amd.mcmc import Chain
    s = _sampler()
    d = s.diagnostics(discard=100, tol=1e6)
    assert not d.converged and d.n_steps == 300 and d.n_walkers == 8 and "NO" in repr(d)
    assert np.array_equal(d.tau, s.get_autocorr_time(discard=100, quiet=True))
    assert np.allclose(d.ess, 300 * 8 / d.tau) and np.allclose(d.mcse, d.std / np.sqrt(d.ess))
    flat = s.chain[:, 100:].reshape(-1, 2)
    assert np.allclose(d.mean, flat.mean(axis=0), rtol=1e-12, atol=1e-14) and np.allclose(d.std, flat.std(axis=0), rtol=0.05)
    pf, ep = str(tmp_path / "par.txt"), str(tmp_path / "exp.pkl")
    synth.write_parameter_file(pf, -10.0 * np.ones(2), 10.0 * np.ones(2))
    with open(ep, "wb") as f:
        pickle.dump({"0": {"obs": np.array([[1.0], [0.1]])}}, f)
    ch = Chain(mcmc_path=str(tmp_path / "mcmc" / "c.pkl"), expdata_path=ep, model_parafile=pf)
    c = ch.convergence(s.chain, discard=100, tol=1e6)                        # [nwalkers, nsteps, ndim], as the pickles hold it
    for k in ("tau", "window", "ess", "rhat", "mean", "std", "mcse", "n_constant_walkers", "converged_per_parameter"):
        assert np.array_equal(getattr(c, k), getattr(d, k)), k
    assert c.converged is False and c.names == list(ch.pardict)
    ch.chain = s.chain
    assert np.array_equal(ch.convergence(discard=100).tau, d.tau) and s.diagnostics(tol=0).converged is True
    assert ch.convergence(tol=0).converged is True
    d2 = s.diagnostics(discard=100, thin=2)
    assert d2.n_steps == 150 and np.array_equal(d2.tau, s.get_autocorr_time(discard=100, thin=2, quiet=True))
