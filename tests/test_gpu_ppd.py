"""GPU tier: posterior-predictive summaries of a whole chain on the device — gpb_emu_predict_diag (GPEngine.emu_predict_diag,
Emulator.predict_diag), gpb_ppd_summary (GPEngine.ppd_summary) and Chain.posterior_predictive — against the host model of
tests/ppd_reference.py (np.sort, math.fsum of 0.5 erfc, the restated 64-halving search).

Bars.  Diagonal predict and order statistics: bit equality.  Moments: (ceil(log2 S) + 4) 2^-53 E|term|.  Mixture quantiles and
PIT: on the model's exact CDF at the device's answer, |F_fsum(y_dev) - q| <= k 2^-53 + f 2^-52 max(|a0|, |b0|, b0 - a0)
(ppd_reference.cdf_bar); every case keeps the second term below 1e-9.  The third moment's summand is taken around the DEVICE's
first moment (which has its own bar): around the model's, a row of one repeated value c would be held to ~1e-16 of
(c - fl(fl(S c) / S))^2, a quantity that is itself rounding noise of the mean.  The "wide" rows (1e-300 .. 1e300) have no
representable third moment: the model gives +inf there and the device must too.

Measured on an MI355X, largest ratio to the bar over all cases here: moments 0.162 (half-tied row, S = 256; chain rows 0.155);
mixture quantiles 0.097 (the S = 1 case; chain 0.034); PIT < 0.0005 (chain 0.008).  DESIGN.md section 17."""
import functools

import numpy as np
import pytest
from scipy.special import ndtri

import cv_reference as CV
import ppd_reference as R

pytestmark = pytest.mark.gpu

E_ARG = -1


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _util():
    from gpbayestools_hic_amd import GPEngine
    return GPEngine(0)


def _padded(rows, pad=7):
    """the [M, S] host rows as a device view [:, :S] of an [M, S + pad] array whose padding is NaN"""
    torch, dev = _torch()
    M, S = rows.shape
    full = np.full((M, S + pad), np.nan)
    full[:, :S] = rows
    return torch.as_tensor(full, device=dev)[:, :S]


# ---------------------------------------------------------------------------- 1. diagonal predict
MODES = {"pca": 0, "no_pca": 1, "expdiag": 2, "no_pca_expdiag": 3}
W_DIAG = 130


@functools.lru_cache(maxsize=None)
def _diag_engine(mode, arithmetic):
    """N = 100, d = 3; PCA modes P = 3, M = 5, no-PCA modes P = M = 5"""
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
    if arithmetic == "fp64":
        eng.tune("predict_sliced", 0)
    return eng, M


def _diag_inputs():
    from gpbayestools_hic_amd import synth
    return synth.walkers(W_DIAG, 3, seed=8), np.random.default_rng(9).uniform(0.0, 0.3, W_DIAG)


@pytest.mark.parametrize("arithmetic", ["fp64", "default"])
@pytest.mark.parametrize("with_extra", [False, True])
@pytest.mark.parametrize("mode", list(MODES))
def test_predict_diag_is_emu_predict(mode, with_extra, arithmetic):
    """W = 130 (two 64-walker tiles, the second ragged): mean_T[m][w] == emu_predict's mean[w][m], var_T[m][w] == its cov[w][m][m],
    host path and device path; two slabs (70 + 60) into one NaN-filled [M, 200] pair equal the single call, the columns behind
    stay NaN"""
    torch, dev = _torch()
    eng, M = _diag_engine(mode, arithmetic)
    Xs, es = _diag_inputs()
    es = es if with_extra else None
    mean, cov = eng.emu_predict(Xs, return_cov=True, extra_std=es)
    want_v = np.ascontiguousarray(np.diagonal(cov, axis1=1, axis2=2).T)
    m_T, v_T = eng.emu_predict_diag(Xs, extra_std=es)
    assert m_T.shape == (M, W_DIAG) and np.array_equal(m_T, mean.T) and np.array_equal(v_T, want_v)
    Xd = torch.as_tensor(Xs, device=dev)
    esd = None if es is None else torch.as_tensor(es, device=dev)
    m_d, v_d = eng.emu_predict_diag(Xd, extra_std=esd)
    assert np.array_equal(m_d.cpu().numpy(), mean.T) and np.array_equal(v_d.cpu().numpy(), want_v)
    big_m = torch.full((M, 200), float("nan"), dtype=torch.float64, device=dev)
    big_v = torch.full((M, 200), float("nan"), dtype=torch.float64, device=dev)
    for i0, i1 in ((0, 70), (70, 130)):
        eng.emu_predict_diag(Xd[i0:i1], extra_std=None if esd is None else esd[i0:i1], out=(big_m[:, i0:i1], big_v[:, i0:i1]))
    bm, bv = big_m.cpu().numpy(), big_v.cpu().numpy()
    assert np.array_equal(bm[:, :130], mean.T) and np.array_equal(bv[:, :130], want_v)
    assert np.isnan(bm[:, 130:]).all() and np.isnan(bv[:, 130:]).all()


def test_predict_diag_refuses_a_short_leading_dimension():
    from gpbayestools_hic_amd import _native as nat
    eng, M = _diag_engine("pca", "default")
    Xs, _ = _diag_inputs()
    m, v = np.zeros((M, W_DIAG)), np.zeros((M, W_DIAG))
    rc = eng.lib.gpb_emu_predict_diag(eng.h, nat.ptr(nat.f64(Xs)), W_DIAG, 0, None, nat.ptr(m), nat.ptr(v), W_DIAG - 1)
    assert rc == E_ARG and not m.any() and not v.any()
    torch, dev = _torch()
    with pytest.raises(ValueError):
        eng.emu_predict_diag(torch.as_tensor(Xs, device=dev), out=(torch.empty((M, 100), dtype=torch.float64, device=dev),) * 2)


# ---------------------------------------------------------------------------- 2. order statistics, 3. moments
@functools.lru_cache(maxsize=None)
def _order_case(kind, S):
    rows = R.make_rows(kind, S)
    var = np.abs(R.make_rows("normal", S, seed=3))
    eng = _util()
    mu_d, var_d = _padded(rows), _padded(var)
    out = {q: eng.ppd_summary(mu_d, var_d, q, outputs=("moments", "order")) for q in (R.LEVELS_ORDER, R.LEVELS_16)}
    return rows, var, out


@pytest.mark.parametrize("S", R.ORDER_SIZES)
@pytest.mark.parametrize("kind", R.ROW_KINDS)
def test_order_statistics_are_exact(kind, S):
    """M = 3, ld = S + 7 (NaN padding): mu_(k) and mu_(min(k + 1, S - 1)) equal np.sort(row)[k], [k + 1], five levels and sixteen"""
    rows, _, out = _order_case(kind, S)
    for q, res in out.items():
        assert res["order"].shape == (3, len(q), 2)
        for m in range(3):
            assert np.array_equal(res["order"][m], R.order_stats(rows[m], q)), (kind, S, m)


@pytest.mark.parametrize("S", R.ORDER_SIZES)
@pytest.mark.parametrize("kind", R.ROW_KINDS)
def test_moments(kind, S):
    """|device - fsum model| <= (ceil(log2 S) + 4) 2^-53 E|term| for E mu, E sigma^2 and E (mu - E mu)^2"""
    rows, var, out = _order_case(kind, S)
    mom = out[R.LEVELS_ORDER]["moments"]
    assert np.array_equal(mom, out[R.LEVELS_16]["moments"])
    worst = 0.0
    for m in range(3):
        m1, ev, pv = R.moments(rows[m], var[m], mean=mom[m, 0])
        with np.errstate(over="ignore"):
            terms = (rows[m], var[m], (rows[m] - mom[m, 0]) ** 2)
        for got, want, t in zip(mom[m], (m1, ev, pv), terms):
            if np.isinf(want):
                assert got == want, (kind, S, m)
                continue
            bar = R.moment_bar(S, t)
            assert abs(got - want) <= bar, (kind, S, m, got, want, bar)
            if bar > 0.0:
                worst = max(worst, abs(got - want) / bar)
    print("moments %s S=%d: largest |device - model| / bar = %.3f" % (kind, S, worst))


# ---------------------------------------------------------------------------- 4. mixture quantiles and PIT
def _mix_vadd(var):
    return 0.5 * float(np.median(var))


@functools.lru_cache(maxsize=None)
def _mix_case(name, with_vadd):
    mu, var = R.make_mix(name)
    vadd = _mix_vadd(var) if with_vadd else None
    yobs = float(np.quantile(mu, 0.7))
    rows = np.stack([mu, mu[::-1], mu])            # M = 3: rows 0 and 2 equal, row 1 the same samples in another order
    vrows = np.stack([var, var[::-1], var])
    res = _util().ppd_summary(_padded(rows), _padded(vrows), R.LEVELS_MIX, vadd=None if vadd is None else np.full(3, vadd),
                              yobs=np.full(3, yobs), outputs=("mixq", "pit"))
    return mu, var, vadd, yobs, res


@pytest.mark.parametrize("with_vadd", [False, True])
@pytest.mark.parametrize("name", list(R.MIX_CASES))
def test_mixture_quantiles_and_pit(name, with_vadd):
    """the model's exact CDF at the device's quantile is q within the bar; the PIT is the model's CDF at yobs within the bar"""
    mu, var, vadd, yobs, res = _mix_case(name, with_vadd)
    S = mu.shape[0]
    tau = R.tau_of(var, vadd, S)
    bar, second = R.cdf_bar(mu, tau)
    assert second <= 1e-9, (name, second)
    worst = 0.0
    for i, q in enumerate(R.LEVELS_MIX):
        y = res["mixq"][0, i]
        assert np.isfinite(y)
        err = abs(R.mix_cdf(y, mu, tau) - q)
        worst = max(worst, err / bar)
        assert err <= bar, (name, q, y, err, bar)
    perr = abs(res["pit"][0] - R.mix_cdf(yobs, mu, tau))
    print("mixture %s vadd=%s: largest |F(y_dev) - q| / bar = %.3f, PIT |dev - model| / bar = %.3f (bar %.2e, second term %.2e)"
          % (name, with_vadd, worst, perr / bar, bar, second))
    assert perr <= bar, (name, perr, bar)
    assert np.array_equal(res["mixq"][0], res["mixq"][2]) and res["pit"][0] == res["pit"][2]
    if S == 1:
        for i, q in enumerate(R.LEVELS_MIX):
            want = mu[0] + tau[0] * ndtri(q)
            assert abs(res["mixq"][0, i] - want) <= 1e-14 * abs(want), (q, res["mixq"][0, i], want)


def test_mixture_edges():
    """q = 0 gives -inf and q = 1 +inf; a row with some tau_s = 0 gives finite answers inside the bracket"""
    mu, var = R.make_mix("thousand")
    var = var.copy()
    var[::3] = 0.0
    res = _util().ppd_summary(_padded(mu[None, :]), _padded(var[None, :]), (0.0, 0.16, 0.5, 0.84, 1.0), yobs=np.array([0.1]),
                              outputs=("mixq", "pit"))
    y = res["mixq"][0]
    assert y[0] == -np.inf and y[4] == np.inf and np.isfinite(y[1:4]).all() and np.all(np.diff(y[1:4]) > 0)
    tau = R.tau_of(var, None, mu.shape[0])
    a0, b0 = R.bracket(mu, tau)
    assert a0 < y[1] and y[3] < b0
    # the mixture jumps by 1/S = 1e-3 at every step: F just below y is at most q and F at y at least q (1e-12: far above the
    # rounding of F, far below a jump)
    for yi, q in zip(y[1:4], (0.16, 0.5, 0.84)):
        assert R.mix_cdf(np.nextafter(yi, -np.inf), mu, tau) <= q + 1e-12 and R.mix_cdf(yi, mu, tau) >= q - 1e-12
    assert abs(res["pit"][0] - R.mix_cdf(0.1, mu, tau)) <= (32 + R.clog2(mu.shape[0])) * R.U53       # the bar's first term
    # all tau = 0: the empirical distribution of the means
    res0 = _util().ppd_summary(_padded(mu[None, :]), None, (0.5,), vadd=np.zeros(1), yobs=np.array([0.1]), outputs=("mixq", "pit"))
    assert np.isfinite(res0["mixq"][0, 0]) and res0["pit"][0] == np.count_nonzero(mu <= 0.1) / mu.shape[0]


# ---------------------------------------------------------------------------- 5. properties
def test_rows_calls_and_outputs_do_not_change_the_bits():
    torch, dev = _torch()
    eng = _util()
    S = 257
    rows = np.stack([R.make_rows("normal", S)[0], R.make_mix("narrow_tau")[0], R.make_rows("half_tied", S)[1]])
    var = np.abs(R.make_rows("normal", S, seed=5)) * 0.1
    vadd, yobs, q = np.array([0.01, 0.0, 0.3]), np.array([0.2, -0.1, 0.0]), R.LEVELS_MIX
    mu_d, var_d = _padded(rows), _padded(var)
    full = eng.ppd_summary(mu_d, var_d, q, vadd=vadd, yobs=yobs)
    assert sorted(full) == ["mixq", "moments", "order", "pit"]
    again = eng.ppd_summary(mu_d, var_d, q, vadd=vadd, yobs=yobs)
    dev_out = eng.ppd_summary(mu_d, var_d, q, vadd=vadd, yobs=yobs, on_device=True)
    for k in full:
        assert np.array_equal(full[k], again[k]), k                        # two calls
        assert np.array_equal(full[k], dev_out[k].cpu().numpy()), k        # host outputs == device outputs
        one = eng.ppd_summary(mu_d, var_d, q, vadd=vadd, yobs=yobs, outputs=(k,))
        assert list(one) == [k] and np.array_equal(one[k], full[k]), k     # one output alone
    for m in range(3):                                                     # a row alone (M = 1, contiguous: another ld)
        alone = eng.ppd_summary(torch.as_tensor(rows[m:m + 1], device=dev), torch.as_tensor(var[m:m + 1], device=dev), q,
                                vadd=vadd[m:m + 1], yobs=yobs[m:m + 1])
        for k in full:
            assert np.array_equal(alone[k][0], full[k][m]), (k, m)
    # what is returned follows what was given
    assert sorted(eng.ppd_summary(mu_d, None, q)) == ["moments", "order"]
    assert sorted(eng.ppd_summary(mu_d, var_d, q)) == ["mixq", "moments", "order"]
    assert np.array_equal(eng.ppd_summary(mu_d, None, q)["moments"][:, 1], np.zeros(3))


def test_bad_arguments_are_refused():
    from gpbayestools_hic_amd._native import GPBError
    eng = _util()
    rows = R.make_rows("normal", 50)
    mu_d = _padded(rows)
    var_d = _padded(np.abs(rows))
    ok = (0.1, 0.9)
    for q in ((), tuple(np.linspace(0.1, 0.9, 17)), (-0.1, 0.5), (0.5, 1.5), (float("nan"),)):
        with pytest.raises(GPBError, match="code -1"):
            eng.ppd_summary(mu_d, var_d, q)
    for q in ((1e-16, 0.5), (0.5, float(np.nextafter(1.0, 0.0)))):
        with pytest.raises(GPBError, match="code -1"):
            eng.ppd_summary(mu_d, var_d, q)
        assert sorted(eng.ppd_summary(mu_d, var_d, q, outputs=("moments", "order"))) == ["moments", "order"]
    with pytest.raises(GPBError, match="code -1"):
        eng.ppd_summary(mu_d, None, ok, outputs=("mixq",))                 # mixq with neither var_T nor vadd
    with pytest.raises(GPBError, match="code -1"):
        eng.ppd_summary(mu_d, var_d, ok, outputs=("pit",))                 # pit without yobs
    with pytest.raises(GPBError, match="code -1"):
        eng.ppd_summary(mu_d, var_d, ok, S=0)
    with pytest.raises(ValueError):
        eng.ppd_summary(mu_d, var_d, ok, S=51)                             # more samples than columns
    with pytest.raises(GPBError, match="code -1"):
        eng.ppd_summary(mu_d[:0], None, ok)                                # M < 1


# ---------------------------------------------------------------------------- 6. Chain.posterior_predictive
SPECS = [(100, 5, 3, "RBF"), (130, 4, 2, "Matern25")]


@functools.lru_cache(maxsize=None)
def _chain(mapped):
    import tempfile
    from gpbayestools_hic_amd import synth, workload
    chain, emus, info = workload.build_multi_chain(SPECS, 20, workdir=tempfile.mkdtemp(prefix="gpb_ppd_"), mapped=mapped)
    X = synth.walkers(300, 20, seed=31)
    mean, cov = chain._predict(X)
    return chain, X, mean, np.ascontiguousarray(np.diagonal(cov, axis1=1, axis2=2))


@pytest.mark.parametrize("mapped", [False, True])
def test_chain_posterior_predictive(mapped):
    chain, X, mean, var = _chain(mapped)
    S, nobs = X.shape[0], 9
    assert chain.nobs == nobs
    engs, mu_T, var_T = chain._ppd_arrays(X)
    assert np.array_equal(mu_T.cpu().numpy(), mean.T) and np.array_equal(var_T.cpu().numpy(), var.T)
    pp = chain.posterior_predictive(X)
    q = np.array([0.05, 0.16, 0.5, 0.84, 0.95])
    mom = engs[0].ppd_summary(mu_T, var_T, q, outputs=("moments",))["moments"]       # the fields are these, and their roots
    assert np.array_equal(pp.mean, mom[:, 0]) and np.array_equal(pp.std_emulator, np.sqrt(mom[:, 1]))
    assert np.array_equal(pp.std_parameter, np.sqrt(mom[:, 2])) and np.array_equal(pp.std, np.sqrt(mom[:, 1] + mom[:, 2]))
    assert np.array_equal(pp.quantiles, q) and pp.n_samples == S
    assert pp.band.shape == (5, nobs) and pp.predictive.shape == (5, nobs) and pp.pit.shape == (nobs,)
    assert np.array_equal(pp.band, np.percentile(mean, 100.0 * q, axis=0))
    vexp, yobs = np.diag(chain.expdata_cov), chain.expdata[0]
    worst_m = worst_q = worst_p = 0.0
    for m in range(nobs):
        m1, ev, pv = R.moments(mean[:, m], var[:, m], mean=mom[m, 0])
        for got, want, t in zip(mom[m], (m1, ev, pv), (mean[:, m], var[:, m], (mean[:, m] - mom[m, 0]) ** 2)):
            bar = R.moment_bar(S, t)
            worst_m = max(worst_m, abs(got - want) / bar)
            assert abs(got - want) <= bar, (m, got, want, bar)
        tau = R.tau_of(var[:, m], None, S)
        bar, second = R.cdf_bar(mean[:, m], tau)
        assert second <= 1e-9
        for i, ql in enumerate(q):
            err = abs(R.mix_cdf(pp.predictive[i, m], mean[:, m], tau) - ql)
            worst_q = max(worst_q, err / bar)
            assert err <= bar, (m, ql, err, bar)
        tau = R.tau_of(var[:, m], vexp[m], S)
        bar, second = R.cdf_bar(mean[:, m], tau)
        assert second <= 1e-9
        perr = abs(pp.pit[m] - R.mix_cdf(yobs[m], mean[:, m], tau))
        worst_p = max(worst_p, perr / bar)
        assert perr <= bar, (m, perr, bar)
    print("chain mapped=%s: ratios to the bars: moments %.3f, predictive %.3f, pit %.3f" % (mapped, worst_m, worst_q, worst_p))
    # the same rows as a stored [nwalkers, nsteps, ndim] chain, and in three slabs
    fields = ("mean", "std_emulator", "std_parameter", "std", "band", "predictive", "pit")
    pp3 = chain.posterior_predictive(X.reshape(3, 100, 20))
    chain.ppd_slab_rows = 128
    try:
        pps = chain.posterior_predictive(X)
    finally:
        chain.ppd_slab_rows = None
    for f in fields:
        assert np.array_equal(getattr(pp3, f), getattr(pp, f)), f
        assert np.array_equal(getattr(pps, f), getattr(pp, f)), f


def test_emulator_predict_diag():
    chain, X, _, _ = _chain(True)
    for emu in chain.emuList:
        es = 0.01 * X[:, -1]
        m, c = emu.predict(X, return_cov=True, extra_std=es)
        md, vd = emu.predict_diag(X, extra_std=es)
        assert np.array_equal(md, m) and np.array_equal(vd, np.diagonal(c, axis1=1, axis2=2))


def test_chain_refuses_foreign_emulators_and_shards():
    chain, X, _, _ = _chain(False)

    class Foreign:
        nobs = 4

        def predict(self, X, return_cov=True, extra_std=0):
            return np.zeros((X.shape[0], 4)), np.zeros((X.shape[0], 4, 4))

    class TwoRanks:
        world, rank = 2, 0

    keep = list(chain.emuList)
    try:
        chain.emuList = [keep[0], Foreign()]
        with pytest.raises(NotImplementedError, match="foreign"):
            chain.posterior_predictive(X)
        chain.emuList = keep
        chain.sharding = TwoRanks()
        with pytest.raises(NotImplementedError, match="sharded"):
            chain.posterior_predictive(X)
    finally:
        chain.emuList, chain.sharding = keep, None
