"""CPU tier: the host model of the rank-normalised diagnostics (tests/rank_reference.py) against what is known in closed form, the
point of the feature on chains that differ in scale only, the margins of every decision the GPU tests rely on, and the Python
names of the feature."""
import numpy as np
import pytest

import acf_reference as A
import rank_reference as M


def _ar1(seed, n_t, n_w, phi):
    rng = np.random.default_rng(seed)
    e = rng.standard_normal((n_t, n_w))
    x = np.empty((n_t, n_w))
    x[0] = e[0]
    for t in range(1, n_t):
        x[t] = phi * x[t - 1] + np.sqrt(1.0 - phi * phi) * e[t]
    return x


def test_python_names_exist():
    from gpbayestools_hic_amd import diagnostics
    from gpbayestools_hic_amd.mcmc import Chain
    from gpbayestools_hic_amd.sampler import LoggingEnsembleSampler
    assert callable(diagnostics.rank_diagnose) and isinstance(diagnostics.RankDiagnostics, type)
    assert callable(Chain.rank_convergence) and callable(LoggingEnsembleSampler.rank_diagnostics)
    from gpbayestools_hic_amd import _native
    assert "gpb_chain_rank_diag" in _native.BOUNDARY


def test_fft_autocovariance_is_the_direct_lag_sum():
    """A(t) of the model's FFT against direct lag sums in long double, on the bulk series of the 300 x 6 chain (parameter 1: the
    offset of 1e3 is gone after the rank transform) and on its raw values: within 1e-14 of A(0)"""
    x = M.mh_chain(*M.SHAPES[3])[:, :, 1]
    v = M.kept(x)
    for a in (M.split(M.z_of(M.rank2(v), v.size), 6), M.split(v, 6)):
        f, d = M.acov_fft(a), M.acov_direct(a)
        assert f.shape == d.shape == (150,)
        assert float(np.max(np.abs(f - d))) <= 1e-14 * float(d[0])


def test_bulk_ess_of_a_tie_free_ar1_chain():
    """8000 x 4 draws of a Gaussian AR(1) chain with phi = 1/2: the rank transform of a normal margin is close to the identity,
    so bulk-ESS estimates n (1 - phi) / (1 + phi) = n / 3.  The estimator's own Monte-Carlo error was obtained by running this
    model on 40 independent chains of the same shape (seeds 1000 ... 1039): the ratio to n / 3 had mean 0.995 and standard
    deviation 0.033 (range 0.905 ... 1.051).  Bar: four standard deviations, 0.13."""
    x = _ar1(1000, 8000, 4, 0.5)
    v = M.kept(x)
    assert len(np.unique(v)) == v.size
    ess, stop, margin = M.ess_of(M.split(M.z_of(M.rank2(v), v.size), 4))
    ratio = ess / (v.size / 3.0)
    print("bulk-ESS %.1f of n / 3 = %.1f: ratio %.4f, stop %d, margin %.3g" % (ess, v.size / 3.0, ratio, stop, margin))
    assert abs(ratio - 1.0) <= 4 * 0.033


def test_scale_difference_is_seen_by_the_folded_rhat_only():
    """eight chains of 200 independent normal draws that share their mean, four of them twice as wide: section 18's classic
    split-R-hat stays below 1.01, the rank-normalised one (the larger of bulk and folded) does not"""
    for seed in range(3):
        x = np.random.default_rng(seed).standard_normal((200, 8, 1))
        x[:, 4:, 0] *= 2.0
        out = M.rank_diag(x)
        classic = M.classic_split_rhat(x)[0]
        ld, _ = A.split_rhat(x)[1], None
        assert abs(classic - float(ld[0])) <= 1e-12                           # the same statistic as tests/acf_reference.py
        print("seed %d: classic %.4f, bulk %.4f, folded %.4f" % (seed, classic, out["rhat"][0, 0], out["rhat"][0, 1]))
        assert classic < 1.01 and out["rhat"][0, 0] < 1.01 < out["rhat"][0, 1]


def test_ties_and_the_dropped_middle_step():
    """65 steps: the middle step enters nothing; a value repeated in time shares its average rank"""
    x = np.array(M.mh_chain(*M.SHAPES[1]))
    y = x.copy()
    y[32] = 1e9                                                               # the dropped step
    a, b = M.rank_diag(x), M.rank_diag(y)
    for k in ("rank2", "median", "quant", "rhat", "ess", "stop", "sd"):
        assert np.array_equal(a[k], b[k])
    r2 = a["rank2"][0]
    assert r2.shape == (64 * 17,) and r2.sum() == r2.size * (r2.size + 1)    # average ranks keep the sum of 1 .. n
    assert np.any(r2 % 2 == 1)                                                # ties of two: half-integer ranks


@pytest.mark.parametrize("case", M.gpu_inputs(), ids=lambda c: c[0])
def test_no_decision_of_the_first_loop_is_close(case):
    """every pair (re, ro) the first loop examines on an input of the GPU tests has |re + ro| >= 1e-9: no rounding moves max_t"""
    label, x, max_lag = case
    out = M.rank_diag(x, M.PROBS, max_lag)
    print("%s: margin %.3g, stop %s" % (label, out["margin"], out["stop"].tolist()))
    assert out["margin"] >= M.MARGIN


def test_the_long_chain_reaches_every_block_diagonal():
    """the slowly mixing chain of the GPU tests: one series stops at lag 133 and reads up to 135, the others run to the end of the
    first loop (stop 345, lags up to 347 = h - 3), so lags of all six block diagonals of the band enter results; and a band is
    flagged exactly when it ends below what a series reads"""
    ref = M.long_reference()
    assert sorted(set(ref["stop"].reshape(-1).tolist())) == [133, 345]
    for L in M.LONG_BAND_LAGS:
        out = M.long_reference(L)
        flagged = out["stop"] >= M.NO_BAND
        assert np.array_equal(flagged, ref["stop"] + 2 > L)
        assert np.array_equal(out["stop"][~flagged], ref["stop"][~flagged]) and np.array_equal(out["ess"][~flagged], ref["ess"][~flagged])
        assert np.all(out["stop"][flagged] == (L | M.NO_BAND)) and np.all(np.isnan(out["ess"][flagged]))
    assert M.long_reference(134)["stop"][0, 2] == (134 | M.NO_BAND) and M.long_reference(135)["stop"][0, 2] == 133


def test_constant_series():
    x = np.array(M.mh_chain(*M.SHAPES[2]))
    x[:, :, 0] = 0.7
    out = M.rank_diag(x)
    assert np.all(np.isnan(out["ess"][0])) and np.all(out["stop"][0] == -1) and np.all(np.isnan(out["rhat"][0]))
    assert out["sd"][0] == 0.0 and out["median"][0] == 0.7 and np.all(out["quant"][0] == 0.7)
    assert np.all(out["rank2"][0] == out["rank2"].shape[1] + 1)
    ref = M.reference(M.SHAPES[2])
    for k in ("rank2", "median", "quant", "rhat", "ess", "stop", "sd"):
        assert np.array_equal(out[k][1:], ref[k][1:])
