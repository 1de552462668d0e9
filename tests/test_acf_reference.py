"""CPU tier: the host model of the chain diagnostics (tests/acf_reference.py) against what it restates — the FFT form against
long-double direct sums, tau against the AR(1) value, the two deviations from emcee — and, for every input the GPU tests use, that
no rounding can move a window: the least |m - c taus[m]| over m <= window + 2 is far above the model's own error."""
import numpy as np
import pytest

import acf_reference as R


@pytest.mark.parametrize("shape", R.SHAPES)
def test_fft_form_is_the_direct_lag_sum(shape):
    """walker-mean acf, FFT in double against direct sums in long double.  Bar: the two transforms of length N = 2 next_pow_two(n)
    <= 2048 each carry a relative 2-norm error of at most ~5 eps log2 N (Higham, Accuracy and Stability, section 24.1), at worst
    sqrt(N) times that in one entry: 2 * 5 * 2.2e-16 * 11 * 45 = 1.1e-12 of acf[0] = 1.  Seen: 4e-17 .. 8e-15 — either way two
    orders below the 1e-10 the device is held to against this model."""
    x = R.ar1_chain(*shape)
    f_fft, _ = R.walker_mean_acf(x)
    f_dir, _ = R.walker_mean_acf(x, acf=R.function_1d_direct)
    err = np.max(np.abs(f_fft - f_dir))
    print("shape %s: FFT against long-double direct sums, max |diff| = %.3g" % (shape, err))
    assert err < 1.1e-12
    assert np.all(f_fft[0] == 1.0)


def test_tau_of_a_long_ar1_chain():
    """tau -> (1 + phi) / (1 - phi); 4000 steps x 32 walkers: loosely (the estimator's own scatter is a few per cent)"""
    x = R.ar1_chain(4000, 32, 3, seed=7)
    out = R.integrated_time(x)
    want = np.array([(1 + p) / (1 - p) for p in R.PHIS])
    print("tau", out["tau"], "expected", want, "window", out["window"])
    assert np.all(out["window"] < R.NO_WINDOW)
    assert np.allclose(out["tau"], want, rtol=0.15)


@pytest.mark.parametrize("case", R.gpu_inputs(), ids=lambda c: "%dx%dx%d-L%s" % (c[0] + (c[1],)))
def test_window_decisions_of_the_gpu_inputs_are_safe(case):
    """a device rho within 1e-10 of the model's moves taus[m] by at most 2 (m + 1) 1e-10: with a margin above 1e-6 the device must
    find the model's window"""
    shape, max_lag = case
    ref = R.reference(*shape, max_lag=max_lag)
    for j in range(shape[2]):
        w = int(ref["window"][j]) & ~R.NO_WINDOW
        margin = R.window_margin(ref["taus"][j], w, R.C)
        print("shape %s max_lag %s parameter %d: window %d%s, margin %.3g"
              % (shape, max_lag, j, w, " (none inside)" if ref["window"][j] & R.NO_WINDOW else "", margin))
        assert margin > 1e-6


def test_band_prefix_of_the_model():
    """the model restricted to max_lag agrees with the full one on the leading lags, and on tau / window when the window is inside"""
    shape = R.SHAPES[-1]
    full = R.reference(*shape)
    for L in R.BAND_LAGS:
        part = R.reference(*shape, max_lag=L)
        assert np.array_equal(part["rho"], full["rho"][:, :L + 1])
        for j in range(shape[2]):
            if full["window"][j] <= L:
                assert part["window"][j] == full["window"][j] and part["tau"][j] == full["tau"][j]
            else:
                assert part["window"][j] == (L | R.NO_WINDOW) and part["tau"][j] == full["taus"][j][L]


def test_constant_walkers():
    """the deviation: a walker that never moved is left out and counted; emcee's form (switch off) gives NaN for the parameter"""
    x = np.array(R.ar1_chain(300, 6, 3))
    x[:, 2, 0] = 0.25
    out = R.integrated_time(x)
    assert list(out["nconst"]) == [1, 0, 0] and np.all(np.isfinite(out["tau"]))
    rest = R.integrated_time(np.delete(x, 2, axis=1)[:, :, :1])
    assert out["tau"][0] == rest["tau"][0] and out["window"][0] == rest["window"][0]
    f, _ = R.walker_mean_acf(x, skip_constant=False)
    assert np.isnan(f[:, 0]).all() and np.isfinite(f[:, 1:]).all()
    x[:, :, 0] = 0.25
    out = R.integrated_time(x)
    assert out["nconst"][0] == 6 and np.isnan(out["tau"][0]) and out["window"][0] == -1 and np.isnan(out["rho"][0]).all()


def test_argmin_quirk():
    """every m still inside: emcee's argmin gives 0, the model (and the library) the last index"""
    taus = np.linspace(10.0, 20.0, 8)
    assert R.auto_window(taus, 5.0, emcee_argmin_quirk=True) == 0
    assert R.auto_window(taus, 5.0) == 7
    assert R.auto_window(np.array([1.0, 1.5, 0.3, 5.0]), 1.0) == 2          # the first m >= c taus[m]
    assert R.auto_window(-np.ones(4), 5.0) == 3                              # none inside: emcee's own last index


def test_split_rhat_model():
    """independent draws: R-hat near 1; walkers apart: well above; an odd length drops the middle draw"""
    rng = np.random.default_rng(3)
    x = rng.standard_normal((401, 8, 2))
    x[:, :, 1] += 3.0 * np.arange(8)[None, :]
    mom, rhat = R.split_rhat(x)
    assert abs(float(rhat[0]) - 1.0) < 0.02 and float(rhat[1]) > 3.0
    assert abs(float(mom[0, 0]) - x[:, :, 0].mean()) < 1e-15
    y = np.delete(x, 200, axis=0)
    mom_y, rhat_y = R.split_rhat(y)
    assert np.array_equal(mom[:, 1:], mom_y[:, 1:]) and np.array_equal(rhat, rhat_y)
