"""CPU tier: the host model of the posterior-predictive summaries (tests/ppd_reference.py) against closed forms and numpy, and
the two new entry points in the boundary header and the binding table."""
import os
import re

import numpy as np
import pytest
from scipy.special import ndtri

import ppd_reference as R
from conftest import REPO


@pytest.mark.parametrize("mu,tau", [(5.0, 0.3), (-3.0, 0.01), (120.0, 7.0), (1.0, 1e-6)])
def test_one_component_quantile_is_the_normal_quantile(mu, tau):
    """S = 1: F is one normal CDF, its q-quantile mu + tau ndtri(q); the 64 halvings of [mu - 9 tau, mu + 9 tau] reach it to
    1e-14 relative.  (|y| >= 1 in every case: at q = 0.9987 a CDF near 1 resolves y to 2^-53 / density = 7.5e-15 tau / 0.3 in
    absolute terms, whatever evaluates it in float64.)"""
    m, t = np.array([mu]), np.array([tau])
    for q in R.LEVELS_MIX:
        y, want = R.mix_quantile(q, m, t), mu + tau * ndtri(q)
        assert abs(y - want) <= 1e-14 * abs(want), (q, y, want)
    assert R.mix_quantile(0.0, m, t) == -np.inf and R.mix_quantile(1.0, m, t) == np.inf


def test_step_components_give_finite_quantiles():
    """tau = 0 samples are steps at mu_s: the mixture of three steps has its median at the middle one"""
    mu, tau = np.array([1.0, 2.0, 3.0]), np.zeros(3)
    assert R.mix_cdf(2.0, mu, tau) == 2.0 / 3.0 and R.mix_cdf(1.5, mu, tau) == 1.0 / 3.0
    y = R.mix_quantile(0.5, mu, tau)
    assert np.isfinite(y) and abs(y - 2.0) < 1e-15 * 4


@pytest.mark.parametrize("S", R.ORDER_SIZES)
@pytest.mark.parametrize("kind", R.ROW_KINDS)
def test_band_is_numpy_percentile(S, kind):
    """np.percentile(row, 100 q) for the levels the package is used with; np.quantile(row, q) — the same routine without the
    division by 100 — for the sixteen levels k / 15, where fl(fl(100 q) / 100) is not always q"""
    rows = R.make_rows(kind, S)
    for q in (R.LEVELS_ORDER, R.LEVELS_16, (0.05, 0.16, 0.5, 0.84, 0.95)):
        q = np.asarray(q)
        exact = np.array_equal(100.0 * q / 100.0, q)
        assert exact or q.shape[0] == 16
        for row in rows:
            with np.errstate(over="ignore", invalid="ignore"):
                want = np.percentile(row, 100.0 * q) if exact else np.quantile(row, q)
                got = R.band(row, q)
            ok = np.isfinite(want)                # (the "wide" rows: hi - lo overflows in numpy's own interpolation too)
            assert np.array_equal(got[ok], want[ok]) and np.array_equal(np.isfinite(got), ok), (S, kind, q)


def test_package_band_rule_is_the_models():
    from gpbayestools_hic_amd.emulator import percentile_from_order
    rows = R.make_rows("normal", 257)
    q = np.asarray(R.LEVELS_16)
    order = np.stack([R.order_stats(r, q) for r in rows])
    assert np.array_equal(percentile_from_order(order, q, 257), np.stack([R.band(r, q) for r in rows]))
    assert np.array_equal(percentile_from_order(order, q, 257), np.quantile(rows, q, axis=1).T)
    q = np.array([0.05, 0.16, 0.5, 0.84, 0.95])
    order = np.stack([R.order_stats(r, q) for r in rows])
    assert np.array_equal(percentile_from_order(order, q, 257), np.percentile(rows, 100.0 * q, axis=1).T)


def test_moments_model():
    rng = np.random.default_rng(5)
    mu, var = 3.0 + rng.standard_normal(1000), rng.uniform(0.1, 0.2, 1000)
    m, ev, pv = R.moments(mu, var)
    assert abs(m - mu.mean()) < 1e-13 and abs(ev - var.mean()) < 1e-14 and abs(pv - mu.var()) < 1e-13
    assert R.moments(mu)[1] == 0.0
    assert R.moments(np.array([1e300, -1e300]))[2] == np.inf


def test_narrow_case_keeps_the_second_term_small():
    """every mixture case keeps f 2^-52 max(|a0|, |b0|, b0 - a0) <= 1e-9, so that the bar says something; a float64 numpy
    restatement of the search stays well inside the bar"""
    worst = 0.0
    for name in R.MIX_CASES:
        mu, var = R.make_mix(name)
        tau = R.tau_of(var, None, mu.shape[0])
        bar, second = R.cdf_bar(mu, tau)
        assert second <= 1e-9, (name, second)

        def cdf64(y, m, t):
            from scipy.special import erfc
            return float(np.sum(0.5 * erfc((m - y) / (t * R.SQRT2))) / m.shape[0])
        for q in R.LEVELS_MIX:
            y = R.mix_quantile(q, mu, tau, cdf=cdf64)
            worst = max(worst, abs(R.mix_cdf(y, mu, tau) - q) / bar)
    print("numpy float64 search: largest |F(y) - q| / bar = %.3f" % worst)
    assert worst <= 1.0


def _declared(header="gpbayes.h"):
    txt = open(os.path.join(REPO, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(gpb_[a-z0-9_]+)\s*\(", txt))


def test_header_and_binding_have_the_entry_points():
    from gpbayestools_hic_amd import _native
    for name in ("gpb_emu_predict_diag", "gpb_ppd_summary"):
        assert name in _declared(), name
        assert name in _native.BOUNDARY, name
    assert len(_native.BOUNDARY["gpb_emu_predict_diag"][1]) == 8 and len(_native.BOUNDARY["gpb_ppd_summary"][1]) == 15
