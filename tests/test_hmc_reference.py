"""CPU tier: the HMC step of tests/hmc_reference.py — the restatement the device loop (csrc/gpb_hmc.hip) is held to — on analytic
targets: the leapfrog with reflecting walls is reversible, the chain leaves a box-truncated Gaussian stationary, and the
dual-averaging update (also the host build of csrc/hmc_step.h) steers the acceptance to its target."""
import numpy as np
from scipy.stats import truncnorm

import hmc_reference as R
from test_hmc_step_host import dual_average_errors, run_host_program


def test_leapfrog_with_reflections_is_reversible():
    """L = 32 leapfrogs in the unit box on a Gaussian of sigma = 0.1 whose modes lie near walls, the momentum negated, 32 more:
    the start comes back within 1e-10 — the rounding accumulated over the trajectory, L 2^-53 times the curvature 1 / sigma^2 =
    100, lies five orders below that bound and any error of the algorithm (a wall rule that is not an involution, a kick out of
    place) ten orders above it."""
    d, C, L = 3, 64, 32
    lo, hi = np.zeros(d), np.ones(d)
    target = R.boxed_gaussian(np.array([0.05, 0.9, 0.5]), np.full(d, 0.1), lo, hi)
    rng = np.random.default_rng(7)
    x0 = rng.uniform(0.02, 0.98, (C, d))
    minv = np.full(d, 0.01)
    p0 = rng.standard_normal((C, d)) / np.sqrt(minv)
    _, g0 = target(x0)
    x1, p1, _, g1, esc1, nrefl, _, _ = R.trajectory(x0, p0, g0, 0.25, minv, lo, hi, L, target)
    assert not esc1.any() and nrefl >= C * L // 10            # the walls are exercised
    assert np.max(np.abs(x1 - x0)) > 0.05
    x2, p2, _, _, esc2, nback, _, _ = R.trajectory(x1, -p1, g1, 0.25, minv, lo, hi, L, target)
    assert not esc2.any() and nback == nrefl
    assert np.max(np.abs(x2 - x0)) <= 1e-10, np.max(np.abs(x2 - x0))
    assert np.max(np.abs(p2 + p0) * np.sqrt(minv)) <= 1e-9


def test_stationary_on_a_truncated_gaussian():
    """A product of Gaussians truncated by the unit box, two modes within one sigma of a wall: 512 chains x 400 steps after a
    warm-up of two windows.  Mean and variance of every coordinate within 5 standard errors of scipy.stats.truncnorm's, the
    standard error from the spread of the per-chain time averages over the independent chains.  At least 10 % of all drifts
    reflect (measured: 25 %).  The seed is fixed: the outcome is deterministic."""
    mean, sig = np.array([0.08, 0.5, 0.95, 0.3]), np.array([0.1, 0.15, 0.2, 0.05])
    d, C, L = 4, 512, 8
    lo, hi = np.zeros(d), np.ones(d)
    target = R.boxed_gaussian(mean, sig, lo, hi)
    rng = np.random.default_rng(1234)
    X0 = rng.uniform(0.02, 0.98, (C, d))
    minv = (hi - lo) ** 2 / 12.0
    st = R.start_state(0.1 * d ** -0.25)
    state, st, _, stored, _, _, _ = R.run(target, X0, 60, L, minv, lo, hi, rng, st, adapt=True, keep=True)
    minv = stored[30:].reshape(-1, d).var(0)
    state, st, _, _, _, _, _ = R.run(target, state["x"], 60, L, minv, lo, hi, rng, R.start_state(np.exp(st[1])), adapt=True)
    state, st, acc, stored, nrefl, ndrift, nesc = R.run(target, state["x"], 400, L, minv, lo, hi, rng,
                                                        R.start_state(np.exp(st[1])), keep=True)
    assert nesc == 0
    print("reflecting drifts: %.3f of all; mean accept probability %.3f" % (nrefl / ndrift, acc.mean()))
    assert nrefl >= 0.10 * ndrift
    a, b = (lo - mean) / sig, (hi - mean) / sig
    tm, tv = truncnorm.mean(a, b, loc=mean, scale=sig), truncnorm.var(a, b, loc=mean, scale=sig)
    per_chain = stored.mean(0)
    se = per_chain.std(0, ddof=1) / np.sqrt(C)
    zm = (per_chain.mean(0) - tm) / se
    per_chain_v = ((stored - tm) ** 2).mean(0)               # unbiased for the variance: the true mean is known
    sev = per_chain_v.std(0, ddof=1) / np.sqrt(C)
    zv = (per_chain_v.mean(0) - tv) / sev
    print("mean: z", zm, " variance: z", zv)
    assert np.all(np.abs(zm) <= 5.0), zm
    assert np.all(np.abs(zv) <= 5.0), zv


def test_dual_averaging(tmp_path):
    """the host program's update (csrc/hmc_step.h) equals the restated one to 1e-15; after 100 adaptive steps on a 20-d Gaussian
    (256 chains, unit metric, sigma from 0.5 to 2) the mean acceptance of the next 50 steps lies in [0.65, 0.95] — a sanity
    band, not a measurement (the restatement gives 0.83 for the target 0.8)."""
    errs = dual_average_errors(run_host_program(tmp_path))
    assert len(errs) >= 60 and np.max(errs) <= 1e-15, np.max(errs)
    d = 20
    sig = np.linspace(0.5, 2.0, d)
    lo, hi = np.full(d, -20.0), np.full(d, 20.0)
    target = R.boxed_gaussian(np.zeros(d), sig, lo, hi)
    rng = np.random.default_rng(5)
    X0 = rng.standard_normal((256, d)) * sig
    minv = np.ones(d)
    state, st, _, _, _, _, _ = R.run(target, X0, 100, 8, minv, lo, hi, rng, R.start_state(0.1 * d ** -0.25), adapt=True)
    assert st[4] == 100.0
    state, st, acc, _, _, _, _ = R.run(target, state["x"], 50, 8, minv, lo, hi, rng, R.start_state(np.exp(st[1])))
    print("step size %.4f, mean acceptance %.3f" % (np.exp(st[0]), acc.mean()))
    assert 0.65 <= acc.mean() <= 0.95, acc.mean()


def test_reseed_rows_keeps_the_most_likely_chains():
    """hmc.reseed_rows: the best ceil(C / keep) rows by lp, in turn, C rows again; NaN and -inf last; a pure function"""
    from gpbayestools_hic_amd.hmc import reseed_rows, window_lengths
    X = np.arange(20.0).reshape(10, 2)
    lp = np.array([-5.0, -1.0, np.nan, -3.0, -np.inf, -2.0, -9.0, -1.5, -7.0, -4.0])
    out = reseed_rows(X, lp, keep=4)                          # ceil(10 / 4) = 3 rows: 1, 7, 5
    assert np.array_equal(out, X[[1, 7, 5, 1, 7, 5, 1, 7, 5, 1]])
    assert np.array_equal(reseed_rows(X, lp, keep=1), X[np.argsort(-np.where(np.isnan(lp), -np.inf, lp), kind="stable")])
    assert np.array_equal(reseed_rows(X[:1], lp[:1]), X[:1])
    assert np.array_equal(reseed_rows(X, lp, keep=100), np.repeat(X[1:2], 10, axis=0))
    assert window_lengths(200, 3) == [40, 80, 80] and window_lengths(10, 1) == [10] and sum(window_lengths(37, 4)) == 37
