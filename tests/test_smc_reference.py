"""CPU tier of the SMC sampler: the numpy restatement (tests/smc_reference.py) against closed forms — its Philox counters,
the bisection, the systematic resampling and an analytic evidence."""
import math

import numpy as np
import pytest

import smc_reference as R
from oracle.stretch_oracle import philox4x32_10, u01


def test_philox_counters():
    """normals from (i, k, pair, 9), the accept draw from (i, k, 0, 10), the resampling uniform from (stage, 0, 0, 8)"""
    seed, stage, k, N, d = 2 ** 40 + 17, 5, 123, 7, 5
    key = (seed & 0xFFFFFFFF, seed >> 32)
    dr = R.device_draws(seed, stage, k, N, d)
    assert dr["normals"].shape == (N, d) and dr["logu_accept"].shape == (N,)
    for i in (0, 3, 6):
        for j in range(3):
            x, y, z, w = (int(v) for v in philox4x32_10(key, (i, k, j, 9)))
            u1, u2 = float(u01(x, y)), float(u01(z, w))
            rad, a = math.sqrt(-2.0 * math.log(1.0 - u1)), 2.0 * math.pi * u2
            assert abs(dr["normals"][i, 2 * j] - rad * math.cos(a)) <= 1e-15 * max(1.0, rad)
            if 2 * j + 1 < d:
                assert abs(dr["normals"][i, 2 * j + 1] - rad * math.sin(a)) <= 1e-15 * max(1.0, rad)
        x, y, _, _ = (int(v) for v in philox4x32_10(key, (i, k, 0, 10)))
        assert dr["logu_accept"][i] == np.log(u01(x, y))
    x, y, _, _ = (int(v) for v in philox4x32_10(key, (stage, 0, 0, 8)))
    assert dr["u_resample"] == float(u01(x, y)) and 0.0 <= dr["u_resample"] < 1.0
    # a stage's draws depend on (seed, stage, k) only; the tags keep them apart from PTLMC's (2, 3, 4)
    assert R.device_draws(seed, stage, k + 1, N, d)["u_resample"] == dr["u_resample"]
    assert R.device_draws(seed, stage + 1, k, N, d)["u_resample"] != dr["u_resample"]
    assert np.array_equal(R.device_draws(seed, stage + 1, k, N, d)["normals"], dr["normals"])
    assert not np.array_equal(R.device_draws(seed, stage, k + 1, N, d)["normals"], dr["normals"])
    x, y, z, w = (int(v) for v in philox4x32_10(key, (0, k, 0, 2)))
    assert abs(dr["normals"][0, 0] - math.sqrt(-2.0 * math.log(1.0 - float(u01(x, y)))) * math.cos(2 * math.pi * float(u01(z, w)))) > 1e-6
    big = R.device_draws(11, 0, 0, 4096, 4)
    assert abs(big["normals"].mean()) < 0.03 and abs(big["normals"].std() - 1.0) < 0.03
    assert abs(np.exp(big["logu_accept"]).mean() - 0.5) < 0.03


@pytest.mark.parametrize("beta_prev,scale", [(0.0, 50.0), (0.0, 5e4), (0.3, 400.0), (0.01, 3.0)])
def test_bisection_lands_on_target(beta_prev, scale):
    rng = np.random.default_rng(3)
    N = 1000
    logl = -scale * rng.chisquare(4, size=N)
    logl[17] = np.nan
    rw = R.reweight(logl, beta_prev, 0.5)
    if R.ess(logl, 1.0 - beta_prev) >= 0.5 * N:
        assert rw["beta"] == 1.0
    else:
        assert beta_prev < rw["beta"] < 1.0
        assert abs(rw["ess"] / (0.5 * N) - 1.0) <= 1e-12
    assert rw["nan_weights"] == 1 and rw["w"][17] == 0.0
    db = rw["beta"] - beta_prev
    ok = ~np.isnan(logl)
    ref = np.log(np.sum(np.exp(db * logl[ok] - np.max(db * logl[ok])))) + np.max(db * logl[ok]) - np.log(N)
    assert abs(rw["dlogz"] - ref) <= 1e-12 * max(1.0, abs(ref))


def test_bisection_returns_one_when_ess_suffices():
    logl = np.linspace(-0.5, 0.0, 64)
    rw = R.reweight(logl, 0.2, 0.5)
    assert rw["beta"] == 1.0 and rw["ess"] >= 32.0


def test_systematic_resampling_counts():
    """every index is drawn floor(N w) or ceil(N w) times"""
    rng = np.random.default_rng(5)
    for N in (2, 17, 512, 4097):
        w = rng.exponential(size=N) ** 3
        w[rng.integers(0, N, size=N // 8)] = 0.0
        if not np.any(w > 0):
            w[0] = 1.0
        for u in (0.0, rng.uniform(), 1.0 - 2.0 ** -53):
            anc, cum, pos = R.resample(w, u)
            assert anc.min() >= 0 and anc.max() <= N - 1 and np.all(np.diff(anc) >= 0)
            counts = np.bincount(anc, minlength=N)
            nw = N * w / np.sum(w)
            assert np.all((counts >= np.floor(nw - 1e-9)) & (counts <= np.ceil(nw + 1e-9)))
            assert np.all(counts[w == 0.0] == 0)


def test_device_scan_model():
    """the chunked scan against np.cumsum: monotone, flat exactly over zero weights (also across a chunk boundary), 1 at the
    end, and np.cumsum itself when every thread owns at most one entry"""
    rng = np.random.default_rng(8)
    for N in (5, 1024, 1027, 2051, 4096, 16389):
        w = rng.exponential(size=N)
        w[rng.integers(0, N, size=N // 4)] = 0.0
        C = -(-N // R.RW_THREADS)
        w[max(3 * C - 2, 0):3 * C + 2] = 0.0
        w[0], w[N - 1] = 0.0, 0.5
        cum = R.device_scan(w)
        ref = np.cumsum(w) / np.sum(w)
        assert cum.shape == (N,) and cum[-1] == 1.0 and np.all(np.diff(cum) >= 0)
        assert np.all(np.diff(cum)[w[1:] == 0.0] == 0.0) and cum[0] == 0.0
        assert np.max(np.abs(cum - ref)) <= 2 * N * 2.0 ** -53
        if N <= R.RW_THREADS:
            c1 = np.cumsum(w)
            assert np.array_equal(cum, c1 / c1[-1])
    # three threads over eight weights: chunks [0:3], [3:6], [6:8], bases 0, 6, 21 of a total of 36
    assert np.array_equal(R.device_scan(np.arange(1.0, 9.0), threads=3), np.array([1, 3, 6, 10, 15, 21, 28, 36]) / 36.0)


@pytest.mark.parametrize("beta_prev", [0.0, 0.37])
@pytest.mark.parametrize("N", R.INJECTED_SIZES)
def test_injected_weights_edges_under_both_scans(N, beta_prev):
    """what the cap of 2 knife-edge ancestors per stage in tests/test_gpu_smc.py rests on, where no GPU is needed: with the
    injected log-likelihoods the ancestors under np.cumsum and under the device's chunked scan differ at knife edges only,
    and those number at most 2"""
    logl = R.injected_logl(N)
    assert int(np.sum(np.isnan(logl))) == 6
    rw = R.reweight(logl, beta_prev, 0.5)
    assert rw["nan_weights"] == 6 and beta_prev < rw["beta"] < 1.0
    zero = rw["w"] == 0.0
    assert zero[:3].all() and zero[N - 2:].all() and int(zero.sum()) == 13
    worst = 0.0
    for u in (0.0, 0.31, 0.999999, R.device_draws(11, 0, 0, 2, 1)["u_resample"]):     # the last: the GPU tier's seed and stage
        anc, cum, pos = R.resample(rw["w"], u)
        anc_dev, cum_dev, _ = R.resample(rw["w"], u, scan=R.device_scan)
        edge = R.knife_edges(anc, cum, pos)
        worst = max(worst, float(np.max(np.abs(cum_dev - cum))))
        assert int(edge.sum()) <= 2, (u, int(edge.sum()))
        assert np.array_equal(anc_dev[~edge], anc[~edge]), u
        for a in (anc, anc_dev):
            assert np.all(np.diff(a) >= 0) and not np.any(zero[a])
    print("N=%d beta_prev=%g: the two scans differ by at most %.3g" % (N, beta_prev, worst))
    assert worst <= 2 * N * 2.0 ** -53          # either scan: sums of at most N positive terms, each addition within 2^-53


def test_preconditioner_and_degenerate_ensemble():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((300, 5)) @ rng.standard_normal((5, 5)) + 3.0
    mean, cov, Lc = R.precondition(x)
    assert np.allclose(mean, x.mean(0), rtol=0, atol=1e-13) and np.allclose(cov, np.cov(x.T, bias=True), rtol=0, atol=1e-12)
    assert np.allclose(Lc @ Lc.T, cov, rtol=0, atol=1e-12) and np.all(np.triu(Lc, 1) == 0)
    mean, cov, Lc = R.precondition(np.tile(rng.uniform(size=(1, 5)), (37, 1)))
    assert np.all(cov == 0.0) and Lc is None


def _phi(z):
    return 0.5 * (1.0 + math.erf(z / math.sqrt(2.0)))


# standard deviations over the 16 seeds below of one run's logz, particle mean and particle variance (each averaged over
# the dimensions), measured when this test was written: (d, sd logz, sd mean, sd variance)
RECORDED = {2: (0.0674, 1.20e-3, 7.12e-5), 6: (0.138, 5.66e-4, 5.40e-5)}


@pytest.mark.parametrize("d", [2, 6])
def test_analytic_evidence(d):
    """An isotropic Gaussian of width 0.05 centred in the unit box, N = 1024, nmcmc = 10, 16 seeds: the mean logz against
    sum ln[Phi((1 - m) / s) - Phi(-m / s)], the particle mean and variance against the truncated Gaussian's, each within four
    standard errors of the 16 runs.  Spreads of one run measured when the test was written (RECORDED): d = 2: logz 0.0674,
    mean 1.20e-3, variance 7.12e-5 (4 stages); d = 6: logz 0.138, mean 5.66e-4, variance 5.40e-5 (7 stages).  The spread itself may not exceed twice
    the recorded value, so a noisy sampler cannot pass by widening its own margin."""
    m, s = 0.5, 0.05
    f = R.gaussian_box_loglike(m, s, np.zeros(d), np.ones(d))
    a, b = (0.0 - m) / s, (1.0 - m) / s
    Z1 = _phi(b) - _phi(a)
    pdf = lambda z: math.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)          # noqa: E731
    logz_true = d * math.log(Z1)
    mean_true = m + s * (pdf(a) - pdf(b)) / Z1
    var_true = s * s * (1.0 + (a * pdf(a) - b * pdf(b)) / Z1 - ((pdf(a) - pdf(b)) / Z1) ** 2)
    runs = [R.run(f, np.zeros(d), np.ones(d), 1024, 0.5, 10, 200, seed) for seed in range(16)]
    for r in runs:
        assert r["beta"][-1] == 1.0 and np.all(np.diff(r["beta"]) > 0)
        assert np.array_equal(r["logl"], f(r["x"]))
    stats = np.array([[r["logz"], r["x"].mean(), r["x"].var(axis=0).mean()] for r in runs])
    truth = np.array([logz_true, mean_true, var_true])
    sd = stats.std(axis=0, ddof=1)
    err = np.abs(stats.mean(axis=0) - truth)
    print("d=%d sd %s err %s se %s stages %d" % (d, sd, err, sd / 4.0, len(runs[0]["beta"])))
    assert np.all(sd <= 2.0 * np.array(RECORDED[d])), (sd, RECORDED[d])
    assert np.all(err <= 4.0 * sd / math.sqrt(len(runs))), (err, sd)
