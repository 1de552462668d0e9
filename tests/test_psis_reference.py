"""CPU tier: the numpy model of tests/psis_reference.py against things that are not the model — the Zhang-Stephens fit written
directly from the paper, conditioning a Gaussian by deleting a row and a column, a conjugate model whose exact leave-one-out
density is closed-form — and the conditions the GPU tier's input sets must meet."""
import math

import numpy as np
import pytest
import scipy.special
import scipy.stats

import psis_reference as R


def zhang_stephens(x):
    """Zhang & Stephens (2009), section 4, in their notation and with scalar loops: theta_j = 1 / x_(n) + (1 - sqrt(m / (j - 1/2)))
    / (3 x*), x* the first quartile x_(floor(n / 4 + 1/2)); k(theta) = -mean log(1 - theta x); the profile log-likelihood
    l(theta) = n (log(theta / k) + k - 1); w_j = 1 / sum_t exp(l(theta_t) - l(theta_j)); theta_hat = sum theta_j w_j.  Their k is
    minus the shape, so the shape estimate is mean log(1 - theta_hat x)."""
    x = sorted(float(v) for v in x)
    n = len(x)
    m = 30 + int(math.floor(math.sqrt(n)))
    xstar = x[int(math.floor(n / 4 + 0.5)) - 1]
    theta = [1 / x[-1] + (1 - math.sqrt(m / (j - 0.5))) / (3 * xstar) for j in range(1, m + 1)]

    def k_of(th):
        return -sum(math.log1p(-th * v) for v in x) / n
    ell = [n * (math.log(th / k_of(th)) + k_of(th) - 1) for th in theta]
    w = [1 / sum(math.exp(lt - lj) for lt in ell) for lj in ell]
    th_hat = sum(t * v for t, v in zip(theta, w))
    return -k_of(th_hat)


@pytest.mark.parametrize("k", [0.1, 0.5, 0.9])
@pytest.mark.parametrize("n", [50, 200, 425])
def test_gpd_recovery(n, k):
    """Excesses placed exactly on the quantiles p_j = (j - 1/2) / n of a generalised Pareto distribution with shape k carry no
    sampling noise: what separates khat from the prior-shrunk (n k + 5) / (n + 10) is the estimator's finite-n bias, O(1 / n).
    Measured with the independent fit above: n |bias| = 1.42, 0.30, 0.81 (n = 50), 1.78, 0.44, 0.90 (n = 200), 1.76, 0.43, 0.95
    (n = 425) for k = 0.1, 0.5, 0.9; the bar is 3 / n.  The model and the independent fit agree within 1e-12 (measured 2e-15)."""
    t = R.gpd_quantile((np.arange(n) + 0.5) / n, k, 1.0)
    khat, sigma = R.gpd_fit(t)
    indep = (n * zhang_stephens(t) + 5) / (n + 10)
    target = (n * k + 5) / (n + 10)
    print("gpd recovery n=%d k=%g: khat %.6f target %.6f n|bias| %.3f (independent fit %.3f), model - independent %.1e"
          % (n, k, khat, target, n * abs(khat - target), n * abs(indep - target), khat - indep))
    assert abs(khat - indep) <= 1e-12
    assert abs(indep - target) <= 3.0 / n
    assert abs(khat - target) <= 3.0 / n
    assert abs(sigma - 1.0) <= 0.05


@pytest.mark.parametrize("M", [1, 2, 5])
def test_conditionals_equal_deleting_a_row_and_a_column(M):
    """ll_T and zc_T of the LOO model (from the precision matrix) against conditioning N(0, Cw) on all other observables through
    the Schur complement: an identity; bar 1e-12 (condition number <= 100, relative to 1 + |value|)."""
    y, C, yexp, Cadd = R.well_conditioned_cov(3, M, seed=4, with_add=True)
    ll, zc = R.loo_pointwise(y, C, yexp, Cadd)
    worst = 0.0
    for w in range(3):
        for m in range(M):
            l2, z2 = R.loo_by_deletion(y[w], C[w] + Cadd, yexp, m)
            worst = max(worst, abs(ll[m, w] - l2) / (1 + abs(l2)), abs(zc[m, w] - z2) / (1 + abs(z2)))
    print("conditional identity M=%d: worst %.1e" % (M, worst))
    assert worst <= 1e-12
    if M == 1:                                                 # nothing to condition on: the marginal density
        assert np.allclose(ll[0], scipy.stats.norm.logpdf(y[:, 0], yexp[0], np.sqrt(C[:, 0, 0] + Cadd[0, 0])), rtol=1e-13, atol=0)


def test_psis_loo_of_a_conjugate_model_against_the_exact_density():
    """y_i ~ N(theta, 1), theta ~ N(0, 10^2), twelve observations, one of them 3.5 sigma out: the posterior and every leave-one-out
    predictive density are normal in closed form.  With S = 20000 posterior draws PSIS-LOO of every observation lies within three
    Monte-Carlo standard errors of the exact value (the delta-method error of the self-normalised estimate, sqrt(sum w^2
    (p - p_hat)^2) / p_hat), and lppd - elpd_loo > 0."""
    r = np.random.default_rng(42)
    N, tau2, S = 12, 100.0, 20000
    yv = r.standard_normal(N) + 0.3
    yv[4] += 3.5
    prec = 1 / tau2 + N
    theta = yv.sum() / prec + r.standard_normal(S) / np.sqrt(prec)
    ll = scipy.stats.norm.logpdf(yv[:, None], theta[None, :], 1.0)
    out = R.psis_loo(ll)
    for i in range(N):
        p_i = 1 / tau2 + (N - 1)
        exact = scipy.stats.norm.logpdf(yv[i], (yv.sum() - yv[i]) / p_i, np.sqrt(1 / p_i + 1.0))
        lw = R.psis_row(-ll[i])[0]
        w, p = np.exp(lw), np.exp(ll[i])
        se = np.sqrt(np.sum(w * w * (p - np.exp(out[i, 0])) ** 2)) / np.exp(out[i, 0])
        print("exact loo, observation %d: psis %.6f exact %.6f (%.2f se), khat %.3f" % (i, out[i, 0], exact, (out[i, 0] - exact) / se,
                                                                                        out[i, 3]))
        assert abs(out[i, 0] - exact) <= 3 * se
        assert out[i, 1] > out[i, 0]
        assert out[i, 3] < 0.7


def test_decision_margins_of_the_gpu_input_sets():
    """On every input set of the GPU tier no Zhang-Stephens weight lies within a relative 1e-6 of the 10 eps threshold (measured:
    the nearest is 1.9e-2 away), n_tail is at or below 4 only in the sets made for it, and smoothing changes every tail value's
    weight relative to the body's either by more than 1e-7 (measured: 2.5e-6 at least) or, where the largest value is truncated
    back to 0, by less than 1e-12; outside the tail the change is below 1e-12 — tests/test_gpu_psis.py compares the set of
    changed samples (psis_reference.changed_set) exactly."""
    thr = 10 * np.finfo(np.float64).eps
    nearest, least_change, most_noise = np.inf, np.inf, 0.0
    for name, lr in R.all_gpu_sets().items():
        d = {}
        lw, khat, n, _ = R.psis_row(lr, details=d)
        assert (n < R.MIN_TAIL) == (name in R.SHORT_TAIL_SETS), (name, n)
        ch = R.change_of_weights(lr, lw)
        body = np.ones(lr.shape[0], dtype=bool)
        if n >= R.MIN_TAIL:
            assert n >= R.MIN_TAIL + (0 if name in ("edge_S25", "edge_S26") else 1), (name, n)
            nearest = min(nearest, np.min(np.abs(d["fit"]["w"] / thr - 1)))
            assert d["smoothed"]
            body[d["tail"]] = False
            big = ch[d["tail"]] > 1e-10
            assert big.sum() >= n - 1 and np.all(big[:-1]), name          # only the largest tail value may stay where it was
            least_change = min(least_change, ch[d["tail"]][big].min())
            most_noise = max(most_noise, ch[d["tail"]][~big].max(initial=0.0))
        most_noise = max(most_noise, ch[body].max())
    print("decision margins: nearest weight %.2e of the threshold away, least change of a smoothed value %.2e, rounding %.1e"
          % (nearest, least_change, most_noise))
    assert nearest > 1e-6
    assert least_change > 1e-7 and most_noise < 1e-12


def test_model_in_float64_against_longdouble():
    """The model's own rounding on the GPU tier's sets, float64 against np.longdouble: khat within 1e-13 (measured 2.9e-15), the log
    weights within 1e-12 (measured 5.8e-14, the wide-range set; 3.5e-14 otherwise), ess within 1e-12 relative (measured 5.4e-14).
    The GPU tier's bars (khat 1e-12, lw 1e-11) are more than 100 times these.  The classes khat <= 0.5, (0.5, 0.7], (0.7, 1] and
    above 1 all occur; the tied set gives n_tail = 192 and the all-equal row n_tail = 0, khat = inf."""
    dk = dl = de = 0.0
    classes = set()
    for name, lr in R.named_sets().items():
        lw, khat, n, ess = R.psis_row(lr)
        lw2, khat2, n2, ess2 = R.psis_row(lr, np.longdouble)
        assert n == n2
        if np.isfinite(khat):
            dk = max(dk, abs(float(khat - khat2)))
            classes.add(int(np.searchsorted([0.5, 0.7, 1.0], khat)))
        else:
            assert not np.isfinite(khat2)
        dl = max(dl, float(np.abs(lw - lw2).max()))
        de = max(de, abs(float(ess - ess2)) / float(ess2))
    print("float64 against longdouble: khat %.1e, lw %.1e, ess %.1e relative" % (dk, dl, de))
    assert dk <= 1e-13 and dl <= 1e-12 and de <= 1e-12
    assert classes == {0, 1, 2, 3}
    d = {}
    assert R.psis_row(R.tied_ratios(), details=d)[2] == 192
    lw, khat, n, ess = R.psis_row(R.all_equal())
    assert n == 0 and khat == np.inf and np.all(lw == lw[0]) and abs(ess - 640.0) < 1e-9


def test_tail_rule_and_edge_sets():
    """M at the sizes where its two terms cross and where the ceil acts; the clamp at ln DBL_MIN; values equal to the cutoff"""
    assert [R.tail_max(S) for S in (20, 25, 26, 225, 226, 4096, 4097, 20000, 1 << 24)] == [4, 5, 5, 45, 45, 192, 193, 425, 12288]
    d = {}
    _, _, n, _ = R.psis_row(R.wide_range(), details=d)
    assert n == 40 and d["cutoff"] == np.log(np.finfo(np.float64).tiny)
    _, _, n, _ = R.psis_row(R.cutoff_ties(), details=d)
    assert n == R.tail_max(640) - 3 and np.sum(d["x"] == d["cutoff"]) == 5


def test_waic_columns_against_scipy():
    ll = -0.5 * np.random.default_rng(2).standard_normal((3, 500)) ** 2 - 1.0
    zc = np.random.default_rng(3).standard_normal((3, 500))
    out = R.psis_loo(ll, zc)
    assert np.allclose(out[:, 1], scipy.special.logsumexp(ll, axis=1) - np.log(500), rtol=1e-14)
    assert np.allclose(out[:, 2], ll.var(axis=1, ddof=1), rtol=1e-14)
    assert np.all((out[:, 6] > 0) & (out[:, 6] < 1)) and np.all(out[:, 7] == ll.min(axis=1))
