"""CPU tier: the host model of gpb_gof_accumulate / gpb_gof_influence (tests/gof_reference.py) against itself and against closed
forms, the binding table, the accumulator layout and the public surface of gof.py."""
import os
import pickle
import re

import numpy as np
import scipy.linalg

import gof_reference as R
from conftest import REPO


def _case(W, M, seed, jitter=1e-6):
    _, y, C, _ = R.spd_case(W, M, 1, seed, jitter)
    rng = np.random.default_rng(seed + 1)
    yexp = rng.uniform(0.5, 2.0, M)
    Cadd = np.diag(rng.uniform(0.1, 1.0, M))
    return y, C, yexp, Cadd


def test_longdouble_and_scipy_routes_agree():
    for M, seed in ((1, 3), (6, 4), (33, 5)):
        y, C, yexp, Cadd = _case(7, M, seed)
        r = R.rows(y, C, yexp, Cadd)
        assert not r["bad"].any() and not r["bad64"].any()
        for a, b in (("chi2_64", "chi2"), ("logdet64", "logdet"), ("ll64", "ll"), ("z64", "z")):
            assert R.err(r[a], r[b]) < 1e-9, (M, a)
        assert np.allclose((r["z"] * r["z"]).sum(1).astype(float), r["chi2"].astype(float), rtol=1e-15)
        assert np.allclose(r["ll"].astype(float), (-r["chi2"] / 2 - r["logdet"] / 2).astype(float), rtol=1e-15)


def test_ll_is_the_references_mvn_loglike():
    y, C, yexp, Cadd = _case(5, 17, 11)
    r = R.rows(y, C, yexp, Cadd)
    for w in range(5):
        want = R.mvn_loglike_restated(y[w] - yexp, C[w] + Cadd)
        assert abs(float(r["ll"][w]) - want) <= 1e-9 * max(abs(want), 1.0)


def test_p_is_uniform_for_rows_drawn_from_the_model():
    """y = yexp + L xi with xi ~ N(0, 1): chi2 is chi2_M exactly, p uniform on (0, 1), and the mean of n values lies within four
    standard deviations 4 / sqrt(12 n) of 1/2"""
    n, M = 400, 5
    rng = np.random.default_rng(21)
    _, _, C, _ = R.spd_case(n, M, 1, 22, jitter=1e-2)
    yexp = rng.uniform(0.5, 2.0, M)
    L = np.linalg.cholesky(C)
    y = yexp[None, :] + np.einsum("wij,wj->wi", L, rng.standard_normal((n, M)))
    r = R.rows(y, C, yexp)
    assert abs(r["p"].mean() - 0.5) <= 4.0 / np.sqrt(12.0 * n)
    assert abs(float(r["chi2"].astype(float).mean()) - M) <= 4.0 * np.sqrt(2.0 * M / n)


def test_whitened_residuals_of_a_diagonal_covariance_are_the_pulls():
    rng = np.random.default_rng(31)
    W, M = 4, 9
    var = rng.uniform(0.2, 3.0, (W, M))
    C = np.stack([np.diag(v) for v in var])
    y, yexp = rng.standard_normal((W, M)), rng.standard_normal(M)
    r = R.rows(y, C, yexp)
    assert np.allclose(r["z"].astype(float), r["pull"], rtol=1e-15)
    assert np.allclose(r["pull"], (y - yexp) / np.sqrt(var), rtol=1e-15)


def test_skip_rules_of_the_sums():
    y, C, yexp, _ = _case(6, 4, 41)
    C[2] = -C[2]
    C[4, 0, 0] = np.nan
    wt = np.array([1.0, 0.0, 2.0, 0.5, 0.0, 3.0])
    r = R.rows(y, C, yexp)
    assert r["bad"].tolist() == [False, False, True, False, True, False]
    s = R.sums(r, wt)
    assert float(s["wsum"]) == 4.5 and s["n_bad"] == 1            # (row 4 is weightless: not evaluated, not counted)
    want = 1.0 * r["z"][0] + 0.5 * r["z"][3] + 3.0 * r["z"][5]
    assert np.allclose(s["z"].astype(float), want.astype(float), rtol=1e-14)


def test_influence_weights_recover_the_leave_one_out_posterior_of_a_conjugate_toy():
    """theta ~ N(0, 1), three data sets y_e ~ N(theta, s_e^2): the posterior and the posterior without e are Gaussians in closed
    form.  Rows drawn from the full posterior, reweighted with exp(-ll_e), give the mean without e within five standard errors
    std_-e / sqrt(ess) and its standard deviation within 10 %"""
    rng = np.random.default_rng(51)
    ye, se = np.array([0.4, -0.3, 0.9]), np.array([0.8, 1.1, 0.6])
    prec = 1.0 + np.sum(1.0 / se ** 2)
    mu, sd = np.sum(ye / se ** 2) / prec, 1.0 / np.sqrt(prec)
    S = 20000
    th = mu + sd * rng.standard_normal(S)
    ll_T = np.stack([-0.5 * ((ye[e] - th) / se[e]) ** 2 - np.log(se[e]) for e in range(3)])
    out, _ = R.influence(ll_T, th[:, None])
    for e in range(3):
        prec_e = prec - 1.0 / se[e] ** 2
        mu_e, sd_e = (np.sum(ye / se ** 2) - ye[e] / se[e] ** 2) / prec_e, 1.0 / np.sqrt(prec_e)
        ess = out[e, 0] ** 2 / out[e, 1]
        m = out[e, 2] / out[e, 0]
        s = np.sqrt(out[e, 3] / out[e, 0] - m * m)
        assert 1000 < ess <= S
        assert abs(m - mu_e) <= 5.0 * sd_e / np.sqrt(ess), (e, m, mu_e)
        assert abs(s / sd_e - 1.0) < 0.1
    # rows with a NaN ll or a zero weight are left out, and a row of the result does not depend on the others
    ll_n = ll_T.copy()
    ll_n[1, 7] = np.nan
    wt = np.ones(S)
    wt[9] = 0.0
    o2, _ = R.influence(ll_n, th[:, None], wt)
    keep = np.ones(S, dtype=bool)
    keep[[7, 9]] = False
    o3, _ = R.influence(ll_T[1:2, keep], th[keep, None])
    assert np.array_equal(o2[1], o3[0])


def test_binding_and_layout():
    from gpbayestools_hic_amd import _native as nat
    from gpbayestools_hic_amd.engine import GPEngine
    assert len(nat.BOUNDARY["gpb_gof_accumulate"][1]) == 12 and len(nat.BOUNDARY["gpb_chi2_sf"][1]) == 5
    assert len(nat.BOUNDARY["gpb_gof_influence"][1]) == 9
    assert GPEngine.gof_acc_doubles(7) == 2 + 4 * 7
    M = max(m for m in range(1, 200) if GPEngine.gof_path(m) == "lds")
    assert (M + 1) * (M | 1) <= GPEngine.GOF_LDS_DOUBLES < (M + 2) * ((M + 1) | 1)
    assert GPEngine.gof_path(M + 1) == "global" and GPEngine.gof_path(130) == "global" and GPEngine.gof_path(1) == "lds"
    txt = open(os.path.join(REPO, "include", "gpbayes.h")).read()

    def macro(name):
        return re.search(r"#define %s (.+)" % re.escape(name), txt).group(1).strip()
    assert int(macro("GPB_GOF_LDS_DOUBLES")) == GPEngine.GOF_LDS_DOUBLES and GPEngine.GOF_LDS_DOUBLES * 8 <= 64 * 1024
    assert (int(macro("GPB_GOF_MAX_M")), int(macro("GPB_GOF_MAX_D")), int(macro("GPB_GOF_MAX_E"))) \
        == (GPEngine.GOF_MAX_M, GPEngine.GOF_MAX_D, GPEngine.GOF_MAX_E)
    assert (macro("GPB_GOF_ACC_W"), macro("GPB_GOF_ACC_P"), macro("GPB_GOF_ACC_Z")) == ("0", "1", "2")
    ev = lambda name, M: eval(macro(name + "(M)").replace("(int64_t)", ""), {"M": M})      # noqa: E731
    assert [ev(n, 7) for n in ("GPB_GOF_ACC_Z2", "GPB_GOF_ACC_PULL", "GPB_GOF_ACC_PULL2", "GPB_GOF_ACC_DOUBLES")] == [9, 16, 23, 30]
    # gof_unpack cuts the accumulator at those offsets
    a = np.arange(30.0)
    u = GPEngine.gof_unpack(a, np.array([5, 1]), 7)
    assert u["wsum"] == 0.0 and u["p"] == 1.0 and u["z"][0] == 2.0 and u["z_sq"][0] == 9.0 and u["pull"][0] == 16.0
    assert u["pull_sq"].tolist() == list(range(23, 30)) and (u["n_rows"], u["n_bad"]) == (5, 1)
    chi2_h = open(os.path.join(REPO, "gpbayestools_hic_amd", "csrc", "chi2_sf.h")).read()
    assert int(re.search(r"#define GPB_CHI2_SF_MAX_ITER (\d+)", chi2_h).group(1)) >= 300


def test_public_surface_and_pickle():
    import gpbayestools_hic_amd as pkg
    from gpbayestools_hic_amd import gof as G
    from gpbayestools_hic_amd.mcmc import Chain
    from gpbayestools_hic_amd.sampler import StretchSampler
    assert pkg.GoodnessOfFit is G.GoodnessOfFit and pkg.posterior_gof is G.posterior_gof
    assert callable(Chain.goodness_of_fit) and callable(StretchSampler.goodness_of_fit)
    rng = np.random.default_rng(8)
    q = np.array([0.05, 0.16, 0.5, 0.84, 0.95])
    quant = np.sort(rng.uniform(1.0, 9.0, (2, 5)), axis=1)
    tot = G.GofTotal(0, 7, 6.5, np.sort(rng.uniform(3.0, 12.0, 5)), 2.5, 3, np.zeros(3), 0.41, False)
    infl = G.DataSetInfluence(np.array([10.0, 4.0]), rng.standard_normal((2, 3)), rng.uniform(size=(2, 3)), ["a", "b", "c"])
    res = G.GoodnessOfFit(10, [0, 1], [3, 4], q, quant.mean(1), quant, quant[:, 0], np.array([1, 2]), np.zeros((2, 3)),
                          np.array([0.3, 0.7]), tot, None, np.zeros(7), np.ones(7), np.zeros(7), np.ones(7), infl,
                          dict(chi2=np.ones((10, 2)), loglike=np.zeros((10, 2))), ["a", "b", "c"])
    back = pickle.loads(pickle.dumps(res))
    for k in ("n_bad", "ndf", "chi2_mean", "chi2_quantiles", "chi2_min", "ppp", "resid_mean", "resid_rms", "pull_mean", "pull_rms"):
        assert np.array_equal(getattr(back, k), getattr(res, k)), k
    assert back.n_samples == 10 and back.total.ndf == 7 and back.total.ppp == 0.41 and back.names == ["a", "b", "c"]
    assert np.array_equal(back.influence.shift, infl.shift) and np.array_equal(back.rows["chi2"], res.rows["chi2"])
    text = repr(back)
    assert "data set" in text and "chi2/ndf (median, 68 %)" in text and "ppp" in text and "emulator 1" in text and "total" in text
    assert "%.3f" % (quant[1, 2] / 4.0) in text
    none = G.GoodnessOfFit(10, [0], [3], q, quant[:1].mean(1), quant[:1], quant[:1, 0], np.array([1]), np.zeros((1, 3)),
                           np.array([0.3]), None, "too many observables", np.zeros(3), np.ones(3), np.zeros(3), np.ones(3))
    assert "too many observables" in repr(none) and none.influence is None and none.rows is None
