"""CPU tier: the joint-covariance helpers of tests/cov_reference.py, which tests/test_gpu_predict_cov.py holds csrc/gpb_cov.hip
to, at that file's shapes and inputs (L^-1 and K* from the oracle here, from the device there):
  * the long-double evaluation equals oracle.gp_oracle.gp_predict_cov (a triangular solve instead of the explicit inverse) to
    1e-11 of the largest entry — a decade inside the 1e-10 the device is held to against that oracle; the expected size is
    cond(L) Np u, about 3e-12, from the explicit inverse;
  * numpy's own fp64 evaluation of the formula stays inside the rounding bound B, elementwise;
  * max B <= 1e-11 x the prior variance: the bound is never wider than a tenth of the package's covariance bar, so an error it
    lets pass could not have failed that bar either;
  * the per-entry factor G of B's kernel term covers, with its one-evaluation half, the oracle's fp64 k(X*, X*) against a
    long-double evaluation from the same theta."""
import numpy as np
import pytest

import cov_reference as R
from conftest import maxrel
from oracle import gp_oracle as O


@pytest.fixture(scope="module", params=R.SHAPES, ids=lambda s: "N%d-d%d-%s-W%d" % s)
def case(request):
    N, d, kernel, W = request.param
    kind = O.KIND_NAMES[kernel]
    X, Z, theta, Xs = R.problem(N, d, W)
    gps = []
    for p in range(R.P):
        Linv, Kstar = R.host_operands(X, theta[p], kind, Xs)
        gps.append(dict(Linv=Linv, Kstar=Kstar, ref=R.joint_cov_ld(Linv, Kstar, Xs, theta[p], kind),
                        B=R.joint_cov_bound(Linv, Kstar, Xs, theta[p], kind)))
    return dict(N=N, d=d, W=W, kind=kind, X=X, Z=Z, theta=theta, Xs=Xs, gps=gps)


def test_long_double_evaluation_equals_the_oracle(case):
    for p, g in enumerate(case["gps"]):
        L, a = O.gp_factor(case["X"], case["Z"][p], case["theta"][p], case["kind"], R.ALPHA)
        _, cov = O.gp_predict_cov(case["Xs"], case["X"], case["theta"][p], L, a, case["kind"])
        assert g["ref"].dtype == np.longdouble and g["ref"].shape == (case["W"], case["W"])
        assert maxrel(g["ref"].astype(float), cov) < 1e-11


def test_plain_fp64_evaluation_stays_inside_the_bound(case):
    worst = 0.0
    for p, g in enumerate(case["gps"]):
        got = R.joint_cov_f64(g["Linv"], g["Kstar"], case["Xs"], case["theta"][p], case["kind"])
        err = np.abs(got - g["ref"]).astype(float)
        assert np.all(g["B"] > 0) and np.array_equal(g["B"], g["B"].T)
        assert np.all(err <= g["B"])
        worst = max(worst, float(np.max(err / g["B"])))
    print("numpy fp64 error / B: %.3g" % worst)


def test_the_bound_is_capped_by_a_tenth_of_the_covariance_bar(case):
    for p, g in enumerate(case["gps"]):
        prior = O.prior_var(case["theta"][p], case["d"])
        print("max B / prior: %.3g" % (np.max(g["B"]) / prior))
        assert np.max(g["B"]) <= 1e-11 * prior


def test_the_bound_counts_the_padded_design(case):
    """Np enters linearly in three of the four terms: the default is the device's padded length, not N"""
    g, th = case["gps"][0], case["theta"][0]
    assert R.padded(case["N"]) % 64 == 0 and 0 <= R.padded(case["N"]) - case["N"] < 64
    B2 = R.joint_cov_bound(g["Linv"], g["Kstar"], case["Xs"], th, case["kind"], Np=2 * R.padded(case["N"]))
    assert np.all(B2 > g["B"]) and np.all(B2 < 2 * g["B"])


def test_the_kernel_term_covers_one_fp64_evaluation_of_kss(case):
    """u G / 2 |Kss| is the share of ONE fp64 evaluation against exact arithmetic: the oracle's against long double"""
    ld, d, Xs = np.longdouble, case["d"], case["Xs"]
    for th in case["theta"]:
        Q = Xs.astype(ld) / np.exp(th[1:1 + d].astype(ld))
        r2 = ((Q[:, None, :] - Q[None, :, :]) ** 2).sum(-1)
        if case["kind"] == O.KIND_RBF:
            f = np.exp(-r2 / 2)
        elif case["kind"] == O.KIND_MATERN15:
            t = np.sqrt(3 * r2); f = (1 + t) * np.exp(-t)
        else:
            t = np.sqrt(5 * r2); f = (1 + t + t * t / 3) * np.exp(-t)
        exact = np.exp(ld(th[0])) * f
        exact[np.diag_indices_from(exact)] += np.exp(ld(th[-1]))
        G, K = R.kss_rounding_factor(Xs, th), R.kss(Xs, th, case["kind"])
        assert np.array_equal(G, G.T) and np.all(G >= 8.0) and np.max(G) < 1000.0
        err = np.abs(K - exact).astype(float)
        print("oracle Kss error / (u G |Kss| / 2): %.3g, G in [%.0f, %.0f]" % (np.max(err / (R.U * G / 2 * np.abs(K))), G.min(), G.max()))
        assert np.all(err <= R.U * G / 2 * np.abs(K))


def test_inputs_are_what_the_bound_and_the_gpu_tests_assume(case):
    N, W, Xs, X = case["N"], case["W"], case["Xs"], case["X"]
    k = R.n_design_rows(W)
    assert k == min(W // 3, 20) and all(np.any(np.all(X == Xs[i], axis=1)) for i in range(k))
    if k:
        assert np.array_equal(Xs[0], X[0]) and np.array_equal(Xs[k - 1], X[N - 1])
    if W >= 2:
        assert np.array_equal(Xs[-1], Xs[-2]) and not np.array_equal(Xs[-2], Xs[-3])
    assert case["theta"].shape == (R.P, case["d"] + 2) and np.all(Xs >= 0) and np.all(Xs < 1)
