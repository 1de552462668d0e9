"""CPU tier: the host model of gpb_sens_accumulate (tests/sens_reference.py) against itself and against closed forms, the binding
of the new entry point, and the public module's result class."""
import pickle

import numpy as np
import pytest

import sens_reference as R


@pytest.mark.parametrize("M,d", [(1, 1), (3, 2), (17, 5), (33, 20), (5, 64)])
def test_longdouble_and_scipy_routes_agree(M, d):
    """well-conditioned inputs (jitter 1e-2): the two routes agree to a few hundred ulp of the largest entry"""
    J, y, C, x = R.spd_case(4, M, d, seed=M * 100 + d, jitter=1e-2)
    r = R.rows(J, y, C, None, x)
    assert not r["bad"].any() and not r["bad64"].any()
    for w in range(4):
        assert R.err(r["F64"][w], r["F"][w]) < 1e-11


def test_fisher_is_symmetric_positive_semidefinite():
    J, y, C, x = R.spd_case(3, 12, 5, seed=3)
    F = R.fisher_longdouble(J, C)[0].astype(np.float64)
    for w in range(3):
        assert np.allclose(F[w], F[w].T, rtol=0, atol=1e-12 * np.abs(F[w]).max())
        assert np.linalg.eigvalsh(0.5 * (F[w] + F[w].T)).min() > -1e-12 * np.abs(F[w]).max()
    # fewer observables than parameters: rank M, still positive semi-definite
    J, y, C, x = R.spd_case(1, 2, 5, seed=4)
    F = R.fisher_longdouble(J, C)[0][0].astype(np.float64)
    ev = np.linalg.eigvalsh(0.5 * (F + F.T))
    assert ev.min() > -1e-12 * ev.max() and np.sum(ev > 1e-9 * ev.max()) == 2


def test_fisher_is_the_hessian_of_a_linear_model():
    """y = B x with constant C: chi2(x) = 1/2 (B x - y0)^T C^-1 (B x - y0) is quadratic, so its central second differences ARE its
    Hessian B^T C^-1 B up to rounding"""
    rng = np.random.default_rng(5)
    M, d = 7, 3
    B = rng.standard_normal((M, d))
    A = rng.standard_normal((M, M))
    C = A @ A.T + 0.5 * np.eye(M)
    y0 = rng.standard_normal(M)
    F = R.fisher_longdouble(B[None], C[None])[0][0].astype(np.float64)
    Ci = np.linalg.inv(C)

    def chi2(x):
        r = B @ x - y0
        return 0.5 * r @ Ci @ r
    x0, h = rng.standard_normal(d), 0.5
    H = np.zeros((d, d))
    for i in range(d):
        for j in range(d):
            ei, ej = np.eye(d)[i] * h, np.eye(d)[j] * h
            H[i, j] = (chi2(x0 + ei + ej) - chi2(x0 + ei - ej) - chi2(x0 - ei + ej) + chi2(x0 - ei - ej)) / (4 * h * h)
    assert np.allclose(H, F, rtol=0, atol=1e-10 * np.abs(F).max())


def test_response_is_the_limit_of_the_notebooks_formula():
    """y_m(x) = a_m exp(b_m . x): J_mj = b_mj y_m, so R_mj = x_j b_mj.  The notebook's central differences at relative steps h and
    2 h differ from each other by three times FD(h)'s truncation error (Richardson): |R - FD(h)| <= |FD(2h) - FD(h)| + 1e-9 max(1, |R|)"""
    rng = np.random.default_rng(6)
    M, d = 9, 4
    a, b = rng.uniform(0.5, 2.0, M), rng.standard_normal((M, d))
    x0 = rng.uniform(0.3, 1.5, d)

    def f(x):
        return a * np.exp(b @ x)
    J = (b * f(x0)[:, None])[None]
    Rm = R.response(J, f(x0)[None], x0[None])[0]
    assert np.allclose(Rm, x0[None, :] * b, rtol=1e-14)
    for h in (1e-4, 1e-2):
        f1, f2 = R.notebook_response(f, x0, h), R.notebook_response(f, x0, 2 * h)
        assert np.all(np.abs(Rm - f1) <= np.abs(f2 - f1) + 1e-9 * np.maximum(1.0, np.abs(Rm)))


def test_sums_leave_out_bad_and_weightless_rows():
    J, y, C, x = R.spd_case(6, 5, 3, seed=7)
    C[2] = -C[2]
    wt = np.array([1.0, 0.0, 2.0, 0.5, 0.0, 3.0])
    r = R.rows(J, y, C, None, x)
    assert r["bad"].tolist() == [False, False, True, False, False, False] and r["bad64"].tolist() == r["bad"].tolist()
    s = R.sums(r, wt)
    assert float(s["wsum"]) == 4.5 and s["n_bad"] == 1
    want = 1.0 * r["R"][0] + 0.5 * r["R"][3] + 3.0 * r["R"][5]
    assert np.allclose(s["response"].astype(np.float64), want, rtol=1e-14)


def test_binding_and_layout():
    from gpbayestools_hic_amd import _native as nat
    from gpbayestools_hic_amd.engine import GPEngine
    assert len(nat.BOUNDARY["gpb_sens_accumulate"][1]) == 12
    assert GPEngine.sens_acc_doubles(7, 3) == 1 + 9 + 3 * 21
    # the switch between the LDS and the in-place path: M (M | 1) + M d against SENS_LDS_DOUBLES
    M = max(m for m in range(1, 200) if GPEngine.sens_path(m, 20) == "lds")
    assert M * (M | 1) + 20 * M <= GPEngine.SENS_LDS_DOUBLES < (M + 1) * ((M + 1) | 1) + 20 * (M + 1)
    assert GPEngine.sens_path(M + 1, 20) == "global" and GPEngine.sens_path(130, 20) == "global"
    import os
    import re
    from conftest import REPO
    txt = open(os.path.join(REPO, "include", "gpbayes.h")).read()
    assert int(re.search(r"#define GPB_SENS_LDS_DOUBLES (\d+)", txt).group(1)) == GPEngine.SENS_LDS_DOUBLES


def test_public_module_imports_and_result_pickles():
    from gpbayestools_hic_amd import sensitivity as S
    from gpbayestools_hic_amd.mcmc import Chain
    from gpbayestools_hic_amd.sampler import StretchSampler
    assert callable(Chain.sensitivity) and callable(StretchSampler.sensitivity) and callable(S.posterior_sensitivity)
    rng = np.random.default_rng(8)
    A = rng.standard_normal((2, 3, 3))
    F = A @ np.swapaxes(A, 1, 2)
    res = S.PosteriorSensitivity(10, [0, 1], rng.standard_normal((5, 3)), rng.uniform(size=(5, 3)), rng.uniform(size=(5, 3)), F,
                                 np.zeros(3), np.eye(3), [1.0, 2.0, 0.5], names=["a", "b", "c"])
    back = pickle.loads(pickle.dumps(res))
    for k in ("response_mean", "response_std", "obs_information", "fisher", "fisher_total", "information", "param_mean",
              "param_cov", "n_bad"):
        assert np.array_equal(getattr(back, k), getattr(res, k)), k
    assert back.n_samples == 10 and back.names == ["a", "b", "c"] and "PosteriorSensitivity" in repr(back)
    assert np.array_equal(res.information, np.stack([np.diag(F[0]), np.diag(F[1])]) * np.array([1.0, 4.0, 0.25]))
    assert np.allclose(res.forecast_cov() @ res.fisher_total, np.eye(3), atol=1e-10)
    ev, vec = res.stiff_directions()
    assert np.all(np.diff(ev) <= 0) and vec.shape == (3, 3)
    sing = S.PosteriorSensitivity(1, [0], np.zeros((1, 3)), np.zeros((1, 3)), np.zeros((1, 3)), np.ones((1, 3, 3)), np.zeros(3),
                                  np.eye(3), np.ones(3))
    with pytest.raises(np.linalg.LinAlgError):
        sing.forecast_cov()
