"""CPU tier: the closed-form hold-out predictions (tests/cv_reference.closed_form, on the oracle's Cholesky factor) equal the
brute-force refits (cv_reference.brute_force: gp_factor on the remaining rows + gp_predict_cov) at the shapes and
hyper-parameters of tests/test_gpu_cv.py.  This pins the model the device kernels are held to.
Bars: mean 1e-12 x max(|z|, 1), variance (relative) and fold covariance (relative to its largest entry) 1e-11."""
import numpy as np
import pytest

import cv_reference as R
from conftest import maxrel, relerr

MEAN_BAR, VAR_BAR = 1e-12, 1e-11


def _agree(X, z, theta, kind, folds):
    cf = R.closed_form(X, z, theta, kind, R.ALPHA, folds)
    bf = R.brute_force(X, z, theta, kind, R.ALPHA, folds)
    for F, (mc, cc), (mb, cb) in zip(folds, cf, bf):
        em = R.mean_err(mc, mb, z[np.asarray(F)])
        ev, ec = relerr(np.diag(cc), np.diag(cb)), maxrel(cc, cb)
        assert em < MEAN_BAR and ev < VAR_BAR and ec < VAR_BAR, (em, ev, ec)


@pytest.mark.parametrize("kernel", ["RBF", "Matern", "Matern25"])
def test_leave_one_out(kernel):
    N, d = 100, 3
    X, Z = R.make_data(N, d, 3, seed=11)
    for p, name in enumerate(("mid", "hard", "aniso")):
        _agree(X, Z[p], R.theta_of(name, d), R.KINDS[kernel], [[i] for i in range(N)])


@pytest.mark.parametrize("kernel", ["RBF", "Matern", "Matern25"])
def test_folds(kernel):
    N, d = 150, 5
    X, Z = R.make_data(N, d, 3, seed=12)
    for folds in (R.contiguous_folds(N, 7), R.contiguous_folds(N, 64), R.shuffled_folds(N, 37, seed=5)):
        for p, name in enumerate(("mid", "hard", "aniso")):
            _agree(X, Z[p], R.theta_of(name, d), R.KINDS[kernel], folds)
    assert [len(f) for f in R.contiguous_folds(N, 64)] == [64, 64, 22]
    assert len(R.shuffled_folds(N, 37, seed=5)[-1]) == 2


@pytest.mark.parametrize("N,d", [(64, 1), (64, 8), (65, 1), (65, 8)])
def test_edges(N, d):
    X, Z = R.make_data(N, d, 2, seed=13)
    rest = np.setdiff1d(np.arange(N), [0, N - 1, 7])
    folds = [np.array([N - 1, 0])] + [rest[i:i + 9] for i in range(0, 36, 9)]        # some points are in no fold
    for p, name in enumerate(("mid", "hard")):
        _agree(X, Z[p], R.theta_of(name, d), R.KINDS["RBF"], folds)
        _agree(X, Z[p], R.theta_of(name, d), R.KINDS["Matern25"], folds[:1])


@pytest.mark.parametrize("kernel", ["RBF", "Matern25"])
def test_larger_shape_sample(kernel):
    N, d = 1000, 8
    X, Z = R.make_data(N, d, 4, seed=14)
    kf = R.kfold(N, 16, seed=6)
    assert sorted({len(f) for f in kf}) == [62, 63]
    folds = [[i] for i in (0, 1, 499, 998, 999)] + [kf[0], kf[7], kf[15]]
    for p, name in enumerate(("mid", "hard")):
        _agree(X, Z[p], R.theta_of(name, d), R.KINDS[kernel], folds)
