"""CPU tier of the nearest-neighbour distances (gpb_chain_knn): the host model of tests/knn_reference.py,
which tests/test_gpu_knn.py compares the library with bit for bit, is pinned to scipy.spatial.cKDTree on tie-free cases, its
rules for ties, repeated rows, skipped rows and short lists to hand-made cases, and the estimators built on the distances to
closed forms."""
import math
import os
import re

import numpy as np
import pytest
from scipy.spatial import cKDTree

import knn_reference as R
from conftest import REPO

EPS = 2.0 ** -53


# ---------------------------------------------------------------------------- 1. against cKDTree
@pytest.mark.parametrize("n, m, d, k", ((300, 0, 3, 8), (257, 190, 1, 1), (200, 333, 20, 16), (150, 150, 33, 5), (64, 500, 64, 4)))
def test_model_matches_ckdtree(n, m, d, k):
    """tie-free random rows: the neighbours are cKDTree's, the squared distances agree within 2 (d + 3) 2^-53 relative — each
    of the d non-negative terms carries at most 3 roundings (the scaling is exact here apart from one, the difference, the
    square), the sum at most d - 1 more, on either side"""
    rng = np.random.default_rng(1000 * d + k)
    scale = rng.uniform(0.5, 2.0, d)
    A = rng.standard_normal((n, d))
    B = rng.standard_normal((m, d)) if m else None
    got = R.knn(A, B, 1.0 / scale, k)
    ZA = A * (1.0 / scale)
    ZB = ZA if B is None else B * (1.0 / scale)
    dist, idx = cKDTree(ZB).query(ZA, k=k + 1 if B is None else k)
    dist, idx = dist.reshape(n, -1), idx.reshape(n, -1)
    if B is None:
        assert np.array_equal(idx[:, 0], np.arange(n))                       # the row itself, excluded by its number
        dist, idx = dist[:, 1:], idx[:, 1:]
    assert np.all(np.diff(dist, axis=1) > 0)                                  # (the case is tie-free)
    assert np.array_equal(got["idx"], idx.astype(np.int32)) and got["idx"].dtype == np.int32
    assert np.max(np.abs(got["r2"] - dist ** 2) / dist ** 2) <= 2 * (d + 3) * EPS
    assert np.all(got["zeros"] == 0) and got["zeros"].dtype == np.int32 and got["n_skipped"] == (0, 0)


# ---------------------------------------------------------------------------- 2. the rules
def test_ties_go_to_the_lower_row():
    rng = np.random.default_rng(5)
    A = rng.integers(0, 4, (300, 3)).astype(np.float64)
    got = R.knn(A, None, None, 8, skip_zero=False)
    D = R.pair_r2(A, A)
    for i in (0, 17, 299):
        cand = [(D[i, j], j) for j in range(300) if j != i]
        want = sorted(cand)[:8]
        assert [int(v) for v in got["idx"][i]] == [j for _, j in want] and got["r2"][i].tolist() == [v for v, _ in want]
    assert np.any(np.diff(got["r2"], axis=1) == 0)


def test_repeated_rows_and_skip_zero():
    A = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 0.0], [3.0, 0.0], [1.0, 0.0]])
    a = R.knn(A, None, None, 3, skip_zero=True)
    assert a["zeros"].tolist() == [0, 2, 2, 0, 2]
    assert a["idx"].tolist() == [[1, 2, 4], [0, 3, -1], [0, 3, -1], [1, 2, 4], [0, 3, -1]]
    assert a["r2"][1].tolist() == [1.0, 4.0, np.inf]
    b = R.knn(A, None, None, 3, skip_zero=False)
    assert b["zeros"].tolist() == [0, 2, 2, 0, 2] and b["idx"][1].tolist() == [2, 4, 0] and b["r2"][1].tolist() == [0.0, 0.0, 1.0]
    c = R.knn(A[:2], A, None, 2, skip_zero=True)                               # cross mode: the row's own copy in B counts
    assert c["zeros"].tolist() == [1, 3] and c["idx"].tolist() == [[1, 2], [0, 3]]


def test_nonfinite_rows_and_short_lists():
    A = np.array([[0.0, 1.0], [np.nan, 0.0], [2.0, 1.0], [np.inf, 5.0], [5.0, 1.0]])
    B = np.array([[0.5, 1.0], [0.0, -np.inf], [4.0, 1.0]])
    a = R.knn(A, B, None, 3)
    assert a["n_skipped"] == (2, 1)
    assert a["idx"].tolist() == [[0, 2, -1], [-1, -1, -1], [0, 2, -1], [-1, -1, -1], [2, 0, -1]]
    assert np.all(np.isinf(a["r2"][[1, 3]])) and a["r2"][0].tolist() == [0.25, 16.0, np.inf]
    s = R.knn(A, None, None, 5)
    assert s["n_skipped"] == (2, 0) and s["idx"][0].tolist() == [2, 4, -1, -1, -1] and s["r2"].shape == (5, 5)
    huge = R.knn(np.array([[1e300], [0.0]]), None, np.array([1e10]), 1)        # the SCALED coordinate decides
    assert huge["n_skipped"] == (1, 0) and huge["idx"].tolist() == [[-1], [-1]]


def test_scaling_rounds_once():
    rng = np.random.default_rng(8)
    A, inv = rng.standard_normal((50, 4)), 1.0 / rng.uniform(0.1, 3.0, 4)
    got = R.knn(A, None, inv, 2)
    Z = A * inv
    assert np.array_equal(got["r2"], R.knn(Z, None, None, 2)["r2"])
    i, j = 0, int(got["idx"][0, 0])
    acc = 0.0
    for c in range(4):
        t = Z[i, c] - Z[j, c]
        acc = acc + t * t
    assert got["r2"][0, 0] == acc


# ---------------------------------------------------------------------------- 3. the estimators against closed forms
def _tree_r2(A, B, k):
    """the kth-neighbour squared distances by cKDTree, in the model's output form"""
    if B is None:
        return cKDTree(A).query(A, k=k + 1)[0][:, 1:] ** 2
    return cKDTree(B).query(A, k=k)[0].reshape(A.shape[0], -1) ** 2


@pytest.mark.parametrize("seed", range(8))
def test_estimators_against_closed_forms(seed):
    """d = 3, n = m = 2000, k = 4: the entropy of N(0, I) is d/2 ln(2 pi e); D(N(0, I) || N(0.5 1, 1.3^2 I)) = (d / s^2 + d mu^2
    / s^2 - d + 2 d ln s) / 2; D(A || A') of two independent N(0, I) sets is 0.  Within 0.15 nats each: with the cKDTree form of
    the same estimators the largest errors over these seeds were 0.058 and 0.099, the tolerance is that plus half again (the
    run-to-run spread at n = 2000 does not shrink; a tighter bound would test the seed)."""
    d, n, k, mu, s, tol = 3, 2000, 4, 0.5, 1.3, 0.15
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, d))
    B = mu + s * rng.standard_normal((n, d))
    A2 = rng.standard_normal((n, d))
    aa = R.knn(A, None, None, k)
    ab = R.knn(A, B, None, k)
    aa2 = R.knn(A, A2, None, k)
    assert np.allclose(aa["r2"], _tree_r2(A, None, k), rtol=1e-13, atol=0)
    assert np.allclose(ab["r2"], _tree_r2(A, B, k), rtol=1e-13, atol=0)
    h = R.kl_entropy(aa["r2"], d)[k - 1]
    assert abs(h - 0.5 * d * math.log(2.0 * math.pi * math.e)) <= tol
    kl = R.wkv_divergence(aa["r2"], ab["r2"], d, n)[k - 1]
    assert abs(kl - 0.5 * (d / s ** 2 + d * mu ** 2 / s ** 2 - d + 2 * d * math.log(s))) <= tol
    assert abs(R.wkv_divergence(aa["r2"], aa2["r2"], d, n)[k - 1]) <= tol


def test_estimator_pieces():
    from scipy.special import digamma, gammaln
    for n in (1, 2, 7, 63, 64, 65, 2000, 10 ** 6):
        assert abs(R.digamma_int(n) - digamma(n)) <= 4e-15 * max(1.0, abs(digamma(n)))
    for d in (1, 2, 3, 20, 64):
        assert abs(R.log_unit_ball(d) - (0.5 * d * math.log(math.pi) - gammaln(0.5 * d + 1))) <= 1e-13
    r2 = np.array([[1.0, 4.0], [1.0, np.inf]])
    assert np.isnan(R.kl_entropy(r2, 2)[1]) and np.isfinite(R.kl_entropy(r2, 2)[0])
    assert np.isnan(R.kl_entropy(np.array([[0.0], [1.0]]), 2)[0])             # a repeated row listed at distance 0


# ---------------------------------------------------------------------------- 4. the binding
def test_binding_has_the_headers_argument_count():
    from gpbayestools_hic_amd import _native
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "gpbayes.h")).read(), flags=re.S)
    decl = re.search(r"\bgpb_chain_knn\s*\(([^)]*)\)", txt)
    assert decl, "include/gpbayes.h does not declare gpb_chain_knn"
    res, args = _native.BOUNDARY["gpb_chain_knn"]
    assert len(args) == len(decl.group(1).split(",")) == 21
    assert re.search(r"#define\s+GPB_KNN_WS_MB\s+\d+", txt)
