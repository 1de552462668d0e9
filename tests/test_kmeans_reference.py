"""CPU tier of the posterior clusters (gpb_chain_kmeans): the host model of tests/kmeans_reference.py
against scikit-learn where it is installed; the guard that keeps the GPU tier's comparisons honest (no label and no seed of
its cases can turn on rounding); the binding's argument count; sort_chain_likelihood against the arrays restated in numpy."""
import os
import pickle
import re

import numpy as np
import pytest

import kmeans_reference as R
from conftest import REPO

# (S, d, k, weighted, seed): the shapes the Lloyd restatement was compared with sklearn at when it was written
SK_CASES = ((257, 3, 2, False, 1), (1000, 20, 10, False, 2), (4099, 20, 10, True, 3), (513, 5, 7, True, 4), (3000, 20, 16, False, 5))


@pytest.mark.parametrize("case", SK_CASES, ids=lambda c: "x".join(str(v) for v in c[:3]))
def test_model_matches_sklearn(case):
    """KMeans(init=C0, n_init=1, algorithm="lloyd") started from the model's centres: equal labels and n_iter, centres within
    1e-12, inertia within 1e-12 relative; StandardScaler gives the model's unweighted moments.  sklearn measures tol against the
    UNWEIGHTED variance of what it is given, the model against the weighted one: sklearn gets the tol that makes the absolute
    thresholds equal."""
    cluster = pytest.importorskip("sklearn.cluster")
    prep = pytest.importorskip("sklearn.preprocessing")
    S, d, k, weighted, seed = case
    rng = np.random.default_rng(seed)
    X = R.chain(S, 1, d, k, seed).reshape(S, d)
    w = rng.exponential(1.0, S) if weighted else None
    C0 = X[rng.choice(S, k, replace=False)]
    m = R.kmeans(X, w, k, 1, init=C0[None])
    assert m["min_gap"] > 1e-9
    if not weighted:
        sc = prep.StandardScaler().fit(X)
        assert np.allclose(sc.mean_, m["mean"], rtol=1e-13, atol=0) and np.allclose(sc.scale_, m["scale"], rtol=1e-13, atol=0)
    z = (X - m["mean"]) / m["scale"]
    tol_sk = m["tolabs"] / np.var(z, axis=0).mean()
    km = cluster.KMeans(n_clusters=k, init=(C0 - m["mean"]) / m["scale"], n_init=1, algorithm="lloyd", tol=tol_sk,
                        max_iter=R.MAX_ITER).fit(z, sample_weight=w)
    assert km.n_iter_ == m["n_iter"][0] and m["converged"][0]
    assert np.array_equal(km.labels_, m["labels"][0])
    assert np.max(np.abs(km.cluster_centers_ - m["centers_z"][0])) <= 1e-12
    assert abs(km.inertia_ - m["inertia"][0]) <= 1e-12 * km.inertia_
    if not weighted:                                        # the reference's last step, in standardised units
        assert np.max(np.abs(sc.inverse_transform(km.cluster_centers_) - m["centers"][0]) / m["scale"]) <= 1e-12


def test_model_edge_rules():
    """the rules sklearn does not share: a constant column has scale 1 and mean = its value; a row with a non-finite coordinate
    is skipped; an empty cluster keeps its centre; ties go to the lowest index; the seeding takes the first row whose running
    sum exceeds the target"""
    X = np.array([[0.0, 7.5], [1.0, 7.5], [2.0, 7.5], [np.nan, 7.5], [3.0, 7.5]])
    mu, sc, var_z, weff, nskip = R.moments(X)
    assert mu[1] == 7.5 and sc[1] == 1.0 and var_z[1] == 0.0 and nskip == 1 and weff.tolist() == [1, 1, 1, 0, 1]
    assert mu[0] == 1.5 and sc[0] == np.sqrt(1.25)
    far = np.array([[0.0, 7.5], [3.0, 7.5], [400.0, 7.5]])
    m = R.kmeans(X, None, 3, 1, init=far[None], standardize=False)
    assert m["size"][0].tolist() == [2, 2, 0] and np.array_equal(m["centers"][0, 2], far[2]) and m["labels"][0].tolist() == [0, 0, 1, -1, 1]
    tie = R.kmeans(np.array([[0.0], [1.0], [2.0]]), None, 2, 1, init=np.array([[[0.0], [2.0]]]), standardize=False)
    assert tie["labels"][0].tolist() == [0, 0, 1] and tie["min_gap"] == 0.0
    idx, margin = R.seed_rows(np.array([[0.0], [1.0], [5.0]]), np.array([1.0, 0.0, 3.0]), np.array([0.25, 0.5]))
    assert idx.tolist() == [2, 0] and margin == 0.0           # 0.25 * 4 = 1 is not exceeded by row 0's running sum 1


@pytest.mark.parametrize("run", R.runs(), ids=lambda r: "%s-%s-%s" % ("x".join(str(v) for v in R.CASES[r[0]][0]), r[1], r[2]))
def test_gpu_cases_are_far_from_rounding(run):
    """every case of tests/test_gpu_kmeans.py, with given centres and seeded, in every row order the library sees: no row's two
    nearest centres are closer than 1e-6 (relative) in any iteration of any restart, no seeding target is within 1e-9 of a
    running-sum boundary.  A 1e-10 difference of the centres moves a squared distance by about 1e-10 relative, the running sums
    differ by rounding: at this spacing no label and no seed can differ between the model and the library.  (Two restarts
    that reach the same partition tie for the best; the model reports that as best_margin and the GPU tier accepts either.)"""
    m = R.model(*run)
    assert m["min_gap"] >= 1e-6, m["min_gap"]
    assert m["seed_margin"] >= 1e-9, m["seed_margin"]
    assert np.all(m["converged"]) and m["n_iter"].max() < R.MAX_ITER


def test_binding_has_the_headers_argument_count():
    from gpbayestools_hic_amd import _native
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "gpbayes.h")).read(), flags=re.S)
    decl = re.search(r"\bgpb_chain_kmeans\s*\(([^)]*)\)", txt)
    assert decl, "include/gpbayes.h does not declare gpb_chain_kmeans"
    res, args = _native.BOUNDARY["gpb_chain_kmeans"]
    assert len(args) == len(decl.group(1).split(",")) == 27


def test_sort_chain_likelihood(tmp_path):
    from gpbayestools_hic_amd.clusters import sort_chain_likelihood
    rng = np.random.default_rng(3)
    S = 57
    run = {"chain": rng.standard_normal((S, 4)), "weights": rng.exponential(1.0, S), "logl": rng.standard_normal(S),
           "logp": rng.standard_normal(S), "logz": -12.5, "logz_err": 0.25}
    path = str(tmp_path / "poco.pkl")
    with open(path, "wb") as f:
        pickle.dump(run, f)
    out = sort_chain_likelihood(path)
    assert out == str(tmp_path / "poco_sorted.pkl")
    with open(out, "rb") as f:
        got = pickle.load(f)
    order = np.argsort(run["logl"])[::-1]
    assert list(got) == ["chain", "weights", "logl", "logp", "logz", "logz_err"]
    assert np.all(np.diff(got["logl"]) <= 0)
    for key in ("chain", "weights", "logl", "logp"):
        assert np.array_equal(got[key], run[key][order]), key
    assert got["logz"] == -12.5 and got["logz_err"] == 0.25
