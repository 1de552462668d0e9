"""CPU tier: the host model of history matching (tests/hm_reference.py) against independent statements of the same definitions — its
counts are np.histogram's and np.histogram2d's, its minima a Python loop's over the bins, its top-K np.sort's, its candidate rows
slab-invariant, uniform and inside the box, its special values the ones include/gpbayes.h lists; the boundary binding of the three
entry points."""
import re
from pathlib import Path

import numpy as np
import pytest

import hm_reference as R

ROOT = Path(__file__).resolve().parents[1]


def _case(S=3000, d=3, B=7, seed=3):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-0.1, 1.1, (S, d))
    edges = np.stack([np.linspace(0.0, 1.0, B + 1) ** (1.0 + 0.5 * j) for j in range(d)])
    X[:5, 0] = edges[0, 2]                       # on an edge
    X[5:9, 1] = edges[1, B]                      # on the last edge: closed
    X[9:12, 2] = np.nan
    score = rng.gamma(2.0, 1.5, S)
    score[::17] = 3.0                            # exactly the cutoff: not NROY
    score[::29] = np.inf
    return X, score, 3.0, edges


def test_counts_are_numpy_histograms():
    X, score, cutoff, edges = _case()
    m = R.maps(X, score, cutoff, edges)
    pairs = R.all_pairs(X.shape[1])
    keep = score < cutoff
    for j in range(X.shape[1]):
        assert np.array_equal(m["cnt1"][j], np.histogram(X[:, j], bins=edges[j])[0])
        assert np.array_equal(m["nroy1"][j], np.histogram(X[keep, j], bins=edges[j])[0])
    for p, (i, j) in enumerate(pairs):
        ok = ~np.isnan(X[:, i]) & ~np.isnan(X[:, j])
        assert np.array_equal(m["cnt2"][p], np.histogram2d(X[ok, i], X[ok, j], bins=(edges[i], edges[j]))[0].astype(np.int64))
        assert np.array_equal(m["nroy2"][p], np.histogram2d(X[ok & keep, i], X[ok & keep, j], bins=(edges[i], edges[j]))[0].astype(np.int64))
    assert m["cnt1"].sum() > 0 and (m["nroy1"] < m["cnt1"]).any()


def test_minimum_is_a_loop_over_bins():
    X, score, cutoff, edges = _case(S=800, B=5)
    m = R.maps(X, score, cutoff, edges)
    B = edges.shape[1] - 1

    def inbin(v, e, b):
        return (v >= e[b]) & ((v < e[b + 1]) | ((b == B - 1) & (v == e[B])))
    for j in range(X.shape[1]):
        for b in range(B):
            k = inbin(X[:, j], edges[j], b)
            assert m["min1"][j, b] == (score[k].min() if k.any() else np.inf)
    for p, (i, j) in enumerate(R.all_pairs(X.shape[1])):
        for a in range(B):
            for b in range(B):
                k = inbin(X[:, i], edges[i], a) & inbin(X[:, j], edges[j], b)
                assert m["min2"][p, a, b] == (score[k].min() if k.any() else np.inf)


def test_maps_accumulate_over_slabs_and_swapped_pairs():
    X, score, cutoff, edges = _case(S=1000)
    pairs = np.array([[2, 0], [0, 1]])
    whole = R.maps(X, score, cutoff, edges, pairs)
    acc = None
    for i0, i1 in ((0, 1), (1, 400), (400, 1000)):
        acc = R.maps(X[i0:i1], score[i0:i1], cutoff, edges, pairs, into=acc)
    assert all(np.array_equal(whole[k], acc[k]) for k in whole)
    straight = R.maps(X, score, cutoff, edges, np.array([[0, 2]]))
    assert np.array_equal(whole["cnt2"][0], straight["cnt2"][0].T) and np.array_equal(whole["min2"][0], straight["min2"][0].T)


def test_topk_is_numpy_sort():
    rng = np.random.default_rng(5)
    M, S = 70, 257
    mu, var = rng.normal(size=(M, S)), rng.uniform(0.1, 2.0, (M, S))
    y, vadd = rng.normal(size=M), rng.uniform(0.0, 1.0, M)
    mu[3], var[3], y[3], vadd[3] = mu[11], var[11], y[11], vadd[11]                # two observables tied everywhere
    for K in (1, 4):
        r = R.implausibility(mu, var, y, vadd, [(0, 10), (10, 11), (5, 70)], K)
        I = np.abs(y[:, None] - mu) / np.sqrt(var + vadd[:, None])
        assert np.array_equal(r["I"], I)
        assert np.array_equal(r["top"], np.sort(I, axis=0)[::-1][:K])
        assert np.array_equal(r["arg"], np.argmax(I, axis=0))                       # (the first of equal maxima)
        assert np.array_equal(r["gmax"], np.stack([I[0:10].max(0), I[10:11].max(0), I[5:70].max(0)]))
        assert r["n_bad"] == 0
    mu[11, :] = y[11] + 50.0                                                       # the tie is the maximum: the lower index wins
    mu[3, :] = y[3] + 50.0
    assert np.all(R.implausibility(mu, var, y, vadd, None, 2)["arg"] == 3)


def test_special_values():
    y = np.zeros(6)
    mu = np.array([[0.0], [1.0], [1.0], [2.0], [np.nan], [np.inf]])
    var = np.array([[0.0], [0.0], [-1.0], [1.0], [1.0], [1.0]])
    vadd = np.array([0.0, 0.0, 0.5, np.inf, 0.0, np.inf])
    I, bad = R.implausibility_matrix(mu, var, y, vadd)
    assert I[0, 0] == 0.0                        # v = 0, r = 0
    assert I[1, 0] == np.inf                     # v = 0, r > 0
    assert I[2, 0] == np.inf                     # v < 0
    assert I[3, 0] == 0.0                        # masked
    assert I[4, 0] == np.inf                     # NaN mean
    assert I[5, 0] == 0.0                        # masked, whatever the mean
    assert bad[0] and not np.any(np.isnan(I))
    for rows, nbad in (([0], 0), ([1], 1), ([2], 1), ([3], 0), ([4], 1), ([0, 3, 5], 0), ([1, 2, 4], 1)):
        assert R.implausibility(mu[rows], var[rows], y[rows], vadd[rows], None, 1)["n_bad"] == nbad
    I, bad = R.implausibility_matrix(np.array([[1.0]]), np.array([[np.nan]]), np.zeros(1), None)
    assert I[0, 0] == np.inf and bad[0]          # NaN variance


def test_uniform_rows():
    lo, hi = np.array([-1.0, 0.0, 10.0]), np.array([1.0, 1e-3, 11.5])
    X = R.uniform_rows(lo, hi, 0, 100000, 7)
    assert np.all(X >= lo) and np.all(X < hi)
    u = (X - lo) / (hi - lo)
    n = u.shape[0]
    assert np.all(np.abs(u.mean(axis=0) - 0.5) < 5.0 * np.sqrt(1.0 / 12.0 / n))
    # Var of the sample variance of a uniform: (mu4 - sigma^4) / n = (1/80 - 1/144) / n
    assert np.all(np.abs(u.var(axis=0) - 1.0 / 12.0) < 5.0 * np.sqrt((1.0 / 80.0 - 1.0 / 144.0) / n))
    for Rabs in (0, 5, 99999):
        assert np.array_equal(X[Rabs], R.uniform_rows(lo, hi, Rabs, 1, 7)[0])
    big = 2 ** 32 - 3                            # crosses the 32-bit counter word
    Y = R.uniform_rows(lo, hi, big, 8, 7)
    assert np.array_equal(Y[5], R.uniform_rows(lo, hi, big + 5, 1, 7)[0])
    assert not np.array_equal(Y[3], R.uniform_rows(lo, hi, 0, 1, 7)[0])           # row 2^32: the high word counts
    assert not np.array_equal(X[:8], R.uniform_rows(lo, hi, 0, 8, 8))


def test_history_match_fields():
    rng = np.random.default_rng(2)
    S, d, M = 500, 2, 6
    X = rng.uniform(size=(S, d))
    mu, var = rng.normal(size=(M, S)), rng.uniform(0.5, 1.0, (M, S))
    edges = np.stack([np.linspace(0, 1, 5)] * d)
    r = R.history_match(X, mu, var, np.zeros(M), np.full(M, 0.1), [(0, 2), (2, 6)], 2, 1.2, edges, keep=10)
    I = np.abs(mu) / np.sqrt(var + 0.1)
    second = np.sort(I, axis=0)[-2]
    assert r["n_nroy"] == np.count_nonzero(second < 1.2) and 0 < r["n_nroy"] < S
    assert r["ruled_out_by"].sum() == np.count_nonzero(I.max(axis=0) >= 1.2)
    assert np.array_equal(r["nroy_samples"], X[second < 1.2][:10])
    assert np.array_equal(r["dataset_nroy_fraction"], [np.mean(I[:2].max(0) < 1.2), np.mean(I[2:].max(0) < 1.2)])
    assert r["cnt1"].sum() == S * d and r["nroy1"].sum() == r["n_nroy"] * d


def test_boundary_binding():
    from gpbayestools_hic_amd import _native
    header = (ROOT / "include" / "gpbayes.h").read_text()
    for name, nargs in (("gpb_hm_uniform", 9), ("gpb_hm_implausibility", 16), ("gpb_hm_maps", 18)):
        decl = re.search(r"GPB_API int %s\(([^;]*)\);" % name, header)
        assert decl, name
        args = re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S)
        assert len(args.split(",")) == nargs == len(_native.BOUNDARY[name][1]), name
    import gpbayestools_hic_amd as G
    assert G.HistoryMatch is G.history.HistoryMatch and callable(G.implausibility_maps) and callable(G.implausibility)
    build = (ROOT / "gpbayestools_hic_amd" / "build.py").read_text()
    assert '"gpb_hm.hip": ["-ffp-contract=off"]' in build


def test_history_match_result_refocus(tmp_path):
    from gpbayestools_hic_amd.history import HistoryMatch
    h = HistoryMatch(n_samples=10, cutoff=3.0, kth=2, n_nroy=4, nroy_fraction=0.4, nroy_fraction_se=0.15, n_bad=0,
                     nroy_box=np.array([[0.2, 0.4], [0.0, 1.0]]), bounds=np.array([[0.0, 1.0], [0.0, 1.0]]))
    assert np.allclose(h.refocus(0.5), [[0.1, 0.5], [0.0, 1.0]])
    h.save(tmp_path / "hm.pkl")
    g = HistoryMatch.load(tmp_path / "hm.pkl")
    assert g.n_nroy == 4 and np.array_equal(g.nroy_box, h.nroy_box) and "nroy_fraction=0.4" in repr(g)
    h.n_nroy = 0
    with pytest.raises(ValueError):
        h.refocus()
