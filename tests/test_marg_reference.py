"""CPU tier: the host model of the chain marginals (tests/marg_reference.py) against numpy itself — its counts are np.histogram's and
np.histogram2d's for explicit edges, for bins / range, for the data's own range, with every edge planted in the data next to both of
its one-ulp neighbours, and with values outside the range and NaN; the integer-weight model against np.histogram(weights=w); the
credible-level thresholds on a table worked out by hand; the boundary binding of gpb_chain_marginals."""
import numpy as np
import pytest

import marg_reference as R


def _np_counts(x, edges, pairs):
    """numpy's own counts; NaN rows are dropped per histogram, as the bin rule leaves them outside (np.histogram refuses NaN only
    when it has to find the range itself)"""
    d = edges.shape[0]
    h1 = np.array([np.histogram(x[:, j][~np.isnan(x[:, j])], bins=edges[j])[0] for j in range(d)])
    h2 = []
    for i, j in pairs:
        ok = ~np.isnan(x[:, i]) & ~np.isnan(x[:, j])
        h2.append(np.histogram2d(x[ok, i], x[ok, j], bins=[edges[i], edges[j]])[0])
    return h1, np.array(h2).reshape(len(pairs), edges.shape[1] - 1, edges.shape[1] - 1)


@pytest.mark.parametrize("uniform", (True, False), ids=("uniform", "nonuniform"))
@pytest.mark.parametrize("B", (1, 7, 20, 64))
def test_explicit_edges(B, uniform):
    d = 4
    edges = R.edges_of(d, B, uniform=uniform, seed=B)
    x = R.chain(301, 3, d).reshape(-1, d)
    h1, h2, outside = R.counts(x, edges)
    n1, n2 = _np_counts(x, edges, R.all_pairs(d))
    assert np.array_equal(h1, n1) and np.array_equal(h2, n2.astype(np.int64))
    assert np.array_equal(h1.sum(axis=1) + outside, np.full(d, x.shape[0])) and outside.min() > 0


@pytest.mark.parametrize("B", (5, 20))
def test_bins_and_range(B):
    """np.histogram(x, bins=B, range=(lo, hi)) and histogram2d's form take the edges np.linspace(lo, hi, B + 1)"""
    d = 3
    x = R.chain(500, 2, d).reshape(-1, d)
    lo, hi = np.array([-1.5, -2.0, 0.0]), np.array([1.0, 2.5, 3.0])
    edges = np.stack([np.linspace(lo[j], hi[j], B + 1) for j in range(d)])
    h1, h2, _ = R.counts(x, edges)
    for j in range(d):
        n, e = np.histogram(x[:, j], bins=B, range=(lo[j], hi[j]))
        assert np.array_equal(e, edges[j]) and np.array_equal(n, h1[j])
    for p, (i, j) in enumerate(R.all_pairs(d)):
        n = np.histogram2d(x[:, i], x[:, j], bins=B, range=[(lo[i], hi[i]), (lo[j], hi[j])])[0]
        assert np.array_equal(n.astype(np.int64), h2[p])


def test_data_range_and_a_constant_column():
    """bins=20 alone: the edges are np.linspace(min, max, 21), widened by 0.5 when a column is constant"""
    x = np.array(R.chain(400, 1, 3).reshape(-1, 3))
    x[:, 2] = 0.25
    lo, hi = x.min(axis=0), x.max(axis=0)
    lo[2], hi[2] = lo[2] - 0.5, hi[2] + 0.5
    edges = np.stack([np.linspace(lo[j], hi[j], 21) for j in range(3)])
    h1, h2, outside = R.counts(x, edges)
    assert np.all(outside == 0)
    for j in range(3):
        n, e = np.histogram(x[:, j], bins=20)
        assert np.array_equal(e, edges[j]) and np.array_equal(n, h1[j])
    for p, (i, j) in enumerate(R.all_pairs(3)):
        n, ei, ej = np.histogram2d(x[:, i], x[:, j], bins=20)
        assert np.array_equal(ei, edges[i]) and np.array_equal(ej, edges[j]) and np.array_equal(n.astype(np.int64), h2[p])


@pytest.mark.parametrize("uniform", (True, False), ids=("uniform", "nonuniform"))
@pytest.mark.parametrize("B", (1, 7, 20, 64))
def test_planted_edges_outside_values_and_nan(B, uniform):
    d = 3
    edges = R.edges_of(d, B, uniform=uniform, seed=B)
    x = R.planted(edges)
    c = R.codes(x, edges)
    for j in range(d):
        e = edges[j]
        for b in range(B + 1):
            at = c[x[:, j] == e[b], j]
            assert np.all(at == min(b, B - 1))                                                 # the edge itself: its bin, the last one closed
            below = c[x[:, j] == np.nextafter(e[b], -np.inf), j]
            above = c[x[:, j] == np.nextafter(e[b], np.inf), j]
            assert np.all(below == (b - 1 if b > 0 else R.OUT)) and np.all(above == (b if b < B else R.OUT))
        assert np.all(c[~np.isfinite(x[:, j]), j] == R.OUT)
    h1, h2, outside = R.counts(x, edges)
    n1, n2 = _np_counts(x, edges, R.all_pairs(d))
    assert np.array_equal(h1, n1) and np.array_equal(h2, n2.astype(np.int64))
    # the bins / range form on the same planted values (uniform edges only: that form has no other)
    if uniform:
        for j in range(d):
            v = x[:, j][~np.isnan(x[:, j])]
            assert np.array_equal(np.histogram(v, bins=B, range=(edges[j, 0], edges[j, -1]))[0], h1[j])


def test_integer_weights_against_numpy():
    """weights over 12 decades: the integer model is within S 2^-33 of np.histogram(weights=w), relative to the largest bin (every
    weight is rounded by at most half a unit of 2^-32 max w)"""
    S, d, B = 4099, 2, 20
    rng = np.random.default_rng(9)
    x = R.chain(S, 1, d).reshape(-1, d)
    w = 10.0 ** rng.uniform(-12.0, 0.0, S)
    q = R.int_weights(w)
    assert q.max() == 1 << 32 and q.min() >= 0
    edges = R.edges_of(d, B)
    h1, h2, outside = R.counts(x, edges, q=q)
    unit = w.max() / R.TWO32
    for j in range(d):
        ref = np.histogram(x[:, j], bins=edges[j], weights=w)[0]
        assert np.max(np.abs(h1[j] * unit - ref)) <= S * 2.0 ** -33 * ref.max()
    ref = np.histogram2d(x[:, 0], x[:, 1], bins=[edges[0], edges[1]], weights=w)[0]
    assert np.max(np.abs(h2[0] * unit - ref)) <= S * 2.0 ** -33 * ref.max()
    # equal weights are 2^32 times the plain counts; NaN, negative and overflowing weights clamp
    e1, e2, eo = R.counts(x, edges, q=R.int_weights(np.full(S, 0.37)))
    p1, p2, po = R.counts(x, edges)
    assert np.array_equal(e1, p1 << 32) and np.array_equal(e2, p2 << 32) and np.array_equal(eo, po << 32)
    assert list(R.int_weights([np.nan, -1.0, 0.5, 2.0, 1e-11], wscale=R.TWO32)) == [0, 0, 1 << 31, 1 << 32, 0]
    assert list(R.int_weights([0.5, 1.5, 2.5], wscale=1.0)) == [0, 2, 2]                          # round half to even


def test_credible_levels_by_hand():
    """counts 4, 3, 2, 1 (total 10): 68 % is reached at the second bin (4 + 3 = 7 >= 6.8), 95 % at the last (10 >= 9.5)"""
    tile = np.array([[0, 1, 0], [3, 4, 0], [0, 2, 0]])
    assert list(R.credible_levels(tile, (0.68, 0.95))) == [3, 1]
    assert list(R.credible_levels(tile, (0.4, 0.41, 0.7, 1.0))) == [4, 3, 3, 1]
    assert list(R.credible_levels(np.zeros((3, 3), dtype=np.int64))) == [0, 0]
    from gpbayestools_hic_amd.marginals import PosteriorMarginals, weighted_quantile
    m = PosteriorMarginals(np.zeros((2, 4)), np.zeros((2, 3), dtype=np.int64), tile[None], np.array([[1, 0]]), np.zeros(2, dtype=np.int64),
                           10, np.array([0.5]), np.zeros((1, 2)), np.zeros(2), np.zeros(2), np.zeros(2))
    assert list(m.credible_levels(1, 0)) == [3, 1] and list(m.credible_levels(0, 1, (0.4, 0.41, 0.7, 1.0))) == [4, 3, 3, 1]
    assert np.array_equal(m.pair(1, 0), tile) and np.array_equal(m.pair(0, 1), tile.T)
    with pytest.raises(KeyError):
        m.pair(0, 2)
    # the weighted quantile: samples 1, 2, 3, 4 with weights 1, 1, 6, 2: the cumulative shares are 0.1, 0.2, 0.8, 1
    x, w = np.array([[3.0], [1.0], [4.0], [2.0]]), np.array([6.0, 1.0, 2.0, 1.0])
    q = (0.05, 0.1, 0.15, 0.5, 0.8, 0.9, 1.0)
    assert list(R.weighted_quantile(x, w, q)[:, 0]) == [1.0, 1.0, 2.0, 3.0, 3.0, 4.0, 4.0]
    assert np.array_equal(weighted_quantile(x, w, q), R.weighted_quantile(x, w, q))


def test_boundary_binding():
    from gpbayestools_hic_amd import _native
    assert len(_native.BOUNDARY["gpb_chain_marginals"][1]) == 17
    import gpbayestools_hic_amd as G
    assert G.PosteriorMarginals is G.marginals.PosteriorMarginals and callable(G.marginals.marginals)
