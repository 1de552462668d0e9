"""Host model of the chain marginals (a helper module, not a test file): the numpy restatement of what gpb_chain_marginals counts.
A value's code is its bin by np.searchsorted on the edges with the right-edge rule (e[b] <= x < e[b + 1], the last bin closed,
everything else — NaN included — 255 = outside); the counts are np.add.at of integer weights (1, or rint(w 2^32 / max w) clamped to
[0, 2^32]); plus the credible-level thresholds and the weighted quantile of gpbayestools_hic_amd/marginals.py restated."""
import functools

import numpy as np

OUT = 255
TWO32 = 4294967296.0

# (nsteps, nwalkers, ndim, bins) of the GPU tests: one value; below one wave with an odd B; a few workgroup strides; 66 pairs at
# B = 64 (more B x B tables than one workgroup keeps); a flat set whose size is no multiple of anything.  The last two are
# beyond the list the feature was specified with: 40 parameters at B = 64 are two parameter chunks of the coding kernel
SHAPES = ((1, 1, 1, 1), (7, 3, 2, 7), (65, 5, 5, 20), (257, 16, 12, 64), (4099, 1, 20, 20), (33, 2, 40, 64))


def codes(x, edges):
    """[..., d] uint8 codes of x [..., d] in edges [d, B + 1]"""
    x = np.asarray(x, dtype=np.float64)
    edges = np.asarray(edges, dtype=np.float64)
    B = edges.shape[1] - 1
    c = np.full(x.shape, OUT, dtype=np.uint8)
    for j in range(x.shape[-1]):
        e, v = edges[j], x[..., j]
        b = np.searchsorted(e, v, side="right") - 1          # e[b] <= v < e[b + 1]; v < e[0]: -1; v >= e[B] or NaN: B
        b = np.where(v == e[B], B - 1, b)                    # the last bin is closed
        ok = (b >= 0) & (b < B) & ~np.isnan(v)
        c[..., j] = np.where(ok, b, OUT).astype(np.uint8)
    return c


def all_pairs(d):
    return np.array([(i, j) for i in range(d) for j in range(i + 1, d)], dtype=np.int32).reshape(-1, 2)


def int_weights(w, wscale=None):
    """q [S] int64: rint(w wscale) clamped to [0, 2^32], NaN -> 0; wscale defaults to 2^32 / max w"""
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    if wscale is None:
        wscale = TWO32 / float(np.max(w))
    with np.errstate(invalid="ignore"):
        z = np.rint(w * wscale)
    z = np.where(np.isnan(z), 0.0, np.clip(z, 0.0, TWO32))
    return z.astype(np.int64)


def counts(x, edges, pairs=None, q=None):
    """(h1 [d, B], h2 [npairs, B, B], outside [d]) int64 of the samples x [S, d] (any leading axes are flattened), q [S] the
    integer weights (default 1)"""
    edges = np.asarray(edges, dtype=np.float64)
    d, B = edges.shape[0], edges.shape[1] - 1
    c = codes(np.asarray(x, dtype=np.float64).reshape(-1, d), edges).astype(np.int64)
    S = c.shape[0]
    q = np.ones(S, dtype=np.int64) if q is None else np.asarray(q, dtype=np.int64)
    pairs = all_pairs(d) if pairs is None else np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    h1 = np.zeros((d, B), dtype=np.int64)
    outside = np.zeros(d, dtype=np.int64)
    h2 = np.zeros((len(pairs), B, B), dtype=np.int64)
    for j in range(d):
        ok = c[:, j] != OUT
        np.add.at(h1[j], c[ok, j], q[ok])
        outside[j] = q[~ok].sum()
    for p, (i, j) in enumerate(pairs):
        ok = (c[:, i] != OUT) & (c[:, j] != OUT)
        np.add.at(h2[p], (c[ok, i], c[ok, j]), q[ok])
    return h1, h2, outside


def credible_levels(tile, levels=(0.68, 0.95)):
    """count thresholds of the highest-density regions of a B x B table: counts sorted descending, the count of the first bin at
    which the cumulative count reaches level * total"""
    c = np.sort(np.asarray(tile).reshape(-1))[::-1]
    cum = np.cumsum(c)
    out = []
    for lv in np.atleast_1d(levels):
        if cum[-1] == 0:
            out.append(0)
            continue
        k = 0
        while k < len(c) - 1 and cum[k] < lv * float(cum[-1]):
            k += 1
        out.append(c[k])
    return np.array(out)


def weighted_quantile(x, w, q):
    """[nq, d]: the smallest sample of each column whose cumulative normalised weight reaches q"""
    x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    out = np.empty((len(q), x.shape[1]))
    for j in range(x.shape[1]):
        o = np.argsort(x[:, j], kind="stable")
        cw = np.cumsum(w[o])
        for a, lv in enumerate(q):
            k = 0
            while k < len(o) - 1 and cw[k] < lv * cw[-1]:
                k += 1
            out[a, j] = x[o[k], j]
    return out


def edges_of(d, B, lo=-2.0, hi=2.0, uniform=True, seed=0):
    """[d, B + 1]: np.linspace(lo - 0.1 j, hi + 0.2 j, B + 1) per parameter, or (uniform=False) sorted random cuts of it"""
    rng = np.random.default_rng(100 + seed)
    rows = []
    for j in range(d):
        a, b = lo - 0.1 * j, hi + 0.2 * j
        if uniform:
            rows.append(np.linspace(a, b, B + 1))
        else:
            cuts = np.sort(rng.uniform(a, b, B - 1)) if B > 1 else np.empty(0)
            rows.append(np.concatenate([[a], cuts, [b]]))
    e = np.array(rows)
    assert np.all(np.diff(e, axis=1) > 0)
    return e


@functools.lru_cache(maxsize=None)
def chain(n, nw, d, seed=3):
    """a read-only synthetic chain [n, nw, d]: standard normal draws scaled so that a few per cent fall outside edges_of's box"""
    x = np.random.default_rng(seed).standard_normal((n, nw, d)) * 1.1
    x.setflags(write=False)
    return x


def planted(edges, seed=4):
    """[S, d]: every edge of every parameter with its two neighbours one ulp away, values far outside on both sides, NaN and
    both infinities, in a shuffled order per column"""
    rng = np.random.default_rng(seed)
    cols = []
    for e in np.asarray(edges, dtype=np.float64):
        v = np.concatenate([e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf),
                            [e[0] - 1.0, e[-1] + 1.0, np.nan, np.inf, -np.inf, 0.5 * (e[0] + e[-1])]])
        cols.append(rng.permutation(v))
    return np.stack(cols, axis=1)
