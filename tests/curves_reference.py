"""Host model of the posterior curves (a helper module, not a test file): the numpy restatement of what gpb_chain_curves and
gpb_chain_trace_hist compute (include/gpbayes.h) — curve_value one grid point at a time, every operation
in csrc/curve_fn.h's order; exact order statistics by np.partition; the closure distance with its sequential sum; the trace
counts by np.searchsorted — and a chain builder that imitates emcee's store.  tests/test_curves_reference.py pins the model to
the notebook's own functions (tests/golden/g15_curves.npz) and to np.histogram2d."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g15_curves.npz")
ZETA, ETA, YLOSS, DELTA = 0, 1, 2, 3
NPAR = {ZETA: 4, ETA: 3, YLOSS: 3}
# (fn, col0 .. col3) of the three default curves: the reference's parameter indices
DESC20 = np.array([[ZETA, 15, 16, 17, 18], [ETA, 12, 13, 14, -1], [YLOSS, 2, 3, 4, -1]], dtype=np.int32)
GRID_RANGE = {ZETA: 0.5, ETA: 0.6, YLOSS: 6.2, DELTA: 1.0}
DELTA_ROW = np.array([[DELTA, -1, -1, -1, -1]], dtype=np.int32)
# d = 5: columns out of order and shared between the curves
DESC5 = np.array([[ZETA, 3, 1, 0, 2], [ETA, 4, 0, 2, -1], [YLOSS, 4, 0, 2, -1]], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def prior_ranges():
    """the notebook's prior box [20, 2], as the golden recorded it"""
    return np.load(GOLDEN)["prior_ranges"]


def curve_value(fn, par, g, aux=None):
    """[S]: curve fn at the ONE grid value g for the rows of par [S, 3 or 4] (fn 3: the rows of theta [S, d], aux = truth | width)"""
    par = np.asarray(par, dtype=np.float64)
    g = np.float64(g)
    if fn == ZETA:
        zmax, T0, sp, sm = par[:, 0], par[:, 1], par[:, 2], par[:, 3]
        s = np.where(g < T0, sm, sp)
        dt = g - T0
        with np.errstate(all="ignore"):
            return zmax * np.exp(-(dt * dt) / (2.0 * (s * s)))
    if fn == ETA:
        e0, e2, e4 = par[:, 0], par[:, 1], par[:, 2]
        if 0.0 <= g <= 0.2:
            return e0 + (e2 - e0) * (g / np.float64(0.2))
        if 0.2 < g < 0.4:
            return e2 + (e4 - e2) * ((g - np.float64(0.2)) / np.float64(0.2))
        return e4.copy() if g >= 0.4 else np.zeros(par.shape[0])
    if fn == YLOSS:
        y2, y4, y6 = par[:, 0], par[:, 1], par[:, 2]
        if 0.0 <= g <= 2.0:
            return y2 * (g / np.float64(2.0))
        if 2.0 < g < 4.0:
            return y2 + (y4 - y2) * ((g - np.float64(2.0)) / np.float64(2.0))
        return y4 + (y6 - y4) * ((g - np.float64(4.0)) / np.float64(2.0)) if g >= 4.0 else np.zeros(par.shape[0])
    d = par.shape[1]
    aux = np.asarray(aux, dtype=np.float64)
    acc = np.zeros(par.shape[0])
    for j in range(d):                                  # j ascending, one add after the other
        z = (par[:, j] - aux[j]) / aux[d + j]
        acc = acc + z * z
    return acc / np.float64(d)


def values(x, desc, grid, aux=None):
    """[ncurves, G, S]: v(c, g, s) for the samples x [S, d] in their order"""
    x = np.asarray(x, dtype=np.float64)
    desc, grid = np.asarray(desc).reshape(-1, 5), np.asarray(grid, dtype=np.float64)
    out = np.empty((desc.shape[0], grid.shape[1], x.shape[0]))
    for c, k in enumerate(desc):
        par = x if k[0] == DELTA else x[:, list(k[1:1 + NPAR[int(k[0])]])]
        for gi in range(grid.shape[1]):
            out[c, gi] = curve_value(int(k[0]), par, grid[c, gi], aux)
    return out


def order_stats(v, q):
    """[..., nq, 2]: v_(k), v_(min(k + 1, S - 1)) along the last axis of v, k = floor(q (S - 1)): exact, by np.partition"""
    v = np.asarray(v)
    S = v.shape[-1]
    q = np.asarray(q, dtype=np.float64).reshape(-1)
    k = np.floor(q * np.float64(S - 1)).astype(np.int64)
    k1 = np.minimum(k + 1, S - 1)
    part = np.partition(v, np.unique(np.concatenate([k, k1])), axis=-1)
    return np.stack([part[..., k], part[..., k1]], axis=-1)


def levels_q(levels=(68, 95, 99.7)):
    pct = [50.0]
    for v in levels:
        pct += [50.0 - v / 2.0, 50.0 + v / 2.0]
    return np.asarray(pct) / 100.0


def trace_counts(x3, edges):
    """(hist [d, nsteps, B], outside [d, nsteps]) of a chain [nsteps, nwalkers, d]: the bin rule of gpb_chain_marginals"""
    n, nw, d = x3.shape
    B = edges.shape[1] - 1
    hist, outside = np.zeros((d, n, B), dtype=np.int64), np.zeros((d, n), dtype=np.int64)
    for j in range(d):
        e = edges[j]
        v = x3[:, :, j]
        b = np.searchsorted(e, v, side="right") - 1
        b = np.where(v == e[B], B - 1, b)
        ok = (v >= e[0]) & (v <= e[B])                   # (NaN: neither)
        flat = (np.arange(n)[:, None] * B + b)[ok]
        hist[j] = np.bincount(flat, minlength=n * B).reshape(n, B)
        outside[j] = nw - ok.sum(axis=1)
    return hist, outside


def data_edges(x3, B):
    """[d, B + 1]: np.linspace over every parameter's extent over the whole chain, as np.histogram2d takes it"""
    lo, hi = x3.min(axis=(0, 1)), x3.max(axis=(0, 1))
    same = lo == hi
    lo, hi = np.where(same, lo - 0.5, lo), np.where(same, hi + 0.5, hi)
    return np.ascontiguousarray(np.stack([np.linspace(lo[j], hi[j], B + 1) for j in range(x3.shape[2])]))


def box(d):
    """[d, 2]: the notebook's prior box for d = 20, else a box in which every column serves as any curve parameter"""
    return prior_ranges() if d == 20 else np.tile(np.array([[0.05, 0.45]]), (d, 1))


AMPLITUDES20 = (2, 3, 4, 12, 13, 14, 15)


@functools.lru_cache(maxsize=None)
def chain(nsteps, nwalkers, d, seed=0, stay=0.6):
    """[nsteps, nwalkers, d] as emcee stores a run: a walker keeps its previous row with probability `stay` (many exact ties),
    else moves to a fresh draw from the box; one fresh row in eight carries negative amplitudes (keys of both signs)."""
    rng = np.random.default_rng(2500 + seed)
    b = box(d)
    amp = np.array(AMPLITUDES20 if d == 20 else (0, 4))

    def fresh(k):
        r = b[:, 0] + (b[:, 1] - b[:, 0]) * rng.random((k, d))
        neg = rng.random(k) < 0.125
        r[np.ix_(neg, amp)] *= -1.0
        return r
    rows = fresh(nsteps * nwalkers).reshape(nsteps, nwalkers, d)
    keep = rng.random((nsteps, nwalkers)) < stay
    keep[0] = False
    src = np.maximum.accumulate(np.where(keep, 0, np.arange(nsteps)[:, None]), axis=0)     # the step a row was last drawn at
    x = rows[src, np.arange(nwalkers)[None, :]]
    x.setflags(write=False)
    return x


def grids(desc, G):
    """[ncurves, G]: np.linspace(0, the notebook's upper end, G) per curve (G = 1: the upper end's half, inside a branch)"""
    return np.stack([np.linspace(0.0, GRID_RANGE[int(k[0])], G) if G > 1 else np.array([0.5 * GRID_RANGE[int(k[0])]])
                     for k in np.asarray(desc).reshape(-1, 5)])
