"""CPU tier of the posterior curves (gpb_chain_curves, gpb_chain_trace_hist): the host model of
tests/curves_reference.py, and the package's own host functions (curves.py), against what examples/PlotMCMC.ipynb's functions
gave for 48 samples (tests/golden/g15_curves.npz, written by tools/make_goldens.py g15_curves) and against np.histogram2d; the
boundary binding of the two entry points."""
import os
import re

import numpy as np
import pytest

import curves_reference as R
from conftest import REPO, golden

NAMES = {"zeta": ("zeta_over_s", 0), "eta": ("eta_over_s", 1), "yloss": ("y_loss", 2)}


@pytest.fixture(scope="module")
def g15():
    return golden("g15_curves.npz")


@pytest.mark.parametrize("key", ["eta", "yloss", "zeta"])
def test_model_curves_and_percentiles_are_the_notebooks(g15, key):
    """the model's [S, 100] curves and their median / 68 / 95 / 99.7 % percentiles (exact order statistics + numpy's
    interpolation rule) equal the notebook's bit for bit — zeta/s too: both sides take numpy's exp"""
    from gpbayestools_hic_amd.emulator import percentile_from_order
    name, row = NAMES[key]
    x, grid = g15["samples"], g15[key + "_grid"]
    v = R.values(x, R.DESC20[row:row + 1], grid[None, :])[0]                    # [G, S]
    assert np.array_equal(v.T, g15[key + "_curves"])
    q = R.levels_q(g15["levels"])
    pct = percentile_from_order(R.order_stats(v, q), q, x.shape[0])             # [G, nq]
    assert np.array_equal(pct.T, g15[key + "_pct"])


@pytest.mark.parametrize("key", ["eta", "yloss", "zeta"])
def test_package_host_functions_are_the_notebooks(g15, key):
    from gpbayestools_hic_amd import curves as C
    name, row = NAMES[key]
    spec = C.CURVES[name]
    assert spec["fn"] == row and list(spec["columns"]) == [c for c in R.DESC20[row, 1:] if c >= 0]
    assert np.array_equal(spec["grid"], g15[key + "_grid"])
    assert np.array_equal(C.curve_on_host(name, g15["samples"], spec["columns"], spec["grid"]), g15[key + "_curves"])
    assert np.array_equal(C.curve_on_host(name, g15["truth"][None, :], spec["columns"], spec["grid"])[0], g15[key + "_truth"])


def test_closure_distance_against_the_notebooks_sum(g15):
    """the sequential sum over j is within (d + 2) 2^-53 relative of the notebook's np.sum form: the worst case of reordering d
    non-negative terms"""
    from gpbayestools_hic_amd import curves as C
    x, truth, pr = g15["samples"], g15["truth"], g15["prior_ranges"]
    d = x.shape[1]
    width = pr[:, 1] - pr[:, 0]
    want = g15["Delta_d_distribution"]
    for got in (R.curve_value(R.DELTA, x, 0.0, np.concatenate([truth, width])), C.closure_distance(x, truth, width)):
        assert np.max(np.abs(got - want) / want) <= (d + 2) * 2.0 ** -53
    # Delta_d is the distances' mean: two summation orders of S non-negative terms, each within (S + 2) 2^-53 of the exact sum
    assert abs(np.mean(want) - float(g15["Delta_d"])) <= 2 * (x.shape[0] + 2) * 2.0 ** -53 * float(g15["Delta_d"])


@pytest.mark.parametrize("n", [1, 2, 7, 64])
def test_trace_counts_are_histogram2d(n):
    """np.histogram2d(step, value, bins=[n, 30]) per parameter, as plot_chain_histogram calls it on the [nwalkers, nsteps]
    values: step t lands in bin t, the values in the model's bins"""
    nw, d, B = 9, 5, 30
    x3 = R.chain(n, nw, d, seed=n)
    hist, outside = R.trace_counts(x3, R.data_edges(x3, B))
    assert not outside.any()
    xw = x3.transpose(1, 0, 2)                                                   # [nwalkers, nsteps, d]
    for j in range(d):
        h2, xe, ye = np.histogram2d(np.tile(np.arange(n), nw), xw[:, :, j].reshape(-1), bins=[n, B])
        assert np.array_equal(h2.astype(np.int64), hist[j])
        assert np.array_equal(ye, R.data_edges(x3, B)[j])


def test_order_stats_and_chain_builder():
    x = R.chain(64, 4, 20)
    flat = x.reshape(-1, 20)
    assert len(np.unique(flat, axis=0)) < flat.shape[0] // 2                     # exact ties
    v = R.values(flat, R.DESC20, R.grids(R.DESC20, 7))
    assert (v < 0).any() and (v > 0).any()                                       # keys of both signs
    q = np.array([0.0, 1.0, 0.5, 0.999999])
    o = R.order_stats(v, q)
    s = np.sort(v, axis=-1)
    S = flat.shape[0]
    assert np.array_equal(o[..., 0, :], np.stack([s[..., 0], s[..., 1]], -1))
    assert np.array_equal(o[..., 1, :], np.stack([s[..., S - 1], s[..., S - 1]], -1))
    assert np.array_equal(o[..., 3, :], np.stack([s[..., S - 2], s[..., S - 1]], -1))


def test_boundary_binding():
    from gpbayestools_hic_amd import _native
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "gpbayes.h")).read(), flags=re.S)
    for name in ("gpb_chain_curves", "gpb_chain_trace_hist"):
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, txt)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(_native.BOUNDARY[name][1]), name
