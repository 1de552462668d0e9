"""CPU tier of the MaxPro Latin-hypercube generator (gpb_maxpro_lhd): the host model of
tests/maxpro_reference.py against itself — the ratio update against a recomputation, permutations, B = 1 against textbook
sequential annealing, the invariances of ln psi, the proposal decoding — and the conditions under which tests/test_gpu_maxpro.py
may compare its cases with the device bit for bit."""
import math
import os
import re

import numpy as np
import pytest

import maxpro_reference as M
from conftest import REPO


def _is_lhd(levels):
    n = levels.shape[0]
    return np.array_equal(np.sort(levels, axis=0), np.broadcast_to(np.arange(n)[:, None], levels.shape))


def test_ratio_update_matches_recomputation_after_every_accepted_swap():
    n, d = 23, 4
    start = M.random_starts(5, 1, n, d)[0]
    seen = []

    def check(T, S, lev):
        T2 = M.pair_matrix(lev, M.scale(n))
        assert np.allclose(T, T2, rtol=1e-12, atol=0.0) and np.array_equal(T, T.T)
        assert abs(S - M.pair_sum(T2)) <= 1e-12 * S
        assert _is_lhd(lev)
        seen.append(S)

    out = M.anneal(start, 7, 0, 3, 40, 4, 0.1, 0.5, check=check)
    assert len(seen) == out["accepted"] > 20
    assert _is_lhd(out["levels"]) and out["f_best"] <= out["f_start"]
    assert abs(out["f_best"] - math.log(min(seen + [math.exp(out["f_start"])]))) < 1e-10
    tr = out["trace"]
    assert out["consumed"] == int(np.sum(np.where(tr < 0, 4, tr + 1))) and out["accepted"] == int(np.sum(tr >= 0))


def test_block_of_one_is_textbook_sequential_annealing():
    n, d, steps, temp = 11, 3, 120, 0.1
    start = M.random_starts(3, 1, n, d)[0]
    out = M.anneal(start, 21, 2, 1, steps, 1, temp, 1.0)
    assert out["margin"] > 1e-9
    lev, flags = M.sequential_anneal(start, 21, 2, steps, temp)
    assert np.array_equal(flags, out["trace"] == 0) and 5 < flags.sum() < steps
    # (the textbook loop ends on the current state, the generator returns the best it has seen)
    assert M.levels_sum(out["levels"]) <= M.levels_sum(lev) * (1 + 1e-12)


def test_lnpsi_scale_and_invariances():
    rng = np.random.default_rng(0)
    for n, d in ((4, 2), (9, 3), (30, 7), (12, 64)):
        lev = M.random_starts(n + d, 1, n, d)[0]
        X = M.design_of(lev)
        a = M.lnpsi(X)
        assert abs(a - M.lnpsi_bruteforce(X)) < 1e-11 * max(1.0, abs(a))
        assert abs(a - M.lnpsi_from_f(math.log(M.levels_sum(lev)), n, d)) < 1e-12 * max(1.0, abs(a))
        assert abs(a - M.lnpsi(X[rng.permutation(n)][:, rng.permutation(d)])) < 1e-12 * max(1.0, abs(a))
    X = rng.random((8, 3))
    X[5, 1] = X[2, 1]
    assert M.lnpsi(X) == np.inf


def test_proposal_decoding_ranges_and_coverage():
    for n, d in ((4, 2), (7, 3), (65, 64), (4096, 20)):
        c, a, b, u = M.proposals(99, np.arange(4000)[:, None] % 4000, 3, 64, n, d)
        assert np.all(a != b) and a.min() >= 0 and a.max() < n and b.min() >= 0 and b.max() < n
        assert c.min() == 0 and c.max() == d - 1 and len(np.unique(c)) == d
        assert np.all(u > 0.0) and np.all(u < 1.0)
        if n <= 65:
            assert len(np.unique(a)) == n and len(np.unique(b)) == n
    # the corners of the word range
    top = 0xFFFFFFFF
    c, a, b, u = M.decode([0, top, top, 0], [0, top, 0, top], [0, top, top, 0], [0, top, 0, top], 7, 3)
    assert list(c) == [0, 2, 2, 0] and list(a) == [0, 6, 0, 6] and list(b) == [1, 5, 6, 0]
    assert u[0] == 0.5 / 2 ** 32 and u[1] == 1.0 - 0.5 / 2 ** 32


def test_header_constants_are_restated():
    txt = open(os.path.join(REPO, "gpbayestools_hic_amd", "csrc", "maxpro_index.h")).read()
    assert float(re.search(r"MP_E15 = ([0-9.]+)", txt).group(1)) == M.E15 == math.exp(1.5)
    assert int(re.search(r"MP_TAG = (\d+)", txt).group(1)) == M.TAG
    assert float(re.search(r"MP_BEST_EPS = ([0-9.e-]+)", txt).group(1)) == M.BEST_EPS
    lim = re.search(r"MP_MIN_N = (\d+), MP_MAX_N = (\d+), MP_MIN_D = (\d+), MP_MAX_D = (\d+), MP_MAX_R = (\d+), MP_MAX_BLOCK = (\d+)", txt)
    assert tuple(int(v) for v in lim.groups()) == (M.MIN_N, M.MAX_N, M.MIN_D, M.MAX_D, M.MAX_R, M.MAX_BLOCK)
    philox = open(os.path.join(REPO, "gpbayestools_hic_amd", "csrc", "philox.h")).read()
    assert "11 the swap proposals" in philox


def test_binding_matches_the_header():
    from gpbayestools_hic_amd import _native
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "gpbayes.h")).read(), flags=re.S)
    for name in ("gpb_maxpro_lhd", "gpb_maxpro_criterion", "gpb_maxpro_run_order"):
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, txt)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(_native.BOUNDARY[name][1]), name


@pytest.mark.parametrize("name", sorted(M.CASES))
def test_gpu_cases_are_far_from_rounding(name):
    """what tests/test_gpu_maxpro.py relies on: no decision of a case is nearer to its threshold than MIN_MARGIN (the device's f
    carries about 1e-13), and the first five cases walk all three paths of a block"""
    res = M.case_reference(name)
    for m in res:
        assert m["margin"] >= M.MIN_MARGIN and m["best_margin"] >= M.MIN_BEST_MARGIN, (m["margin"], m["best_margin"])
        assert _is_lhd(m["levels"])
    if name in M.PATH_CASES:
        assert M.trace_paths(name) == (True, True, True)
    elif name == "hot":
        assert all(np.all(m["trace"] == 0) for m in res)
    else:
        assert all(m["f_best"] < m["f_start"] for m in res)


def test_run_order_model():
    X = M.design_of(M.random_starts(8, 1, 9, 2)[0])
    order, margin = M.run_order(X)
    assert sorted(order) == list(range(9)) and order[0] == M.centre_row(X) and margin > 0
    T = M.pair_matrix(X, M.E15)
    for k in range(1, 9):
        rest = [j for j in range(9) if j not in order[:k]]
        assert order[k] == min(rest, key=lambda j: (T[order[:k], j].sum(), j))
    # a design that is symmetric about the centre row: every mirror pair ties exactly at the first step, the lower index is taken
    order, margin = M.run_order(M.TIE_DESIGN, first=1)
    t1 = M.pair_matrix(M.TIE_DESIGN, M.E15)[1]
    low = sorted(t1[[0, 2, 3, 4, 5, 6]])
    assert margin == 0.0 and low[0] == low[1] and order[0] == 1
    assert order[1] == min(j for j in (0, 2, 3, 4, 5, 6) if t1[j] == low[0])
