"""GPU tier: MaxPro Latin-hypercube designs — gpb_maxpro_lhd, gpb_maxpro_criterion, gpb_maxpro_run_order (GPEngine.maxpro_*)
and design.py (generate_lhs, Design) — against the host model of tests/maxpro_reference.py, whose cases
tests/test_maxpro_reference.py shows to be far from rounding (every acceptance margin >= 1e-8, asserted here again before
anything is compared)."""
import math

import numpy as np
import pytest

import maxpro_reference as M

pytestmark = pytest.mark.gpu

SUM_RTOL = 1e-12         # all terms positive, nothing cancels: (2 d + 2 + the summation depth) roundings stay under 5e-13


@pytest.fixture(scope="module")
def eng():
    from gpbayestools_hic_amd import GPEngine
    return GPEngine(0)


def _designs(n, d):
    """a random hypercube and a real design that is none"""
    rng = np.random.default_rng(1000 * n + d)
    return M.design_of(M.random_starts(n + d, 1, n, d)[0]), rng.random((n, d))


# ---------------------------------------------------------------------------------------------------------------- criterion
@pytest.mark.parametrize("n,d", [(4, 2), (7, 2), (64, 3), (65, 3), (130, 20), (20, 64), (1100, 4)])
def test_criterion_matches_brute_force(eng, n, d):
    for X in _designs(n, d):
        want = M.design_sum(X)
        lnpsi, got = eng.maxpro_criterion(X, return_sum=True)
        print(n, d, "sum rel err %.2e" % (abs(got - want) / want))
        assert abs(got - want) <= SUM_RTOL * want
        assert abs(lnpsi - M.lnpsi_from_f(math.log(want), n, d)) <= 1e-12 * max(1.0, abs(lnpsi))
        assert abs(lnpsi - M.lnpsi_bruteforce(X)) <= 1e-10 * max(1.0, abs(lnpsi))


def test_criterion_of_a_repeated_coordinate_is_inf(eng):
    X = np.random.default_rng(3).random((65, 3))
    X[40, 2] = X[7, 2]
    assert eng.maxpro_criterion(X) == np.inf


# ---------------------------------------------------------------------------------------------------------------- trajectory
def _run(eng, name, rows=None, restart0=0):
    n, d, R, B, ns, bps, temp0, cool, seed = M.CASES[name]
    init = M.case_starts(name)
    if rows is not None:
        init = init[rows]
    return eng.maxpro_lhd(init, seed, ns, bps, B, temp0, cool, restart0=restart0, return_trace=True)


@pytest.mark.parametrize("name", sorted(M.CASES))
def test_trajectory_matches_the_host_model(eng, name):
    n, d, R, B = M.CASES[name][:4]
    ref = M.case_reference(name)
    for m in ref:                                                  # the condition of the comparison: never skipped
        assert m["margin"] >= M.MIN_MARGIN and m["best_margin"] >= M.MIN_BEST_MARGIN
    if name in M.PATH_CASES:
        assert M.trace_paths(name) == (True, True, True)
    elif name == "hot":
        assert all(np.all(m["trace"] == 0) for m in ref)
    out = _run(eng, name)
    for r, m in enumerate(ref):
        assert np.array_equal(out["trace"][r], m["trace"]), (r, np.flatnonzero(out["trace"][r] != m["trace"])[:5])
        assert out["accepted"][r] == m["accepted"] and out["consumed"][r] == m["consumed"]
        assert np.array_equal(out["levels"][r], m["levels"])
        s_ref = M.levels_sum(m["levels"])
        # f = ln of the sum: an absolute error of f is a relative error of the sum (|f| < 1024, so f itself resolves 2.3e-13)
        print(name, r, "f_best - ln(sum of the model's levels) = %.2e" % (out["f_best"][r] - math.log(s_ref)))
        assert abs(out["f_best"][r] - math.log(s_ref)) <= SUM_RTOL and abs(out["f_start"][r] - m["f_start"]) <= SUM_RTOL
        assert abs(out["lnpsi"][r] - M.lnpsi(M.design_of(m["levels"]))) <= 1e-12 * max(1.0, abs(out["lnpsi"][r]))
    if name == "cold":
        assert np.all(out["f_best"] < out["f_start"])


# ---------------------------------------------------------------------------------------------------------------- independence
def test_a_restart_depends_on_its_start_and_index_alone(eng):
    name = "n130_d20_R3_B32"
    all3 = _run(eng, name)
    again = _run(eng, name)
    for k in all3:
        assert np.array_equal(all3[k], again[k]), k
    for r in range(3):
        one = _run(eng, name, rows=slice(r, r + 1), restart0=r)
        for k in all3:
            assert np.array_equal(all3[k][r], one[k][0]), (r, k)
    other = _run(eng, name, rows=slice(0, 1), restart0=1)            # (the index does enter the draws)
    assert not np.array_equal(other["trace"][0], all3["trace"][0])


# ---------------------------------------------------------------------------------------------------------------- run order
@pytest.mark.parametrize("n,d", [(7, 2), (65, 3), (130, 20)])
def test_run_order_matches_the_host_model(eng, n, d):
    X = _designs(n, d)[0]
    for first in (-1, n // 3):
        want, margin = M.run_order(X, first)
        assert margin >= 1e-9
        got = eng.maxpro_run_order(X, first)
        assert np.array_equal(got, want) and got[0] == (M.centre_row(X) if first < 0 else first)


def test_run_order_gives_an_exact_tie_to_the_lower_index(eng):
    want, margin = M.run_order(M.TIE_DESIGN, 1)
    assert margin == 0.0
    assert np.array_equal(eng.maxpro_run_order(M.TIE_DESIGN, 1), want)


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_engine_usable(eng):
    from gpbayestools_hic_amd import _native as nat
    good = M.random_starts(1, 1, 9, 3)

    def raw(init, n, d, R=1, B=4, ns=1, bps=2, temp0=0.1, cool=0.5):
        init = np.ascontiguousarray(init, dtype=np.int32)
        lev = np.empty_like(init)
        f = np.empty((2, max(R, 1)))
        cnt = np.empty((2, max(R, 1)), dtype=np.int64)
        rc = eng.lib.gpb_maxpro_lhd(eng.h, n, d, R, 0, nat.ptr(init), 5, ns, bps, B, temp0, cool, nat.ptr(lev), nat.ptr(f[0]), nat.ptr(f[1]),
                                    nat.ptr(cnt[0]), nat.ptr(cnt[1]), None)
        return rc, eng.lib.gpb_last_error(eng.h).decode()

    assert raw(good, 9, 3)[0] == 0
    bad = good.copy()
    bad[0, 4, 1] = bad[0, 5, 1]
    wide = np.repeat(np.arange(1200, dtype=np.int32)[None, :, None], 64, axis=2)     # every row adjacent to the next in every column
    cases = [(raw(bad, 9, 3), "permutation"), (raw(np.zeros((1, 9, 1)), 9, 1), "d outside"), (raw(np.zeros((1, 3, 3)), 3, 3), "n outside"),
             (raw(np.zeros((1, 8, 2)), 4097, 2), "n outside"), (raw(np.zeros((1, 8, 2)), 8, 65), "d outside"),
             (raw(good, 9, 3, B=0), "block outside"), (raw(good, 9, 3, B=65), "block outside"), (raw(good, 9, 3, R=0), "R outside"),
             (raw(good, 9, 3, R=17), "R outside"), (raw(good, 9, 3, temp0=0.0), "temp0"), (raw(good, 9, 3, ns=0), "n_stages"),
             (raw(wide, 1200, 64), "not finite")]
    for (rc, msg), what in cases:
        assert rc == -1 and "gpb_maxpro_lhd" in msg and what in msg, (rc, msg, what)
    for call in (lambda: eng.maxpro_lhd(bad, 5, 1, 2), lambda: eng.maxpro_lhd(np.zeros((1, 9, 1), dtype=np.int32), 5, 1, 2),
                 lambda: eng.maxpro_lhd(np.zeros((1, 3, 3), dtype=np.int32), 5, 1, 2), lambda: eng.maxpro_lhd(good, 5, 1, 2, block=0),
                 lambda: eng.maxpro_lhd(np.zeros((1, 4097, 2), dtype=np.int32), 5, 1, 2),
                 lambda: eng.maxpro_lhd(np.zeros((1, 8, 65), dtype=np.int32), 5, 1, 2),
                 lambda: eng.maxpro_criterion(np.zeros((3, 3))), lambda: eng.maxpro_run_order(np.zeros((9, 1))),
                 lambda: eng.maxpro_run_order(M.TIE_DESIGN, 7)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(nat.GPBError, match="not finite"):
        eng.maxpro_lhd(wide, 5, 1, 2)
    X = M.TIE_DESIGN
    rc = eng.lib.gpb_maxpro_criterion(eng.h, nat.ptr(X), 7, 1, nat.ptr(np.zeros(1)), None)
    assert rc == -1 and "d outside" in eng.lib.gpb_last_error(eng.h).decode()
    rc = eng.lib.gpb_maxpro_run_order(eng.h, nat.ptr(X), 7, 2, 7, nat.ptr(np.zeros(7, dtype=np.int32)))
    assert rc == -1 and "first outside" in eng.lib.gpb_last_error(eng.h).decode()
    out = eng.maxpro_lhd(good, 5, 1, 2, block=4, temp0=0.1, cool=0.8)                    # and the engine still works
    assert M.anneal(good[0], 5, 0, 1, 2, 4, 0.1, 0.8)["margin"] >= M.MIN_MARGIN
    assert np.array_equal(out["levels"][0], M.anneal(good[0], 5, 0, 1, 2, 4, 0.1, 0.8)["levels"])


# ---------------------------------------------------------------------------------------------------------------- end to end
def test_generate_lhs_and_design_end_to_end(eng, tmp_path):
    from gpbayestools_hic_amd import design as D
    n, d, seed = 64, 6, 17
    cache = tmp_path / "cache" / "lhs"
    lhs = D.generate_lhs(n, d, seed, cache_dir=cache)
    assert lhs.shape == (n, d + 1) and lhs.dtype == np.float64 and np.array_equal(lhs[:, 0], np.arange(1, n + 1))
    for c in range(1, d + 1):
        assert np.array_equal(np.sort(lhs[:, c]), (np.arange(n) + 0.5) / n)
    assert (cache / "npoints64_ndim6_seed17.npy").exists()
    res = D.maxpro_design(n, d, seed, eng=eng)
    assert np.array_equal(res.design, lhs[:, 1:]) and sorted(res.order) == list(range(n))
    assert res.lnpsi[res.best] < res.lnpsi_start[res.best] and res.best == int(np.argmin(res.lnpsi))
    assert abs(D.maxpro_criterion(lhs[:, 1:], eng=eng) - res.lnpsi[res.best]) < 1e-12 * abs(res.lnpsi[res.best])
    assert np.array_equal(D.run_order(res.design, eng=eng), np.arange(n))       # (already in run order)
    marker = lhs.copy()
    marker[0, 1] = -1.0
    np.save(cache / "npoints64_ndim6_seed17.npy", marker)          # a second call loads the cache, whatever it holds
    assert np.array_equal(D.generate_lhs(n, d, seed, cache_dir=cache), marker)
    np.save(cache / "npoints64_ndim6_seed17.npy", lhs)
    par = tmp_path / "pars.txt"
    par.write_text("".join("p%d: $p_%d$, %g, %g  # a parameter\n" % (k, k, -1.0 - k, 2.0 * k + 0.5) for k in range(d)))
    des = D.Design(par, npoints=n, seed=seed, cache_dir=cache)
    lo, hi = des.min, des.max
    assert des.ndim == d and des.array.shape == (n, d) and np.all(des.array > lo) and np.all(des.array < hi)
    assert np.array_equal(des.array, lo + (hi - lo) * lhs[:, 1:]) and np.array_equal(np.asarray(des), des.array)
