"""GPU tier: goodness of fit on the device — gpb_gof_accumulate, gpb_chi2_sf, gpb_gof_influence (GPEngine.gof_accumulate /
gof_unpack / chi2_sf / gof_influence) and Chain.goodness_of_fit — against the host model of tests/gof_reference.py.

Bars.  chi2, ll, logdet and z of a row: err(A) = max |A - A_longdouble| / max |A_longdouble| over the rows of a case, with
err(device) <= max(8 err(scipy fp64 route), 64 2^-53) (sens_reference.f_bar).  p: relative error against mpmath at the device's own
chi2 <= the bar of tests/test_chi2_sf_host.py, max(8 x scipy gammaincc's worst error on that test's grid, 64 2^-53)
(gof_reference.host_sf_bar), wherever the true Q >= 1e-290.  Weighted sums: 1e-13 sum wt
|term| (a tree of depth <= 16 + 16 + 3 plus each term's rounding, ~4e-15, with a margin of 25).  Slabs against one call, a bad row
against a weightless one, an emulator alone against the same emulator among others: bit equality."""
import functools
import os

import numpy as np
import pytest
import scipy.special

import gof_reference as R

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -2


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _util():
    from gpbayestools_hic_amd import GPEngine
    return GPEngine(0)


def _dev(a):
    torch, dev = _torch()
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), device=dev)


def _case(W, M, seed, jitter=1e-6):
    _, y, C, _ = R.spd_case(W, M, 1, seed, jitter)
    rng = np.random.default_rng(seed + 1)
    return y, C, rng.uniform(0.5, 2.0, M), np.diag(rng.uniform(0.1, 1.0, M))


def _run(y, C, yexp, Cadd, wt=None, splits=None):
    """(unpacked sums, acc, cnt, chi2 [W], ll [W]) of the rows, accumulated in the slabs `splits` (row counts; default one call)"""
    torch, dev = _torch()
    eng = _util()
    W, M = y.shape
    acc = torch.zeros(eng.gof_acc_doubles(M), dtype=torch.float64, device=dev)
    cnt = torch.zeros(2, dtype=torch.int64, device=dev)
    chi2 = torch.full((W,), 7.0, dtype=torch.float64, device=dev)
    ll = torch.full((W,), 7.0, dtype=torch.float64, device=dev)
    yd, Cd = _dev(yexp), _dev(Cadd)
    i0 = 0
    for n in splits or [W]:
        i1 = i0 + n
        eng.gof_accumulate(_dev(y[i0:i1]), _dev(C[i0:i1]), yd, Cd, None if wt is None else _dev(wt[i0:i1]), chi2[i0:i1], ll[i0:i1],
                           acc, cnt)
        i0 = i1
    assert i0 == W
    return eng.gof_unpack(acc, cnt, M), acc.cpu().numpy(), cnt.cpu().numpy(), chi2.cpu().numpy(), ll.cpu().numpy()


def _lds_edge():
    from gpbayestools_hic_amd import GPEngine
    return max(m for m in range(1, 400) if GPEngine.gof_path(m) == "lds")


def _p_errors(p, chi2, M):
    """(worst relative error of p against mpmath at chi2, scipy's worst on the same inputs) over the entries with Q >= 1e-290"""
    e_dev = e_ref = 0.0
    for pv, c in zip(p, chi2):
        e, true = R.sf_relerr(pv, c, M)
        if true >= 1e-290:
            e_dev = max(e_dev, e)
            e_ref = max(e_ref, R.sf_relerr(float(scipy.special.gammaincc(M / 2.0, c / 2.0)), c, M)[0])
        else:
            assert 0.0 <= pv <= 1e-289
    return e_dev, e_ref


# ---------------------------------------------------------------------------- 1. accuracy of a row
def _shapes():
    Me = _lds_edge()
    return [1, 2, 17, 33, 64, Me, Me + 1, 130]


@pytest.mark.parametrize("idx", range(8))
def test_row_accuracy(idx):
    """W = 5 rows of C = B B^T + 1e-6 tr / M I plus a diagonal Cadd, every row on its own (one call per row: acc then holds the
    row's z and p themselves, no sum enters).  chi2, ll and z against the long-double model as one array per case, at f_bar of
    the scipy route's error.  logdet from a second call per row with y = yexp: chi2 is then exactly 0 and ll = -logdet / 2 without
    a rounding of its own (in the first call -2 ll - chi2 would carry the rounding of ll, 2^-53 |ll|, which exceeds the bar on
    logdet wherever chi2 >> logdet).  p against mpmath at the device's chi2.
    Measured ratios err(device) / err(scipy), profiles/gof_accuracy.txt: chi2, ll and z 0.15 to 1.94; logdet up to 9.2 at M = 64,
    where scipy's error is 6.5e-17 and the bar is its floor, 64 2^-53.  p: 1.2e-14 at worst (M = 64), bar 3.6e-12."""
    from gpbayestools_hic_amd import GPEngine
    M = _shapes()[idx]
    if idx in (5, 6):
        assert GPEngine.gof_path(M) == ("lds" if idx == 5 else "global")
    y, C, yexp, Cadd = _case(5, M, 2000 + idx)
    r = R.rows(y, C, yexp, Cadd)
    assert not r["bad"].any() and not r["bad64"].any()
    zd, chi2d, lld, ldd, pd = np.zeros((5, M)), np.zeros(5), np.zeros(5), np.zeros(5), np.zeros(5)
    for w in range(5):
        u, _, cnt, c2, ll = _run(y[w:w + 1], C[w:w + 1], yexp, Cadd)
        assert cnt.tolist() == [1, 0] and u["wsum"] == 1.0
        zd[w], chi2d[w], lld[w], pd[w] = u["z"], c2[0], ll[0], u["p"]
        assert np.array_equal(u["z_sq"], u["z"] * u["z"]) and np.array_equal(u["pull_sq"], u["pull"] * u["pull"])
        assert np.array_equal(u["pull"], r["pull"][w])
        u0, _, _, c0, l0 = _run(yexp[None, :], C[w:w + 1], yexp, Cadd)
        assert c0[0] == 0.0 and u0["p"] == 1.0 and not u0["z"].any()
        ldd[w] = -2.0 * l0[0]
    lines = []
    for name, got, want, ref64 in (("chi2", chi2d, r["chi2"], r["chi2_64"]), ("ll", lld, r["ll"], r["ll64"]),
                                   ("logdet", ldd, r["logdet"], r["logdet64"]), ("z", zd, r["z"], r["z64"])):
        e_dev, e_ref = R.err(got, want), R.err(ref64, want)
        lines.append("M=%d path=%s %s err_device=%.3e err_scipy=%.3e ratio=%.2f bar=%.3e"
                     % (M, GPEngine.gof_path(M), name, e_dev, e_ref, e_dev / e_ref if e_ref > 0 else float("inf"), R.f_bar(e_ref)))
        print(lines[-1])
    e_p, e_p_ref = _p_errors(pd, chi2d, M)
    lines.append("M=%d path=%s p err_device=%.3e err_scipy=%.3e (on these inputs) bar=%.3e"
                 % (M, GPEngine.gof_path(M), e_p, e_p_ref, R.host_sf_bar()))
    print(lines[-1])
    out = os.environ.get("GPB_GOF_ACCURACY_OUT")            # (the record in profiles/gof_accuracy.txt is made this way)
    if out:
        with open(out, "a") as f:
            f.write("\n".join(lines) + "\n")
    for name, got, want, ref64 in (("chi2", chi2d, r["chi2"], r["chi2_64"]), ("ll", lld, r["ll"], r["ll64"]),
                                   ("logdet", ldd, r["logdet"], r["logdet64"]), ("z", zd, r["z"], r["z64"])):
        assert R.err(got, want) <= R.f_bar(R.err(ref64, want)), (name, lines)
    assert e_p <= R.host_sf_bar(), lines[-1]


def test_both_paths_are_taken():
    from gpbayestools_hic_amd import GPEngine
    paths = [GPEngine.gof_path(M) for M in _shapes()]
    assert paths == ["lds"] * 6 + ["global"] * 2


# ---------------------------------------------------------------------------- 2. slab independence
def test_slabs_give_the_bits_of_one_call():
    torch, dev = _torch()
    eng = _util()
    from gpbayestools_hic_amd import _native as nat
    y, C, yexp, Cadd = _case(600, 17, 11)
    wt = np.random.default_rng(12).uniform(0.0, 2.0, 600)
    for weights in (None, wt):
        _, a1, c1, x1, l1 = _run(y, C, yexp, Cadd, weights)
        assert c1.tolist() == [600, 0] and np.isfinite(x1).all() and np.isfinite(l1).all()
        for splits in ((256, 344), (512, 88)):
            _, a, c, x, l = _run(y, C, yexp, Cadd, weights, splits)
            assert np.array_equal(a, a1) and np.array_equal(c, c1) and np.array_equal(x, x1) and np.array_equal(l, l1), splits
    # the split [100, 500]: the second call does not start on a chunk boundary, is refused and writes nothing
    acc = torch.zeros(eng.gof_acc_doubles(17), dtype=torch.float64, device=dev)
    cnt = torch.zeros(2, dtype=torch.int64, device=dev)
    out = torch.full((2, 600), 7.0, dtype=torch.float64, device=dev)
    yd, Cd = _dev(yexp), _dev(Cadd)
    eng.gof_accumulate(_dev(y[:100]), _dev(C[:100]), yd, Cd, None, out[0, :100], out[1, :100], acc, cnt)
    a0, c0, o0 = acc.cpu().numpy(), cnt.cpu().numpy(), out.cpu().numpy()
    Cs = _dev(C[100:])
    rc = eng.lib.gpb_gof_accumulate(eng.h, 500, 17, nat.ptr(_dev(y[100:])), nat.ptr(Cs), nat.ptr(yd), nat.ptr(Cd), None,
                                    nat.ptr(out[0, 100:]), nat.ptr(out[1, 100:]), nat.ptr(acc), nat.ptr(cnt))
    assert rc == E_STATE
    assert np.array_equal(acc.cpu().numpy(), a0) and np.array_equal(cnt.cpu().numpy(), c0) and c0.tolist() == [100, 0]
    assert np.array_equal(out.cpu().numpy(), o0) and (o0[:, 100:] == 7.0).all() and np.array_equal(Cs.cpu().numpy(), C[100:])
    with pytest.raises(nat.GPBError, match="256"):
        eng.gof_accumulate(_dev(y[100:]), Cs, yd, Cd, None, out[0, 100:], out[1, 100:], acc, cnt)


# ---------------------------------------------------------------------------- 3. weighted sums
@functools.lru_cache(maxsize=None)
def _sum_case(M):
    """513 well-conditioned rows (C = B B^T + tr / M I, cond ~ 5) and their model, computed once per M; the smaller W take its
    first rows.  Well conditioned, because the bar below is the bar of the SUMMATION: a term of the device differs from the
    long-double term by the factorisation's own error, cond(C) 2^-53, which at the cond ~ 1e6 of the accuracy cases would exceed
    the 4e-15 per term the bar allows for (those rows are test_row_accuracy's)."""
    y, C, yexp, Cadd = _case(513, M, 300 + M, jitter=1.0)
    rng = np.random.default_rng(23)
    wt = rng.uniform(0.0, 3.0, 513)
    wt[rng.choice(513, 60, replace=False)] = 0.0
    wt[0] = 1.5
    r = R.rows(y, C, yexp, Cadd)
    r["p"] = np.array([float(R.chi2_sf(float(c), M)) for c in r["chi2"]])        # (mpmath's, not scipy's: the bar is the sums')
    assert not r["bad"].any()
    return y, C, yexp, Cadd, wt, r


@pytest.mark.parametrize("W", [1, 255, 256, 257, 513])
@pytest.mark.parametrize("big", [False, True])
def test_weighted_sums_against_the_model(W, big):
    M = _lds_edge() + 1 if big else 6
    y, C, yexp, Cadd, wt, r = _sum_case(M)
    rw = {k: (v[:W] if isinstance(v, np.ndarray) else v) for k, v in r.items()}
    for weights in (None, wt[:W]):
        u, _, cnt, _, _ = _run(y[:W], C[:W], yexp, Cadd, weights)
        s = R.sums(rw, weights)
        assert cnt.tolist() == [W, 0]
        assert abs(u["wsum"] - float(s["wsum"])) <= 1e-13 * float(s["wsum"])
        worst = 0.0
        for k in ("p", "z", "z_sq", "pull", "pull_sq"):
            diff = np.abs(np.asarray(u[k], dtype=np.longdouble) - s[k]).astype(np.float64)
            bar = R.sum_bar(s["abs_" + k])
            worst = max(worst, float(np.max(diff / bar)))
            assert np.all(diff <= bar), (k, float(np.max(diff / bar)))
        print("W=%d M=%d weights=%s: sums' worst ratio to the bar %.3f" % (W, M, weights is not None, worst))


# ---------------------------------------------------------------------------- 4. bad and weightless rows
@pytest.mark.parametrize("big", [False, True])
def test_bad_and_weightless_rows(big):
    """seven rows: row 3 is C - 2 lambda_max I (negative definite: its first pivot fails), row 4 has weight 0 and NaNs in its C.
    The sums are those of the five other rows bit for bit, cnt = [7, 1], and both rows' own outputs are NaN."""
    M = _lds_edge() + 1 if big else 6
    y, C, yexp, Cadd = _case(7, M, 31)
    Cb = C.copy()
    Cb[3] = C[3] - 2.0 * np.linalg.eigvalsh(C[3] + Cadd)[-1] * np.eye(M)
    Cb[4, 0, 0] = Cb[4, M - 1, 0] = np.nan
    wt = np.array([1.0, 0.5, 2.0, 1.5, 0.0, 1.0, 0.25])
    _, a_bad, c_bad, x_bad, l_bad = _run(y, Cb, yexp, Cadd, wt)
    assert c_bad.tolist() == [7, 1] and np.isfinite(a_bad).all()
    assert np.isnan(x_bad[[3, 4]]).all() and np.isnan(l_bad[[3, 4]]).all()
    keep = [0, 1, 2, 5, 6]
    assert np.isfinite(x_bad[keep]).all() and np.isfinite(l_bad[keep]).all()
    # rows 3 and 4 weightless and valid: the same tree with the same zeros in their places
    w0 = wt.copy()
    w0[3] = 0.0
    _, a_0, c_0, x_0, l_0 = _run(y, C, yexp, Cadd, w0)
    assert c_0.tolist() == [7, 0] and np.array_equal(a_bad, a_0)
    assert np.array_equal(x_bad[keep], x_0[keep]) and np.array_equal(l_bad[keep], l_0[keep])
    # the five remaining rows alone: a skipped row adds +0.0 to its run, which changes no bit
    _, a_k, c_k, x_k, l_k = _run(y[keep], C[keep], yexp, Cadd, wt[keep])
    assert c_k.tolist() == [5, 0] and np.array_equal(a_k, a_bad) and np.array_equal(x_k, x_bad[keep]) and np.array_equal(l_k, l_bad[keep])
    # without weights the bad row is left out just the same
    _, a_u, c_u, _, _ = _run(y[:4], Cb[:4], yexp, Cadd)
    assert c_u.tolist() == [4, 1] and a_u[0] == 3.0 and np.isfinite(a_u).all()


# ---------------------------------------------------------------------------- 5. gpb_chi2_sf
def test_chi2_sf_on_the_device(tmp_path):
    """The host program's grid (tests/host/chi2_sf_check.cpp, built here without sanitizers) on the device: every value at the
    host bar against mpmath, max(8 x scipy's worst error on the grid, 64 2^-53) wherever Q >= 1e-290, else inside [0, 1e-289];
    NaN in gives NaN, x <= 0 gives 1.  The device's lgamma / exp / log differ from the host libm's: 94 of the 96 values were
    the host program's bits when measured, so bit equality is not asserted and the host bar against mpmath is; the count of
    equal values is printed.  Measured worst error 7.9e-13 (ndf = 2048), bar 3.6e-12."""
    from test_chi2_sf_host import grid_errors, run_host_program
    torch, dev = _torch()
    eng = _util()
    vals, _, _ = run_host_program(tmp_path, sanitize=False)
    grid = vals[:-4]
    got = []
    for ndf in sorted({v[0] for v in grid}):
        xs = np.array([v[1] for v in grid if v[0] == ndf])
        q = eng.chi2_sf(_dev(xs), ndf).cpu().numpy()
        got += [(ndf, x, float(qv), 0) for x, qv in zip(xs, q)]
    host = {(v[0], v[1]): v[2] for v in grid}
    same = sum(1 for v in got if host[(v[0], v[1])] == v[2])
    errs = grid_errors(got)
    err_scipy = max(e[3] for e in errs)
    w = max(errs, key=lambda e: e[2])
    print("chi2_sf device: %d of %d values are the host program's bits; worst relative error %.3e at ndf=%g x/ndf=%.6g; "
          "scipy's worst %.3e; bar %.3e" % (same, len(got), w[2], w[0], w[1] / w[0], err_scipy, R.sf_bar(err_scipy)))
    for ndf, x, e, _ in errs:
        assert e <= R.sf_bar(err_scipy), (ndf, x, e)
    sp = eng.chi2_sf(_dev(np.array([np.nan, -1.0, -0.0, np.inf, 0.0])), 3.0).cpu().numpy()
    assert np.isnan(sp[0]) and sp[1:].tolist() == [1.0, 1.0, 0.0, 1.0]
    out = torch.full((3,), 7.0, dtype=torch.float64, device=dev)
    assert eng.chi2_sf(_dev(np.array([1.0, 2.0, 3.0])), 2.0, out=out) is out
    assert np.allclose(out.cpu().numpy(), np.exp(-np.array([0.5, 1.0, 1.5])), rtol=1e-14)
    with pytest.raises(ValueError):
        eng.chi2_sf(_dev(np.ones(3)), 0.0)


# ---------------------------------------------------------------------------- 6. gpb_gof_influence
@pytest.mark.parametrize("d", [1, 20])
@pytest.mark.parametrize("S", [1, 256, 700])
def test_influence_against_the_fsum_model(S, d):
    torch, dev = _torch()
    eng = _util()
    rng = np.random.default_rng(1000 + 7 * S + d)
    ll = rng.normal(-40.0, 3.0, (3, S))
    x = rng.uniform(-1.0, 2.0, (S, d))
    wt = rng.uniform(0.0, 2.0, S)
    if S > 1:
        ll[0, rng.choice(S, S // 10, replace=False)] = np.nan
        ll[2, S - 1] = np.nan
        wt[rng.choice(S, S // 8, replace=False)] = 0.0
        wt[0] = 1.0
    ld = S + 5                                               # a view of a wider array
    wide = torch.full((3, ld), float("nan"), dtype=torch.float64, device=dev)
    wide[:, :S] = _dev(ll)
    for weights in (None, wt):
        got = eng.gof_influence(wide[:, :S], _dev(x), None if weights is None else _dev(weights), S=S).cpu().numpy()
        want, ab = R.influence(ll, x, weights)
        assert got.shape == (3, 2 + 2 * d)
        diff, bar = np.abs(got - want), 1e-13 * ab
        assert np.all(diff <= bar), float(np.max(diff / np.maximum(bar, 1e-300)))
        for e in range(3):                                   # alone, a row has the same bits
            one = eng.gof_influence(_dev(ll[e:e + 1]), _dev(x), None if weights is None else _dev(weights)).cpu().numpy()
            assert np.array_equal(one[0], got[e]), e
    # an emulator without a usable row leaves zeros
    none = eng.gof_influence(_dev(np.full((1, S), np.nan)), _dev(x)).cpu().numpy()
    assert not none.any()


# ---------------------------------------------------------------------------- 7. argument errors
def test_argument_errors_write_nothing():
    torch, dev = _torch()
    from gpbayestools_hic_amd import _native as nat
    eng = _util()
    W, M = 4, 3
    y, C, yexp, _ = _case(W, M, 41)
    f7 = lambda n: torch.full((n,), 7.0, dtype=torch.float64, device=dev)        # noqa: E731
    t = dict(y=_dev(y), C=_dev(C), yexp=_dev(yexp), chi2=f7(W), ll=f7(W), acc=f7(9000), cnt=torch.zeros(2, dtype=torch.int64, device=dev))

    def call(W=W, M=M, ctx=True, **null):
        p = {k: (None if null.get(k) else nat.ptr(v)) for k, v in t.items()}
        return eng.lib.gpb_gof_accumulate(eng.h if ctx else None, W, M, p["y"], p["C"], p["yexp"], None, None, p["chi2"], p["ll"],
                                          p["acc"], p["cnt"])
    assert call(ctx=False) == E_ARG
    for name in t:
        assert call(**{name: True}) == E_ARG, name
    assert call(W=-1) == E_ARG and call(M=0) == E_ARG and call(M=2049) == E_ARG and call(W=2 ** 31) == E_ARG
    assert call(W=0) == 0                                   # a no-op
    for k in ("chi2", "ll", "acc"):
        assert (t[k] == 7.0).all().item(), k
    assert t["cnt"].tolist() == [0, 0] and np.array_equal(t["C"].cpu().numpy(), C)
    # gpb_gof_influence
    S, d = 5, 2
    ti = dict(ll=_dev(np.zeros((2, S))), x=_dev(np.ones((S, d))), out=f7(70 * 1100))

    def infl(E=2, S=S, ld=S, d=d, ctx=True, **null):
        p = {k: (None if null.get(k) else nat.ptr(v)) for k, v in ti.items()}
        return eng.lib.gpb_gof_influence(eng.h if ctx else None, p["ll"], E, S, ld, p["x"], d, None, p["out"])
    assert infl(ctx=False) == E_ARG and all(infl(**{k: True}) == E_ARG for k in ti)
    assert infl(d=513) == E_ARG and infl(d=0) == E_ARG and infl(E=65) == E_ARG and infl(E=0) == E_ARG
    assert infl(S=0) == E_ARG and infl(ld=S - 1) == E_ARG
    assert (ti["out"] == 7.0).all().item()
    # gpb_chi2_sf
    xs, out = _dev(np.ones(4)), f7(4)
    assert eng.lib.gpb_chi2_sf(None, nat.ptr(xs), 4, 3.0, nat.ptr(out)) == E_ARG
    assert eng.lib.gpb_chi2_sf(eng.h, None, 4, 3.0, nat.ptr(out)) == E_ARG and eng.lib.gpb_chi2_sf(eng.h, nat.ptr(xs), 4, 3.0, None) == E_ARG
    assert eng.lib.gpb_chi2_sf(eng.h, nat.ptr(xs), -1, 3.0, nat.ptr(out)) == E_ARG
    assert eng.lib.gpb_chi2_sf(eng.h, nat.ptr(xs), 4, 0.0, nat.ptr(out)) == E_ARG
    assert eng.lib.gpb_chi2_sf(eng.h, nat.ptr(xs), 0, 3.0, nat.ptr(out)) == 0 and (out == 7.0).all().item()
    # the Python layer refuses wrong shapes before the library sees them
    acc = torch.zeros(eng.gof_acc_doubles(M), dtype=torch.float64, device=dev)
    with pytest.raises(ValueError):
        eng.gof_accumulate(t["y"], t["C"][:, :2], t["yexp"], None, None, t["chi2"], t["ll"], acc, t["cnt"])
    with pytest.raises(ValueError):
        eng.gof_accumulate(t["y"], t["C"], t["yexp"], None, None, t["chi2"], t["ll"], acc[:-1], t["cnt"])
    with pytest.raises(ValueError):
        eng.gof_accumulate(t["y"], t["C"], t["yexp"], None, None, t["chi2"][:3], t["ll"], acc, t["cnt"])
    with pytest.raises(ValueError):
        eng.gof_accumulate(t["y"].cpu(), t["C"], t["yexp"], None, None, t["chi2"], t["ll"], acc, t["cnt"])


# ---------------------------------------------------------------------------- 8. Chain.goodness_of_fit
SPECS = [(100, 5, 3, "RBF"), (130, 4, 2, "Matern25"), (90, 6, 3, "RBF")]
FIELDS = ("n_bad", "ndf", "chi2_mean", "chi2_quantiles", "chi2_min", "chi2_min_index", "chi2_min_params", "ppp", "resid_mean",
          "resid_rms", "pull_mean", "pull_rms")
TOTAL = ("n_bad", "ndf", "chi2_mean", "chi2_quantiles", "chi2_min", "chi2_min_index", "chi2_min_params", "ppp", "joint")


def _same(a, b):
    for f in FIELDS:
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    for f in TOTAL:
        assert np.array_equal(getattr(a.total, f), getattr(b.total, f)), f
    if a.influence is not None:
        for f in ("ess", "shift", "scale"):
            assert np.array_equal(getattr(a.influence, f), getattr(b.influence, f)), f


@functools.lru_cache(maxsize=None)
def _chain(mapped):
    import tempfile
    from gpbayestools_hic_amd import synth, workload
    chain, emus, info = workload.build_multi_chain(SPECS, 20, workdir=tempfile.mkdtemp(prefix="gpb_gof_"), mapped=mapped)
    X = synth.walkers(300, 20, seed=31)
    return chain, X, chain.goodness_of_fit(X, return_rows=True), info


@pytest.mark.parametrize("mapped", [False, True])
def test_chain_goodness_of_fit(mapped):
    chain, X, res, _ = _chain(mapped)
    S, d = X.shape
    assert res.n_samples == S and res.n_bad.tolist() == [0, 0, 0] and res.ndf.tolist() == [5, 4, 6] and res.names == list(chain.pardict)
    chi2, ll = res.rows["chi2"], res.rows["loglike"]
    assert chi2.shape == (S, 3) and ll.shape == (S, 3) and np.isfinite(chi2).all() and np.isfinite(ll).all()
    # the blocks add up to the chain's likelihood
    lp = chain.log_likelihood(X)
    inside = np.all((X > chain.min) & (X < chain.max), axis=1)
    assert inside.sum() > 250
    tot = ll[:, 0] + ll[:, 1] + ll[:, 2]
    assert np.array_equal(tot, res.rows["loglike_total"])
    diff = np.abs(tot + chain.inside_const - lp)[inside] / np.maximum(np.abs(lp[inside]), 1.0)
    print("mapped=%s: sum of the blocks against log_likelihood, worst %.3e" % (mapped, diff.max()))
    assert np.all(diff <= 1e-10)
    # the rows against the host model on the emulators' own predictions
    r0 = 0
    for k, emu in enumerate(chain.emuList):
        M = emu.nobs
        y, C = emu.predict(X, return_cov=True)
        r = R.rows(y, C, chain.expdata[0][r0:r0 + M], chain.expdata_cov[r0:r0 + M, r0:r0 + M])
        for name, got, want, ref in (("chi2", chi2[:, k], r["chi2"], r["chi2_64"]), ("ll", ll[:, k], r["ll"], r["ll64"])):
            e_dev, e_ref = R.err(got, want), R.err(ref, want)
            print("mapped=%s emulator %d %s: err_device=%.3e err_scipy=%.3e" % (mapped, k, name, e_dev, e_ref))
            assert e_dev <= R.f_bar(e_ref), name
        s = R.sums(r)
        for got, key in ((res.resid_mean[r0:r0 + M] * S, "z"), (res.resid_rms[r0:r0 + M] ** 2 * S, "z_sq"),
                         (res.pull_mean[r0:r0 + M] * S, "pull"), (res.pull_rms[r0:r0 + M] ** 2 * S, "pull_sq")):
            assert np.allclose(got, s[key].astype(np.float64), rtol=1e-9, atol=1e-9 * float(np.max(s["abs_" + key]))), key
        r0 += M
    # quantiles, mean, minimum: numpy on the returned rows, bit for bit
    assert np.array_equal(res.chi2_quantiles, np.percentile(chi2, 100.0 * res.quantiles, axis=0).T)
    assert np.array_equal(res.chi2_min, chi2.min(0)) and np.array_equal(res.chi2_min_index, chi2.argmin(0))
    assert np.array_equal(res.chi2_min_params, X[chi2.argmin(0)])
    assert np.allclose(res.chi2_mean, chi2.mean(0), rtol=1e-13)
    # ppp: the mean of Q over the rows, per emulator and in total, against mpmath at the returned chi2
    c_tot = chi2[:, 0] + chi2[:, 1] + chi2[:, 2]
    assert np.array_equal(c_tot, res.rows["chi2_total"]) and res.total.ndf == 15 and not res.total.joint and res.total.n_bad == 0
    assert np.array_equal(res.total.chi2_quantiles, np.percentile(c_tot, 100.0 * res.quantiles))
    assert res.total.chi2_min == c_tot.min() and res.total.chi2_min_index == c_tot.argmin()
    for name, got, col, ndf in [("emulator %d" % k, res.ppp[k], chi2[:, k], int(res.ndf[k])) for k in range(3)] \
            + [("total", res.total.ppp, c_tot, 15)]:
        exact = [R.chi2_sf(float(c), ndf) for c in col]
        want = float(sum(exact) / S)
        # (the mean of S values within the host bar each, plus its own summation: 1e-13 as for the sums)
        assert abs(got - want) <= (R.host_sf_bar() + 1e-13) * want, (name, got, want)
    # influence: the model on the returned rows
    inf = res.influence
    assert inf.shift.shape == (3, d) and inf.scale.shape == (3, d) and inf.names == list(chain.pardict)
    want, _ = R.influence(ll.T, X)
    base, _ = R.influence(np.zeros((3, S)), X)
    assert np.allclose(inf.ess, want[:, 0] ** 2 / want[:, 1], rtol=1e-11) and np.all((inf.ess >= 1.0) & (inf.ess <= S))
    m1, m0 = want[:, 2:2 + d] / want[:, :1], base[:, 2:2 + d] / base[:, :1]
    s0 = np.sqrt(base[:, 2 + d:] / base[:, :1] - m0 * m0)
    assert np.allclose(inf.shift, (m1 - m0) / s0, rtol=1e-8, atol=1e-10)
    # slabs, unit weights: the same bits; a stored [nwalkers, nsteps, ndim] chain: another row order
    chain.gof_slab_rows = 256
    try:
        r_slab = chain.goodness_of_fit(X, return_rows=True)
    finally:
        chain.gof_slab_rows = None
    _same(r_slab, res)
    assert np.array_equal(r_slab.rows["chi2"], chi2) and np.array_equal(r_slab.rows["loglike"], ll)
    r_ones = chain.goodness_of_fit(X, weights=np.ones(S))
    for f in ("n_bad", "chi2_quantiles", "chi2_min", "ppp", "resid_mean", "pull_rms"):
        assert np.array_equal(getattr(r_ones, f), getattr(res, f)), f
    assert np.allclose(r_ones.chi2_mean, res.chi2_mean, rtol=1e-12) and abs(r_ones.total.ppp - res.total.ppp) <= 1e-13
    assert r_ones.rows is None and chain.goodness_of_fit(X, influence=False).influence is None
    half = chain.goodness_of_fit(X.reshape(3, 100, d), discard=50, quantiles=[0.5])
    assert half.n_samples == 150 and half.chi2_quantiles.shape == (3, 1)
    assert "chi2/ndf (median, 68 %)" in repr(res) and "emulator 2" in repr(res)


def test_weighted_chain_call():
    """weights: zero-weight rows are not evaluated (NaN rows, not bad), the weighted mean and ppp follow the weights"""
    chain, X, res, _ = _chain(False)
    S = X.shape[0]
    w = np.random.default_rng(3).uniform(0.0, 2.0, S)
    w[::7] = 0.0
    rw = chain.goodness_of_fit(X, weights=w, return_rows=True)
    chi2 = res.rows["chi2"]
    assert rw.n_bad.tolist() == [0, 0, 0] and rw.total.n_bad == 0
    assert np.isnan(rw.rows["chi2"][::7]).all() and np.array_equal(rw.rows["chi2"][w != 0], chi2[w != 0])
    assert np.allclose(rw.chi2_mean, (w[:, None] * chi2).sum(0) / w.sum(), rtol=1e-12)
    assert np.allclose(rw.total.chi2_mean, (w * chi2.sum(1)).sum() / w.sum(), rtol=1e-12)
    assert np.array_equal(rw.chi2_quantiles, np.percentile(chi2[w != 0], 100.0 * rw.quantiles, axis=0).T)
    p = scipy.special.gammaincc(res.ndf[None, :] / 2.0, chi2 / 2.0)
    assert np.allclose(rw.ppp, (w[:, None] * p).sum(0) / w.sum(), rtol=1e-11)


def test_chain_refusals():
    chain, X, res, _ = _chain(False)

    class Foreign:
        nobs = 4

        def predict(self, X, return_cov=True, extra_std=0):
            return np.zeros((X.shape[0], 4)), np.zeros((X.shape[0], 4, 4))

    class TwoRanks:
        world, rank = 2, 0

    keep = list(chain.emuList)
    try:
        chain.emuList = [keep[0], Foreign()]
        with pytest.raises(NotImplementedError, match="foreign"):
            chain.goodness_of_fit(X)
        chain.emuList = keep
        chain.sharding = TwoRanks()
        with pytest.raises(NotImplementedError, match="sharded"):
            chain.goodness_of_fit(X)
    finally:
        chain.emuList, chain.sharding = keep, None
    for bad in (X[:, :19], X.reshape(2, 3, 50, 20), np.zeros((0, 20))):
        with pytest.raises(ValueError):
            chain.goodness_of_fit(bad)
    Xn = X.copy()
    Xn[5, 2] = np.inf
    with pytest.raises(ValueError):
        chain.goodness_of_fit(Xn)
    for w in (-np.ones(300), np.zeros(300), np.ones(299)):
        with pytest.raises(ValueError):
            chain.goodness_of_fit(X, weights=w)
    with pytest.raises(ValueError):
        chain.goodness_of_fit(X.reshape(3, 100, 20), weights=np.ones(300))
    for q in ([-0.1], [1.5], []):
        with pytest.raises(ValueError):
            chain.goodness_of_fit(X, quantiles=q)
    assert np.array_equal(chain.goodness_of_fit(X).chi2_quantiles, res.chi2_quantiles)     # the chain is as it was


# ---------------------------------------------------------------------------- 9. a coupled experimental covariance
def test_coupled_chain(tmp_path):
    """the chain (A) of tests/test_gpu_coupled_like.py, one normalisation source shared by all observables: total is the chi2 of
    the joint matrix, and its ll + const is the chain's coupled likelihood; the emulators' blocks are what the same call gives
    with the off-block entries removed; no influence"""
    from gpbayestools_hic_amd import synth
    from gpbayestools_hic_amd.workload import build_multi_chain
    chain, emus, info = build_multi_chain([(48, 12, 3, "RBF"), (64, 20, 5, "Matern25")], 5, workdir=str(tmp_path))
    X = synth.walkers(300, 5, seed=5)
    chain.set_systematics(0.03 * chain.expdata[0][None, :])
    cov = chain.expdata_cov
    res = chain.goodness_of_fit(X, return_rows=True)
    assert chain._coupled and res.influence is None and res.total is not None and res.total.joint and res.total.ndf == 32
    lp = chain.log_likelihood(X)
    inside = np.all((X > chain.min) & (X < chain.max), axis=1)
    assert inside.sum() > 250
    diff = np.abs(res.rows["loglike_total"] + chain.inside_const - lp)[inside] / np.maximum(np.abs(lp[inside]), 1.0)
    print("coupled: joint ll against log_likelihood, worst %.3e" % diff.max())
    assert np.all(diff <= 1e-10)
    c_tot = res.rows["chi2_total"]
    assert np.array_equal(res.total.chi2_quantiles, np.percentile(c_tot, 100.0 * res.quantiles))
    assert not np.allclose(c_tot, res.rows["chi2"].sum(1), rtol=1e-6)            # (the joint chi2 is not the sum of the blocks)
    blocks = np.zeros_like(cov)
    blocks[:12, :12], blocks[12:, 12:] = cov[:12, :12], cov[12:, 12:]
    chain.expdata_cov = blocks
    un = chain.goodness_of_fit(X, return_rows=True)
    assert not chain._coupled and un.influence is not None and not un.total.joint
    for f in FIELDS:
        assert np.array_equal(getattr(un, f), getattr(res, f)), f
    assert np.array_equal(un.rows["chi2"], res.rows["chi2"]) and np.array_equal(un.rows["loglike"], res.rows["loglike"])


# ---------------------------------------------------------------------------- 10. the sampler
def test_sampler_goodness_of_fit_is_the_chains_on_the_stored_rows():
    from gpbayestools_hic_amd import StretchSampler, synth
    chain, _, _, _ = _chain(False)
    s = StretchSampler(chain, 40, seed=5)
    with pytest.raises(AttributeError):
        s.goodness_of_fit()
    s.run(synth.walkers_ball(40, np.full(20, 0.5), 0.02, seed=6), 12)
    for discard, thin in ((0, 1), (3, 2)):
        a = s.goodness_of_fit(discard=discard, thin=thin)
        rows = s._chain_dev[discard::thin].reshape(-1, 20).cpu().numpy()
        b = chain.goodness_of_fit(rows)
        assert a.n_samples == rows.shape[0] == 40 * len(range(discard, 12, thin))
        _same(a, b)
    with pytest.raises(ValueError):
        s.goodness_of_fit(thin=0)


# ---------------------------------------------------------------------------- 11. closure
def test_closure_pseudo_data_from_the_model_itself():
    """pseudo-data drawn from the chain's own predictive distribution at a known row x0, y ~ N(mu(x0), C(x0) + C_exp), and 200
    rows in a ball of radius 0.002 around x0: every emulator's ppp lies in (0.01, 0.99) — first for the host model on the
    emulators' predictions (the seed is judged by the reference alone), then on the device"""
    from gpbayestools_hic_amd import synth
    chain, _, _, info = _chain(False)
    x0 = info["xstar"]
    X = synth.walkers_ball(200, x0, 0.002, seed=77)
    rng = np.random.default_rng(78)
    keep = chain.expdata
    pseudo, r0 = [], 0
    ref = []
    for emu in chain.emuList:
        M = emu.nobs
        mu, C = emu.predict(x0[None, :], return_cov=True)
        Ce = chain.expdata_cov[r0:r0 + M, r0:r0 + M]
        yk = mu[0] + np.linalg.cholesky(C[0] + Ce) @ rng.standard_normal(M)
        pseudo.append(yk)
        y, Cx = emu.predict(X, return_cov=True)
        ref.append(float(np.mean(R.rows(y, Cx, yk, Ce)["p"])))
        r0 += M
    print("closure: reference ppp %s" % ref)
    assert all(0.01 < p < 0.99 for p in ref)
    try:
        chain.expdata = np.concatenate(pseudo)[None, :]
        res = chain.goodness_of_fit(X)
    finally:
        chain.expdata = keep
    print("closure: device ppp %s" % res.ppp.tolist())
    assert np.all((res.ppp > 0.01) & (res.ppp < 0.99))
    assert np.allclose(res.ppp, ref, rtol=1e-8)
