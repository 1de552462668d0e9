"""GPU tier: history matching on the device — gpb_hm_uniform, gpb_hm_implausibility, gpb_hm_maps (GPEngine.hm_uniform /
hm_implausibility / hm_maps), Chain.implausibility and Chain.history_match — against the numpy model of tests/hm_reference.py,
which tests/test_hm_reference.py pins to numpy's own histograms, sorts and loops.  Every comparison is BIT equality: each operation
is a correctly rounded IEEE operation with contraction off, the minima are exact and the rest are integers, so there is no
tolerance to choose.  DESIGN.md section 34."""
import functools
import warnings

import numpy as np
import pytest

import hm_reference as R

pytestmark = pytest.mark.gpu

E_ARG = -1


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _eng():
    from gpbayestools_hic_amd import GPEngine
    return GPEngine(0)


def _dev(a, dtype=None):
    torch, dev = _torch()
    return torch.as_tensor(np.array(a, dtype=dtype), device=dev)


def _bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------ 1. gpb_hm_uniform
def _box(d):
    return -1.0 - 0.25 * np.arange(d), 0.5 + np.arange(d) ** 2 * 1e-3


@pytest.mark.parametrize("row0", [0, 2 ** 32 - 3])
@pytest.mark.parametrize("d", [1, 5, 20])
def test_uniform_rows(d, row0):
    lo, hi = _box(d)
    for S in (1, 64, 65, 1000):
        assert _bits(_eng().hm_uniform(lo, hi, S, seed=11, row0=row0).cpu().numpy(), R.uniform_rows(lo, hi, row0, S, 11)), S


def test_uniform_ld_and_slabs():
    torch, dev = _torch()
    d, S = 5, 1000
    lo, hi = _box(d)
    ref = R.uniform_rows(lo, hi, 7, S, 3)
    wide = torch.full((S, d + 3), -7.0, dtype=torch.float64, device=dev)
    _eng().hm_uniform(lo, hi, S, seed=3, row0=7, out=wide)
    w = wide.cpu().numpy()
    assert _bits(np.ascontiguousarray(w[:, :d]), ref) and np.all(w[:, d:] == -7.0)
    out = torch.empty((S, d), dtype=torch.float64, device=dev)
    for i0, i1 in ((0, 1), (1, 338), (338, S)):
        _eng().hm_uniform(lo, hi, i1 - i0, seed=3, row0=7 + i0, out=out[i0:i1])
    assert _bits(out.cpu().numpy(), ref)


# ------------------------------------------------------------------------------------------------ 2. gpb_hm_implausibility
def _impl_case(M, S, seed=0):
    rng = np.random.default_rng(1000 * M + S + seed)
    mu, var = rng.normal(size=(M, S)), rng.uniform(0.05, 2.0, (M, S))
    y, vadd = rng.normal(size=M), rng.uniform(0.0, 1.0, M)
    if M >= 3:                                   # two observables tied for the maximum in column 0, bit for bit: equal r and v
        y[0] = y[2] = 0.5
        mu[0, 0], mu[2, 0] = 40.5, -39.5
        var[0, 0] = var[2, 0] = 0.5
        vadd[0] = vadd[2] = 0.25
        assert abs(y[0] - mu[0, 0]) == abs(y[2] - mu[2, 0])
    return mu, var, y, vadd


def _ranges(M, G):
    if G == 0:
        return None
    if G == 1:
        return np.array([[0, M]], dtype=np.int32)
    if M < 3:
        return np.array([[0, 1]] * 3, dtype=np.int32)
    return np.array([[0, 1], [1, M - 1], [M - 1, M]], dtype=np.int32)        # one-observable ranges at both ends


def _raw_impl(mu, var, y, vadd, ranges, K, pad=3, want_arg=True, want_gmax=True):
    """the C call with ld and ldo larger than S; returns host arrays and what lies behind the S columns"""
    torch, dev = _torch()
    eng = _eng()
    M, S = mu.shape
    ld, ldo = S + pad, S + pad + 2
    G = 0 if ranges is None else len(ranges)

    def wide(a, w):
        t = torch.full((a.shape[0], w), 9.0, dtype=torch.float64, device=dev)
        t[:, :S] = _dev(a)
        return t
    mu_d, var_d = wide(mu, ld), None if var is None else wide(var, ld)
    top = torch.full((K, ldo), -5.0, dtype=torch.float64, device=dev)
    arg = torch.full((S,), -5, dtype=torch.int32, device=dev) if want_arg else None
    gmax = torch.full((max(G, 1), ldo), -5.0, dtype=torch.float64, device=dev) if (G and want_gmax) else None
    bad = torch.zeros((1,), dtype=torch.int64, device=dev)
    from gpbayestools_hic_amd import _native as nat
    y_d, vadd_d = _dev(y), None if vadd is None else _dev(vadd)
    rg = None if ranges is None else np.ascontiguousarray(ranges, dtype=np.int32)
    rc = eng.lib.gpb_hm_implausibility(eng.h, nat.ptr(mu_d), nat.ptr(var_d), M, S, ld, nat.ptr(y_d), nat.ptr(vadd_d), nat.ptr(rg), G, K, nat.ptr(top),
                                       nat.ptr(arg), nat.ptr(gmax), ldo, nat.ptr(bad))
    assert rc == 0, eng.lib.gpb_last_error(eng.h)
    t = top.cpu().numpy()
    assert np.all(t[:, S:] == -5.0)
    out = {"top": np.ascontiguousarray(t[:, :S]), "n_bad": int(bad.item())}
    if want_arg:
        out["arg"] = arg.cpu().numpy()
    if gmax is not None:
        g = gmax.cpu().numpy()
        assert np.all(g[:, S:] == -5.0)
        out["gmax"] = np.ascontiguousarray(g[:G, :S])
    return out


def _check_impl(out, ref, keys=("top", "arg", "gmax")):
    for k in keys:
        if k in out:
            assert _bits(out[k], ref[k]), k
    assert out["n_bad"] == ref["n_bad"]


@pytest.mark.parametrize("M", [1, 3, 64, 70])
def test_implausibility_shapes(M):
    for S in (1, 63, 64, 65, 257):
        mu, var, y, vadd = _impl_case(M, S)
        for K in sorted({1, min(4, M)}):
            for G in (0, 1, 3):
                rg = _ranges(M, G)
                _check_impl(_raw_impl(mu, var, y, vadd, rg, K), R.implausibility(mu, var, y, vadd, rg, K))


def test_implausibility_null_inputs_and_tie():
    mu, var, y, vadd = _impl_case(70, 65)
    rg = _ranges(70, 3)
    _check_impl(_raw_impl(mu, None, y, vadd, rg, 4), R.implausibility(mu, None, y, vadd, rg, 4))
    _check_impl(_raw_impl(mu, var, y, None, rg, 4), R.implausibility(mu, var, y, None, rg, 4))
    ref = R.implausibility(mu, var, y, vadd, rg, 2)
    assert ref["arg"][0] == 0 and ref["top"][0, 0] == ref["top"][1, 0]            # the tie: the lowest index, the value twice
    out = _raw_impl(mu, var, y, vadd, rg, 2)
    assert out["arg"][0] == 0 and out["top"][0, 0] == out["top"][1, 0]
    # outputs not requested leave the others unchanged
    part = _raw_impl(mu, var, y, vadd, rg, 2, want_arg=False, want_gmax=False)
    assert _bits(part["top"], out["top"]) and "arg" not in part and "gmax" not in part


def test_implausibility_special_values():
    y = np.zeros(7)
    mu = np.array([[0.0], [1.0], [1.0], [2.0], [np.nan], [np.inf], [1.0]])
    var = np.array([[0.0], [0.0], [-1.0], [1.0], [1.0], [1.0], [np.nan]])
    vadd = np.array([0.0, 0.0, 0.5, np.inf, 0.0, np.inf, 0.0])
    expect = [0.0, np.inf, np.inf, 0.0, np.inf, 0.0, np.inf]
    for m in range(7):
        out = _raw_impl(mu[m:m + 1], var[m:m + 1], y[m:m + 1], vadd[m:m + 1], None, 1)
        assert out["top"][0, 0] == expect[m] and out["n_bad"] == int(expect[m] == np.inf), m
    # many columns, some of them bad in several observables: each counted once, the counter is added to
    rng = np.random.default_rng(4)
    S = 257
    MU, VAR = np.repeat(mu, S, axis=1), np.repeat(var, S, axis=1)
    good = rng.random(S) < 0.5
    MU[:, good], VAR[:, good] = rng.normal(size=(7, good.sum())), 1.0
    ref = R.implausibility(MU, VAR, y, vadd, [(0, 7)], 4)
    assert ref["n_bad"] == S - good.sum()
    _check_impl(_raw_impl(MU, VAR, y, vadd, [(0, 7)], 4), ref)
    torch, dev = _torch()
    bad = torch.full((1,), 100, dtype=torch.int64, device=dev)
    r = _eng().hm_implausibility(_dev(MU), _dev(VAR), y, vadd, None, 1, bad=bad, on_device=True)
    assert int(r["bad"].item()) == 100 + ref["n_bad"] and not torch.isnan(r["top"]).any()


def test_implausibility_columns_alone():
    """a sample's bits depend on its own column only: inside a larger S, and with the ranges in another order (the walk per range)"""
    mu, var, y, vadd = _impl_case(70, 257)
    rg = _ranges(70, 3)
    full = _raw_impl(mu, var, y, vadd, rg, 4)
    sub = _raw_impl(mu[:, 100:165], var[:, 100:165], y, vadd, rg, 4)
    for k in ("top", "arg", "gmax"):
        assert _bits(sub[k], np.ascontiguousarray(full[k][..., 100:165])), k
    swapped = rg[[2, 0, 1]]
    overl = np.array([[5, 70], [0, 10], [10, 11]], dtype=np.int32)
    for other in (swapped, overl):
        out = _raw_impl(mu, var, y, vadd, other, 4)
        assert _bits(out["top"], full["top"]) and _bits(out["arg"], full["arg"])
        assert _bits(out["gmax"], R.implausibility(mu, var, y, vadd, other, 4)["gmax"])
    assert _bits(_raw_impl(mu, var, y, vadd, swapped, 4)["gmax"], full["gmax"][[2, 0, 1]])


# ------------------------------------------------------------------------------------------------ 3. gpb_hm_maps
def _maps_case(S, d, B, seed=0):
    rng = np.random.default_rng(100 * S + 10 * d + B + seed)
    edges = np.stack([np.linspace(0.0, 1.0, B + 1) ** (1.0 + 0.25 * j) for j in range(d)])
    X = rng.uniform(-0.05, 1.05, (S, d))
    n = min(S, 12)
    X[0:n:4, 0] = edges[0, B // 2]               # on an edge
    X[1:n:4, d - 1] = edges[d - 1, B]            # on the last edge: closed
    X[2:n:4, 0] = 2.0                            # outside
    if S > 8:
        X[3:n:4, 1] = np.nan
    score = rng.gamma(2.0, 1.5, S)
    score[::7] = 3.0                             # exactly the cutoff: not NROY
    score[3::11] = np.inf
    return X, score, 3.0, edges


KEYS = ("min1", "cnt1", "nroy1", "min2", "cnt2", "nroy2")


def _same_maps(out, ref, keys=KEYS):
    for k in keys:
        assert _bits(out[k], ref[k]), k


@pytest.mark.parametrize("B", [1, 7, 20, 64])
@pytest.mark.parametrize("d", [2, 5])
def test_maps_shapes(d, B):
    for S in (1, 255, 256, 257, 5000):
        X, score, cutoff, edges = _maps_case(S, d, B)
        ref = R.maps(X, score, cutoff, edges)
        out = _eng().hm_maps(_dev(X), _dev(score), cutoff, edges)
        _same_maps(out, ref)
        if S == 1 and B > 1:
            assert (out["cnt1"] == 0).any() and np.all(out["min1"][out["cnt1"] == 0] == np.inf) and np.all(out["nroy1"][out["cnt1"] == 0] == 0)


def test_maps_concentrated_pairs_outputs_slabs_stride():
    torch, dev = _torch()
    eng = _eng()
    S, d, B = 5000, 5, 20
    X, score, cutoff, edges = _maps_case(S, d, B)
    # a concentrated set: every row in one bin pair
    Xc = np.full((S, d), 0.31) + np.random.default_rng(1).uniform(0, 1e-4, (S, d))
    ref = R.maps(Xc, score, cutoff, edges)
    assert np.count_nonzero(ref["cnt2"][0]) == 1
    _same_maps(eng.hm_maps(_dev(Xc), _dev(score), cutoff, edges), ref)
    # explicit pairs, (j, i) with j > i among them
    pairs = np.array([[3, 1], [0, 4], [4, 0]], dtype=np.int32)
    refp = R.maps(X, score, cutoff, edges, pairs)
    outp = eng.hm_maps(_dev(X), _dev(score), cutoff, edges, pairs)
    _same_maps(outp, refp)
    assert np.array_equal(outp["cnt2"][1], outp["cnt2"][2].T) and np.array_equal(outp["min2"][1], outp["min2"][2].T)
    # only the 1-D outputs, only the 2-D outputs
    one = eng.hm_maps(_dev(X), _dev(score), cutoff, edges, pairs, outputs=("1d",))
    two = eng.hm_maps(_dev(X), _dev(score), cutoff, edges, pairs, outputs=("2d",))
    assert sorted(one) == ["cnt1", "min1", "nroy1"] and sorted(two) == ["cnt2", "min2", "nroy2"]
    _same_maps(one, refp, KEYS[:3])
    _same_maps(two, refp, KEYS[3:])
    # one call against three uneven slabs with init = 0
    acc = None
    Xd, sd = _dev(X), _dev(score)
    for i0, i1 in ((0, 1), (1, 1703), (1703, S)):
        acc = eng.hm_maps(Xd[i0:i1], sd[i0:i1], cutoff, edges, pairs, into=acc, on_device=True)
    _same_maps({k: v.cpu().numpy() for k, v in acc.items()}, refp)
    # a row stride above d
    wide = torch.full((S, d + 3), float("nan"), dtype=torch.float64, device=dev)
    wide[:, :d] = Xd
    _same_maps(eng.hm_maps(wide[:, :d], sd, cutoff, edges, pairs), refp)
    # empty bins read +inf, 0, 0
    empty = refp["cnt2"] == 0
    assert empty.any() and np.all(outp["min2"][empty] == np.inf) and np.all(outp["nroy2"][empty] == 0)


# ------------------------------------------------------------------------------------------------ 4. argument errors
def test_argument_errors():
    torch, dev = _torch()
    from gpbayestools_hic_amd import _native as nat
    eng = _eng()
    lib, h = eng.lib, eng.h
    # gpb_hm_uniform
    X = torch.full((8, 4), -3.0, dtype=torch.float64, device=dev)
    lo, hi = np.zeros(4), np.ones(4)

    def uni(lo=lo, hi=hi, d=4, S=8, ld=4):
        return lib.gpb_hm_uniform(h, nat.ptr(nat.f64(lo)), nat.ptr(nat.f64(hi)), d, 0, S, 1, nat.ptr(X), ld)
    big = np.zeros(513)
    assert uni(d=0) == E_ARG and uni(lo=big, hi=big + 1, d=513, ld=513) == E_ARG and uni(S=0) == E_ARG and uni(ld=3) == E_ARG
    assert uni(hi=np.array([1.0, 0.0, 1.0, 1.0])) == E_ARG and uni(hi=np.array([1.0, np.inf, 1.0, 1.0])) == E_ARG
    assert uni(lo=np.array([0.0, np.nan, 0.0, 0.0])) == E_ARG
    assert bool((X == -3.0).all())
    # gpb_hm_implausibility
    M, S = 6, 10
    mu = torch.zeros((M, S), dtype=torch.float64, device=dev)
    y = torch.zeros((M,), dtype=torch.float64, device=dev)
    top = torch.full((4, S), -3.0, dtype=torch.float64, device=dev)
    gmax = torch.full((2, S), -3.0, dtype=torch.float64, device=dev)
    arg = torch.full((S,), -3, dtype=torch.int32, device=dev)
    bad = torch.full((1,), 5, dtype=torch.int64, device=dev)
    okr = np.array([[0, 3], [3, 6]], dtype=np.int32)

    def imp(M=M, S=S, ld=S, rg=okr, G=2, K=2, ldo=S):
        return lib.gpb_hm_implausibility(h, nat.ptr(mu), None, M, S, ld, nat.ptr(y), None, nat.ptr(rg), G, K, nat.ptr(top), nat.ptr(arg),
                                         nat.ptr(gmax), ldo, nat.ptr(bad))
    assert imp(M=0) == E_ARG and imp(M=4097) == E_ARG
    assert imp(K=0) == E_ARG and imp(K=5) == E_ARG and imp(M=1, K=2, G=0) == E_ARG
    assert imp(G=-1) == E_ARG and imp(G=65) == E_ARG
    assert imp(rg=np.array([[0, 3], [3, 3]], dtype=np.int32)) == E_ARG and imp(rg=np.array([[0, 3], [3, 7]], dtype=np.int32)) == E_ARG
    assert imp(rg=np.array([[-1, 3], [3, 6]], dtype=np.int32)) == E_ARG
    assert imp(ld=S - 1) == E_ARG and imp(ldo=S - 1) == E_ARG and imp(S=0) == E_ARG and imp(S=2 ** 31, ld=2 ** 31, ldo=2 ** 31) == E_ARG
    assert bool((top == -3.0).all()) and bool((gmax == -3.0).all()) and bool((arg == -3).all()) and int(bad.item()) == 5
    # gpb_hm_maps
    d, B, S = 3, 4, 10
    x = torch.rand((S, d), dtype=torch.float64, device=dev)
    sc = torch.rand((S,), dtype=torch.float64, device=dev)
    edges = np.ascontiguousarray(np.stack([np.linspace(0, 1, B + 1)] * d))
    o1 = [torch.full((d, B), -3.0, dtype=torch.float64, device=dev)] + [torch.full((d, B), -3, dtype=torch.int64, device=dev) for _ in range(2)]
    o2 = [torch.full((3, B, B), -3.0, dtype=torch.float64, device=dev)] + [torch.full((3, B, B), -3, dtype=torch.int64, device=dev) for _ in range(2)]

    def mp(B=B, edges=edges, pairs=None, npairs=3, cutoff=3.0, row_stride=d, S=S, init=1, o1=o1):
        return lib.gpb_hm_maps(h, nat.ptr(x), S, d, row_stride, nat.ptr(sc), cutoff, nat.ptr(edges), B, nat.ptr(pairs), npairs, init,
                               *[nat.ptr(t) for t in list(o1) + o2])
    e65 = np.ascontiguousarray(np.stack([np.linspace(0, 1, 66)] * d))
    bad_e, nan_e = edges.copy(), edges.copy()
    bad_e[1, 2], nan_e[2, 0] = bad_e[1, 1], np.nan
    assert mp(B=0) == E_ARG and mp(B=65, edges=e65) == E_ARG and mp(edges=bad_e) == E_ARG and mp(edges=nan_e) == E_ARG
    assert mp(pairs=np.array([[0, 3], [0, 1], [1, 2]], dtype=np.int32)) == E_ARG
    assert mp(pairs=np.array([[0, 1], [1, 1], [1, 2]], dtype=np.int32)) == E_ARG
    assert mp(npairs=2) == E_ARG and mp(npairs=-1) == E_ARG
    assert mp(B=64, edges=e65[:, :65].copy(), pairs=np.zeros((1, 2), dtype=np.int32), npairs=2 ** 19) == E_ARG      # npairs B^2 above 2^31 - 1
    assert mp(cutoff=np.inf) == E_ARG and mp(cutoff=np.nan) == E_ARG and mp(row_stride=d - 1) == E_ARG and mp(S=0) == E_ARG
    assert mp(init=2) == E_ARG and mp(o1=[o1[0], None, o1[2]]) == E_ARG
    for t in o1 + o2:
        assert bool((t == -3).all())
    assert mp() == 0 and int(o1[1].sum().item()) > 0


# ------------------------------------------------------------------------------------------------ 5. end to end
@functools.lru_cache(maxsize=None)
def _chain():
    from gpbayestools_hic_amd.workload import build_multi_chain
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return build_multi_chain([(48, 12, 3, "RBF"), (64, 20, 5, "Matern25")], 5)


N_E2E, KEEP = 4096, 300
FIELDS = {"min_implausibility_1d": "min1", "count_1d": "cnt1", "nroy_count_1d": "nroy1", "min_implausibility_2d": "min2",
          "count_2d": "cnt2", "nroy_count_2d": "nroy2"}


@functools.lru_cache(maxsize=None)
def _e2e_model(cutoff, kth, disc):
    """the model on the rows uniform_rows gives and on what Chain._predict returns for them: computed once per setting"""
    chain, emus, info = _chain()
    X = R.uniform_rows(chain.min, chain.max, 0, N_E2E, 5)
    mean, cov = chain._predict(X)
    mu_T, var_T = np.ascontiguousarray(mean.T), np.ascontiguousarray(np.diagonal(cov, axis1=1, axis2=2).T)
    vadd = np.diagonal(chain.expdata_cov) + disc
    edges = np.stack([np.linspace(chain.min[j], chain.max[j], 21) for j in range(chain.ndim)])
    return X, edges, R.history_match(X, mu_T, var_T, chain.expdata[0], vadd, [(0, 12), (12, 32)], kth, cutoff, edges, keep=KEEP)


def _check_e2e(hm, edges, ref):
    S = N_E2E
    assert hm.n_samples == S and hm.n_nroy == ref["n_nroy"] and hm.n_bad == ref["n_bad"] == 0
    print("history_match: n_nroy = %d of %d" % (hm.n_nroy, S))
    assert hm.nroy_fraction == ref["n_nroy"] / S
    f = hm.nroy_fraction
    assert hm.nroy_fraction_se == float(np.sqrt(f * (1 - f) / S))
    assert _bits(hm.ruled_out_by, ref["ruled_out_by"]) and _bits(hm.dataset_nroy_fraction, ref["dataset_nroy_fraction"])
    assert _bits(hm.edges, edges) and _bits(hm.pairs, R.all_pairs(5))
    for k, r in FIELDS.items():
        assert _bits(getattr(hm, k), ref[r]), k
    with np.errstate(invalid="ignore"):
        assert _bits(hm.optical_depth_1d, np.where(ref["cnt1"] > 0, ref["nroy1"] / np.maximum(ref["cnt1"], 1), np.nan))
        assert _bits(hm.optical_depth_2d, np.where(ref["cnt2"] > 0, ref["nroy2"] / np.maximum(ref["cnt2"], 1), np.nan))
    assert _bits(hm.nroy_samples, ref["nroy_samples"]) and _bits(hm.nroy_box, ref["nroy_box"])


@pytest.mark.parametrize("slab", [None, 1000])
def test_history_match_equals_model(slab):
    chain, emus, info = _chain()
    # the cutoff / discrepancy of a first wave: wide enough that part of the box survives (the model decides, not this test)
    for cutoff, kth, disc in ((3.0, 2, 0.0), (3.0, 1, 0.25)):
        X, edges, ref = _e2e_model(cutoff, kth, disc)
        chain.hm_slab_rows = slab
        try:
            hm = chain.history_match(n_samples=N_E2E, cutoff=cutoff, kth=kth, discrepancy=disc, keep=KEEP, seed=5)
        finally:
            chain.hm_slab_rows = None
        _check_e2e(hm, edges, ref)
        if hm.n_nroy:
            b = hm.refocus(0.1)
            assert np.all(b[:, 0] >= chain.min) and np.all(b[:, 1] <= chain.max) and np.all(b[:, 0] <= hm.nroy_box[:, 0])
    # explicit rows: the same implausibilities as the drawn ones
    Xs = X[:700]
    r = chain.implausibility(Xs, kth=1, discrepancy=0.25)
    mean, cov = chain._predict(Xs)
    m = R.implausibility(mean.T, np.diagonal(cov, axis1=1, axis2=2).T, chain.expdata[0], np.diagonal(chain.expdata_cov) + 0.25,
                         [(0, 12), (12, 32)], 1)
    assert _bits(r["top"], m["top"]) and _bits(r["arg"], m["arg"]) and _bits(r["gmax"], m["gmax"]) and r["bad"] == 0


def test_truth_point_mask_and_kth():
    chain, emus, info = _chain()
    r = chain.implausibility(info["xstar"])
    assert np.all(r["top"] == 0.0) and np.all(r["gmax"] == 0.0) and r["bad"] == 0
    hm = chain.history_match(X=info["xstar"][None, :], cutoff=1e-300, bins=4)
    assert hm.n_nroy == 1 and hm.nroy_fraction == 1.0 and _bits(hm.nroy_samples, info["xstar"][None, :])
    mask = np.ones(chain.nobs, dtype=bool)
    mask[:12] = False
    hm = chain.history_match(n_samples=512, observable_mask=mask, seed=1)
    assert hm.dataset_nroy_fraction[0] == 1.0 and np.all(hm.ruled_out_by[:12] == 0)
    mask[:] = False
    mask[5] = True
    with pytest.raises(ValueError):
        chain.history_match(n_samples=64, kth=2, observable_mask=mask)
    with pytest.raises(ValueError):
        chain.implausibility(info["xstar"], kth=2, observable_mask=mask)
    assert chain.history_match(n_samples=64, kth=1, observable_mask=mask).n_samples == 64
