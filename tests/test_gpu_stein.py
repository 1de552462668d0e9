"""GPU tier: Stein thinning and the kernel Stein discrepancy of resident rows — gpb_stein_thin, gpb_stein_ksd (GPEngine.stein_thin,
GPEngine.stein_ksd) — and what thinning.py builds on them (stein_thin, ksd, the Chain / sampler / SMC / closure methods) against
the host model of tests/stein_reference.py, which tests/test_stein_reference.py pins to torch.autograd.  idx, ksd, obj, row_sum,
ksd2 and n_skipped are compared with np.array_equal: nothing is excluded and there are no tolerances, except where the full
discrepancy of the picked rows is set beside the thinning's running value (two sums in different orders).  DESIGN.md section 35."""
import functools

import numpy as np
import pytest

import stein_reference as R

pytestmark = pytest.mark.gpu

E_ARG = -1


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _eng():
    from gpbayestools_hic_amd import GPEngine
    return GPEngine(0)


def _dev(a):
    torch, dev = _torch()
    return torch.as_tensor(np.array(a, order="C"), device=dev)


def _spd(rng, d):
    a = rng.standard_normal((d, d))
    inv = np.linalg.inv(a @ a.T + d * np.eye(d))
    return 0.5 * (inv + inv.T)


# ---------------------------------------------------------------------------- 1. shapes
# (n, d, m): every padded width (8, 16, 20, 24, 32, 48, 64), one lane past a 256-row tile, a single row, m > n, several column
# chunks and row chunks, and with 70001 rows more workgroup partials (274) than one wave reduces and three slabs of query rows
SHAPES = ((257, 20, 40), (1, 3, 5), (256, 1, 16), (65, 8, 65), (300, 16, 10), (130, 24, 9), (1000, 33, 64), (513, 32, 7),
          (300, 64, 10), (70001, 5, 8))
# the query rows of the 70001-row case whose row_sum the model computes (all columns): the ends, and the rows on either side of
# the slab boundaries 30208 and 60416 (GPB_STEIN_PART_MB = 16 and 69 column chunks) and of a column chunk's end
BIG_ROWS = np.r_[0:40, 1020:1030, 30200:30216, 60410:60422, 69990:70001]


@functools.lru_cache(maxsize=None)
def _shape_case(i):
    n, d, m = SHAPES[i]
    rng = np.random.default_rng(300 + i)
    x = rng.standard_normal((n, d)) * rng.uniform(0.5, 2.0, d)
    g = -(x - rng.standard_normal(d)) @ (_spd(rng, d) * d)
    ginv = _spd(rng, d)
    return x, g, ginv, m


@functools.lru_cache(maxsize=None)
def _thin_model(i):
    x, g, ginv, m = _shape_case(i)
    return R.thin(x, g, ginv, m)


IDS = ["x".join(str(v) for v in s) for s in SHAPES]


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_thinning_matches_the_model(i):
    x, g, ginv, m = _shape_case(i)
    want = _thin_model(i)
    out = _eng().stein_thin(_dev(x), _dev(g), ginv, m, return_obj=True)
    assert out["idx"].dtype == np.int32 and out["idx"].shape == (m,) and out["ksd"].shape == (m,) and out["obj"].shape == (x.shape[0],)
    assert np.array_equal(out["idx"], want["idx"])
    assert np.array_equal(out["ksd"], want["ksd"])
    assert np.array_equal(out["obj"], want["obj"])
    assert out["n_skipped"] == want["n_skipped"] == 0


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_full_ksd_matches_the_model(i):
    """row_sum and ksd2 bit for bit.  With 70001 rows the model's pair matrix would take minutes: there the model computes the
    row sums of BIG_ROWS against all columns, and the total from the device's row sums in the header's order."""
    x, g, ginv, _ = _shape_case(i)
    out = _eng().stein_ksd(_dev(x), _dev(g), ginv, return_rows=True)
    if x.shape[0] > 5000:
        assert np.array_equal(out["row_sum"][BIG_ROWS], R.row_sums(x, g, ginv, rows=BIG_ROWS))
        want = R.ksd_full(x, g, ginv, row_sum=out["row_sum"])
    else:
        want = R.ksd_full(x, g, ginv)
        assert np.array_equal(out["row_sum"], want["row_sum"])
    assert out["ksd2"] == want["ksd2"] and out["n_skipped"] == 0 and out["ksd"] == float(np.sqrt(want["ksd2"]))


# ---------------------------------------------------------------------------- 2. ties
def test_ties_go_to_the_lower_row():
    rng = np.random.default_rng(5)
    x = rng.integers(-2, 3, (150, 3)).astype(np.float64)
    x = np.concatenate([x, x[::-1], x[:77]])                                 # every row has copies, 377 rows
    want = R.thin(x, -x, np.eye(3), 60, return_ties=True)
    assert np.sum(want["ties"] > 1) >= 10 and want["ties"].max() >= 3         # (the case: several rows at the minimum)
    for t in np.flatnonzero(want["ties"] > 1):                               # the model's pick is the lowest of its equals
        assert not np.any(np.all(x[:want["idx"][t]] == x[want["idx"][t]], axis=1))
    out = _eng().stein_thin(_dev(x), _dev(-x), np.eye(3), 60, return_obj=True)
    assert np.array_equal(out["idx"], want["idx"]) and np.array_equal(out["ksd"], want["ksd"]) and np.array_equal(out["obj"], want["obj"])
    # the same rows spread over 274 workgroups: the tie is settled between workgroups too
    big = np.tile(x, (186, 1))[:70001]
    wb = R.thin(big, -big, np.eye(3), 6, return_ties=True)
    assert wb["ties"].min() > 100
    ob = _eng().stein_thin(_dev(big), _dev(-big), np.eye(3), 6, return_obj=True)
    assert np.array_equal(ob["idx"], wb["idx"]) and np.array_equal(ob["ksd"], wb["ksd"]) and np.array_equal(ob["obj"], wb["obj"])


# ---------------------------------------------------------------------------- 3. rows that are not finite
def test_nonfinite_rows_are_skipped_and_counted():
    rng = np.random.default_rng(8)
    x = rng.standard_normal((600, 4))
    g = -x.copy()
    x[5, 2], x[256, 0], g[300, 1], g[599, 3] = np.nan, np.inf, -np.inf, np.nan
    x[77, 1] = 1e308                                                         # finite, but Ginv x is not
    ginv = 4.0 * np.eye(4)
    want = R.thin(x, g, ginv, 30)
    out = _eng().stein_thin(_dev(x), _dev(g), ginv, 30, return_obj=True)
    bad = [5, 77, 256, 300, 599]
    assert want["n_skipped"] == out["n_skipped"] == 5 and not np.isin(out["idx"], bad).any()
    assert np.array_equal(out["idx"], want["idx"]) and np.array_equal(out["ksd"], want["ksd"])
    assert np.array_equal(out["obj"], want["obj"], equal_nan=True) and np.isnan(out["obj"][bad]).all() and np.isfinite(np.delete(out["obj"], bad)).all()
    full, wf = _eng().stein_ksd(_dev(x), _dev(g), ginv, return_rows=True), R.ksd_full(x, g, ginv)
    assert np.array_equal(full["row_sum"], wf["row_sum"], equal_nan=True) and np.isnan(full["row_sum"][bad]).all()
    assert full["ksd2"] == wf["ksd2"] and full["n_skipped"] == 5
    keep = np.setdiff1d(np.arange(600), bad)                                 # left out of every sum: the clean rows' numbers
    clean = _eng().stein_ksd(_dev(x[keep]), _dev(g[keep]), ginv, return_rows=True)
    assert np.allclose(clean["row_sum"], full["row_sum"][keep], rtol=1e-13, atol=0) and abs(clean["ksd2"] - full["ksd2"]) <= 1e-13 * full["ksd2"]


def test_no_valid_row():
    x = np.full((300, 2), np.nan)
    out = _eng().stein_thin(_dev(x), _dev(np.zeros((300, 2))), np.eye(2), 7, return_obj=True)
    assert out["idx"].tolist() == [-1] * 7 and np.isnan(out["ksd"]).all() and np.isnan(out["obj"]).all() and out["n_skipped"] == 300
    full = _eng().stein_ksd(_dev(x), _dev(np.zeros((300, 2))), np.eye(2), return_rows=True)
    assert np.isnan(full["ksd2"]) and np.isnan(full["row_sum"]).all() and full["n_skipped"] == 300


# ---------------------------------------------------------------------------- 4. splits, slabs, placement, strides
@functools.lru_cache(maxsize=None)
def _split_case():
    rng = np.random.default_rng(12)
    x = rng.standard_normal((5000, 3))                                      # five column chunks
    g = -x @ (_spd(rng, 3) * 3)
    ginv = _spd(rng, 3)
    return x, g, ginv, R.ksd_full(x, g, ginv)


def test_splits_change_no_bit():
    x, g, ginv, want = _split_case()
    for splits in (1, 2, 7, 0):
        out = _eng().stein_ksd(_dev(x), _dev(g), ginv, splits=splits, return_rows=True)
        assert np.array_equal(out["row_sum"], want["row_sum"]) and out["ksd2"] == want["ksd2"], splits


def test_slabs_and_splits_change_no_bit_at_70001_rows():
    """three slabs of query rows (csrc/stein_plan.h; tests/host/stein_plan_check.cpp shows that this size gives three): one
    range of columns, 64 and the automatic choice give the same bits, on the device and on the host; the model's rows on
    either side of the slab boundaries are compared in test_full_ksd_matches_the_model"""
    torch, dev = _torch()
    x, g, ginv, _ = _shape_case(len(SHAPES) - 1)
    xd, gd = _dev(x), _dev(g)
    one = _eng().stein_ksd(xd, gd, ginv, splits=1, on_device=True, return_rows=True)
    for splits in (2, 7, 64, 0):
        many = _eng().stein_ksd(xd, gd, ginv, splits=splits, on_device=True, return_rows=True)
        assert torch.equal(one["row_sum"], many["row_sum"]) and torch.equal(one["ksd2"], many["ksd2"]), splits
    host = _eng().stein_ksd(xd, gd, ginv, return_rows=True)
    assert np.array_equal(host["row_sum"], one["row_sum"].cpu().numpy()) and host["ksd2"] == float(one["ksd2"][0])


def test_on_device_outputs_and_optional_outputs():
    torch, dev = _torch()
    x, g, ginv, m = _shape_case(0)
    want, wf = _thin_model(0), R.ksd_full(x, g, ginv)
    on = _eng().stein_thin(_dev(x), _dev(g), ginv, m, on_device=True, return_obj=True)
    assert on["idx"].is_cuda and on["idx"].dtype == torch.int32 and on["ksd"].is_cuda and on["obj"].is_cuda
    for key in ("idx", "ksd", "obj"):
        assert np.array_equal(on[key].cpu().numpy(), want[key]), key
    for on_device in (False, True):
        out = _eng().stein_thin(_dev(x), _dev(g), ginv, m, on_device=on_device)
        assert "obj" not in out and np.array_equal(out["idx"].cpu().numpy() if on_device else out["idx"], want["idx"])
        full = _eng().stein_ksd(_dev(x), _dev(g), ginv, on_device=on_device)
        assert "row_sum" not in full and float(full["ksd2"][0] if on_device else full["ksd2"]) == wf["ksd2"]
    fr = _eng().stein_ksd(_dev(x), _dev(g), ginv, on_device=True, return_rows=True)
    assert np.array_equal(fr["row_sum"].cpu().numpy(), wf["row_sum"])


def test_strided_views_give_the_bits_of_the_packed_copy():
    x, g, ginv, m = _shape_case(0)
    want, wf = _thin_model(0), R.ksd_full(x, g, ginv)
    n, d = x.shape
    discard, thin = 11, 3
    rng = np.random.default_rng(1)
    xl, gl = rng.standard_normal((discard + thin * n, d)), rng.standard_normal((discard + thin * n, d + 5))
    xl[discard::thin], gl[discard::thin, :d] = x, g
    xv, gv = _dev(xl)[discard::thin], _dev(gl)[discard::thin, :d]
    assert xv.stride(0) == thin * d and gv.stride(0) == thin * (d + 5) and not xv.is_contiguous()
    out = _eng().stein_thin(xv, gv, ginv, m, return_obj=True)
    for key in ("idx", "ksd", "obj"):
        assert np.array_equal(out[key], want[key]), key
    full = _eng().stein_ksd(xv, gv, ginv, return_rows=True)
    assert np.array_equal(full["row_sum"], wf["row_sum"]) and full["ksd2"] == wf["ksd2"]


# ---------------------------------------------------------------------------- 5. the full discrepancy of the picks
@pytest.mark.parametrize("i", (0, 3, 6, 8), ids=[IDS[i] for i in (0, 3, 6, 8)])
def test_full_ksd_of_the_picked_rows_is_the_running_value(i):
    """1e-12 relative: the two sums run in different orders"""
    x, g, ginv, m = _shape_case(i)
    want = _thin_model(i)
    p = want["idx"]
    full = _eng().stein_ksd(_dev(x[p]), _dev(g[p]), ginv)
    print(full["ksd"], want["ksd"][-1])
    assert abs(full["ksd"] - want["ksd"][-1]) <= 1e-12 * want["ksd"][-1]


# ---------------------------------------------------------------------------- 6. errors
def test_argument_errors():
    from gpbayestools_hic_amd import _native as nat
    torch, dev = _torch()
    eng = _eng()
    n, d, m = 50, 3, 4
    rng = np.random.default_rng(0)
    x, g = torch.as_tensor(rng.standard_normal((n, d)), device=dev), torch.as_tensor(rng.standard_normal((n, d)), device=dev)
    ginv0 = np.eye(64)[:d, :d].copy()
    idx, ksd, obj = np.full(8, -7, dtype=np.int32), np.full(8, -7.0), np.full(n, -7.0)
    rows, ksd2 = np.full(n, -7.0), np.full(1, -7.0)
    skipped = np.full(1, -7, dtype=np.int64)

    def thin(x=x, g=g, n=n, d=d, xs=d, gs=d, ginv=ginv0, m=m, on_device=0, idx=idx, ksd=ksd, obj=obj, nsk=skipped):
        return eng.lib.gpb_stein_thin(eng.h, nat.ptr(x), nat.ptr(g), n, d, xs, gs, nat.ptr(ginv), m, on_device, nat.ptr(idx),
                                      nat.ptr(ksd), nat.ptr(obj), nat.ptr(nsk))

    def full(x=x, g=g, n=n, d=d, xs=d, gs=d, ginv=ginv0, splits=0, on_device=0, rows=rows, ksd2=ksd2, nsk=skipped):
        return eng.lib.gpb_stein_ksd(eng.h, nat.ptr(x), nat.ptr(g), n, d, xs, gs, nat.ptr(ginv), splits, on_device, nat.ptr(rows),
                                     nat.ptr(ksd2), nat.ptr(nsk))

    def with_value(at, v):
        a = ginv0.copy()
        a[at] = v
        return a
    big = np.zeros((65, 65))
    shared = [(dict(x=None), "x_dev is NULL"), (dict(g=None), "g_dev is NULL"), (dict(n=0), "n outside"), (dict(n=1 << 31), "n outside"),
              (dict(d=0), "d outside"), (dict(d=65, xs=65, gs=65, ginv=big), "d outside"), (dict(xs=d - 1), "x_row_stride"),
              (dict(gs=d - 1), "g_row_stride"), (dict(xs=-d), "x_row_stride"), (dict(ginv=None), "ginv_host is NULL"),
              (dict(ginv=with_value((0, 1), np.nan)), "ginv_host must be finite"), (dict(ginv=with_value((2, 2), np.inf)), "ginv_host must be finite"),
              (dict(ginv=with_value((1, 1), 0.0)), "positive diagonal"), (dict(ginv=with_value((1, 1), -1.0)), "positive diagonal"),
              (dict(on_device=2), "on_device"), (dict(on_device=-1), "on_device"), (dict(nsk=None), "n_skipped is NULL")]
    cases = [(thin, "gpb_stein_thin", shared + [(dict(m=0), "m outside"), (dict(m=(1 << 20) + 1), "m outside"), (dict(idx=None), "idx is NULL"),
                                                  (dict(ksd=None), "ksd is NULL")]),
             (full, "gpb_stein_ksd", shared + [(dict(splits=-1), "splits"), (dict(splits=65), "splits"), (dict(ksd2=None), "ksd2 is NULL")])]
    for fn, name, bad in cases:
        for kw, what in bad:
            assert fn(**kw) == E_ARG, (name, kw)
            msg = eng.lib.gpb_last_error(eng.h).decode()
            assert name in msg and what in msg, (name, kw, msg)
    for a in (idx, ksd, obj, rows, ksd2, skipped):                          # nothing was written
        assert np.all(a == -7)
    assert thin() == 0 and np.all(idx[:m] >= 0) and np.all(idx[m:] == -7) and np.all(ksd[m:] == -7.0) and skipped[0] == 0
    assert thin(obj=None) == 0 and full() == 0 and full(rows=None) == 0 and ksd2[0] > 0
    for call in (lambda: eng.stein_thin(x.cpu(), g, ginv0, m), lambda: eng.stein_thin(x, g[:, :2], ginv0, m),
                 lambda: eng.stein_thin(x, g, np.eye(2), m), lambda: eng.stein_ksd(x.t(), g.t(), np.eye(n)),
                 lambda: eng.stein_ksd(x.float(), g, ginv0),
                 lambda: eng.stein_thin(torch.zeros((4, 65), dtype=torch.float64, device=dev), torch.zeros((4, 65), dtype=torch.float64, device=dev), np.eye(65), 2)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(nat.GPBError):
        eng.stein_thin(x, g, ginv0, 0)


# ---------------------------------------------------------------------------- 7. the Python layer
@functools.lru_cache(maxsize=None)
def _py_case():
    rng = np.random.default_rng(21)
    lo, hi = np.array([-6.0, -5.0, -8.0, -4.0]), np.array([6.0, 7.0, 4.0, 4.5])
    s = np.array([1.0, 0.7, 1.5, 0.4])
    x = rng.standard_normal((700, 4)) * s
    x[13, 2] = lo[2]                                                        # a row on a wall
    return x, -x / s ** 2, lo, hi


@pytest.mark.parametrize("transform", ("logit", None))
@pytest.mark.parametrize("kind", ("id", "med", "sclmed", "smpcov", "diag", "matrix"))
def test_module_functions_are_the_model_on_the_transformed_rows(kind, transform):
    from gpbayestools_hic_amd import SteinDiscrepancy, SteinThinning, thinning as T
    x, g, lo, hi = _py_case()
    pre = np.diag([2.0, 1.0, 3.0, 0.5]) + 0.1 if kind == "matrix" else kind
    res = T.stein_thin(x, g, 25, preconditioner=pre, lo=lo, hi=hi, transform=transform, names=list("abcd"))
    if transform == "logit":
        z, gz = (a.cpu().numpy() for a in T.logit_transform(_dev(x), _dev(g), lo, hi))
        assert not np.isfinite(z[13]).all()
    else:
        z, gz = x, g
    gamma = T.preconditioner_matrix(z, pre)
    want = R.thin(z, gz, T._gamma_inverse(gamma), 25)
    assert isinstance(res, SteinThinning) and np.array_equal(res.gamma, gamma) and res.transform == transform
    assert np.array_equal(res.idx, want["idx"]) and np.array_equal(res.ksd, want["ksd"]) and np.array_equal(res.points, x[want["idx"]])
    walls = int(np.sum(np.any((x <= lo) | (x >= hi), axis=1)))              # row 13 and the few rows of the tails outside the box
    assert res.n_skipped == want["n_skipped"] == (walls if transform == "logit" else 0) and walls >= 1 and res.n_samples == 700
    text = repr(res)
    assert text.startswith("SteinThinning(n_samples=700, ndim=4, m=25") and all(nm in text for nm in "abcd")
    full = T.ksd(x, g, preconditioner=pre, lo=lo, hi=hi, transform=transform)
    wf = R.ksd_full(z, gz, T._gamma_inverse(gamma))
    assert isinstance(full, SteinDiscrepancy) and full.ksd2 == wf["ksd2"] and np.array_equal(full.row_sum, wf["row_sum"], equal_nan=True)
    assert full.n_valid == 700 - want["n_skipped"] and full.ksd == float(np.sqrt(wf["ksd2"])) and repr(full).startswith("SteinDiscrepancy(ksd=")


def test_layouts_defaults_and_savetxt(tmp_path):
    from gpbayestools_hic_amd import thinning as T
    x, g, lo, hi = _py_case()
    a = T.stein_thin(x, g, 10, lo=lo, hi=hi)
    b = T.stein_thin(x.reshape(70, 10, 4), g.reshape(70, 10, 4), 10, lo=lo, hi=hi, layout="steps")
    c = T.stein_thin(_dev(x), _dev(g), 10, lo=lo, hi=hi, transform="logit", preconditioner="sclmed")
    assert np.array_equal(a.idx, b.idx) and np.array_equal(a.idx, c.idx) and np.array_equal(a.ksd, c.ksd) and a.transform == "logit"
    assert T.stein_thin(x, g, 10).transform is None                          # no box: x as it is
    path = str(tmp_path / "picks.txt")
    a.savetxt(path)
    assert np.allclose(np.loadtxt(path), a.points.T, rtol=0, atol=5e-7) and np.loadtxt(path).shape == (4, 10)
    for bad in (dict(lo=lo), dict(lo=lo, hi=hi, transform="probit"), dict(layout="rows"), dict(preconditioner="nope")):
        with pytest.raises(ValueError):
            T.stein_thin(x, g, 10, **bad)
    with pytest.raises(ValueError):
        T.stein_thin(np.zeros((5, 65)), np.zeros((5, 65)), 2)
    with pytest.raises(ValueError):
        T.stein_thin(x, g[:10], 10)


SPECS = [(100, 5, 3, "RBF")]


@functools.lru_cache(maxsize=None)
def _sampler():
    import tempfile
    from gpbayestools_hic_amd import StretchSampler, synth, workload
    chain, _, _ = workload.build_multi_chain(SPECS, 5, workdir=tempfile.mkdtemp(prefix="gpb_stein_"))
    s = StretchSampler(chain, 40, seed=5)
    with pytest.raises(AttributeError):
        s.stein_thin()
    s.run(synth.walkers_ball(40, np.full(5, 0.5), 0.02, seed=6), 30)
    return chain, s


def _same_thinning(a, b):
    return (np.array_equal(a.idx, b.idx) and np.array_equal(a.ksd, b.ksd) and np.array_equal(a.points, b.points)
            and np.array_equal(a.gamma, b.gamma) and a.n_skipped == b.n_skipped and a.n_samples == b.n_samples)


def test_chain_methods(tmp_path):
    import pickle
    from gpbayestools_hic_amd import thinning as T
    chain, s = _sampler()
    host = s.chain                                                           # [nwalkers, nsteps, ndim]
    rows = np.ascontiguousarray(host[:, 6::3]).reshape(-1, 5)               # walker-major
    grad = chain.log_posterior(rows, return_grad=True)[1]
    a = chain.stein_thin(host, m=20, discard=6, thin=3)
    b = T.stein_thin(rows, grad, 20, lo=chain.min, hi=chain.max)
    assert _same_thinning(a, b) and a.names == list(chain.pardict) and a.transform == "logit" and a.n_samples == 40 * 8
    assert np.array_equal(a.points, rows[a.idx]) and np.all(np.isfinite(a.ksd))
    path = str(tmp_path / "chain.pkl")
    with open(path, "wb") as f:
        pickle.dump({"chain": host}, f)
    assert _same_thinning(chain.stein_thin(path, m=20, discard=6, thin=3), b)
    assert _same_thinning(chain.stein_thin(rows, m=20), b)                   # a flat set
    k = chain.ksd(host, discard=6, thin=3, preconditioner=a.gamma)
    kb = T.ksd(rows, grad, lo=chain.min, hi=chain.max, preconditioner=a.gamma)
    assert k.ksd2 == kb.ksd2 and np.array_equal(k.row_sum, kb.row_sum) and k.n_valid == 320
    picks = chain.ksd(a.points, preconditioner=a.gamma)                      # arbitrary rows: the picks against the whole chain
    assert abs(picks.ksd - a.ksd[-1]) <= 1e-12 * a.ksd[-1]
    with pytest.raises(ValueError):
        chain.stein_thin(host, discard=30)
    with pytest.raises(ValueError):
        chain.ksd(np.zeros((4, 3)))


def test_sampler_smc_and_closure_methods_are_the_module_functions_on_the_host_copy():
    from gpbayestools_hic_amd import thinning as T
    from gpbayestools_hic_amd.smc import SMCSampler
    chain, s = _sampler()
    lo, hi = chain.min, chain.max
    for discard, thin in ((0, 1), (6, 3)):
        rows = s._chain_dev[discard::thin].reshape(-1, 5).cpu().numpy()      # step-major, as the store lies
        grad = chain.log_posterior(rows, return_grad=True)[1]
        assert _same_thinning(s.stein_thin(m=15, discard=discard, thin=thin), T.stein_thin(rows, grad, 15, lo=lo, hi=hi))
        a, b = s.ksd(discard=discard, thin=thin), T.ksd(rows, grad, lo=lo, hi=hi)
        assert a.ksd2 == b.ksd2 and np.array_equal(a.row_sum, b.row_sum)
    with pytest.raises(ValueError):
        s.stein_thin(thin=0)
    p = SMCSampler(chain, 256, 0.5, 11)
    p.init_uniform()
    p.run(nmcmc=5)
    x = p.x.cpu().numpy()
    grad = chain.log_posterior(x, return_grad=True)[1]
    assert _same_thinning(p.stein_thin(m=12), T.stein_thin(x, grad, 12, lo=lo, hi=hi))
    assert p.ksd().ksd2 == T.ksd(x, grad, lo=lo, hi=hi).ksd2
    truths = np.random.default_rng(5).uniform(0.3, 0.7, (2, 5))
    res = chain.run_closure(chain.pseudo_data(truths), truths=truths, nsteps=30, nburnsteps=10, nwalkers=12, nthin=1, seed=9)
    rows = np.ascontiguousarray(res.chain[1][:, 3::2]).reshape(-1, 5)        # walker-major
    grad = chain.log_posterior(rows, return_grad=True)[1]
    assert _same_thinning(res.stein_thin(chain, 1, m=9, discard=3, thin=2), T.stein_thin(rows, grad, 9, lo=lo, hi=hi, names=res.names))
    assert res.ksd(chain, 1, discard=3, thin=2).ksd2 == T.ksd(rows, grad, lo=lo, hi=hi).ksd2


@pytest.mark.parametrize("kind", ("id", "sclmed"))
def test_thinning_corrects_a_biased_sample_on_the_device(kind):
    """the mixture case of tests/test_stein_reference.py on the device, the same three conditions: at most 10 of 100 picks from
    the shifted half, the picks' mean within 0.05 of 0, their KSD below 0.3 of all rows'"""
    from gpbayestools_hic_amd import thinning as T
    from test_stein_reference import mixture_case
    x, g = mixture_case()
    res = T.stein_thin(x, g, 100, preconditioner=kind)
    full = T.ksd(x, g, preconditioner=res.gamma)
    shifted, mean = int(np.sum(res.idx >= 1000)), np.abs(res.points.mean(axis=0)).max()
    print(kind, "shifted picks", shifted, "mean", mean, "ksd picks", res.ksd[-1], "ksd all", full.ksd)
    assert shifted <= 10
    assert mean <= 0.05
    assert res.ksd[-1] < 0.3 * full.ksd
