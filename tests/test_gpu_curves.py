"""GPU tier: posterior bands of the parametrised curves, the closure distance and the trace histograms of a resident chain —
gpb_chain_curves / gpb_chain_trace_hist (GPEngine.chain_curves, chain_trace_hist), curves.posterior_curves, closure_delta,
trace_histogram, and the Chain and StretchSampler methods — against the host model of tests/curves_reference.py, which
tests/test_curves_reference.py pins to the notebook's own functions and to np.histogram2d.  The select is compared with the
exact order statistics of the device's OWN values (equality); the values with the model: eta/s, y_loss and the closure distance
bit for bit, zeta/s within 2^-49 relative (device exp and numpy exp each within an ulp of the truth, one rounded multiply on
each side: at most 3 ulp, doubled for the ulp-versus-relative factor).  Counts are integers: equality.  DESIGN.md section 25."""
import functools
import math
import pickle

import numpy as np
import pytest

import curves_reference as R
import marg_reference as M

pytestmark = pytest.mark.gpu

E_ARG = -1
Q1 = (0.5,)
Q7 = tuple(R.levels_q())
# 0 and 1 (k + 1 clamps at S - 1), the median, levels next to both ends, and a spread
Q16 = (0.0, 1.0, 0.5, 1e-12, 1.0 - 1e-12, 0.999, 0.001, 0.16, 0.84, 0.025, 0.975, 0.3333333333333333, 0.25, 0.75, 0.9, 0.61803)
# (nsteps, nwalkers, d, G, levels): every shape of the issue; G in {1, 7, 100, 129} and nq in {1, 7, 16} spread over them
CASES = [(1, 1, 20, 7, Q16), (3, 5, 20, 129, Q7), (64, 4, 20, 100, Q16), (257, 1, 20, 1, Q7), (33, 31, 20, 100, Q1),
         (40, 103, 20, 129, Q16), (70001, 1, 20, 7, Q7), (33, 31, 5, 100, Q7), (3, 5, 5, 1, Q1)]
_ids = lambda c: "%dx%dx%d-G%d-q%d" % (c[0], c[1], c[2], c[3], len(c[4]))                      # noqa: E731


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _eng():
    from gpbayestools_hic_amd import GPEngine
    return GPEngine(0)


def _dev(a):
    torch, dev = _torch()
    return torch.as_tensor(np.array(a), device=dev)


def _setup(case):
    """(desc, grid, aux) of a case: the three curves (d = 5: columns out of order and shared) and the closure distance"""
    n, nw, d, G, q = case
    desc = np.concatenate([R.DESC20 if d == 20 else R.DESC5, R.DELTA_ROW])
    b = R.box(d)
    aux = np.concatenate([0.5 * (b[:, 0] + b[:, 1]) + 0.01, b[:, 1] - b[:, 0]])
    return desc, R.grids(desc, G), aux


@functools.lru_cache(maxsize=None)
def _device(case):
    """the device's order statistics and values of a case, steps layout, host outputs: computed once"""
    n, nw, d, G, q = case
    desc, grid, aux = _setup(case)
    return _eng().chain_curves(_dev(R.chain(n, nw, d)), "steps", desc, grid, q, aux=aux, values=True)


@functools.lru_cache(maxsize=None)
def _model(case):
    n, nw, d, G, q = case
    desc, grid, aux = _setup(case)
    return R.values(R.chain(n, nw, d).reshape(-1, d), desc, grid, aux)


def _zeta_close(got, want):
    """zeta/s: within 2^-49 relative, or 1e-300 absolute where the result is denormal; returns the largest relative error seen"""
    tiny = np.abs(want) < np.finfo(np.float64).tiny
    err = np.abs(got - want)
    assert np.all(err[tiny] <= 1e-300)
    rel = err[~tiny] / np.abs(want[~tiny])
    worst = float(rel.max()) if rel.size else 0.0
    print("zeta/s: largest relative difference %.3g (bound %.3g)" % (worst, 2.0 ** -49))
    assert worst <= 2.0 ** -49
    return worst


# ---------------------------------------------------------------------------- 1. the select against the device's own values
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_select_is_exact_on_the_devices_own_values(case):
    n, nw, d, G, q = case
    out = _device(case)
    assert out["order"].shape == (4, G, len(q), 2) and out["values"].shape == (4, G, n * nw)
    assert np.array_equal(out["order"], R.order_stats(out["values"], q))


# ---------------------------------------------------------------------------- 2. the values against the host model
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_values_and_order_against_the_model(case):
    n, nw, d, G, q = case
    out, ref = _device(case), _model(case)
    assert np.array_equal(out["values"][1:], ref[1:])                                           # eta/s, y_loss, delta: bit for bit
    ref_order = R.order_stats(ref, q)
    assert np.array_equal(out["order"][1:], ref_order[1:])
    _zeta_close(out["values"][0], ref[0])
    _zeta_close(out["order"][0], ref_order[0])                           # (order statistics are 1-Lipschitz in the sup norm)


# ---------------------------------------------------------------------------- 3. percentiles of eta/s and y_loss
@pytest.mark.parametrize("shape", [(33, 31, 20), (40, 103, 20), (257, 1, 20)], ids=lambda s: "x".join(map(str, s)))
def test_percentiles_are_np_percentile(shape):
    from gpbayestools_hic_amd import curves as C
    x = R.chain(*shape)
    res = C.posterior_curves(x, curves=("eta_over_s", "y_loss"), levels=(68, 95, 99.7), truth=x[0, 0])
    assert res.n_samples == shape[0] * shape[1] and list(res) == ["eta_over_s", "y_loss"]
    for nm in res:
        b = res[nm]
        host = C.curve_on_host(nm, x.reshape(-1, 20), C.CURVES[nm]["columns"], C.CURVES[nm]["grid"])      # [S, 100]
        assert np.array_equal(b.median, np.percentile(host, 50, axis=0))
        for CL in (68, 95, 99.7):
            low, high = np.percentile(host, [50 - CL / 2., 50 + CL / 2.], axis=0)
            assert np.array_equal(b.lower[CL], low) and np.array_equal(b.upper[CL], high)
            assert np.array_equal(b.inside[CL], (low <= b.truth_curve) & (b.truth_curve <= high))
        assert np.array_equal(b.truth_curve, host[0])
    assert "truth inside" in repr(res)


# ---------------------------------------------------------------------------- 4. equal bits whatever the route
def _same(a, b, keys=("order", "values")):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in keys)


def test_layouts_views_on_device_and_company():
    case = CASES[5]
    n, nw, d, G, q = case
    eng, joint = _eng(), _device(case)
    desc, grid, aux = _setup(case)
    x = _dev(R.chain(n, nw, d))
    xw = x.permute(1, 0, 2).contiguous()
    assert _same(eng.chain_curves(xw, "walkers", desc, grid, q, aux=aux, values=True), joint)     # the pickles' layout
    dev_out = eng.chain_curves(x, "steps", desc, grid, q, aux=aux, values=True, on_device=True)
    assert all(v.is_cuda for v in dev_out.values())
    assert _same({k: v.cpu().numpy() for k, v in dev_out.items()}, joint)
    assert _same(eng.chain_curves(x, "steps", desc, grid, q, aux=aux), joint, ("order",))         # order without values
    assert _same(eng.chain_curves(x, "steps", desc, grid, None, aux=aux, values=True), joint, ("values",))
    for c in range(4):                                                                            # one curve alone
        one = eng.chain_curves(x, "steps", desc[c:c + 1], grid[c:c + 1], q, aux=aux, values=True)
        assert np.array_equal(one["order"][0], joint["order"][c]) and np.array_equal(one["values"][0], joint["values"][c])
    for layout, full in (("steps", x), ("walkers", xw)):                                          # a thinned view: nothing is copied
        view = full[10::3] if layout == "steps" else full[:, 10::3]
        assert not view.is_contiguous()
        a = eng.chain_curves(view, layout, desc, grid, q, aux=aux, values=True)
        assert _same(a, eng.chain_curves(view.contiguous(), layout, desc, grid, q, aux=aux, values=True))
        ref = R.values(R.chain(n, nw, d)[10::3].reshape(-1, d), desc, grid, aux)
        assert np.array_equal(a["values"][1:], ref[1:]) and np.array_equal(a["order"][1:], R.order_stats(ref, q)[1:])


# ---------------------------------------------------------------------------- 5. massive duplicates
def test_planted_ties():
    """the eta/s columns take three distinct values each: every grid point >= 0.4 is a row of three values, 5000 samples"""
    rng = np.random.default_rng(77)
    x = np.array(R.chain(50, 100, 20, seed=5))
    vals = np.array([[0.05, -0.11, 0.2], [0.07, 0.07000000000000002, 0.3], [0.1, 0.10000000000000002, -0.1]])
    for i, c in enumerate((12, 13, 14)):
        x[:, :, c] = vals[i][rng.integers(0, 3, (50, 100))]
    desc, grid = R.DESC20[1:2], np.linspace(0.0, 0.6, 129)[None, :]
    out = _eng().chain_curves(_dev(x), "steps", desc, grid, Q16, values=True)
    ref = R.values(x.reshape(-1, 20), desc, grid)
    assert len(np.unique(ref[0, -1])) == 3
    assert np.array_equal(out["values"], ref) and np.array_equal(out["order"], R.order_stats(ref, Q16))


# ---------------------------------------------------------------------------- 6. the closure metric
@pytest.mark.parametrize("shape", [(64, 4, 20), (40, 103, 20)], ids=lambda s: "x".join(map(str, s)))
def test_closure_delta(shape):
    from gpbayestools_hic_amd import curves as C
    x = R.chain(*shape)
    S = shape[0] * shape[1]
    pr = R.prior_ranges()
    truth = 0.5 * (pr[:, 0] + pr[:, 1]) + 0.01
    width = pr[:, 1] - pr[:, 0]
    res = C.closure_delta(x, truth, pr, bins=30, quantiles=(0.16, 0.5, 0.84), return_values=True)
    dist = R.curve_value(R.DELTA, x.reshape(-1, 20), 0.0, np.concatenate([truth, width]))
    assert np.array_equal(res.values, dist)
    exact = math.fsum(dist) / S
    print("delta: relative difference from fsum %.3g" % (abs(res.delta - exact) / exact))
    assert abs(res.delta - exact) <= (math.ceil(math.log2(S)) + 8) * 2.0 ** -53 * exact
    hist, edges = np.histogram(dist, bins=30)
    assert np.array_equal(res.hist, hist) and np.array_equal(res.edges, edges) and res.hist.sum() == S
    assert np.array_equal(res.quantiles, np.percentile(dist, [16, 50, 84]))
    per = np.mean(((x.reshape(-1, 20) - truth) / width) ** 2, axis=0)
    assert np.allclose(res.per_parameter, per, rtol=1e-12, atol=0) and abs(res.per_parameter.mean() - exact) <= 1e-12 * exact
    walkers = C.closure_delta(np.ascontiguousarray(x.transpose(1, 0, 2)), truth, pr, layout="walkers", return_values=True)
    assert walkers.delta == res.delta and np.array_equal(walkers.hist, res.hist) and np.array_equal(walkers.values, dist)


# ---------------------------------------------------------------------------- 7. the trace histogram
@pytest.mark.parametrize("B", (1, 30, 64))
def test_trace_hist_matches_the_model(B):
    eng = _eng()
    for n, nw, d in sorted({c[:3] for c in CASES}):
        x3 = R.chain(n, nw, d)
        edges = R.data_edges(x3, B)
        if n * nw > 1:
            edges[0] = np.linspace(edges[0, 0] + 0.1 * (edges[0, B] - edges[0, 0]), edges[0, B], B + 1)    # some walkers outside
        hist, outside = R.trace_counts(x3, edges)
        out = eng.chain_trace_hist(_dev(x3), "steps", edges)
        assert out["hist"].dtype == np.int64 and out["hist"].shape == (d, n, B)
        assert np.array_equal(out["hist"], hist) and np.array_equal(out["outside"], outside)
        assert np.array_equal(out["hist"].sum(axis=2) + out["outside"], np.full((d, n), nw))
        if n * nw <= 5000:
            w = eng.chain_trace_hist(_dev(x3).permute(1, 0, 2).contiguous(), "walkers", edges, on_device=True)
            assert np.array_equal(w["hist"].cpu().numpy(), hist) and np.array_equal(w["outside"].cpu().numpy(), outside)
            only = eng.chain_trace_hist(_dev(x3), "steps", edges, outputs=("hist",))
            assert list(only) == ["hist"] and np.array_equal(only["hist"], hist)


@pytest.mark.parametrize("B", (1, 30, 64))
def test_trace_hist_planted_edges_nan_and_infinities(B):
    """every edge with both one-ulp neighbours, values beyond both ends, NaN and the infinities: as the walkers of one step,
    as the steps of one walker, and spread over the steps of several walkers, in both layouts"""
    eng, d = _eng(), 3
    for uniform in (True, False):
        edges = M.edges_of(d, B, uniform=uniform, seed=B)
        x = M.planted(edges)
        x = x[: x.shape[0] // 3 * 3]
        for x3 in (x[None, :, :], x[:, None, :], x.reshape(3, -1, d), x.reshape(-1, 3, d)):
            hist, outside = R.trace_counts(x3, edges)
            assert outside.sum() >= 7 * d - 9
            for layout, xd in (("steps", _dev(x3)), ("walkers", _dev(x3).permute(1, 0, 2).contiguous())):
                out = eng.chain_trace_hist(xd, layout, edges)
                assert np.array_equal(out["hist"], hist) and np.array_equal(out["outside"], outside)


def test_trace_histogram_is_the_notebooks_histogram2d():
    from gpbayestools_hic_amd import curves as C
    n, nw, d = 64, 4, 20
    x3 = R.chain(n, nw, d)
    xw = np.ascontiguousarray(x3.transpose(1, 0, 2))                                              # [nwalkers, nsteps, d], a pickle's
    res = C.trace_histogram(xw, bins=30, layout="walkers")
    for j in range(d):
        h2, xe, ye = np.histogram2d(np.tile(np.arange(n), nw), xw[:, :, j].reshape(-1), bins=[n, 30])
        assert np.array_equal(res.hist[j], h2.astype(np.int64)) and np.array_equal(res.edges[j], ye)
    assert not res.outside.any()


# ---------------------------------------------------------------------------- 8. errors
def test_argument_errors():
    from gpbayestools_hic_amd import _native as nat
    torch, dev = _torch()
    eng = _eng()
    n, nw, d, G, nq = 20, 4, 6, 5, 3
    x = torch.full((n, nw, d), 0.1, dtype=torch.float64, device=dev)
    good_desc = np.array([[0, 0, 1, 2, 3], [1, 3, 4, 5, -1], [2, 0, 1, 2, -1]], dtype=np.int32)
    good_grid = np.tile(np.linspace(0.0, 0.5, G), (3, 1))
    good_aux = np.concatenate([np.zeros(d), np.ones(d)])
    good_q = np.array([0.1, 0.5, 0.9])
    order = np.full((3, G, nq, 2), -7.0)
    values = np.full((3, G, n * nw), -7.0)
    big = 1 << 31

    def rc(n=n, nw=nw, d=d, ss=nw * d, ws=d, desc=good_desc, aux=good_aux, grid=good_grid, G=G, q=good_q, nq=nq, want_order=True,
           want_values=True, ldv=n * nw):
        desc = np.ascontiguousarray(np.asarray(desc, dtype=np.int32).reshape(-1, 5))
        return eng.lib.gpb_chain_curves(eng.h, nat.ptr(x), n, nw, d, ss, ws, desc.shape[0], nat.ptr(desc),
                                        nat.ptr(None if aux is None else np.ascontiguousarray(aux)),
                                        nat.ptr(np.ascontiguousarray(grid)), G, nat.ptr(np.ascontiguousarray(q)), nq, 0,
                                        nat.ptr(order) if want_order else None, nat.ptr(values) if want_values else None, ldv)

    assert rc() == 0 and not np.any(order == -7.0) and not np.any(values == -7.0)
    assert rc(nq=0, want_order=False) == 0                                                       # nq is judged when order is requested
    order[:], values[:] = -7.0, -7.0

    def desc_with(c, i, v):
        k = good_desc.copy()
        k[c, i] = v
        return k

    def at(a, i, v):
        a = np.array(a, dtype=np.float64)
        a.reshape(-1)[i] = v
        return a
    delta = np.array([[3, -1, -1, -1, -1]])
    bad = [(dict(n=0), "nsteps >= 1"), (dict(nw=0), "nwalkers >= 1"), (dict(d=0), "d >= 1"),
           (dict(n=big), "2^31 - 1"), (dict(n=1 << 20, nw=1 << 12, ss=d << 12), "nsteps nwalkers above"),
           (dict(ws=d - 1), "stride below d"), (dict(ss=d - 1, ws=n * d), "stride below d"),
           (dict(ss=nw * d - 1), "neither stride spans"), (dict(ss=d, ws=n * d - 1), "neither stride spans"),
           (dict(desc=np.tile(good_desc, (3, 1))), "ncurves outside"),
           (dict(G=0), "G outside"), (dict(G=1025), "G outside"),
           (dict(nq=0), "nq outside"), (dict(nq=17), "nq outside"),
           (dict(q=at(good_q, 1, -0.01)), "level outside"), (dict(q=at(good_q, 2, 1.0000001)), "level outside"),
           (dict(q=at(good_q, 0, np.nan)), "level outside"),
           (dict(desc=desc_with(1, 0, 4)), "fn outside"), (dict(desc=desc_with(0, 0, -1)), "fn outside"),
           (dict(desc=desc_with(0, 4, d)), "column outside"), (dict(desc=desc_with(0, 4, -1)), "column outside"),
           (dict(desc=desc_with(2, 3, -1)), "column outside"), (dict(desc=desc_with(1, 1, d + 3)), "column outside"),
           (dict(desc=delta, aux=None), "needs aux"),
           (dict(desc=delta, aux=at(good_aux, d + 2, 0.0)), "width"), (dict(desc=delta, aux=at(good_aux, d, -1.0)), "width"),
           (dict(desc=delta, aux=at(good_aux, 2 * d - 1, np.inf)), "width"), (dict(desc=delta, aux=at(good_aux, d + 1, np.nan)), "width"),
           (dict(desc=delta, aux=at(good_aux, 1, np.nan)), "truth"),
           (dict(ldv=n * nw - 1), "ldv < S"),
           (dict(grid=at(good_grid, 7, np.nan)), "grid value"), (dict(grid=at(good_grid, 0, np.inf)), "grid value")]
    for kw, what in bad:
        assert rc(**kw) == E_ARG, kw
        msg = eng.lib.gpb_last_error(eng.h).decode()
        assert "gpb_chain_curves" in msg and what in msg, (kw, msg)
    assert np.all(order == -7.0) and np.all(values == -7.0)                                      # nothing was written
    assert rc(desc=desc_with(1, 4, 99)) == 0                                                     # col3 of a three-parameter curve is ignored
    assert rc(ss=d, ws=n * d) == 0                                                               # the other layout's strides are fine

    B = 5
    good_edges = M.edges_of(d, B)
    hist = np.full((d, n, B), -7, dtype=np.int64)

    def rt(n=n, nw=nw, d=d, ss=nw * d, ws=d, edges=good_edges, B=B):
        return eng.lib.gpb_chain_trace_hist(eng.h, nat.ptr(x), n, nw, d, ss, ws, nat.ptr(np.ascontiguousarray(edges)), B, 0,
                                            nat.ptr(hist), None)
    assert rt() == 0 and hist.sum() == n * nw * d
    hist[:] = -7
    bad = [(dict(n=0), "nsteps >= 1"), (dict(nw=0), "nwalkers >= 1"), (dict(d=0), "d >= 1"), (dict(n=big), "2^31 - 1"),
           (dict(ws=d - 1), "stride below d"), (dict(ss=nw * d - 1), "neither stride spans"),
           (dict(B=0), "B outside"), (dict(B=65), "B outside"),
           (dict(edges=at(good_edges, 3, np.nan)), "edges"), (dict(edges=at(good_edges, B, np.inf)), "edges"),
           (dict(edges=at(good_edges, 3, good_edges[0, 2])), "strictly increasing"), (dict(edges=good_edges[:, ::-1]), "strictly increasing")]
    for kw, what in bad:
        assert rt(**kw) == E_ARG, kw
        msg = eng.lib.gpb_last_error(eng.h).decode()
        assert "gpb_chain_trace_hist" in msg and what in msg, (kw, msg)
    assert np.all(hist == -7)
    with pytest.raises(ValueError):
        eng.chain_curves(x, "rows", good_desc, good_grid, good_q)
    with pytest.raises(ValueError):
        eng.chain_curves(x.cpu(), "steps", good_desc, good_grid, good_q)
    with pytest.raises(ValueError):
        eng.chain_trace_hist(x, "steps", good_edges[:2])


# ---------------------------------------------------------------------------- 9. the public surface
def _chain_object(tmp_path):
    from gpbayestools_hic_amd import synth
    from gpbayestools_hic_amd.mcmc import Chain
    pf, ep = str(tmp_path / "par.txt"), str(tmp_path / "exp.pkl")
    pr = R.prior_ranges()
    synth.write_parameter_file(pf, pr[:, 0], pr[:, 1])
    with open(ep, "wb") as f:
        pickle.dump({"0": {"obs": np.array([[1.0], [0.1]])}}, f)
    return Chain(mcmc_path=str(tmp_path / "mcmc" / "c.pkl"), expdata_path=ep, model_parafile=pf)


def _bands_equal(a, b):
    for nm in a:
        for k in ("grid", "median", "percentiles", "truth_curve"):
            assert np.array_equal(getattr(a[nm], k), getattr(b[nm], k)), (nm, k)
        for lv in a.levels:
            assert np.array_equal(a[nm].lower[lv], b[nm].lower[lv]) and np.array_equal(a[nm].upper[lv], b[nm].upper[lv])
            assert np.array_equal(a[nm].inside[lv], b[nm].inside[lv])
    return a.n_samples == b.n_samples and list(a) == list(b)


def test_chain_methods(tmp_path):
    from gpbayestools_hic_amd import curves as C
    ch = _chain_object(tmp_path)
    stored = np.ascontiguousarray(R.chain(64, 4, 20).transpose(1, 0, 2))                          # [nwalkers, nsteps, 20]
    truth = stored[1, 5]
    a = ch.posterior_curves(stored, discard=10, thin=3, truth=truth)
    view = stored[:, 10::3]
    assert _bands_equal(a, C.posterior_curves(view, layout="walkers", truth=truth)) and a.n_samples == 4 * 18
    host = C.curve_on_host("y_loss", view.transpose(1, 0, 2).reshape(-1, 20), (2, 3, 4), a["y_loss"].grid)
    assert np.array_equal(a["y_loss"].upper[95], np.percentile(host, 97.5, axis=0))
    ch.chain = stored
    assert _bands_equal(ch.posterior_curves(discard=10, thin=3, truth=truth), a)
    cd = ch.closure_delta(truth, discard=10, thin=3)
    ref = C.closure_delta(view, truth, R.prior_ranges(), layout="walkers")
    assert cd.delta == ref.delta and np.array_equal(cd.hist, ref.hist) and cd.names == list(ch.pardict)
    tr = ch.trace_histogram(discard=10, thin=3)
    assert tr.hist.shape == (20, 18, 30) and np.array_equal(tr.hist, C.trace_histogram(view, layout="walkers").hist)
    with pytest.raises(ValueError):
        ch.trace_histogram(stored.reshape(-1, 20))


def test_sampler_methods():
    """a short run of 8 walkers over 4 parameters: eta/s and y_loss of columns (0, 1, 2) / (3, 1, 0) of the stored chain"""
    from gpbayestools_hic_amd import LoggingEnsembleSampler
    from gpbayestools_hic_amd import curves as C
    s = LoggingEnsembleSampler(8, 4, lambda X: -0.5 * np.sum((X / np.array([1.0, 3.0, 0.5, 2.0])) ** 2, axis=1), seed=11)
    s.run_mcmc(np.random.default_rng(2).standard_normal((8, 4)), 60)
    kw = dict(curves=("eta_over_s", "y_loss"), columns={"eta_over_s": (0, 1, 2), "y_loss": (3, 1, 0)}, levels=(68, 95))
    for discard, thin in ((0, 1), (20, 3)):
        a = s.curves(discard=discard, thin=thin, **kw)
        host = s.chain[:, discard::thin]                                                         # [nwalkers, nsteps, ndim], the host copy
        b = C.posterior_curves(host, layout="walkers", **kw)
        for nm in a:
            assert np.array_equal(a[nm].percentiles, b[nm].percentiles), nm
        flat = host.transpose(1, 0, 2).reshape(-1, 4)
        assert np.array_equal(a["eta_over_s"].median, np.percentile(C.curve_on_host("eta_over_s", flat, (0, 1, 2), a["eta_over_s"].grid),
                                                                    50, axis=0))
        tr = s.trace_histogram(discard=discard, thin=thin, bins=12)
        assert np.array_equal(tr.hist, C.trace_histogram(host, bins=12, layout="walkers").hist)
        box = np.array([[-9.0, 9.0]] * 4)
        cd = s.closure_delta(np.zeros(4), prior_ranges=box, discard=discard, thin=thin)
        assert cd.delta == C.closure_delta(host, np.zeros(4), box, layout="walkers").delta


def test_weighted_particle_set_takes_the_host_path(tmp_path):
    """a pocoMC / run_SMC pickle's chain [S, ndim] and weights: weighted_quantile of the host-evaluated curves"""
    from gpbayestools_hic_amd import curves as C
    rng = np.random.default_rng(12)
    S = 3001
    x = R.chain(S, 1, 20, seed=9).reshape(S, 20)
    w = rng.exponential(1.0, S)
    ch = _chain_object(tmp_path)
    res = ch.posterior_curves(x, weights=w, levels=(68, 95))
    for nm in res:
        host = C.curve_on_host(nm, x, C.CURVES[nm]["columns"], C.CURVES[nm]["grid"])
        assert np.array_equal(res[nm].percentiles, M.weighted_quantile(host, w, res[nm].q))
    truth = x[17]
    cd = ch.closure_delta(truth, x, weights=w)
    pr = R.prior_ranges()
    dist = R.curve_value(R.DELTA, x, 0.0, np.concatenate([truth, pr[:, 1] - pr[:, 0]]))
    assert abs(cd.delta - np.sum(dist * w) / w.sum()) <= 1e-14 * cd.delta
    assert np.array_equal(cd.hist, np.histogram(dist, bins=30, weights=w)[0])
    with pytest.raises(ValueError):
        C.posterior_curves(np.zeros((4, 2, 20)), weights=np.ones(4))
    with pytest.raises(ValueError):
        ch.posterior_curves(x, weights=-w)
