"""GPU tier: corner-plot marginals of a resident chain — gpb_chain_marginals (GPEngine.chain_marginals), marginals.marginals,
StretchSampler.marginals and Chain.posterior_marginals — against the host model of tests/marg_reference.py, which
tests/test_marg_reference.py pins to np.histogram and np.histogram2d.  Every comparison of counts is exact integer equality: the
library accumulates integers only, so there is no tolerance to choose.  Percentiles: np.array_equal with np.percentile.
DESIGN.md section 19."""
import functools
import pickle

import numpy as np
import pytest

import cv_reference as CV
import marg_reference as R

pytestmark = pytest.mark.gpu

E_ARG = -1
KEYS = ("h1", "h2", "outside")


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


@functools.lru_cache(maxsize=None)
def _dev_chain(shape3, layout="steps"):
    x = _dev(R.chain(*shape3))
    return x if layout == "steps" else x.permute(1, 0, 2).contiguous()


@functools.lru_cache(maxsize=None)
def _joint(shape):
    """the device's answer for a shape of R.SHAPES, steps layout, uniform edges, all pairs, host outputs: computed once"""
    n, nw, d, B = shape
    return _eng().chain_marginals(_dev_chain((n, nw, d)), "steps", R.edges_of(d, B))


@functools.lru_cache(maxsize=None)
def _model(shape, uniform=True):
    n, nw, d, B = shape
    return dict(zip(KEYS, R.counts(R.chain(n, nw, d), R.edges_of(d, B, uniform=uniform))))


def _same(a, b, keys=KEYS):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) and np.asarray(a[k]).shape == np.asarray(b[k]).shape for k in keys)


_ids = lambda s: "x".join(str(v) for v in s)                                                   # noqa: E731


# ---------------------------------------------------------------------------- 1. against the host model
@pytest.mark.parametrize("shape", R.SHAPES, ids=_ids)
def test_counts_match_the_model(shape):
    n, nw, d, B = shape
    out = _joint(shape)
    assert out["h1"].dtype == np.int64 and out["h1"].shape == (d, B) and out["h2"].shape == (d * (d - 1) // 2, B, B)
    assert _same(out, _model(shape))
    assert np.array_equal(out["h1"].sum(axis=1) + out["outside"], np.full(d, n * nw))


@pytest.mark.parametrize("shape", R.SHAPES[1:4], ids=_ids)
def test_nonuniform_edges(shape):
    n, nw, d, B = shape
    out = _eng().chain_marginals(_dev_chain((n, nw, d)), "steps", R.edges_of(d, B, uniform=False))
    assert _same(out, _model(shape, uniform=False))


@pytest.mark.parametrize("B", (1, 7, 20, 64))
def test_planted_edges_outside_values_and_nan(B):
    """every edge with both one-ulp neighbours, values beyond both ends, NaN and the infinities: as a flat set and as walkers"""
    d = 3
    for uniform in (True, False):
        edges = R.edges_of(d, B, uniform=uniform, seed=B)
        x = R.planted(edges)
        ref = dict(zip(KEYS, R.counts(x, edges)))
        assert ref["outside"].min() >= 7
        assert _same(_eng().chain_marginals(_dev(x)[:, None, :], "steps", edges), ref)
        assert _same(_eng().chain_marginals(_dev(x)[None, :, :], "steps", edges), ref)


# ---------------------------------------------------------------------------- 2. equal counts whatever the route
@pytest.mark.parametrize("shape", R.SHAPES, ids=_ids)
def test_layouts_on_device_outputs_alone_and_second_call(shape):
    n, nw, d, B = shape
    eng, edges, joint = _eng(), R.edges_of(d, B), _joint(shape)
    x = _dev_chain((n, nw, d))
    assert _same(eng.chain_marginals(x, "steps", edges), joint)                                  # a second call
    assert _same(eng.chain_marginals(_dev_chain((n, nw, d), "walkers"), "walkers", edges), joint)  # the pickles' layout
    dev_out = eng.chain_marginals(x, "steps", edges, on_device=True)
    assert all(v.is_cuda for v in dev_out.values())
    assert _same({k: v.cpu().numpy() for k, v in dev_out.items()}, joint)
    for k in KEYS:
        one = eng.chain_marginals(x, "steps", edges, outputs=(k,))
        assert list(one) == [k] and _same(one, joint, (k,))


@pytest.mark.parametrize("layout", ("steps", "walkers"))
def test_thinned_view_is_the_thinned_copy(layout):
    eng = _eng()
    n, nw, d, B = R.SHAPES[3]
    edges = R.edges_of(d, B)
    x = _dev_chain((n, nw, d), layout)
    view = x[3::2] if layout == "steps" else x[:, 3::2]
    assert not view.is_contiguous()
    a = eng.chain_marginals(view, layout, edges)
    assert _same(a, eng.chain_marginals(view.contiguous(), layout, edges))
    assert _same(a, dict(zip(KEYS, R.counts(R.chain(n, nw, d)[3::2], edges))))


def test_pair_subset_in_arbitrary_order():
    """a few pairs, out of order, (j, i) with j > i among them and one pair twice: the all-pairs call's tables, transposed for (j, i)"""
    n, nw, d, B = R.SHAPES[3]
    joint, allp = _joint(R.SHAPES[3]), [tuple(p) for p in R.all_pairs(d)]
    pairs = [(7, 2), (0, 1), (11, 10), (3, 9), (0, 1), (5, 4)]
    out = _eng().chain_marginals(_dev_chain((n, nw, d)), "steps", R.edges_of(d, B), pairs=pairs)
    assert out["h2"].shape == (len(pairs), B, B) and _same(out, joint, ("h1", "outside"))
    for p, (i, j) in enumerate(pairs):
        ref = joint["h2"][allp.index((i, j))] if i < j else joint["h2"][allp.index((j, i))].T
        assert np.array_equal(out["h2"][p], ref), (i, j)


@pytest.mark.parametrize("B", (20, 64))
def test_concentrated_chain(B):
    """50 000 identical samples: one bin holds everything; then a chain confined to three bins of every parameter"""
    eng, d, S = _eng(), 4, 50000
    edges = R.edges_of(d, B)
    x = np.tile(np.array([0.3, -0.7, 1.1, 0.0]), (S, 1))
    out = eng.chain_marginals(_dev(x)[:, None, :], "steps", edges)
    c = R.codes(x[:1], edges)[0].astype(int)
    assert np.all(out["outside"] == 0) and out["h1"].sum() == d * S and out["h2"].sum() == 6 * S
    for j in range(d):
        assert out["h1"][j, c[j]] == S
    for p, (i, j) in enumerate(R.all_pairs(d)):
        assert out["h2"][p, c[i], c[j]] == S
    mid = 0.5 * (edges[:, B // 2 - 1: B // 2 + 2] + edges[:, B // 2: B // 2 + 3])               # the centres of three adjacent bins
    pick = np.random.default_rng(6).integers(0, 3, (S, d))
    x3 = mid[np.arange(d)[None, :], pick]
    out = eng.chain_marginals(_dev(x3).reshape(500, 100, d), "steps", edges)
    assert _same(out, dict(zip(KEYS, R.counts(x3, edges))))
    assert np.count_nonzero(out["h1"]) == 3 * d and np.count_nonzero(out["h2"]) == 9 * 6 and np.all(out["outside"] == 0)


def test_weighted():
    """S = 4099 particles, weights over 12 decades: the integer model; equal weights: 2^32 times the plain counts"""
    n, nw, d, B = R.SHAPES[4]
    eng, edges = _eng(), R.edges_of(d, B)
    x = _dev_chain((n, nw, d))
    w = 10.0 ** np.random.default_rng(9).uniform(-12.0, 0.0, n)
    ref = dict(zip(KEYS, R.counts(R.chain(n, nw, d), edges, q=R.int_weights(w))))
    out = eng.chain_marginals(x, "steps", edges, weights=w)
    assert _same(out, ref) and out["h2"].max() >= 1 << 32
    assert _same(eng.chain_marginals(x.permute(1, 0, 2), "walkers", edges, weights=_dev(w)), ref)    # device weights, the other layout
    for k in KEYS:
        assert _same(eng.chain_marginals(x, "steps", edges, weights=w, outputs=(k,)), ref, (k,))
    same = eng.chain_marginals(x, "steps", edges, weights=np.full(n, 0.37))
    plain = _joint(R.SHAPES[4])
    assert all(np.array_equal(same[k], plain[k] << 32) for k in KEYS)
    # B = 64: one 64-bit table per workgroup
    e64 = R.edges_of(d, 64)
    out = eng.chain_marginals(x, "steps", e64, weights=w, pairs=[(0, 1), (19, 3), (4, 5)])
    assert _same(out, dict(zip(KEYS, R.counts(R.chain(n, nw, d), e64, pairs=[(0, 1), (19, 3), (4, 5)], q=R.int_weights(w)))))


def test_sample_groups():
    """the debug library takes a workspace cap (option key 52; the product library refuses it): 4099 samples of 20 parameters in
    groups of 50, and weighted in groups of 35, against the single group of the product library"""
    from conftest import debug_engine
    n, nw, d, B = R.SHAPES[4]
    edges, x = R.edges_of(d, B), _dev_chain((n, nw, d))
    with pytest.raises(Exception):
        _eng().tune("marg_ws_bytes", 1000)
    dbg = debug_engine()
    dbg.tune("marg_ws_bytes", 1000)
    assert _same(dbg.chain_marginals(x, "steps", edges), _joint(R.SHAPES[4]))
    w = 10.0 ** np.random.default_rng(9).uniform(-12.0, 0.0, n)
    assert _same(dbg.chain_marginals(x, "steps", edges, weights=w), _eng().chain_marginals(x, "steps", edges, weights=w))
    n, nw, d, B = R.SHAPES[3]
    dbg.tune("marg_ws_bytes", 12 * 100)                                                          # groups that cut through the walkers of a step
    for layout in ("steps", "walkers"):
        assert _same(dbg.chain_marginals(_dev_chain((n, nw, d), layout), layout, R.edges_of(d, B)), _joint(R.SHAPES[3]))
    dbg.tune("marg_ws_bytes", 0)


# ---------------------------------------------------------------------------- 3. errors, and the context stays as it was
def test_argument_errors():
    from gpbayestools_hic_amd import _native as nat
    torch, dev = _torch()
    eng = _eng()
    n, nw, d, B = 20, 4, 3, 5
    x = torch.zeros((n, nw, d), dtype=torch.float64, device=dev)
    wdev = torch.ones(n, dtype=torch.float64, device=dev)
    good = R.edges_of(d, B)
    h1 = np.full((d, B), -7, dtype=np.int64)
    h2 = np.full((3, B, B), -7, dtype=np.int64)
    big = 1 << 31

    def rc(n=n, nw=nw, d=d, ss=nw * d, ws=d, edges=good, B=B, pairs=None, npairs=3, w=None, wscale=1.0, want_h2=True):
        pairs = None if pairs is None else np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
        return eng.lib.gpb_chain_marginals(eng.h, nat.ptr(x), n, nw, d, ss, ws, nat.ptr(np.ascontiguousarray(edges)), B, nat.ptr(pairs),
                                           npairs, nat.ptr(w), wscale, 0, nat.ptr(h1), nat.ptr(h2) if want_h2 else None, None)

    assert rc() == 0 and h1[:, 2].tolist() == [n * nw] * d and h2.sum() == 3 * n * nw          # (the valid call: zeros, the middle bin)
    assert rc(npairs=17, want_h2=False) == 0                                                    # npairs is checked when h2 is requested
    h1[:], h2[:] = -7, -7

    def edges_with(j, b, v):
        e = good.copy()
        e[j, b] = v
        return e
    bad = [(dict(n=0), "nsteps >= 1"), (dict(nw=0), "nwalkers >= 1"), (dict(d=0), "d >= 1"),
           (dict(n=big), "2^31 - 1"), (dict(nw=big, ss=big * d), "2^31 - 1"), (dict(d=big, ws=big, ss=nw * big), "2^31 - 1"),
           (dict(B=0), "B outside"), (dict(B=65), "B outside"),
           (dict(edges=edges_with(1, 2, np.nan)), "edges"), (dict(edges=edges_with(0, B, np.inf)), "edges"),
           (dict(edges=edges_with(2, 3, good[2, 2])), "strictly increasing"), (dict(edges=good[:, ::-1]), "strictly increasing"),
           (dict(pairs=[(0, 1), (1, 3), (0, 2)]), "pair index"), (dict(pairs=[(0, 1), (-1, 2), (0, 2)]), "pair index"),
           (dict(pairs=[(0, 1), (2, 2), (0, 2)]), "pair (i, i)"),
           (dict(npairs=2), "d (d - 1) / 2"), (dict(npairs=-1), "npairs < 0"),
           (dict(npairs=(big - 1) // (B * B) + 1, want_h2=False), "npairs B^2"),      # (no list and no h2: the count alone is judged)
           (dict(ws=d - 1), "stride below d"), (dict(ss=d - 1, ws=n * d), "stride below d"), (dict(ws=-d), "stride below d"),
           (dict(ss=nw * d - 1), "neither stride spans"), (dict(ss=d, ws=n * d - 1), "neither stride spans"),
           (dict(w=wdev), "nwalkers == 1"),
           (dict(nw=1, ss=d, w=wdev, wscale=0.0), "wscale"), (dict(nw=1, ss=d, w=wdev, wscale=-1.0), "wscale"),
           (dict(nw=1, ss=d, w=wdev, wscale=float("inf")), "wscale"), (dict(nw=1, ss=d, w=wdev, wscale=float("nan")), "wscale")]
    for kw, what in bad:
        assert rc(**kw) == E_ARG, kw
        msg = eng.lib.gpb_last_error(eng.h).decode()
        assert "gpb_chain_marginals" in msg and what in msg, (kw, msg)
    assert np.all(h1 == -7) and np.all(h2 == -7)                                                 # nothing was written
    assert rc(ss=d, ws=n * d) == 0                                                               # the other layout's strides are fine
    assert rc(nw=1, ss=d, w=wdev, wscale=2.0) == 0 and h1[:, 2].tolist() == [2 * n] * d
    with pytest.raises(ValueError):
        eng.chain_marginals(x, "rows", good)
    with pytest.raises(ValueError):
        eng.chain_marginals(x.cpu(), "steps", good)
    with pytest.raises(ValueError):
        eng.chain_marginals(x.permute(0, 2, 1), "steps", good)                                   # the parameters must have unit stride
    with pytest.raises(ValueError):
        eng.chain_marginals(x, "steps", good[:2])


def test_predict_is_untouched():
    """a context with a factorised GP: predict, marginals on the same context, predict again — the same bits"""
    from gpbayestools_hic_amd import GPEngine
    X, Z = CV.make_data(100, 3, 3, 21)
    eng = GPEngine(0)
    eng.set_data(X, 0.3 * Z, "RBF", CV.ALPHA)
    eng.set_theta(CV.thetas_of(("mid", "hard", "aniso"), 3))
    eng.factor()
    Xs = np.random.default_rng(8).uniform(0.0, 1.0, (130, 3))
    before = eng.predict(Xs, return_var=True)
    n, nw, d, B = R.SHAPES[2]
    assert _same(eng.chain_marginals(_dev_chain((n, nw, d)), "steps", R.edges_of(d, B)), _joint(R.SHAPES[2]))
    after = eng.predict(Xs, return_var=True)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))


# ---------------------------------------------------------------------------- 4. Python
QS = (0.05, 0.16, 0.5, 0.84, 0.95)


def test_marginals_percentiles_and_prior_box():
    """marginals.marginals on a device view and Chain.posterior_marginals on a [nwalkers, nsteps, ndim] array: np.percentile exactly,
    np.histogram2d over the given box, density1d, credible levels and the table"""
    from gpbayestools_hic_amd.marginals import marginals
    n, nw, d = 257, 16, 4
    x = R.chain(n, nw, d)
    flat = x[20::2].reshape(-1, d)
    box = np.stack([np.full(d, -2.0), np.array([2.0, 2.5, 1.0, 3.0])], axis=1)
    m = marginals(_dev_chain((n, nw, d))[20::2], bins=20, range=box, names=list("abcd"))
    assert m.n_samples == flat.shape[0] and m.hist1d.shape == (d, 20) and m.hist2d.shape == (6, 20, 20)
    assert np.array_equal(m.percentiles, np.percentile(flat, [100 * q for q in QS], axis=0))
    p16, p50, p84 = np.percentile(flat, [16, 50, 84], axis=0)
    assert np.array_equal(m.median, p50) and np.array_equal(m.lower, p50 - p16) and np.array_equal(m.upper, p84 - p50)
    for p, (i, j) in enumerate(m.pairs):
        ref = np.histogram2d(flat[:, i], flat[:, j], bins=20, range=[box[i], box[j]])[0]
        assert np.array_equal(m.hist2d[p], ref.astype(np.int64)) and np.array_equal(m.pair(j, i), ref.T.astype(np.int64))
    inside = m.hist1d.sum(axis=1) / m.n_samples
    assert m.outside.min() > 0 and np.allclose((m.density1d() * np.diff(m.edges, axis=1)).sum(axis=1), inside, rtol=1e-13, atol=0)
    assert np.array_equal(m.credible_levels(0, 1), R.credible_levels(m.pair(0, 1)))
    assert "PosteriorMarginals(n_samples=%d" % flat.shape[0] in repr(m) and " c " in repr(m)
    # quantiles of the caller's own, without the band's levels: the band is still there
    m2 = marginals(flat, bins=m.edges, quantiles=(0.25,), pairs=[(3, 1)])
    assert np.array_equal(m2.percentiles, np.percentile(flat, [25], axis=0)) and np.array_equal(m2.median, p50)
    assert np.array_equal(m2.hist1d, m.hist1d) and np.array_equal(m2.hist2d[0], m.pair(3, 1))


def test_data_range_is_the_notebooks_hist2d():
    """range="data" (and None): np.histogram2d(a, b, bins=20) and np.histogram(a, bins=20), a constant column included"""
    from gpbayestools_hic_amd.marginals import marginals
    x = np.array(R.chain(300, 7, 3))
    x[:, :, 2] = 0.25
    flat = x.reshape(-1, 3)
    for m in (marginals(x, bins=20, range="data"), marginals(x.transpose(1, 0, 2), bins=20, layout="walkers")):
        assert np.all(m.outside == 0)
        for j in range(3):
            n, e = np.histogram(flat[:, j], bins=20)
            assert np.array_equal(m.edges[j], e) and np.array_equal(m.hist1d[j], n)
            assert np.allclose(m.density1d()[j], np.histogram(flat[:, j], bins=20, density=True)[0], rtol=1e-14, atol=0)
        for p, (i, j) in enumerate(m.pairs):
            assert np.array_equal(m.hist2d[p], np.histogram2d(flat[:, i], flat[:, j], bins=20)[0].astype(np.int64))


@functools.lru_cache(maxsize=None)
def _sampler():
    """LoggingEnsembleSampler over a host Gaussian log-probability: 8 walkers, 2 parameters, 200 steps"""
    from gpbayestools_hic_amd import LoggingEnsembleSampler
    s = LoggingEnsembleSampler(8, 2, lambda X: -0.5 * np.sum((X / np.array([1.0, 3.0])) ** 2, axis=1), seed=11)
    s.run_mcmc(np.random.default_rng(2).standard_normal((8, 2)), 200)
    return s


def _chain_object(tmp_path):
    from gpbayestools_hic_amd import synth
    from gpbayestools_hic_amd.mcmc import Chain
    pf, ep = str(tmp_path / "par.txt"), str(tmp_path / "exp.pkl")
    synth.write_parameter_file(pf, -4.0 * np.ones(2), np.array([4.0, 6.0]))
    with open(ep, "wb") as f:
        pickle.dump({"0": {"obs": np.array([[1.0], [0.1]])}}, f)
    return Chain(mcmc_path=str(tmp_path / "mcmc" / "c.pkl"), expdata_path=ep, model_parafile=pf)


def test_sampler_and_chain_methods(tmp_path):
    from gpbayestools_hic_amd.marginals import marginals
    s = _sampler()
    box = np.array([[-4.0, 4.0], [-4.0, 6.0]])
    for discard, thin in ((0, 1), (50, 3)):
        a = s.marginals(discard=discard, thin=thin, range=box)
        host = s.chain[:, discard::thin]                                                        # [nwalkers, nsteps, ndim], the host copy
        b = marginals(host, layout="walkers", range=box)
        for k in ("edges", "hist1d", "hist2d", "outside", "percentiles", "median", "lower", "upper"):
            assert np.array_equal(getattr(a, k), getattr(b, k)), k
        assert a.n_samples == host.shape[0] * host.shape[1]
    ch = _chain_object(tmp_path)
    c = ch.posterior_marginals(s.chain, discard=50, thin=3)                                     # default range: the prior box
    assert c.names == list(ch.pardict)
    for k in ("edges", "hist1d", "hist2d", "outside", "percentiles"):
        assert np.array_equal(getattr(c, k), getattr(a, k)), k
    flat = s.chain[:, 50::3].reshape(-1, 2)
    ref = np.histogram2d(flat[:, 0], flat[:, 1], bins=20, range=box)[0]
    assert np.array_equal(c.hist2d[0], ref.astype(np.int64))
    ch.chain = s.chain
    assert np.array_equal(ch.posterior_marginals(discard=50, thin=3).hist2d, c.hist2d)
    d = ch.posterior_marginals(range="data", bins=20)
    full = s.chain.reshape(-1, 2)
    assert np.array_equal(d.hist2d[0], np.histogram2d(full[:, 0], full[:, 1], bins=20)[0].astype(np.int64))


def test_weighted_particle_set(tmp_path):
    """a dict shaped like the six-key pickle of a pocoMC / run_SMC run: its chain [S, ndim] and weights"""
    from gpbayestools_hic_amd.marginals import marginals
    rng = np.random.default_rng(12)
    S = 3001
    res = {"chain": rng.standard_normal((S, 2)) * np.array([1.0, 1.5]), "weights": rng.exponential(1.0, S), "logl": np.zeros(S),
           "logp": np.zeros(S), "logz": 0.0, "logz_err": 0.0}
    ch = _chain_object(tmp_path)
    m = ch.posterior_marginals(res["chain"], weights=res["weights"])
    edges = np.stack([np.linspace(-4.0, 4.0, 21), np.linspace(-4.0, 6.0, 21)])
    q = R.int_weights(res["weights"])
    h1, h2, outside = R.counts(res["chain"], edges, q=q)
    assert np.array_equal(m.edges, edges) and np.array_equal(m.hist1d, h1) and np.array_equal(m.hist2d, h2)
    assert np.array_equal(m.outside, outside) and m.weight_scale == R.TWO32 / res["weights"].max() and m.n_samples == S
    assert np.array_equal(m.percentiles, R.weighted_quantile(res["chain"], res["weights"], QS))
    assert np.array_equal(m.median, R.weighted_quantile(res["chain"], res["weights"], (0.5,))[0])
    dens = np.histogram(res["chain"][:, 0], bins=edges[0], weights=res["weights"], density=True)[0]
    share = h1[0].sum() / (h1[0].sum() + outside[0])
    # every weight is rounded by at most 2^-33 of the largest: S 2^-32 of the largest bin bounds the difference generously
    assert np.max(np.abs(m.density1d()[0] - dens * share)) <= S * 2.0 ** -32 * dens.max()
    assert "weighted" in repr(m)
    with pytest.raises(ValueError):
        marginals(np.zeros((4, 2, 2)), weights=np.ones(4))
    with pytest.raises(ValueError):
        ch.posterior_marginals(res["chain"], weights=-res["weights"])
