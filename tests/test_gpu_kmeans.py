"""GPU tier: posterior clusters of a resident chain — gpb_chain_kmeans (GPEngine.chain_kmeans), clusters.posterior_clusters,
Chain.posterior_clusters and StretchSampler.clusters — against the host model of tests/kmeans_reference.py, which
tests/test_kmeans_reference.py pins to scikit-learn and whose cases it shows to be far from rounding (min_gap >= 1e-6,
seed_margin >= 1e-9): seeds, labels, iteration counts, sizes and the best restart are compared for equality, nothing is
excluded.  Centres within 1e-10 in standardised units, inertia within 1e-10 relative, mean and scale within 1e-13 relative.
DESIGN.md section 23."""
import functools
import pickle

import numpy as np
import pytest

import kmeans_reference as R

pytestmark = pytest.mark.gpu

E_ARG = -1
BITS = ("centers", "inertia", "n_iter", "converged", "size", "wsum", "mean", "scale", "seed_index")
VARIANTS = ("steps", "walkers", "view")


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _eng():
    from gpbayestools_hic_amd import GPEngine
    return GPEngine(0)


def _dev(a):          # (np.array would keep the memory order of a transposed view)
    torch, dev = _torch()
    return torch.as_tensor(np.array(a, order="C"), device=dev)


@functools.lru_cache(maxsize=None)
def _dev_chain(i, variant):
    """(tensor, layout) of CASES[i]: the [n, nw, d] array, its [nw, n, d] transpose as a contiguous array, or a
    [DISCARD::THIN] view of a longer array"""
    x = R.case(i)[0]
    if variant == "walkers":
        return _dev(np.ascontiguousarray(x.transpose(1, 0, 2))), "walkers"
    if variant == "view":
        return _dev(R.embed(x))[R.DISCARD::R.THIN], "steps"
    return _dev(x), "steps"


def _call(i, how, variant, **kw):
    (n, nw, d, k, Rn), _ = R.CASES[i]
    x, w, init, u = R.case(i)
    w = None if w is None else _dev(w)
    xd, layout = _dev_chain(i, variant)
    kw.setdefault("return_labels", True)
    out = _eng().chain_kmeans(xd, layout, k, Rn, init=init if how == "init" else None, u=u if how == "u" else None, weights=w,
                              max_iter=R.MAX_ITER, tol=R.TOL, **kw)
    if "labels" in out:
        out["labels"] = out["labels"].cpu().numpy()
    return out


_run = functools.lru_cache(maxsize=None)(_call)


def _same_bits(a, b, keys=BITS):
    return [k for k in keys if not (np.array_equal(a[k], b[k]) and np.asarray(a[k]).dtype == np.asarray(b[k]).dtype)]


def _check(out, m, labels_order=None, seeds=True):
    """the library's answer `out` against the model's `m`; labels_order: the model's row of every row of the library"""
    sc = m["scale"]
    assert out["n_skipped"] == m["n_skipped"]
    assert np.max(np.abs(out["mean"] - m["mean"])) == 0.0 or np.max(np.abs(out["mean"] - m["mean"]) / np.abs(m["mean"])) <= 1e-13
    assert np.max(np.abs(out["scale"] - sc) / sc) <= 1e-13
    if seeds:
        assert np.array_equal(out["seed_index"], m["seed_index"])
    assert np.array_equal(out["n_iter"], m["n_iter"]) and np.array_equal(out["converged"], m["converged"].astype(np.int32))
    assert np.array_equal(out["size"], m["size"]) and out["size"].dtype == np.int64
    assert np.max(np.abs(out["centers"] - m["centers"]) / sc) <= 1e-10
    assert np.max(np.abs(out["inertia"] - m["inertia"]) / m["inertia"]) <= 1e-10
    assert np.max(np.abs(out["wsum"] - m["wsum"])) <= 1e-12 * m["wsum"].sum()
    _best_ok(out["best"], m)
    if "labels" in out:
        want = m["labels"][out["best"]]
        assert out["labels"].dtype == np.int32
        assert np.array_equal(out["labels"], want if labels_order is None else want[labels_order])


def _best_ok(best, m):
    """the model's best restart — or, where the model's two lowest inertias are closer than rounding can tell apart (two
    restarts that reached the same partition), one of those"""
    if m["best_margin"] >= 1e-9:
        assert best == m["best"]
    else:
        assert m["inertia"][best] - m["inertia"].min() <= 1e-10 * m["inertia"].min()


_cid = lambda i: "x".join(str(v) for v in R.CASES[i][0])                                        # noqa: E731


# ---------------------------------------------------------------------------- 1. against the host model
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("how", ("init", "u"))
@pytest.mark.parametrize("i", range(len(R.CASES)), ids=_cid)
def test_matches_the_model(i, how, variant):
    (n, nw, d, k, Rn), _ = R.CASES[i]
    out = _run(i, how, variant)
    assert out["centers"].shape == (Rn, k, d) and out["labels"].shape == (n * nw,)
    walkers = variant == "walkers" and nw > 1 and n > 1
    if walkers and how == "u":
        _check(out, R.model(i, "u", "walkers"))                       # the seeding counts the rows in this layout's order
    elif walkers:                                                     # row w * n + t of this layout is row t * nw + w of the model
        _check(out, R.model(i, "init"), labels_order=np.arange(n * nw).reshape(n, nw).T.reshape(-1))
    else:
        _check(out, R.model(i, how))


# ---------------------------------------------------------------------------- 2. determinism and isolation
@pytest.mark.parametrize("i, how", ((1, "u"), (2, "u"), (4, "init")), ids=[_cid(1), _cid(2), _cid(4)])
def test_two_calls_give_identical_bits(i, how):
    a, b = _run(i, how, "steps"), _call(i, how, "steps")
    assert _same_bits(a, b) == [] and a["best"] == b["best"] and np.array_equal(a["labels"], b["labels"])


@pytest.mark.parametrize("i, rs", ((1, (0, 1, 2)), (2, (0, 9)), (4, (0, 7, 15))), ids=[_cid(1), _cid(2), _cid(4)])
def test_a_restart_does_not_depend_on_the_others(i, rs):
    """restart r of the R-restart call against the call with R = 1 started from r's centres: bit for bit (the restarts of
    case 4 go through in groups of one, those of the others share a workgroup)"""
    (n, nw, d, k, Rn), _ = R.CASES[i]
    x, w, init, u = R.case(i)
    w = None if w is None else _dev(w)
    xd, layout = _dev_chain(i, "steps")
    joint = _run(i, "init", "steps")
    for r in rs:
        one = _eng().chain_kmeans(xd, layout, k, 1, init=init[r:r + 1], weights=w, max_iter=R.MAX_ITER, tol=R.TOL,
                                  return_labels=True)
        for key in ("centers", "inertia", "n_iter", "converged", "size", "wsum"):
            assert np.array_equal(one[key][0], joint[key][r]), (r, key)
        if r == joint["best"]:
            assert np.array_equal(one["labels"].cpu().numpy(), joint["labels"])
    useed = _eng().chain_kmeans(xd, layout, k, 1, u=u[rs[-1]:rs[-1] + 1], weights=w, max_iter=R.MAX_ITER, tol=R.TOL)
    for key in ("centers", "inertia", "n_iter", "size", "wsum", "seed_index"):
        assert np.array_equal(useed[key][0], _run(i, "u", "steps")[key][rs[-1]]), key


@pytest.mark.parametrize("i", (1, 3, 4), ids=_cid)
def test_layouts_give_identical_bits(i):
    """integer sums: from given centres the steps layout, the walkers layout and the thinned view give the same bits (mean and
    scale are fixed-order floating-point sums over the rows in their order: the walkers layout's agree within 1e-13)"""
    (n, nw, d, k, Rn), _ = R.CASES[i]
    s, w, v = (_run(i, "init", variant) for variant in VARIANTS)
    assert _same_bits(s, v) == [] and np.array_equal(s["labels"], v["labels"])
    assert np.max(np.abs(w["mean"] - s["mean"]) / np.abs(s["mean"])) <= 1e-13 and np.max(np.abs(w["scale"] - s["scale"]) / s["scale"]) <= 1e-13
    if np.array_equal(w["mean"], s["mean"]) and np.array_equal(w["scale"], s["scale"]):
        assert _same_bits(s, w) == []
    else:
        assert np.max(np.abs(w["centers"] - s["centers"]) / s["scale"]) <= 1e-10
    for key in ("n_iter", "converged", "size"):
        assert np.array_equal(s[key], w[key])
    assert np.array_equal(w["labels"], s["labels"][np.arange(n * nw).reshape(n, nw).T.reshape(-1)])


def test_unstandardised_layouts_give_identical_bits():
    """standardize=0: z = x, nothing floating-point depends on the order of the rows"""
    (n, nw, d, k, Rn), _ = R.CASES[3]
    x, w, init, u = R.case(3)
    outs = []
    for variant in VARIANTS:
        xd, layout = _dev_chain(3, variant)
        outs.append(_eng().chain_kmeans(xd, layout, k, Rn, init=init, standardize=False))
    assert _same_bits(outs[0], outs[1]) == [] and _same_bits(outs[0], outs[2]) == []
    assert np.all(outs[0]["mean"] == 0.0) and np.all(outs[0]["scale"] == 1.0)


# ---------------------------------------------------------------------------- 3. edge cases
def _flat_call(X, k, Rn, w=None, **kw):
    kw.setdefault("return_labels", True)
    out = _eng().chain_kmeans(_dev(X)[:, None, :], "steps", k, Rn, weights=w, max_iter=R.MAX_ITER, tol=R.TOL, **kw)
    if "labels" in out:
        out["labels"] = out["labels"].cpu().numpy()
    return out


def _guarded(X, w, k, Rn, **kw):
    m = R.kmeans(X, w, k, Rn, **kw)
    assert m["min_gap"] >= 1e-6 and m["seed_margin"] >= 1e-9, (m["min_gap"], m["seed_margin"])      # (the case, not the library)
    return m


def test_constant_column():
    x, w, init, u = R.case(1)
    X = x.reshape(-1, x.shape[2]).copy()
    X[:, 4] = 0.1
    init = init.copy()
    init[:, :, 4] = 0.1
    out = _flat_call(X, 10, 3, init=init)
    assert out["scale"][4] == 1.0 and out["mean"][4] == 0.1 and np.all(out["centers"][:, :, 4] == 0.1)
    _check(out, _guarded(X, None, 10, 3, init=init))
    _check(_flat_call(X, 10, 3, u=u), _guarded(X, None, 10, 3, u=u))


def test_fewer_distinct_rows_than_clusters():
    rows = np.array([[0.0, 1.0, 2.0], [4.0, -1.0, 0.5], [-3.0, 2.0, 7.0]])
    X = rows[np.arange(300) % 3]
    far = np.array([[50.0, 50.0, 50.0], [-60.0, 10.0, 0.0]])
    init = np.concatenate([rows + 0.25, far])[None]
    out = _flat_call(X, 5, 1, init=init, standardize=False)
    assert out["size"][0].tolist() == [100, 100, 100, 0, 0] and out["wsum"][0].tolist() == [100.0, 100.0, 100.0, 0.0, 0.0]
    assert np.array_equal(out["centers"][0, 3:], far) and np.array_equal(out["centers"][0, :3], rows)
    assert out["n_iter"][0] == 2 and out["converged"][0] == 1 and out["inertia"][0] == 0.0
    std = _flat_call(X, 5, 1, init=init)
    assert std["size"][0].tolist() == [100, 100, 100, 0, 0]
    assert np.allclose(std["centers"][0, 3:], far, rtol=1e-14, atol=0) and np.allclose(std["centers"][0, :3], rows, rtol=0, atol=1e-13)
    seeded = _flat_call(X, 5, 1, u=np.array([[0.1, 0.3, 0.6, 0.5, 0.9]]))                  # nothing left to seed from after three
    assert sorted(seeded["size"][0].tolist()) == [0, 0, 100, 100, 100] and seeded["inertia"][0] == 0.0


def test_nonfinite_rows_are_skipped():
    x, w, init, u = R.case(3)
    X = x.reshape(-1, x.shape[2]).copy()
    bad = np.array([0, 7, 255, 256, 700, X.shape[0] - 1])
    X[bad[0], 3], X[bad[1], 0], X[bad[2], 23], X[bad[3], 5], X[bad[4], 11], X[bad[5], 2] = np.nan, np.inf, -np.inf, np.nan, np.inf, np.nan
    good = np.setdiff1d(np.arange(X.shape[0]), bad)
    for kw in (dict(init=init), dict(u=u)):
        out = _flat_call(X, 7, 2, **kw)
        assert out["n_skipped"] == 6 and np.all(out["labels"][bad] == -1) and np.all(out["labels"][good] >= 0)
        _check(out, _guarded(X, None, 7, 2, **kw))
        clean = _guarded(X[good], None, 7, 2, **kw)                    # ... and change nothing else
        assert np.array_equal(out["size"], clean["size"]) and np.array_equal(out["n_iter"], clean["n_iter"])
        assert np.array_equal(out["labels"][good], clean["labels"][out["best"]])
        assert np.max(np.abs(out["centers"] - clean["centers"]) / clean["scale"]) <= 1e-10
        if "u" in kw:
            assert np.array_equal(out["seed_index"], good[clean["seed_index"]])


def test_zero_weight_rows_change_nothing():
    x, w, init, u = R.case(2)
    X = x.reshape(-1, x.shape[2])
    w0 = w.copy()
    zero = np.arange(2, X.shape[0], 11)
    w0[zero] = 0.0
    keep = np.setdiff1d(np.arange(X.shape[0]), zero)
    for kw in (dict(init=init), dict(u=u)):
        out = _flat_call(X, 10, 10, w=w0, **kw)
        _check(out, _guarded(X, w0, 10, 10, **kw))
        less = _guarded(X[keep], w0[keep], 10, 10, **kw)
        assert np.array_equal(out["size"], less["size"]) and np.array_equal(out["n_iter"], less["n_iter"])
        _best_ok(out["best"], less)
        assert np.array_equal(out["labels"][keep], less["labels"][out["best"]]) and np.all(out["labels"][zero] >= 0)
        assert np.max(np.abs(out["centers"] - less["centers"]) / less["scale"]) <= 1e-10
        assert np.max(np.abs(out["inertia"] - less["inertia"]) / less["inertia"]) <= 1e-10


def test_unstandardised():
    x, w, init, u = R.case(0)
    X = x.reshape(-1, 3)
    for kw in (dict(init=init), dict(u=u)):
        out = _flat_call(X, 2, 1, standardize=False, **kw)
        assert np.all(out["mean"] == 0.0) and np.all(out["scale"] == 1.0)
        _check(out, _guarded(X, None, 2, 1, standardize=False, **kw))


def test_max_iter_and_tol():
    """a restart that runs out of iterations is not converged and reports max_iter; a generous tol stops on the shift"""
    x, w, init, u = R.case(1)
    X = x.reshape(-1, x.shape[2])
    xd = _dev(X)[:, None, :]
    for max_iter, tol in ((2, 1e-4), (300, 0.05), (1, 0.0)):
        m = R.kmeans(X, None, 10, 3, init=init, max_iter=max_iter, tol=tol)
        assert m["min_gap"] >= 1e-6
        out = _eng().chain_kmeans(xd, "steps", 10, 3, init=init, max_iter=max_iter, tol=tol)
        assert np.array_equal(out["n_iter"], m["n_iter"]) and np.array_equal(out["converged"], m["converged"].astype(np.int32))
        assert np.array_equal(out["size"], m["size"]) and np.max(np.abs(out["centers"] - m["centers"]) / m["scale"]) <= 1e-10
    assert not np.all(R.kmeans(X, None, 10, 3, init=init, max_iter=2)["converged"])


# ---------------------------------------------------------------------------- 4. errors
def test_argument_errors():
    from gpbayestools_hic_amd import _native as nat
    torch, dev = _torch()
    eng = _eng()
    n, nw, d, k, Rn = 20, 4, 3, 2, 2
    rng = np.random.default_rng(0)
    x = torch.as_tensor(rng.standard_normal((n, nw, d)), device=dev)
    wdev = torch.ones(n, dtype=torch.float64, device=dev)
    init0 = rng.standard_normal((Rn, k, d))
    u0 = rng.random((Rn, k))
    cen = np.full((16, 32, d), -7.0)
    big = 1 << 31

    def rc(n=n, nw=nw, d=d, ss=nw * d, ws=d, w=None, k=k, R=Rn, max_iter=10, tol=1e-4, standardize=1, init=init0, u=None):
        init = None if init is None else np.ascontiguousarray(init)
        u = None if u is None else np.ascontiguousarray(u)
        return eng.lib.gpb_chain_kmeans(eng.h, nat.ptr(x), n, nw, d, ss, ws, nat.ptr(w), k, R, max_iter, tol, standardize, nat.ptr(init),
                                        nat.ptr(u), nat.ptr(cen), None, None, None, None, None, None, None, None, None, None, None)

    assert rc() == 0 and np.all(cen.reshape(-1)[:Rn * k * d] != -7.0) and np.all(cen.reshape(-1)[Rn * k * d:] == -7.0)
    cen[:] = -7.0

    def with_value(a, v):
        a = a.copy()
        a.reshape(-1)[1] = v
        return a
    neg = torch.ones(n, dtype=torch.float64, device=dev)
    neg[3] = -1.0
    nanw = torch.ones(n, dtype=torch.float64, device=dev)
    nanw[5] = float("nan")
    few = torch.zeros(n, dtype=torch.float64, device=dev)
    few[2] = 1.0
    bad = [(dict(n=0), "nsteps >= 1"), (dict(nw=0), "nwalkers >= 1"), (dict(d=0), "d >= 1"), (dict(d=65, ws=65, ss=nw * 65), "d above 64"),
           (dict(n=big), "2^31 - 1"), (dict(n=1 << 16, nw=1 << 15, ws=d, ss=(1 << 15) * d), "2^31 - 1"),
           (dict(ws=d - 1), "stride below d"), (dict(ss=d - 1, ws=n * d), "stride below d"), (dict(ws=-d), "stride below d"),
           (dict(ss=nw * d - 1), "neither stride spans"), (dict(ss=d, ws=n * d - 1), "neither stride spans"),
           (dict(w=wdev), "nwalkers == 1"),
           (dict(k=0), "k outside"), (dict(k=33), "k outside"), (dict(R=0), "R outside"), (dict(R=17), "R outside"),
           (dict(max_iter=0), "max_iter"), (dict(tol=-1.0), "tol"), (dict(tol=float("nan")), "tol"), (dict(tol=float("inf")), "tol"),
           (dict(standardize=2), "standardize"),
           (dict(init=None), "init_host and u_host"), (dict(u=u0), "init_host and u_host"),
           (dict(init=with_value(init0, np.nan)), "init_host"), (dict(init=with_value(init0, np.inf)), "init_host"),
           (dict(init=None, u=with_value(u0, 1.0)), "u_host"), (dict(init=None, u=with_value(u0, -0.25)), "u_host"),
           (dict(init=None, u=with_value(u0, np.nan)), "u_host"),
           (dict(nw=1, ss=d, w=neg), "w_dev"), (dict(nw=1, ss=d, w=nanw), "w_dev"),
           (dict(n=1, nw=1, ss=d), "rows with positive weight"), (dict(nw=1, ss=d, w=few), "rows with positive weight")]
    for kw, what in bad:
        assert rc(**kw) == E_ARG, kw
        msg = eng.lib.gpb_last_error(eng.h).decode()
        assert "gpb_chain_kmeans" in msg and what in msg, (kw, msg)
    assert np.all(cen == -7.0)                                                                   # nothing was written
    assert rc(ss=d, ws=n * d) == 0                                                               # the other layout's strides are fine
    assert rc(nw=1, ss=d, w=wdev) == 0 and rc(init=None, u=u0) == 0
    for call in (lambda: eng.chain_kmeans(x, "rows", k, Rn, init=init0), lambda: eng.chain_kmeans(x.cpu(), "steps", k, Rn, init=init0),
                 lambda: eng.chain_kmeans(x.permute(0, 2, 1), "steps", k, Rn, init=init0),        # the parameters must have unit stride
                 lambda: eng.chain_kmeans(x, "steps", k, Rn, init=init0[:1]), lambda: eng.chain_kmeans(x, "steps", k, Rn, u=u0[:, :1]),
                 lambda: eng.chain_kmeans(x, "steps", k, Rn), lambda: eng.chain_kmeans(x, "steps", k, Rn, init=init0, u=u0)):
        with pytest.raises(ValueError):
            call()


# ---------------------------------------------------------------------------- 5. the Python layer
@functools.lru_cache(maxsize=None)
def _sampler():
    """LoggingEnsembleSampler over a host log-probability with three modes: 8 walkers, 2 parameters, 200 steps"""
    from gpbayestools_hic_amd import LoggingEnsembleSampler
    modes = np.array([[-3.0, 0.0], [3.0, 2.0], [0.0, -4.0]])

    def lp(X):
        return np.logaddexp.reduce(-0.5 * np.sum((X[:, None, :] - modes) ** 2, axis=2) / 0.25, axis=1)
    s = LoggingEnsembleSampler(8, 2, lp, seed=11)
    s.run_mcmc(modes[np.arange(8) % 3] + 0.1 * np.random.default_rng(2).standard_normal((8, 2)), 200)
    return s


def _chain_object(tmp_path):
    from gpbayestools_hic_amd import synth
    from gpbayestools_hic_amd.mcmc import Chain
    pf, ep = str(tmp_path / "par.txt"), str(tmp_path / "exp.pkl")
    synth.write_parameter_file(pf, -6.0 * np.ones(2), np.array([6.0, 6.0]))
    with open(ep, "wb") as f:
        pickle.dump({"0": {"obs": np.array([[1.0], [0.1]])}}, f)
    return Chain(mcmc_path=str(tmp_path / "mcmc" / "c.pkl"), expdata_path=ep, model_parafile=pf)


def test_sampler_and_chain_methods(tmp_path):
    from gpbayestools_hic_amd import PosteriorClusters
    s = _sampler()
    ch = _chain_object(tmp_path)
    for discard, thin in ((0, 1), (50, 3)):
        host = s.chain[:, discard::thin]                                                        # [nwalkers, nsteps, ndim], the host copy
        u = np.random.default_rng(42).random((2, 3))
        a = s.clusters(discard=discard, thin=thin, n_clusters=3, n_init=2, return_labels=True)   # the store: step-major
        m = _guarded(host.transpose(1, 0, 2).reshape(-1, 2), None, 3, 2, u=u)
        assert isinstance(a, PosteriorClusters) and a.n_samples == host.shape[0] * host.shape[1] and a.n_skipped == 0
        assert a.best == m["best"] and np.array_equal(a.sizes, m["size"][m["best"]]) and np.array_equal(a.labels, m["labels"][m["best"]])
        assert np.max(np.abs(a.centers - m["centers"][m["best"]]) / m["scale"]) <= 1e-10 and a.centers.shape == (3, 2)
        assert np.max(np.abs(a.all_inertia - m["inertia"]) / m["inertia"]) <= 1e-10 and a.inertia == a.all_inertia[a.best]
        assert np.allclose(a.weight_share, a.sizes / a.sizes.sum(), rtol=1e-15, atol=0) and a.n_iter == m["n_iter"][m["best"]]
        c = ch.posterior_clusters(s.chain, discard=discard, thin=thin, n_clusters=3, n_init=2, return_labels=True)   # walker-major
        mw = _guarded(host.reshape(-1, 2), None, 3, 2, u=u)
        assert c.names == list(ch.pardict) and c.best == mw["best"] and np.array_equal(c.labels, mw["labels"][mw["best"]])
        assert np.max(np.abs(c.centers - mw["centers"][mw["best"]]) / mw["scale"]) <= 1e-10 and np.array_equal(c.sizes, mw["size"][mw["best"]])
    ch.chain = s.chain
    again = ch.posterior_clusters(discard=50, thin=3, n_clusters=3, n_init=2)
    assert np.array_equal(again.centers, c.centers) and again.labels is None
    with pytest.raises(ValueError):
        ch.posterior_clusters(discard=200)
    path = str(tmp_path / "cluster_centers.txt")
    c.savetxt(path)
    back = np.loadtxt(path)
    assert back.shape == (2, 3) and np.max(np.abs(back - c.centers.T)) <= 0.5e-6
    text = repr(c)
    assert text.startswith("PosteriorClusters(n_samples=%d, ndim=2, k=3, n_init=2" % c.n_samples) and len(text.splitlines()) == 6
    assert all(nm in text for nm in ch.pardict) and "rows" in text and "share" in text


def test_logl_cut_with_a_tie_and_weights():
    """a dict shaped like the six-key pickle of a pocoMC / run_SMC run: the num_samples most likely rows, ties at the cut to the
    higher index; their weights honoured; init pins the centres"""
    from gpbayestools_hic_amd.clusters import posterior_clusters, top_by_logl
    rng = np.random.default_rng(12)
    S, d, ns = 1201, 4, 500
    X = R.chain(S, 1, d, 3, 21).reshape(S, d)
    logl = rng.standard_normal(S)
    cut = np.sort(logl)[::-1][ns - 1]
    tied = np.flatnonzero(logl < cut)[:3]
    logl[tied] = cut                                       # four rows share the value at the cut; one of them is kept
    w = rng.exponential(1.0, S)
    order = np.argsort(logl, kind="stable")[::-1][:ns]
    assert np.isin(max(np.flatnonzero(logl == cut)), order) and np.sum(logl[order] == cut) == 1
    assert np.array_equal(top_by_logl(_dev(logl), ns).cpu().numpy(), order)
    init = X[order][rng.choice(ns, 3, replace=False)] + 0.01
    for weights in (None, w):
        m = _guarded(X[order], None if weights is None else w[order], 3, 1, init=init[None])
        got = posterior_clusters(X, 3, 1, logl=logl, num_samples=ns, weights=weights, init=init, return_labels=True)
        assert got.n_samples == ns and np.array_equal(got.labels, m["labels"][0]) and np.array_equal(got.sizes, m["size"][0])
        assert np.max(np.abs(got.centers - m["centers"][0]) / m["scale"]) <= 1e-10
        assert np.max(np.abs(got.weight_share - m["wsum"][0] / m["wsum"][0].sum())) <= 1e-12
    for kw in (dict(logl=logl), dict(num_samples=5), dict(logl=logl[:5], num_samples=5), dict(weights=-w), dict(weights=w[:7])):
        with pytest.raises(ValueError):
            posterior_clusters(X, 3, 1, **kw)
    with pytest.raises(ValueError):
        posterior_clusters(np.zeros((4, 2, 2)), 2, 1, weights=np.ones(4))
