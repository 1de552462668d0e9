"""GPU tier of the chain evaluation (csrc/gpb_chain.hip): the C routines that evaluate a chain's log-posterior where the
compacted chain call does not apply — inside gpb_chain_logpost_grad and the stretch move's uncompacted loop — against
Chain.log_prob_device with use_chain_call = False, the sequence of public per-emulator calls; and which fault each chain entry
point reports, with which code and message."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SPECS = [(128, 12, 3, "RBF"), (112, 10, 3, "Matern25")]
D = 20
W = 37
E_ARG, E_STATE = -1, -2                                       # include/gpbayes.h

_cache = {}


def _chain(factory, key):
    """the chains of this module, built once: "plain+mapped" / "mapped+plain" (two emulators over 20 parameters, one with
    parameterTrafoPCA, in either order) and "no_pca" (one unmapped emulator with one GP per observable, 8 parameters)"""
    if key not in _cache:
        from gpbayestools_hic_amd.workload import build_chain, build_multi_chain
        tmp = str(factory.mktemp(key.replace("+", "_")))
        if key == "no_pca":
            chain, emu, info = build_chain(1, workdir=tmp, no_pca=True)
            emus = [emu]
        else:
            chain, emus, info = build_multi_chain(SPECS, D, workdir=tmp, mapped=[k == "mapped" for k in key.split("+")])
        chain._prepare_blocks()
        _cache[key] = chain, emus, info
    return _cache[key]


def _ctx_array(engs):
    for g in engs:
        g._track_stream()
    return (ctypes.c_void_p * len(engs))(*[g.h for g in engs])


def _rows(info, seed):
    """W rows around the prior box, every third one outside it (one coordinate past an edge)"""
    d = info["d"]
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.05, 0.95, (W, d))
    out = np.arange(W) % 3 == 1
    X[out, rng.integers(0, d, out.sum())] = np.where(rng.random(out.sum()) < 0.5, -0.1, 1.2)
    assert out.sum() == 12
    return X


def _grad_call_lp(chain, emus, X, outside):
    """the log-posterior gpb_chain_logpost_grad writes"""
    import torch
    from gpbayestools_hic_amd import _native as nat
    engs = [e._engine_ready() for e in emus]
    arr = _ctx_array(engs)
    Xd = torch.as_tensor(np.ascontiguousarray(X), device="cuda")
    ll = torch.empty(len(X), dtype=torch.float64, device="cuda")
    gd = torch.empty(X.shape, dtype=torch.float64, device="cuda")
    lo, hi = chain._box(Xd.device)
    e0 = engs[0]
    e0._ck(e0.lib.gpb_chain_logpost_grad(arr, len(engs), nat.ptr(Xd), len(X), nat.ptr(ll), nat.ptr(gd), nat.ptr(lo), nat.ptr(hi),
                                         float(outside), chain.inside_const))
    return ll.cpu().numpy()


def _python_sequence_lp(chain, X, outside):
    import torch
    chain.use_chain_call = False
    try:
        return chain.log_prob_device(torch.as_tensor(np.ascontiguousarray(X), device="cuda"), outside=outside).cpu().numpy()
    finally:
        chain.use_chain_call = True


def _set_compact(emus, on):
    for e in emus:
        e._engine_ready().tune("compact", 1 if on else 0)


@pytest.mark.parametrize("compact", [True, False])
@pytest.mark.parametrize("key", ["plain+mapped", "mapped+plain"])
def test_gradient_calls_value_equals_the_python_sequence(tmp_path_factory, key, compact):
    """two emulators, the mapped one last (the sum ends in gpb_loglike + gpb_box_finish) or first (it ends in gpb_logpost); as
    built the chain call evaluates, with the compaction off the C per-emulator sequence does: bit for bit the Python one"""
    chain, emus, info = _chain(tmp_path_factory, key)
    X = _rows(info, 3)
    _set_compact(emus, compact)
    try:
        assert (chain._chain_contexts() is not None) == compact
        for outside in (-np.inf, -1e300):
            got = _grad_call_lp(chain, emus, X, outside)
            ref = _python_sequence_lp(chain, X, outside)
            inside = np.all((X > chain.min) & (X < chain.max), axis=1)
            assert inside.sum() == W - 12 and np.all(got[~inside] == outside) and np.all(np.isfinite(got[inside]))
            assert np.array_equal(got, ref), (key, compact, outside, np.flatnonzero(got != ref))
    finally:
        _set_compact(emus, True)


def test_one_unmapped_emulator_without_pca(tmp_path_factory):
    """no block likelihood kernel applies to a no-PCA emulator: the chain call never does, the evaluation is one gpb_logpost"""
    chain, emus, info = _chain(tmp_path_factory, "no_pca")
    X = _rows(info, 4)
    assert chain._chain_contexts() is None
    for outside in (-np.inf, -1e300):
        got = _grad_call_lp(chain, emus, X, outside)
        assert np.array_equal(got, _python_sequence_lp(chain, X, outside)), outside
        assert np.count_nonzero(got == outside) == 12


def test_uncompacted_c_loop_equals_the_host_driven_loop(tmp_path_factory):
    """the same emulator under the stretch move: gpb_chain_emcee_run's uncompacted branch (one unmapped emulator) against the
    loop that calls gpb_stretch_propose / log_prob_device / gpb_stretch_accept from Python"""
    from gpbayestools_hic_amd import StretchSampler, synth
    chain, emus, info = _chain(tmp_path_factory, "no_pca")
    nw = 8
    X0 = synth.walkers(nw, info["d"], seed=31)
    X0[3, 1] = 1.4                                            # a walker that starts outside the prior box
    c = StretchSampler(chain, nw, seed=7)
    assert chain._chain_contexts() is None and c._resident_engine() is not None and c._resident_engine()[2] == 1
    c.run(X0, 3, status=10)
    h = StretchSampler(chain, nw, seed=7)
    h._resident_engine = lambda: None                         # force the host-driven loop
    h.run(X0, 3, status=10)
    assert np.array_equal(c.chain, h.chain) and np.array_equal(c.lnprobability, h.lnprobability)
    assert np.array_equal(c.naccept.cpu().numpy(), h.naccept.cpu().numpy())


# ---------------------------------------------------------------------------- refusals
# (entry point, the name its messages start with).  gpb_chain_emcee_prepare runs gpb_chain_emcee_run's own plan and reports
# under that name.
ENTRY_POINTS = [("gpb_chain_logpost", "gpb_chain_logpost"), ("gpb_chain_logpost_grad", "gpb_chain_logpost_grad"),
                ("gpb_chain_emcee_prepare", "gpb_chain_emcee_run"), ("gpb_chain_ptlmc_run", "gpb_chain_ptlmc_run"),
                ("gpb_chain_smc_move", "gpb_chain_smc_move")]
FAULTS = {"null": (E_ARG, b"null context"), "ndim": (E_ARG, b"disagree on the number of parameters"),
          "no_like": (E_STATE, b"gpb_like_set")}


@pytest.fixture(scope="module")
def refusal_contexts(tmp_path_factory):
    """a sound first context (the first emulator of the two-emulator chain) and, per fault, the second slot of the list"""
    from gpbayestools_hic_amd import GPEngine, synth
    chain, emus, info = _chain(tmp_path_factory, "plain+mapped")
    small, semus, _ = _chain(tmp_path_factory, "no_pca")     # likelihood installed, but over 8 parameters
    bare = GPEngine(0)                                        # fitted over the chain's 20 parameters, no likelihood
    bare.set_data(synth.lhs(64, D), np.random.default_rng(0).standard_normal((2, 64)), "RBF", 0.1)
    bare.set_theta(synth.fixed_theta(D, 2))
    bare.factor()
    e0 = emus[0]._engine_ready()
    second = {"null": None, "ndim": semus[0]._engine_ready(), "no_like": bare}
    yield chain, e0, second
    bare.close()


@pytest.mark.parametrize("fault", sorted(FAULTS))
@pytest.mark.parametrize("entry,name", ENTRY_POINTS)
def test_refusal_table(refusal_contexts, entry, name, fault):
    """one fault in the second slot of the context list: every chain entry point returns the fault's code and reports it
    under its own name with the fault's words; nothing is launched"""
    import torch
    from gpbayestools_hic_amd import _native as nat
    chain, e0, second = refusal_contexts
    other = second[fault]
    e0._track_stream()
    if other is not None:
        other._track_stream()
    arr = (ctypes.c_void_p * 2)(e0.h, None if other is None else other.h)
    lib = e0.lib
    buf = nat.ptr(torch.zeros(4096, dtype=torch.float64, device="cuda"))       # stands for every array argument: none is touched
    lo, hi = (nat.ptr(t) for t in chain._box(torch.device("cuda", 0)))
    ninf = float("-inf")
    if entry == "gpb_chain_logpost":
        rc = lib.gpb_chain_logpost(arr, 2, buf, 4, buf, lo, hi, ninf, 0.0)
    elif entry == "gpb_chain_logpost_grad":
        rc = lib.gpb_chain_logpost_grad(arr, 2, buf, 4, buf, buf, lo, hi, ninf, 0.0)
    elif entry == "gpb_chain_emcee_prepare":
        rc = lib.gpb_chain_emcee_prepare(arr, 2, 8)
    elif entry == "gpb_chain_ptlmc_run":                      # 2 + 2 rungs, one step, no gradient, nothing saved
        rc = lib.gpb_chain_ptlmc_run(arr, 2, 2, 2, 1, 0, 1, 0, 0.25, buf, buf, None, buf, buf, buf, buf, buf, lo, hi, ninf, 0.0,
                                     None, 0, buf, buf)
    else:                                                     # 16 particles, one step
        rc = lib.gpb_chain_smc_move(arr, 2, 16, 1, 0, 0, 1, buf, buf, buf, buf, lo, hi, ninf, 0.0)
    code, words = FAULTS[fault]
    msg = lib.gpb_last_error(e0.h)
    assert rc == code, (entry, fault, rc, msg)
    assert msg.startswith(name.encode()) and words in msg, (entry, fault, msg)
