"""
GPU tier of the coupled chain likelihood: an experimental covariance that couples the emulators of a chain
(gpb_chain_like_set, k_coupled; Chain.expdata_cov / Chain.set_systematics) — against the CPU oracle's full multivariate normal
(oracle.log_prob with chain_predict), the torch restatement of tests/coupled_reference.py for the gradient, and the block path
for a covariance that happens to be block-diagonal.

Covariances (coupled_reference): (a) diag(sigma^2) + two fully correlated sources, 0.03 |y_exp| over all observables and
0.05 |y_exp| over the middle half of the index range (it straddles emulators); (b) sigma_i sigma_j exp(-|i - j| / 5) over the
whole range: full rank.  Chains: (A) P = (3, 5), M = (12, 20); (B) the nine SPECS of test_gpu_multi_emulator (40 GPs, 540
observables); (C) four emulators of 16 GPs, and a fifth of one (64 and 65 GPs: the last order of the kernel's 64-wide
instantiation and the first of its 128-wide one); (D) five and eight emulators of 16 GPs (80, 128); (E) a mapped and a plain
emulator over 20 parameters.
"""
import ctypes

import numpy as np
import pytest

import coupled_reference as CR
import grad_reference as R
from conftest import relerr
from test_gpu_gradient import BAR, _rowerr
from test_gpu_multi_emulator import D as D_B, SPECS as SPECS_B

pytestmark = pytest.mark.gpu

D_A = 5
SPECS_A = [(48, 12, 3, "RBF"), (64, 20, 5, "Matern25")]
SPECS_C64 = [(64, 20, 16, "RBF")] * 4
SPECS_C65 = SPECS_C64 + [(64, 20, 1, "Matern25")]
SPECS_D80 = [(64, 20, 16, "RBF")] * 5
SPECS_D128 = [(64, 20, 16, "RBF")] * 8
CASES = {"A": (SPECS_A, D_A), "B": (SPECS_B, D_B), "C64": (SPECS_C64, D_A), "C65": (SPECS_C65, D_A), "D80": (SPECS_D80, D_A),
         "D128": (SPECS_D128, D_A)}
_built = {}


@pytest.fixture
def chains(tmp_path_factory):
    """name -> (chain, emulators, info), built once per module run and handed out with the experiment file's diagonal
    covariance in place (every test sets its own)"""
    from gpbayestools_hic_amd.workload import build_multi_chain

    def get(name):
        if name not in _built:
            specs, d = CASES[name]
            chain, emus, info = build_multi_chain(specs, d, workdir=str(tmp_path_factory.mktemp("coupled_" + name)))
            info["cov0"] = chain.expdata_cov.copy()
            info["sigma"] = 0.05 * np.abs(info["yexp"])
            _built[name] = (chain, emus, info)
        chain, emus, info = _built[name]
        chain.expdata_cov = info["cov0"].copy()
        chain.use_chain_call = True
        return chain, emus, info
    return get


def _cov(info, which):
    return CR.cov_a(info["yexp"], info["sigma"]) if which == "a" else CR.cov_b(info["sigma"])


def _oracle(info, cexp):
    from gpbayestools_hic_amd import synth
    from oracle import gp_oracle as O
    if "oracle_emus" not in info:
        oes = []
        for i, ((N, M, P, kernel), (X, Y)) in enumerate(zip(info["specs"], info["data"])):
            oe = O.OracleEmulator(X, Y, info["lo"], info["hi"], P, O.KIND_NAMES[kernel])
            oes.append(oe.fit(synth.fixed_theta(info["d"], P, ell=1.2 + 0.1 * i, noise=0.03 + 0.01 * i)))
        info["oracle_emus"] = oes
    oes = info["oracle_emus"]
    return lambda X, **kw: O.log_prob(X, info["lo"], info["hi"], lambda x, e: O.chain_predict(oes, x, e), info["yexp"], cexp, **kw)


def _rows48(info):
    """the 48 rows of the nine-emulator test: one outside the box, one on its boundary, eight near the truth"""
    from gpbayestools_hic_amd import synth
    d = info["d"]
    X = synth.walkers(48, d, seed=5)
    X[3, 1] = 1.25
    X[17, d - 2] = 0.0                                        # on the boundary: outside
    X[40:] = info["xstar"] + 0.01 * np.random.default_rng(1).standard_normal((8, d))
    return X


def _ctx_array(emus):
    engs = [e._engine_ready() for e in emus]
    return engs, (ctypes.c_void_p * len(engs))(*[g.h for g in engs])


def _coupling_applies(chain):
    chain._prepare_blocks()
    return chain._coupled and chain._coupled_why is None


# ------------------------------------------------------------------ 1. oracle parity
@pytest.mark.parametrize("name,which", [("A", "a"), ("A", "b"), ("B", "a"), ("B", "b"), ("C64", "a"), ("C65", "a"), ("C65", "b"),
                                        ("D80", "a"), ("D128", "a")])
def test_coupled_log_posterior_against_the_oracle(chains, name, which):
    chain, emus, info = chains(name)
    cexp = _cov(info, which)
    chain.expdata_cov = cexp
    logpost = _oracle(info, cexp)
    X = _rows48(info)
    ref = logpost(X)
    inside = np.all((X > info["lo"]) & (X < info["hi"]), axis=1)
    assert inside.sum() == 46 and np.all(np.isfinite(ref[inside])) and np.all(np.isneginf(ref[~inside]))
    got = chain.log_posterior(X)
    assert _coupling_applies(chain)
    assert np.array_equal(np.isneginf(got), ~inside)
    print("%s/%s: relerr %.3g" % (name, which, relerr(got[inside], ref[inside])))
    assert relerr(got[inside], ref[inside]) < 1e-10
    fin = chain.log_likelihood(X, finite=True)
    assert np.all(fin[~inside] == -1e300)
    assert relerr(fin[inside], logpost(X, posterior=False, finite=True)[inside]) < 1e-10
    # the coupling is not a small correction here: the block-diagonal part alone is another number
    chain.expdata_cov = info["cov0"].copy() if which == "a" else np.diag(np.diag(cexp))
    assert np.min(np.abs(chain.log_posterior(X)[inside] - ref[inside])) > 1e-3
    # use_chain_call = False has no coupled counterpart: the chain call is used all the same
    chain.expdata_cov = cexp
    chain.use_chain_call = False
    assert np.array_equal(chain.log_posterior(X), got)
    assert np.array_equal(chain.log_likelihood_point_by_point(X), got)


# ------------------------------------------------------------------ 2. a block-diagonal matrix through the coupled path
@pytest.mark.parametrize("name", ["A", "B", "C64", "C65", "D80"])
def test_block_diagonal_matrix_through_the_coupled_kernel(chains, name):
    """gpb_chain_like_set called directly with the experiment's block-diagonal matrix plus ONE off-block entry of 1e-300: the
    coupled kernel serves the chain and gives the block path's values"""
    from gpbayestools_hic_amd import _native as nat
    chain, emus, info = chains(name)
    X = _rows48(info)
    block = chain.log_posterior(X)
    assert not chain._coupled
    engs, arr = _ctx_array(emus)
    cov = nat.f64(info["cov0"]).copy()
    cov[0, cov.shape[0] - 1] = 1e-300
    applies = ctypes.c_int(0)
    lib = engs[0].lib
    assert lib.gpb_chain_like_set(arr, len(engs), nat.ptr(nat.f64(info["yexp"])), nat.ptr(cov), ctypes.byref(applies)) == 0
    assert applies.value == 1
    try:
        coupled = chain.log_posterior(X)                      # (the chain's own signature is unchanged: no re-installation)
    finally:
        assert lib.gpb_chain_like_set(arr, len(engs), nat.ptr(nat.f64(info["yexp"])), None, ctypes.byref(applies)) == 0
        chain._like_sig = None
    ins = np.isfinite(block)
    assert ins.sum() == 46 and np.array_equal(np.isfinite(coupled), ins)
    print("%s: coupled kernel against the block path %.3g" % (name, relerr(coupled[ins], block[ins])))
    assert relerr(coupled[ins], block[ins]) < 1e-12
    assert np.array_equal(chain.log_posterior(X), block)      # cleared: today's path, today's bits


# ------------------------------------------------------------------ 3. independence of the batch
def test_a_rows_value_does_not_depend_on_the_batch(chains):
    from gpbayestools_hic_amd import synth
    chain, emus, info = chains("B")
    chain.expdata_cov = _cov(info, "a")
    engs = [e._engine_ready() for e in emus]
    X = _rows48(info)
    big = synth.walkers(700, D_B, seed=700)
    big[::13, 2] = -0.5                                       # rows outside the box: the compaction moves the others
    big[123], big[699] = X[41], X[7]
    arith = [g.predict_sliced for g in engs]
    try:
        for fp64 in (True, False):
            for g, a in zip(engs, arith):
                g.tune("predict_sliced", 0 if fp64 else a)
            one = chain.log_posterior(X)
            assert _coupling_applies(chain)
            for w in (0, 7, 41, 47):
                assert np.array_equal(chain.log_posterior(X[w:w + 1]), one[w:w + 1]), (fp64, w)
            many = chain.log_posterior(big)
            assert many[123] == one[41] and many[699] == one[7], fp64
            for Xb, ref in ((X, one), (big, many)):
                engs[0].tune("chain_batch", 0)
                assert np.array_equal(chain.log_posterior(Xb), ref), (fp64, len(Xb))
                engs[0].tune("chain_batch", 1)
                for tile in (128, 65, 64, 32):
                    for g in engs:
                        g.force_tile(tile)
                    assert np.array_equal(chain.log_posterior(Xb), ref), (fp64, len(Xb), tile)
                for g in engs:
                    g.force_tile(0)
    finally:
        engs[0].tune("chain_batch", 1)
        for g, a in zip(engs, arith):
            g.force_tile(0)
            g.tune("predict_sliced", a)


# ------------------------------------------------------------------ 4. gradient
@pytest.mark.parametrize("name,which,nrows", [("A", "a", 24), ("A", "b", 24), ("C65", "a", 12), ("B", "a", 8)])
def test_coupled_gradient_against_autograd(chains, name, which, nrows):
    chain, emus, info = chains(name)
    cexp = _cov(info, which)
    chain.expdata_cov = cexp
    d = info["d"]
    X = info["xstar"] + 0.03 * np.random.default_rng(9).standard_normal((nrows, d))
    X[1, 1] = 1.1                                             # outside: zero gradient
    plain = chain.log_posterior(X)
    lp, g = chain.log_posterior(X, return_grad=True)
    assert _coupling_applies(chain)
    assert np.array_equal(lp, plain)                          # bit for bit what gpb_chain_logpost writes
    inside = np.all((X > chain.min) & (X < chain.max), axis=1)
    assert inside.sum() == nrows - 1 and np.all(g[~inside] == 0.0) and np.all(np.isneginf(lp[~inside]))
    states = [R.state_from_emulator(e) for e in emus]
    v, gref = R.value_and_grad(lambda x: CR.log_posterior(states, x, chain.min, chain.max, chain.expdata[0], cexp), X)
    assert relerr(lp[inside], v[inside]) < 1e-10
    err = _rowerr(g[inside], gref[inside])
    print("%s/%s: worst row %.3g of the bar" % (name, which, float(err.max()) / BAR))
    assert np.all(err <= BAR), err
    lf, gf = chain.log_likelihood(X, finite=True, return_grad=True)
    assert np.array_equal(lf, chain.log_likelihood(X, finite=True)) and np.array_equal(gf, g)
    # a row's gradient does not depend on the batch
    l1, g1 = chain.log_posterior(X[2:3], return_grad=True)
    assert np.array_equal(l1, lp[2:3]) and np.array_equal(g1, g[2:3])


# ------------------------------------------------------------------ 5. mapped chain gradient
def test_coupled_gradient_of_a_mapped_chain_against_central_differences(tmp_path):
    """(E): a parameterTrafoPCA emulator and a plain one over 20 parameters; step 1e-6, bar 1e-5 relative to max(|g|_inf, 1)
    as test_log_posterior_grad_nine_mapped_emulators has it (rounding of lp / h and truncation)"""
    from gpbayestools_hic_amd.workload import build_multi_chain
    chain, emus, info = build_multi_chain([(96, 12, 4, "RBF"), (80, 20, 5, "Matern25")], 20, workdir=str(tmp_path),
                                          mapped=[True, False])
    chain.expdata_cov = CR.cov_a(info["yexp"], 0.05 * np.abs(info["yexp"]))
    X = np.clip(info["xstar"] + 0.02 * np.random.default_rng(10).standard_normal((4, 20)), 0.01, 0.99)
    lp, g = chain.log_posterior(X, return_grad=True)
    assert _coupling_applies(chain) and np.all(np.isfinite(lp))
    assert np.array_equal(lp, chain.log_posterior(X))
    h = 1e-6
    fd = np.empty_like(g)
    for q in range(20):
        e = np.zeros(20); e[q] = h
        fd[:, q] = (chain.log_posterior(X + e) - chain.log_posterior(X - e)) / (2 * h)
    assert np.all(_rowerr(g, fd) <= 1e-5), _rowerr(g, fd)


# ------------------------------------------------------------------ 6. stretch sampler
def test_stretch_sampler_on_the_coupled_nine_emulator_chain(chains):
    from gpbayestools_hic_amd import StretchSampler
    from test_gpu_sampler_step import _oracle_chain as emcee_by_the_oracle
    chain, emus, info = chains("B")
    cexp = _cov(info, "a")
    chain.expdata_cov = cexp
    logpost = _oracle(info, cexp)
    nw, seed = 32, 77
    X0 = np.clip(info["xstar"] + 0.05 * np.random.default_rng(4).standard_normal((nw, D_B)), 0.02, 0.98)
    s = StretchSampler(chain, nw, seed=seed)
    assert s._resident_engine()[2] == 9 and _coupling_applies(chain)
    s.run(X0, 3, status=100)
    Xf, lp, nacc, hist = emcee_by_the_oracle(X0, 3, seed, True, s._engine(), logpost)
    assert np.array_equal(s.naccept.cpu().numpy(), nacc) and nacc.sum() > 0
    assert np.array_equal(s.chain[:, -1], Xf)                 # same decisions => same positions, bit for bit
    fin = np.isfinite(lp)
    assert relerr(s.lnprobability[:, -1][fin], lp[fin]) < 1e-10
    assert np.array_equal(s.lnprobability[:, -1], chain.log_posterior(s.chain[:, -1]))


# ------------------------------------------------------------------ 7. SMC, PTLMC, find_map
def test_smc_ptlmc_and_find_map_evaluate_the_coupled_likelihood(chains):
    """The loops' stored log-values are chain.log_likelihood / log_posterior of their final states, bit for bit.  PTLMC stores
    lp / temperature and its exchange rescales it (t_src fval_src / t_dst), so the bits of lp itself are kept on an untempered
    ladder (every temperature 1: x * 1 and x / 1 are exact), which is what the five steps with the gradient run on; a tempered
    ladder is held to the 1e-14 of tests/test_gpu_ptlmc.py."""
    from gpbayestools_hic_amd import ptlmc
    from gpbayestools_hic_amd.smc import SMCSampler
    chain, emus, info = chains("A")
    chain.expdata_cov = _cov(info, "a")
    s = SMCSampler(chain, 256, seed=3)
    s.init_uniform()
    assert _coupling_applies(chain)
    s.reweight()
    s.move(3)
    st = s.state()
    assert st["naccept"] > 0
    assert np.array_equal(st["logl"], chain.log_likelihood(st["x"], finite=True))

    rng = np.random.default_rng(11)
    for numtemps, numchain in ((0, 8), (4, 4)):
        T = numtemps + numchain
        temps = ptlmc.ladder(numtemps, numchain, 20.0)
        theta = np.clip(info["xstar"] + 0.03 * rng.standard_normal((T, D_A)), 0.02, 0.98)
        lp, g = chain.log_posterior(theta, return_grad=True)
        covmat0, hc = ptlmc.proposal_factor(theta)
        p = ptlmc.PTLMCSampler(chain, temps, hc, covmat0, numtemps, numchain, 3, 3, ptlmc.TARACC_GRAD, 11, True)
        p.set_state(theta, lp / temps, g / temps[:, None])
        p.run(5)
        got = p.state()
        assert p.naccept.sum().item() > 0 and not np.array_equal(got["theta"], theta)
        lp5, g5 = chain.log_posterior(got["theta"], return_grad=True)
        assert np.all(np.isfinite(lp5))
        if numtemps == 0:
            assert np.array_equal(got["fval"], lp5) and np.array_equal(got["dfval"], g5)
        else:
            assert relerr(got["fval"] * temps, lp5) <= 1e-14

    X0 = np.random.default_rng(13).uniform(chain.min, chain.max, (4, D_A))
    Xo, lpo = chain.find_map(X0=X0)
    assert Xo.shape == (4, D_A) and np.all(np.diff(lpo) <= 0.0)
    assert lpo[0] >= np.max(chain.log_posterior(X0))
    assert relerr(chain.log_posterior(Xo), lpo) < 1e-12
    Xn, lpn = chain.find_map(nstarts=4, seed=3)
    starts = np.random.default_rng(3).uniform(chain.min, chain.max, (4, D_A))
    assert lpn[0] >= np.max(chain.log_posterior(starts))


# ------------------------------------------------------------------ 8. fallbacks and errors
def test_fallbacks_and_errors(chains, tmp_path):
    import torch
    from gpbayestools_hic_amd import _native as nat
    from gpbayestools_hic_amd.mcmc import Chain
    from oracle import gp_oracle as O
    from test_gpu_gradient import _emulator
    chain, emus, info = chains("A")
    engs, arr = _ctx_array(emus)
    lib = engs[0].lib
    yexp = nat.f64(info["yexp"])
    cexp = _cov(info, "a")

    # set_systematics reproduces case (a)'s matrix exactly, from the errors of the experiment file
    assert chain.set_systematics(CR.sources_a(info["yexp"])) is chain
    assert np.array_equal(chain.expdata_cov, cexp)
    assert np.array_equal(chain.set_systematics(CR.sources_a(info["yexp"]), stat=info["sigma"]).expdata_cov, cexp)
    with pytest.raises(ValueError):
        chain.set_systematics(np.zeros((2, 5)))
    X = _rows48(info)
    good = chain.log_posterior(X)
    ins = np.isfinite(good)
    assert _coupling_applies(chain)

    # an indefinite expdata_cov: applies == 0, nothing installed, no crash; the dense route reports the rows as NaN (the
    # device MVN's convention for a matrix that is not positive definite)
    bad = cexp.copy()
    bad[2, 20] = bad[20, 2] = 1e3 * np.sqrt(cexp[2, 2] * cexp[20, 20])       # (far beyond what the truncation blocks could mend)
    applies = ctypes.c_int(1)
    assert lib.gpb_chain_like_set(arr, 2, nat.ptr(yexp), nat.ptr(nat.f64(bad)), ctypes.byref(applies)) == 0 and applies.value == 0
    chain.expdata_cov = bad
    assert not _coupling_applies(chain) and "positive definite" in chain._coupled_why
    with pytest.raises(NotImplementedError):
        chain.run_SMC(n_particles=64, nmcmc=1, max_stages=1, seed=1)
    assert np.all(np.isnan(chain.log_posterior(X)[ins]))

    # a stale coupling: gpb_like_set on a member, then gpb_chain_logpost -> GPB_E_STATE, never the block-diagonal value
    chain.expdata_cov = cexp
    assert np.array_equal(chain.log_posterior(X), good)
    Xd = torch.as_tensor(np.ascontiguousarray(X), device="cuda")
    out = torch.full((len(X),), 7.0, dtype=torch.float64, device="cuda")
    lo, hi = chain._box(Xd.device)
    call = lambda a, E: lib.gpb_chain_logpost(a, E, nat.ptr(Xd), len(X), nat.ptr(out), nat.ptr(lo), nat.ptr(hi), float("-inf"), 0.0)
    assert call(arr, 2) == 0
    engs[1].set_likelihood(info["yexp"][12:], cexp[12:, 12:])
    GPB_E_STATE = -2
    assert call(arr, 2) == GPB_E_STATE and b"stale" in lib.gpb_last_error(engs[0].h)
    gd = torch.empty((len(X), D_A), dtype=torch.float64, device="cuda")
    assert lib.gpb_chain_logpost_grad(arr, 2, nat.ptr(Xd), len(X), nat.ptr(out), nat.ptr(gd), nat.ptr(lo), nat.ptr(hi),
                                      float("-inf"), 0.0) == GPB_E_STATE
    # ... and for another list of contexts than the one it was set for
    assert lib.gpb_chain_like_set(arr, 2, nat.ptr(yexp), nat.ptr(nat.f64(cexp)), ctypes.byref(applies)) == 0 and applies.value == 1
    assert call(arr, 2) == 0
    assert call((ctypes.c_void_p * 1)(engs[0].h), 1) == GPB_E_STATE
    # cleared: the block path again
    assert lib.gpb_chain_like_set(arr, 2, nat.ptr(yexp), None, ctypes.byref(applies)) == 0 and applies.value == 0
    assert call(arr, 2) == 0
    chain._like_sig = None

    # null and mismatched arguments
    GPB_E_ARG = -1
    assert lib.gpb_chain_like_set(None, 2, nat.ptr(yexp), nat.ptr(nat.f64(cexp)), ctypes.byref(applies)) == GPB_E_ARG
    assert lib.gpb_chain_like_set(arr, 0, nat.ptr(yexp), nat.ptr(nat.f64(cexp)), ctypes.byref(applies)) == GPB_E_ARG
    assert lib.gpb_chain_like_set(arr, 65, nat.ptr(yexp), nat.ptr(nat.f64(cexp)), ctypes.byref(applies)) == GPB_E_ARG
    assert lib.gpb_chain_like_set(arr, 2, None, nat.ptr(nat.f64(cexp)), ctypes.byref(applies)) == GPB_E_ARG
    assert lib.gpb_chain_like_set(arr, 2, nat.ptr(yexp), nat.ptr(nat.f64(cexp)), None) == GPB_E_ARG
    assert lib.gpb_chain_like_set((ctypes.c_void_p * 2)(engs[0].h, None), 2, nat.ptr(yexp), nat.ptr(nat.f64(cexp)),
                                  ctypes.byref(applies)) == GPB_E_ARG
    side = torch.cuda.Stream()
    assert lib.gpb_ctx_set_stream(engs[1].h, nat.VP(side.cuda_stream)) == 0
    try:
        assert lib.gpb_chain_like_set(arr, 2, nat.ptr(yexp), nat.ptr(nat.f64(cexp)), ctypes.byref(applies)) == GPB_E_ARG
    finally:
        engs[1]._stream = None
        engs[1]._track_stream()

    # a perform_no_PCA emulator in a coupled chain: the dense route for log_posterior, NotImplementedError from the loops
    import os
    from gpbayestools_hic_amd import synth
    c1, e1, xstar = _emulator(str(tmp_path / "pca"), 64, D_A, 10, 3)
    c2, e2, _ = _emulator(str(tmp_path / "nopca"), 48, D_A, 6, 3, no_pca=True, seed=7)
    y2 = np.concatenate([c1.expdata[0], c2.expdata[0]])
    sig2 = 0.05 * np.abs(y2)
    cov2 = CR.cov_a(y2, sig2)
    ep = str(tmp_path / "exp2.pkl")
    synth.write_experiment_pickle(ep, y2, sig2)
    mixed = Chain(mcmc_path=str(tmp_path / "mcmc" / "mixed.pkl"), expdata_path=ep, model_parafile=os.path.join(str(tmp_path / "pca"), "par.txt"))
    mixed.emuList = [e1, e2]
    mixed.set_systematics(CR.sources_a(y2))
    assert np.array_equal(mixed.expdata_cov, cov2) and np.any(cov2[:10, 10:] != 0.0)
    Xm = xstar + 0.05 * np.random.default_rng(2).standard_normal((12, D_A))
    Xm[4, 0] = -0.1
    got = mixed.log_posterior(Xm)
    assert mixed._coupled and "PCA" in mixed._coupled_why
    states = [R.state_from_emulator(e1), R.state_from_emulator(e2)]
    ref = CR.log_posterior(states, R._t(Xm), mixed.min, mixed.max, y2, cov2).numpy()
    insm = np.isfinite(ref)
    assert insm.sum() == 11 and np.array_equal(np.isneginf(got), ~insm)
    assert relerr(got[insm], ref[insm]) < 1e-10
    with pytest.raises(NotImplementedError):
        mixed.run_SMC(n_particles=64, nmcmc=1, max_stages=1, seed=1)
    with pytest.raises(NotImplementedError):
        mixed.log_posterior(Xm, return_grad=True)
