"""GPU tier: who owns the device buffers of a context.  Every buffer a context takes from the buffer cache goes back when the
context is destroyed (gpb_debug_pool_live counts what is out), and a context given a new design is the context a fresh one
would be: no workspace sized by the old (P, Np) survives in a form its successor misreads.

Shapes: A = (N 200, d 5, P 3) and B = (N 70, d 3, P 4: Np = 128, 48 rows of padding in front and 10 behind); query batches
of 37 rows, then 200, so the walker workspaces grow once."""
import ctypes
import gc
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = {"A": (200, 5, 3), "B": (70, 3, 4)}
M_OBS = 6
W_SMALL, W_LARGE = 37, 200


def _problem(shape):
    """design, targets, hyper-parameters, a PCA-mode transform and an experiment for one shape (fixed seeds)"""
    from gpbayestools_hic_amd import synth
    N, d, P = SHAPES[shape]
    rng = np.random.default_rng(1000 + N)
    X = synth.lhs(N, d, seed=synth.SEED + N)
    Z = np.ascontiguousarray(synth.observables(X, P, seed=synth.SEED + N + 1).T) - 2.0
    theta = synth.fixed_theta(d, P) + 0.05 * rng.standard_normal((P, d + 2))
    A = rng.standard_normal((P, M_OBS))
    mu = 2.0 + rng.standard_normal(M_OBS)
    c0 = 0.01 * rng.standard_normal((M_OBS, M_OBS))
    cov_trunc = c0 @ c0.T + 1e-3 * np.eye(M_OBS)
    yexp = mu + 0.1 * rng.standard_normal(M_OBS)
    cov_exp = np.diag((0.05 * np.abs(yexp)) ** 2)
    return dict(X=X, Z=Z, theta=theta, A=A, mu=mu, cov_trunc=cov_trunc, yexp=yexp, cov_exp=cov_exp,
                Xq=synth.walkers(W_LARGE, d, seed=synth.SEED + N + 2), lo=np.zeros(d), hi=np.ones(d))


def _pool_live(lib):
    n, b = ctypes.c_int64(-1), ctypes.c_int64(-1)
    assert lib.gpb_debug_pool_live(ctypes.byref(n), ctypes.byref(b)) == 0
    return n.value, b.value


def _shape_b_emulator(tmp):
    """an Emulator at shape B trained at fixed hyper-parameters and a Chain over it (the samplers' workspaces are only
    reachable through a chain)"""
    from gpbayestools_hic_amd import synth
    from gpbayestools_hic_amd.emulator import Emulator
    from gpbayestools_hic_amd.mcmc import Chain
    N, d, P = SHAPES["B"]
    os.makedirs(tmp, exist_ok=True)
    X = synth.lhs(N, d, seed=synth.SEED)
    Y = synth.observables(X, M_OBS, seed=synth.SEED + 1)
    tp, pf, ep = (os.path.join(tmp, n) for n in ("train.pkl", "par.txt", "exp.pkl"))
    synth.write_training_pickle(tp, X, Y, 0.01)
    synth.write_parameter_file(pf, np.zeros(d), np.ones(d))
    emu = Emulator(training_set_path=tp, parameter_file=pf, npc=P, device=0)
    emu.trainEmulator([True] * emu.nev, kernel_type="RBF", thetas=synth.fixed_theta(d, P))
    xstar = synth.truth_point(d)
    yexp = emu.predict(xstar[None, :], return_cov=False)[0]
    synth.write_experiment_pickle(ep, yexp, 0.05 * np.abs(yexp))
    chain = Chain(mcmc_path=os.path.join(tmp, "mcmc", "chain.pkl"), expdata_path=ep, model_parafile=pf, device=0)
    chain.emuList = [emu]
    return chain, emu, xstar


def test_nothing_leaks(tmp_path):
    """Every grown workspace of a context is reached once at shape B; the buffers out of the debug library's cache rise by at
    least the ones that can be named, and close() brings count and bytes exactly back."""
    import torch
    from gpbayestools_hic_amd import GPEngine, _native as nat, mcmc, ptlmc, synth
    from gpbayestools_hic_amd.sampler import StretchSampler
    from gpbayestools_hic_amd.smc import SMCSampler
    if not os.path.exists(nat.LIB_PATHS[True]):
        pytest.fail("libgpbayes_debug.so is not built: gpb_debug_pool_live lives there")
    N, d, P = SHAPES["B"]
    pr = _problem("B")
    dev = torch.device("cuda", 0)
    with nat.debug_library():
        lib = nat.load()
        mcmc._utility_engine()               # (whichever library it binds, it exists before the first reading and stays)
        # (with GPB_DEBUG_LIB=1 the whole suite's engines live in this library: one that an earlier test dropped but the collector
        # has not yet finalised would give its buffers back between two readings)
        gc.collect()
        live0 = _pool_live(lib)

        eng = GPEngine(0)
        assert eng.lib is lib
        eng.set_data(pr["X"], pr["Z"])
        eng.lml(pr["theta"], eval_gradient=True)                                    # gpart
        eng.set_point_noise(np.full((P, N), 1e-3))                                  # pnoise
        eng.set_theta(pr["theta"])
        eng.factor()
        for W in (W_SMALL, W_LARGE):                                                # the digit planes; the walker workspaces grow
            eng.predict(pr["Xq"][:W])
        eng.predict_cov(pr["Xq"][:W_SMALL])                                         # vbuf, covbuf
        eng.predict_grad(pr["Xq"][:W_SMALL])                                        # gbuf
        eng.cross_validate()                                                        # cv_ws
        eng.set_transform(0, pr["mu"], A=pr["A"], cov_trunc=pr["cov_trunc"])        # A, mu, scale, C0
        eng.emu_predict(pr["Xq"][:W_SMALL])
        eng.sobol(pr["lo"], pr["hi"])                                               # sobol_ws
        cand = torch.as_tensor(synth.walkers(40, d, seed=5), device=dev)
        ref = torch.as_tensor(synth.walkers(30, d, seed=6), device=dev)
        eng.design_begin(cand, ref, torch.full((30,), 1.0 / 30, dtype=torch.float64, device=dev), np.ones(P))   # design_ws
        eng.design_run(3)                                                           # design_run (and no design_end)
        eng.set_likelihood(pr["yexp"], pr["cov_exp"])                               # yexp, Cexp, lr_R, lr_v0
        Xd = torch.as_tensor(pr["Xq"], device=dev)
        Xd[3, 0] = 1.5                                                              # a row outside the prior box
        eng.loglike(Xd)
        lo, hi = torch.zeros(d, dtype=torch.float64, device=dev), torch.ones(d, dtype=torch.float64, device=dev)
        eng.logpost(Xd, torch.empty(W_LARGE, dtype=torch.float64, device=dev), False, lo, hi, -np.inf, 0.0)   # cmp_X, cmp_idx
        rng = np.random.default_rng(3)
        r = rng.standard_normal((2, 140, 140))
        eng.mvn_loglike(rng.standard_normal((2, 140)), r @ r.transpose(0, 2, 1) + 140.0 * np.eye(140))       # mvn_ws
        # GPEngine.set_param_map takes the package's three fixed parameter groups, whose map cannot end in d = 3 columns: the
        # smallest map of the C ABI instead — 4 parameters, one group of kind 0 over all four, one component
        tab = np.zeros((1, 5, 100))
        tab[0, 0], tab[0, 2], tab[0, 4] = np.linspace(0.0, 0.5, 100), 1.0, 0.1
        eng._ck(lib.gpb_param_map_set(eng.h, 4, d, nat.ptr(np.array([0, 1, -1], dtype=np.int32)), 1,
                                      nat.ptr(np.array([[0, 0, 1, 2, 3, 1]], dtype=np.int32)), nat.ptr(tab), 1))   # pmap_int, pmap_tab
        eng.pmap_d_in, eng.pmap_d_out = 4, d
        eng.param_map(torch.as_tensor(synth.walkers(W_SMALL, 4, seed=7), device=dev))
        eng.tile_trace(64)                                                          # tile_trace
        eng.sync()
        # the buffers named above plus what every context with GPs holds: notpd, rows_live, n_nan, tile_counter; X, Xsc, xmean,
        # muS, Xc, dnorm, thblk, Z, K, Linv, T, yv, alpha, info, lmlbuf, gpN, kmtiles; Xs, estd, KsT, mpart, spart, mean_pc,
        # var_pc, cmp_idx; slA, slB, sl_scale; out_stage
        planes = 3 if eng.predict_sliced else 0      # (the suite also runs with GPB_PREDICT_SLICED=0: no digit planes then)
        named = 4 + 17 + 8 + planes + 1 + len(("gpart", "pnoise", "vbuf", "covbuf", "gbuf", "cv_ws", "A", "mu", "scale", "C0",
                                          "sobol_ws", "design_ws", "design_run", "yexp", "Cexp", "lr_R", "lr_v0", "cmp_X",
                                          "mvn_ws", "pmap_int", "pmap_tab", "tile_trace"))
        live1 = _pool_live(lib)
        assert live1[0] - live0[0] >= named and live1[1] > live0[1]
        eng.close()
        assert _pool_live(lib) == live0

        chain, emu, xstar = _shape_b_emulator(str(tmp_path))
        e0 = emu._engine_ready()
        assert e0.lib is lib
        st = StretchSampler(chain, 16, seed=5)
        assert st._resident_engine() is not None
        st.run(synth.walkers(16, d, seed=9), 3)                                     # mc_ws
        T = 6
        temps = ptlmc.ladder(4, 2, 20.0)
        th = np.clip(xstar + 0.03 * np.random.default_rng(11).standard_normal((T, d)), 0.02, 0.98)
        covmat0, hc = ptlmc.proposal_factor(th)
        pt = ptlmc.PTLMCSampler(chain, temps, hc, covmat0, 4, 2, 2, 2, ptlmc.TARACC_PLAIN, 11, False)
        pt.set_state(th, chain.log_posterior(th) / temps)
        pt.run(4)                                                                   # ptl_ws
        sm = SMCSampler(chain, 64, 0.5, 11)
        sm.init_uniform()
        sm.reweight()
        sm.move(1)                                                                  # smc_ws
        sm.read_block()
        e0.sync()
        live2 = _pool_live(lib)
        assert live2[0] - live0[0] >= 4 + 17 + 8 + len(("mc_ws", "ptl_ws", "smc_ws"))
        e0.close()
        assert _pool_live(lib) == live0


def _outputs(eng, shape):
    """the calls of the re-set test on whatever the engine held before, from set_data on"""
    pr = _problem(shape)
    eng.set_data(pr["X"], pr["Z"])
    out = list(eng.lml(pr["theta"], eval_gradient=True))
    eng.set_theta(pr["theta"])
    eng.factor()
    for W in (W_SMALL, W_LARGE):
        out += eng.predict(pr["Xq"][:W])
    eng.set_transform(0, pr["mu"], A=pr["A"], cov_trunc=pr["cov_trunc"])
    out += eng.emu_predict(pr["Xq"][:W_SMALL])
    eng.set_likelihood(pr["yexp"], pr["cov_exp"])
    out.append(eng.loglike(pr["Xq"]))
    out += eng.cross_validate()
    out += eng.sobol(pr["lo"], pr["hi"])
    return [np.array(o) for o in out]


@pytest.fixture(scope="module")
def fresh():
    """what a fresh engine gives at each shape (computed once)"""
    from gpbayestools_hic_amd import GPEngine
    ref = {}
    for shape in SHAPES:
        eng = GPEngine(0)
        ref[shape] = _outputs(eng, shape)
        eng.close()
    return ref


def test_a_reset_context_is_a_fresh_context(fresh):
    """one engine through A, B, A: every output after each set_data is bit-equal to a fresh engine's at that shape"""
    from gpbayestools_hic_amd import GPEngine
    eng = GPEngine(0)
    for shape in ("A", "B", "A"):
        got = _outputs(eng, shape)
        assert len(got) == len(fresh[shape])
        for i, (g, f) in enumerate(zip(got, fresh[shape])):
            assert np.all(np.isfinite(f)), (shape, i)
            assert np.array_equal(g, f), (shape, i)
    eng.close()
