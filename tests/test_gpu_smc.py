"""GPU tier of the SMC sampler: gpb_chain_smc_reweight / gpb_chain_smc_move (through smc.SMCSampler and Chain.run_SMC) against
the numpy restatement of tests/smc_reference.py, fed the device's own draws."""
import os
import pickle

import numpy as np
import pytest

import smc_reference as R
from sampler_cases import wide_chain

pytestmark = pytest.mark.gpu


def _emulator(tmp, N, d, M, P, kernel="RBF", ell=1.5, seed=0, lo=None, hi=None):
    """an Emulator trained at fixed hyper-parameters on synthetic data, plus a Chain over it whose experiment is the noiseless
    prediction at the truth point (5 % errors)"""
    from gpbayestools_hic_amd import synth
    from gpbayestools_hic_amd.emulator import Emulator
    from gpbayestools_hic_amd.mcmc import Chain
    os.makedirs(tmp, exist_ok=True)
    lo, hi = (np.zeros(d), np.ones(d)) if lo is None else (lo, hi)
    X = synth.lhs(N, d, seed=synth.SEED + seed)
    Y = synth.observables(X, M, seed=synth.SEED + 1 + seed)
    tp, pf, ep = (os.path.join(tmp, n) for n in ("train.pkl", "par.txt", "exp.pkl"))
    synth.write_training_pickle(tp, X, Y, 0.01)
    synth.write_parameter_file(pf, lo, hi)
    emu = Emulator(training_set_path=tp, parameter_file=pf, npc=P, device=0)
    emu.trainEmulator([True] * emu.nev, kernel_type=kernel, thetas=synth.fixed_theta(d, P, ell=ell))
    xstar = synth.truth_point(d)
    yexp = emu.predict(xstar[None, :], return_cov=False)[0]
    synth.write_experiment_pickle(ep, yexp, 0.05 * np.abs(yexp))
    chain = Chain(mcmc_path=os.path.join(tmp, "mcmc", "chain.pkl"), expdata_path=ep, model_parafile=pf, device=0)
    chain.emuList = [emu]
    return chain, emu, xstar


def _sampler(chain, N, seed=11, ess_fraction=0.5):
    from gpbayestools_hic_amd.smc import SMCSampler
    s = SMCSampler(chain, N, ess_fraction, seed)
    s.init_uniform()
    return s


def _ll(chain):
    return lambda X: chain.log_likelihood(X, finite=True)


def _rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))) if a.size else 0.0


def _check_stage(s, lc_normwise=False):
    """one reweight call against the restatement from the device's state before it; -> boundary cases excluded.
    The C ABI has no covariance output: the covariance the device factorised is Ld Ld^T (Ld is its exact Cholesky factor up
    to the rounding of the factorisation, ~d eps |cov|), and that product is held to the restatement's covariance.
    lc_normwise: Lc within 1e-10 of the largest entry instead of entry by entry (see test_stage_near_the_largest_d)"""
    before = s.state()
    s.reweight()
    got = s.state()
    rw = R.reweight(before["logl"], before["beta"], s.ess_fraction)
    assert abs(got["beta"] - rw["beta"]) <= 1e-10 * rw["beta"], (got["beta"], rw["beta"])
    assert abs(got["dlogz"] - rw["dlogz"]) <= 1e-10 * abs(rw["dlogz"]), (got["dlogz"], rw["dlogz"])
    assert abs(got["logz"] - (before["logz"] + got["dlogz"])) <= 1e-15 * max(1.0, abs(got["logz"]))
    assert abs(got["ess"] - rw["ess"]) <= 1e-8 * rw["ess"]
    u = R.device_draws(s.seed, before["stage"], 0, 2, 1)["u_resample"]
    # the ancestors from the device's own beta (the weights then agree to rounding)
    w, _ = R.weights(before["logl"], got["beta"] - before["beta"])
    anc, cum, pos = R.resample(w, u)
    edge = R.knife_edges(anc, cum, pos)       # within 1e-12 of the scan entry that decides (also tests/test_smc_reference.py)
    dev_anc = s.ancestors.cpu().numpy()
    assert int(edge.sum()) <= 2, int(edge.sum())
    assert np.array_equal(dev_anc[~edge], anc[~edge])
    assert np.array_equal(got["x"], before["x"][dev_anc]) and np.array_equal(got["logl"], before["logl"][dev_anc])
    mean, cov, Lc = R.precondition(got["x"])
    assert np.max(np.abs(s.mean.cpu().numpy() - mean)) <= 1e-12
    Ld = got["Lc"]
    assert np.all(np.triu(Ld, 1) == 0)
    assert np.max(np.abs(Ld @ Ld.T - cov)) <= 1e-12 * max(1.0, np.abs(cov).max())
    if lc_normwise:
        assert np.max(np.abs(Ld - Lc)) <= 1e-10 * np.abs(Lc).max()
    else:
        assert _rel(Ld[np.tril_indices(s.d)], Lc[np.tril_indices(s.d)]) <= 1e-10
    return int(edge.sum())


def _check_step(chain, s, state, x_absolute=False):
    """one move(1) call against the restatement; -> 1 when a knife-edge decision differed (compare on from the next step).
    x_absolute: x within 1e-12 of the unit box's width instead of each entry's own size"""
    before = s.state()
    k = before["k"]
    dr = R.device_draws(s.seed, 0, k, s.N, s.d)
    x, logl, ls, info = R.move_step(before["x"], before["logl"], before["beta"], before["log_sigma"], before["Lc"], before["s"],
                                    dr["normals"], dr["logu_accept"], _ll(chain))
    s.move(1)
    got = s.state()
    took = np.any(got["x"] != before["x"], axis=1) | (got["logl"] != before["logl"])
    tie = np.abs(info["delta"] - dr["logu_accept"]) < 1e-9
    assert np.array_equal(took[~tie], info["accepted"][~tie]), k
    assert got["naccept"] - before["naccept"] == int(took.sum())
    assert np.array_equal(got["logl"], _ll(chain)(got["x"])), k           # bit for bit
    assert np.all((got["x"] > chain.min) & (got["x"] < chain.max))
    if np.any(took != info["accepted"]):
        return 1
    assert (np.max(np.abs(got["x"] - x)) if x_absolute else _rel(got["x"], x)) <= 1e-12, k
    assert abs(got["log_sigma"] - ls) <= 1e-12, k
    return 0


def test_draws_match_restatement():
    import torch
    from gpbayestools_hic_amd import _native as nat
    from gpbayestools_hic_amd.engine import GPEngine
    with nat.debug_library():
        eng = GPEngine(0)
    for (N, d, seed, stage, k) in [(10, 4, 7, 0, 0), (37, 9, 2 ** 40 + 3, 5, 123), (130, 15, 12345, 77, 2999),
                                   (1027, 127, 2 ** 33 + 5, 3, 41), (16389, 5, 99, 1, 7)]:
        nrm = torch.empty((N, d), dtype=torch.float64, device="cuda:0")
        la = torch.empty(N, dtype=torch.float64, device="cuda:0")
        ur = torch.empty(1, dtype=torch.float64, device="cuda:0")
        eng._ck(eng.lib.gpb_test_smc_draws(eng.h, N, d, seed, stage, k, nat.ptr(nrm), nat.ptr(la), nat.ptr(ur)))
        ref = R.device_draws(seed, stage, k, N, d)
        assert ur.cpu().numpy()[0] == ref["u_resample"]
        assert np.max(np.abs(nrm.cpu().numpy() - ref["normals"])) <= 1e-15 * max(1.0, np.abs(ref["normals"]).max())
        assert np.max(np.abs(la.cpu().numpy() - ref["logu_accept"])) <= 1e-15 * max(1.0, np.abs(ref["logu_accept"]).max())
    # the limits of the kernels are errors: d beyond 128, N beyond 2 .. 2^20
    assert eng.lib.gpb_test_smc_draws(eng.h, 16, 129, 1, 0, 0, nat.ptr(nrm), nat.ptr(la), nat.ptr(ur)) == -1
    assert eng.lib.gpb_test_smc_draws(eng.h, 1, 4, 1, 0, 0, nat.ptr(nrm), nat.ptr(la), nat.ptr(ur)) == -1
    eng.close()


def test_stage_by_stage(tmp_path):
    chain, emu, xstar = _emulator(str(tmp_path), 192, 4, 8, 4)
    s = _sampler(chain, 512)
    stages = 0
    while stages < 6 or s.read_block()["beta"] < 1.0:
        _check_stage(s)
        s.move(5)
        stages += 1
        assert stages < 60
    assert stages >= 6


def test_step_by_step_across_a_stage_boundary(tmp_path):
    chain, emu, xstar = _emulator(str(tmp_path), 192, 4, 8, 4)
    s = _sampler(chain, 512)
    near = 0
    for _ in range(3):
        s.reweight()
        for _ in range(12):
            near += _check_step(chain, s, None)
    assert s.k == 36 and near <= 2
    assert s.read_block()["naccept"] > 0


def test_call_splitting(tmp_path):
    chain, emu, xstar = _emulator(str(tmp_path), 192, 4, 8, 4)
    a, b, c = (_sampler(chain, 512) for _ in range(3))
    for _ in range(3):                        # a: whole stages in one call each; b: single steps
        a.reweight()
        a.move(8)
        b.reweight()
        for _ in range(8):
            b.move(1)
    sa, sb = a.state(), b.state()
    for key in sa:
        assert np.array_equal(sa[key], sb[key]), key
    # c: the same run, interrupted at a stage boundary and continued in a new sampler from the state read back
    c.reweight()
    c.move(8)
    st = c.state()
    from gpbayestools_hic_amd.smc import SMCSampler
    c2 = SMCSampler(chain, 512, 0.5, c.seed)
    c2.set_state(st["x"], st["logl"], st["beta"], st["logz"], st["log_sigma"], st["stage"], st["k"], st["s"])
    for _ in range(2):
        c2.reweight()
        c2.move(8)
    sc = c2.state()
    for key in ("x", "logl", "beta", "logz", "log_sigma", "Lc", "stage", "k"):
        assert np.array_equal(sa[key], sc[key]), key


def _short_run(chain, N=256, nmcmc=4, seed=3):
    out = chain.run_SMC(n_particles=N, nmcmc=nmcmc, seed=seed)
    assert out["beta"][-1] == 1.0 and np.all(np.diff(out["beta"]) > 0)
    assert np.array_equal(out["logl"], chain.log_likelihood(out["chain"], finite=True))
    assert np.all((out["chain"] > chain.min) & (out["chain"] < chain.max)) and np.isfinite(out["logz"])
    return out


def test_chain_shapes_two_emulators(tmp_path):
    from gpbayestools_hic_amd.workload import build_multi_chain
    chain, emus, info = build_multi_chain([(128, 12, 3, "RBF"), (112, 10, 3, "Matern25")], 20, workdir=str(tmp_path))
    _short_run(chain)


@pytest.mark.parametrize("rejected", [False, True])
def test_chain_shapes_parameter_trafo_pca(tmp_path, rejected):
    """the second emulator maps its parameters (parameterTrafoPCA).  rejected: with the box compaction switched off
    gpb_chain_supported turns the chain down and the per-emulator sequence (parameter map, gpb_loglike, gpb_box_finish)
    evaluates the proposals; otherwise the chain call does"""
    from gpbayestools_hic_amd.workload import build_multi_chain
    chain, emus, info = build_multi_chain([(128, 12, 3, "RBF"), (112, 10, 3, "Matern25")], 20, workdir=str(tmp_path),
                                          mapped=[False, True])
    if rejected:
        for e in emus:
            e._engine_ready().tune("compact", 0)
    chain._prepare_blocks()
    assert (chain._chain_contexts() is None) == rejected
    _short_run(chain)


def test_chain_shapes_fp64_and_int8_arithmetic(tmp_path):
    chain, emu, xstar = _emulator(str(tmp_path), 192, 4, 8, 4)
    a = _short_run(chain)
    chain.set_predict_arithmetic("fp64")
    b = _short_run(chain)
    assert abs(a["beta"][0] - b["beta"][0]) <= 1e-6 * a["beta"][0]     # the same start particles, logl within ~1e-11
    first = []                                # the first stage's evidence increment in both arithmetics
    for mode in ("fp64", "fp64-int8"):
        chain.set_predict_arithmetic(mode)
        s = _sampler(chain, 256, seed=3)
        s.reweight()
        first.append(s.read_block()["dlogz"])
    assert abs(first[0] - first[1]) <= 1e-6 * abs(first[0]), first


def test_tight_box_rejects_outside_proposals(tmp_path):
    """a box so tight around the truth point that most proposals leave it: none of those is ever accepted"""
    d = 4
    from gpbayestools_hic_amd import synth
    xs = synth.truth_point(d)
    chain, emu, xstar = _emulator(str(tmp_path), 192, d, 8, 4)
    chain.min, chain.max = xs - 1e-3, xs + 1e-3
    chain.prior_volume_ = np.prod(chain.max - chain.min)
    s = _sampler(chain, 256)
    s.reweight()
    # a proposal scale far wider than the box
    st = s.state()
    s.set_state(st["x"], st["logl"], st["beta"], st["logz"], np.log(50.0), st["stage"], st["k"], 0)
    s.Lc.copy_(s.torch.as_tensor(st["Lc"]))
    outside = 0
    for _ in range(6):
        before = s.state()
        dr = R.device_draws(s.seed, 0, before["k"], s.N, s.d)
        xp = R.propose(before["x"], before["log_sigma"], before["Lc"], dr["normals"])
        out = ~np.all((xp > chain.min) & (xp < chain.max), axis=1)
        s.move(1)
        got = s.state()
        assert np.array_equal(got["x"][out], before["x"][out]) and np.array_equal(got["logl"][out], before["logl"][out])
        assert np.all((got["x"] > chain.min) & (got["x"] < chain.max))
        outside += int(out.sum())
    assert outside > 3 * s.N


def test_limits_and_refusals(tmp_path):
    import torch
    from gpbayestools_hic_amd import _native as nat
    from gpbayestools_hic_amd.smc import SMCSampler
    chain, emu, xstar = _emulator(str(tmp_path), 160, 4, 6, 3)
    s = _sampler(chain, 64)
    engs, arr, E = chain._contexts()
    e0 = engs[0]
    lo, hi = chain._box(s.dev)
    big = torch.zeros(8, dtype=torch.float64, device="cuda:0")
    for N in (1, 0, (1 << 20) + 1):           # checked before anything is touched
        assert e0.lib.gpb_chain_smc_reweight(arr, E, N, 0, 1, 0.5, nat.ptr(big), nat.ptr(big), nat.ptr(s.block), nat.ptr(s.Lc),
                                             None, None) == -1
        assert e0.lib.gpb_chain_smc_move(arr, E, N, 1, 0, 0, 1, nat.ptr(big), nat.ptr(big), nat.ptr(s.block), nat.ptr(s.Lc),
                                         nat.ptr(lo), nat.ptr(hi), -1e300, 0.0) == -1
    assert e0.lib.gpb_chain_smc_move(arr, E, 64, 2, 2 ** 32 - 1, 0, 1, nat.ptr(s.x), nat.ptr(s.logl), nat.ptr(s.block),
                                     nat.ptr(s.Lc), nat.ptr(lo), nat.ptr(hi), -1e300, 0.0) == -1
    assert e0.lib.gpb_chain_smc_reweight(arr, E, 64, 0, 1, 1.5, nat.ptr(s.x), nat.ptr(s.logl), nat.ptr(s.block), nat.ptr(s.Lc),
                                         None, None) == -1

    class Sharded:
        world = 2
    chain.sharding = Sharded()
    with pytest.raises(NotImplementedError, match="shard"):
        chain.run_SMC(n_particles=64)
    chain.sharding = None

    class Foreign:
        nobs = emu.nobs

        def predict(self, X, return_cov=True, extra_std=0.0):
            return emu.predict(X, return_cov=return_cov, extra_std=extra_std)
    chain.emuList = [Foreign()]
    with pytest.raises(NotImplementedError, match="foreign"):
        chain.run_SMC(n_particles=64)
    with pytest.raises(NotImplementedError, match="foreign"):
        SMCSampler(chain, 64)


def test_more_parameters_than_the_limit_is_an_argument_error(tmp_path):
    """a chain of 129 parameters: GPB_E_ARG from both entry points, before anything is enqueued"""
    import torch
    from gpbayestools_hic_amd import _native as nat
    chain = wide_chain(str(tmp_path), 129)
    s = _sampler(chain, 64)                   # (the start particles are evaluated by the chain call, which has no such limit)
    assert np.all(np.isfinite(s.logl.cpu().numpy()))
    engs, arr, E = chain._contexts()
    e0 = engs[0]
    lo, hi = chain._box(s.dev)
    assert e0.lib.gpb_chain_smc_reweight(arr, E, 64, 0, 1, 0.5, nat.ptr(s.x), nat.ptr(s.logl), nat.ptr(s.block), nat.ptr(s.Lc),
                                         None, None) == -1
    assert e0.lib.gpb_chain_smc_move(arr, E, 64, 1, 0, 0, 1, nat.ptr(s.x), nat.ptr(s.logl), nat.ptr(s.block), nat.ptr(s.Lc),
                                     nat.ptr(lo), nat.ptr(hi), -1e300, 0.0) == -1
    torch.cuda.synchronize()
    assert s.read_block()["beta"] == 0.0 and s.k == 0


def test_stage_near_the_largest_d(tmp_path):
    """d = 127 (odd: the last normal of a row is half a pair; the lanes of the proposal kernel make a second pass; Lc and the
    normals take 127 KiB of LDS, past the 64 KiB a kernel gets without asking): two stages of a reweighting and three single
    move steps each against the restatement, logl bitwise.
    Lc is held to 1e-10 of its largest entry, not entry by entry: the restatement factorises with LAPACK, whose order of
    operations is not the kernel's, so the two factors differ by the factorisation's own rounding, ~d eps cond(cov) |Lc| =
    127 * 1.1e-16 * cond, and that is 1e-10 for cond up to 7e3; of the 8128 entries of the factor of a sampled covariance
    (|Lc| up to 0.29, typical off-diagonal 0.29 / sqrt(N) = 0.013) the smallest are ~1e-6, where 1e-10 of the entry itself
    is less than that rounding.  x is held to 1e-12 of the unit box for the same reason: entries of x down to 1e-5 occur."""
    chain = wide_chain(str(tmp_path), 127)
    s = _sampler(chain, 512)
    assert s.d == 127
    near = 0
    for _ in range(2):
        _check_stage(s, lc_normwise=True)
        for _ in range(3):
            near += _check_step(chain, s, None, x_absolute=True)
    assert near <= 2 and s.read_block()["naccept"] > 0


def test_degenerate_ensemble_raises(tmp_path):
    """all particles equal: the covariance is exactly zero, the factorisation kernel sets its flag, the host raises"""
    chain, emu, xstar = _emulator(str(tmp_path), 160, 4, 6, 3)
    s = _sampler(chain, 128)
    s.set_state(np.tile(xstar[None, :] * 0.97, (128, 1)))
    s.reweight()
    with pytest.raises(RuntimeError, match="not positive definite"):
        s.read_block()
    with pytest.raises(RuntimeError, match="not positive definite"):
        s.run(2, 3)


def test_end_to_end_against_quadrature(tmp_path):
    """d = 2: logz and the posterior mean of run_SMC over 8 seeds against a 400 x 400 midpoint quadrature of
    exp(log_likelihood) over the box (evaluated on the device, independent of the sampler), within four standard errors; the
    spread over the seeds may not exceed twice that of the host restatement with numpy draws on the same likelihood."""
    chain, emu, xstar = _emulator(str(tmp_path), 160, 2, 6, 3)
    g = (np.arange(400) + 0.5) / 400.0
    G = np.stack(np.meshgrid(chain.min[0] + g * (chain.max[0] - chain.min[0]),
                             chain.min[1] + g * (chain.max[1] - chain.min[1]), indexing="ij"), axis=-1).reshape(-1, 2)
    ll = chain.log_likelihood(G, finite=True)
    mx = ll.max()
    w = np.exp(ll - mx)
    logz_q = mx + np.log(np.mean(w))
    mean_q = (w[:, None] * G).sum(0) / w.sum()
    N, nmcmc = 1024, 10
    dev = [chain.run_SMC(n_particles=N, nmcmc=nmcmc, seed=100 + i) for i in range(8)]
    host = [R.run(_ll(chain), chain.min, chain.max, N, 0.5, nmcmc, 200, 200 + i) for i in range(8)]
    sd_stats = lambda rs, key: np.array([np.concatenate(([r["logz"]], r[key].mean(0))) for r in rs])      # noqa: E731
    a, b = sd_stats(dev, "chain"), sd_stats(host, "x")
    truth = np.concatenate(([logz_q], mean_q))
    sd, sd_host = a.std(0, ddof=1), b.std(0, ddof=1)
    err = np.abs(a.mean(0) - truth)
    print("quadrature", truth, "device mean", a.mean(0), "sd", sd, "host sd", sd_host, "err", err)
    assert np.all(sd <= 2.0 * sd_host), (sd, sd_host)
    assert np.all(err <= 4.0 * sd / np.sqrt(8.0)), (err, sd)


def test_pickle_schema(tmp_path):
    chain, emu, xstar = _emulator(str(tmp_path), 160, 4, 6, 3)
    out = chain.run_SMC(n_particles=256, nmcmc=5, seed=9)
    with open(chain.mcmc_path, "rb") as f:
        data = pickle.load(f)
    assert list(data) == ["chain", "weights", "logl", "logp", "logz", "logz_err"]
    assert data["chain"].shape == (256, 4) and data["weights"].shape == (256,) and data["logl"].shape == (256,)
    assert data["logp"].shape == (256,) and np.all(data["logp"] == -np.log(chain.prior_volume_))
    assert np.all(data["weights"] == 1.0 / 256) and np.isfinite(data["logz"]) and np.isnan(data["logz_err"])
    assert np.array_equal(data["chain"], out["chain"]) and data["logz"] == out["logz"]
    assert out["beta"][-1] == 1.0 and np.all(np.diff(out["beta"]) > 0) and out["beta"][0] > 0
    assert out["acceptance"].shape == out["beta"].shape and np.all((out["acceptance"] >= 0) & (out["acceptance"] <= 1))
    again = chain.run_SMC(n_particles=256, nmcmc=5, seed=9)
    assert np.array_equal(again["chain"], out["chain"]) and again["logz"] == out["logz"]


# ------------------------------------------------------------------ beyond one pass of the kernels' strided loops
# k_smc_reweight: 1024 threads, a contiguous chunk of C = ceil(N / 1024) weights each, the first 16384 logl - max in LDS;
# k_smc_propose: min(ceil(N / 4), 2 CUs) workgroups of four waves striding over the particles; k_smc_resample / k_smc_accept:
# 256 rows per workgroup.  Every size above 1024 gives C > 1, every size that is no multiple of 256 a ragged last workgroup.
def _stages_and_steps(tmp_path, N, d, stages, steps):
    chain, emu, xstar = _emulator(str(tmp_path), 192, d, 8, 4)
    s = _sampler(chain, N)
    near = 0
    for _ in range(stages):
        _check_stage(s)
        for _ in range(steps):
            near += _check_step(chain, s, None)
    assert near <= 2 and s.k == stages * steps and s.read_block()["naccept"] > 0
    return s


def test_ragged_two_entry_chunks(tmp_path):
    """N = 1027 (a multiple of neither 4, 64 nor 256), d = 5: C = 2, thread 513 owns one weight, the threads from 514 on none;
    the last quad of the proposals has one particle, the last workgroup of the resampling and of the accept three rows"""
    _stages_and_steps(tmp_path, 1027, 5, 2, 3)


def test_strided_proposals(tmp_path):
    """N = 8 CUs + 3: workgroup 0 of k_smc_propose makes a second trip in which one of its four waves has no particle"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    N = 8 * cus + 3
    assert N > 8 * cus and -(-N // 4) > 2 * cus               # more quads than workgroups: the particle loop strides
    _stages_and_steps(tmp_path, N, 5, 1, 2)


def test_default_size(tmp_path):
    """run_SMC's default of 4096 particles: C = 4, two trips of the proposal loop on 256 CUs"""
    s = _stages_and_steps(tmp_path, 4096, 5, 1, 2)
    a, b = _sampler(s.chain, 4096), _sampler(s.chain, 4096)
    a.reweight()
    a.move(3)
    b.reweight()
    for _ in range(3):
        b.move(1)
    sa, sb = a.state(), b.state()
    for key in sa:
        assert np.array_equal(sa[key], sb[key]), key


def test_past_the_lds_window(tmp_path):
    """N = 16389, d = 4: C = 17, the last five logl - max are re-read from global memory in every pass of the bisection,
    thread 964 owns one weight and the threads behind it none"""
    _stages_and_steps(tmp_path, 16389, 4, 1, 1)


def _injected(chain, N, logl, beta=0.0):
    s = _sampler(chain, N)
    s.set_state(np.random.default_rng(N).uniform(chain.min, chain.max, (N, s.d)), logl=logl, beta=beta)
    return s


@pytest.mark.parametrize("beta", [0.0, 0.37])
@pytest.mark.parametrize("N", R.INJECTED_SIZES)
def test_injected_weights(tmp_path, N, beta):
    """log-likelihoods set by hand (smc_reference.injected_logl: runs of zero weights at both ends and inside, NaNs across a
    chunk boundary), no chain evaluation: the stage against the restatement, the NaN counter, and no ancestor of weight zero.
    tests/test_smc_reference.py shows on the host that the cap of 2 knife edges hides nothing here."""
    chain, emu, xstar = _emulator(str(tmp_path), 192, 4, 8, 4)
    logl = R.injected_logl(N)
    s = _injected(chain, N, logl, beta)
    _check_stage(s)
    assert s.read_block()["nan_weights"] == 6
    anc = s.ancestors.cpu().numpy()
    assert np.all(np.isfinite(logl[anc]) & (logl[anc] > -1e300))
    assert np.all(np.diff(anc) >= 0)


def test_equal_weights(tmp_path):
    """a constant log-likelihood: one stage reaches beta = 1 with ESS = N, every particle is its own ancestor"""
    N = 1027
    chain, emu, xstar = _emulator(str(tmp_path), 192, 4, 8, 4)
    s = _injected(chain, N, np.full(N, -12.5))
    _check_stage(s)
    blk = s.read_block()
    assert blk["beta"] == 1.0 and blk["ess"] == float(N)       # every weight is exp(0) = 1: the sums are exact
    u = R.device_draws(s.seed, 0, 0, 2, 1)["u_resample"]
    assert 1e-9 < u < 1.0 - 1e-9                               # positions (u + i) / N well inside (i / N, (i + 1) / N)
    assert np.array_equal(s.ancestors.cpu().numpy(), np.arange(N))


@pytest.mark.parametrize("value", [np.nan, -np.inf])
def test_no_finite_weight_raises(tmp_path, value):
    """all NaN / all -inf: every weight is 0, the scan is 0 / 0, the search of k_smc_resample ends at its clamp N - 1; the
    flag is raised on the host and a good state afterwards works"""
    N = 1027
    chain, emu, xstar = _emulator(str(tmp_path), 192, 4, 8, 4)
    s = _injected(chain, N, np.full(N, value))
    s.reweight()
    with pytest.raises(RuntimeError, match="no particle has a finite log-likelihood"):
        s.read_block()
    anc = s.ancestors.cpu().numpy()
    assert np.all((anc >= 0) & (anc <= N - 1))
    s.init_uniform()
    _check_stage(s)
    assert s.read_block()["nan_weights"] == 0


def test_nan_proposals_are_counted_and_rejected(tmp_path):
    """an indefinite experimental covariance makes every block NaN (tests/test_gpu_sampler.py does the same to the stretch
    move).  A proposal outside the box never reaches the blocks: it takes the outside value and is rejected without being
    counted, so first, at the stage's own proposal scale, the counter must equal the number of restated proposals inside the
    box; then, with a proposal scale of 1e-9 that keeps every proposal inside, two move steps change neither x nor logl, count
    2 N NaN proposals, accept nothing, and log_sigma falls by 0.234 / (s + 1) per step"""
    N = 1027
    chain, emu, xstar = _emulator(str(tmp_path), 192, 4, 8, 4)
    s = _sampler(chain, N)
    s.reweight()
    s.move(3)
    before = s.state()
    assert before["nan_moves"] == 0 and before["naccept"] > 0 and before["s"] == 3

    def proposals_inside(st):
        xp = R.propose(st["x"], st["log_sigma"], st["Lc"], R.device_draws(s.seed, 0, st["k"], N, s.d)["normals"])
        return np.all((xp > chain.min) & (xp < chain.max), axis=1)

    good_cov = chain.expdata_cov
    try:
        chain.expdata_cov = -0.5 * np.eye(chain.nobs)
        inside = 0
        for _ in range(2):
            inside += int(proposals_inside(s.state()).sum())
            s.move(1)
        mid = s.state()
        assert 0 < inside < 2 * N and mid["nan_moves"] == inside and mid["naccept"] == before["naccept"]
        assert np.array_equal(mid["x"], before["x"]) and np.array_equal(mid["logl"], before["logl"])
        assert abs(mid["log_sigma"] - (before["log_sigma"] - 0.234 / 4.0 - 0.234 / 5.0)) <= 1e-12
        # the same particles with a tiny proposal scale (set_state zeroes the counters and leaves Lc alone)
        s.set_state(mid["x"], mid["logl"], mid["beta"], mid["logz"], np.log(1e-9), mid["stage"], mid["k"], mid["s"])
        tiny = s.state()
        assert np.array_equal(tiny["Lc"], before["Lc"]) and proposals_inside(tiny).all()
        s.move(2)
        got = s.state()
    finally:
        chain.expdata_cov = good_cov
    assert np.array_equal(got["x"], before["x"]) and np.array_equal(got["logl"], before["logl"])
    assert got["nan_moves"] == 2 * N and got["naccept"] == tiny["naccept"] == 0
    assert abs(got["log_sigma"] - (tiny["log_sigma"] - 0.234 / 6.0 - 0.234 / 7.0)) <= 1e-12
    _check_step(chain, s, None)                                # and the sampler carries on once the cause is gone
