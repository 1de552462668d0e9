"""GPU tier of the HMC sampler: gpb_chain_hmc_run (through hmc.HMCSampler and Chain.run_HMC) against the numpy restatement of
tests/hmc_reference.py, fed the device's own draws (the call's diag outputs) and the device's gradient at the device's own
trajectory points — the same device call on both sides, as tests/test_gpu_ptlmc.py does with _at_rows."""
import pickle

import numpy as np
import pytest

import hmc_reference as R
from sampler_cases import mapped_chain, wide_chain, wide_start
from test_gpu_ptlmc import _emulator, _rel, _rel_inf

pytestmark = pytest.mark.gpu

BAR = 1e-12


@pytest.fixture(scope="module")
def chain3(tmp_path_factory):
    """the d = 3 chain of most tests: N = 64, M = 8, P = 3"""
    chain, emu, xstar = _emulator(str(tmp_path_factory.mktemp("hmc3")), 64, 3, 8, 3)
    return chain, emu, xstar


def _sampler(chain, X, seed=11, L=3, eps=None, **kw):
    from gpbayestools_hic_amd.hmc import HMCSampler
    s = HMCSampler(chain, X.shape[0], seed=seed, nleapfrog=L, **kw)
    s.set_state(X)
    if eps is not None:
        s.set_step_size(eps)
    return s


def _near(chain, centre, C, seed, radius=0.05):
    rng = np.random.default_rng(seed)
    w = chain.max - chain.min
    return np.clip(centre + radius * w * rng.standard_normal((C, chain.ndim)), chain.min + 0.02 * w, chain.max - 0.02 * w)


def _host(s):
    st = s.state.cpu()
    return (dict(x=s.pos.cpu().numpy(), lp=s.lp.cpu().numpy(), grad=s.grad.cpu().numpy()), st.numpy()[:5].copy(),
            st.view(s.torch.int64).numpy()[5:].copy(), s.naccept.cpu().numpy().copy())


def _step_by_step(chain, s, nsteps, adapt, each=None):
    """nsteps single-step calls, each checked against the restatement from the device's state before it -> knife-edge steps"""
    lo, hi, minv = chain.min, chain.max, s.inv_metric
    near_ties = 0
    for _ in range(nsteps):
        before, st0, cnt0, acc0 = _host(s)
        k = s.k
        dg = s.step_with_diagnostics(adapt)
        got, st1, cnt1, acc1 = _host(s)
        took = (acc1 - acc0).astype(bool)

        def lpg(X, l):
            # the restated positions against the device's, then value and gradient at the device's own points
            assert _rel(X, dg["traj"][l]) <= BAR, (k, l)
            return chain.log_posterior(dg["traj"][l], return_grad=True)

        ref, info = R.step(before, dict(p0=dg["p0"], logu=dg["logu"], eps=dg["eps"]), lpg, minv, lo, hi, s.nleapfrog)
        # the step size and the draws themselves against the independent Philox restatement (exp, log, cos, sin of the two sides)
        dr = R.device_draws(s.seed, k, s.nchains, s.ndim)
        assert abs(dg["eps"] - R.step_size(st0[0], s.jitter, dr["u_eps"])) <= 1e-14 * dg["eps"], k
        assert np.max(np.abs(dg["p0"] * np.sqrt(minv) - dr["z"])) <= 1e-14 * max(1.0, np.abs(dr["z"]).max()), k
        assert np.max(np.abs(dg["logu"] - dr["logu"])) <= 1e-14 * max(1.0, np.abs(dr["logu"]).max()), k
        # the energy error: H0 and H1 to 1e-12 relative, so their difference to 1e-12 of the larger
        fin = np.isfinite(info["dH"])
        assert np.array_equal(np.isnan(dg["dH"]), np.isnan(info["dH"])), k
        assert np.array_equal(dg["dH"][~fin & ~np.isnan(info["dH"])], info["dH"][~fin & ~np.isnan(info["dH"])]), k
        scale = np.maximum(np.maximum(np.abs(info["H0"]), np.abs(info["H1"])), 1.0)
        assert np.all(np.abs(dg["dH"][fin] - info["dH"][fin]) <= BAR * scale[fin]), k
        assert np.array_equal(dg["a"][~fin], info["a"][~fin]), k
        assert np.all(np.abs(dg["a"][fin] - info["a"][fin]) <= BAR * scale[fin]), k
        with np.errstate(invalid="ignore"):
            tie = np.abs(info["dH"] + dg["logu"]) < 1e-9
        assert np.array_equal(took[~tie], info["accepted"][~tie]), k
        # the counters: accepted (the device's own decisions), divergent, escaped, NaN rows
        assert cnt1[0] - cnt0[0] == int(took.sum()), k
        assert cnt1[1] - cnt0[1] == int(info["divergent"].sum()), k
        assert cnt1[2] - cnt0[2] == int(info["escaped"].sum()), k
        assert cnt1[3] - cnt0[3] == int(info["nan_rows"].sum()), k
        assert cnt1[4] == 0, k
        # adaptation: from the device's own accept probabilities, or untouched
        if adapt:
            want = R.dual_average(st0, R.a_mean(dg["a"]), s.target_accept)
            assert np.max(np.abs(st1 - want) / np.maximum(np.abs(want), 1.0)) <= BAR, k
        else:
            assert np.array_equal(st1, st0), k
        if each is not None:
            each(before, info, took, dg)
        if np.any(tie & (took != info["accepted"])):
            near_ties += 1                                   # a decision on a knife edge: compare from the next step on
            continue
        assert _rel(got["x"], ref["x"]) <= BAR, k
        assert _rel_inf(got["lp"], ref["lp"]) <= BAR, k
        assert _rel(got["grad"], ref["grad"]) <= BAR, k
        # the stored lp: bit for bit the chain's log-posterior at the stored row
        assert np.array_equal(got["lp"], chain.log_posterior(got["x"])), k
    return near_ties


@pytest.mark.parametrize("C,L,adapt", [(8, 1, False), (8, 3, True), (70, 1, True), (70, 3, False)])
def test_single_steps_match_restatement(chain3, C, L, adapt):
    """C = 8, less than a wave, and C = 70, a wave and a tail; L = 1 and L = 3; adaptation on and off; one chain starts outside
    the box (lp = -inf, a zero gradient): the restatement decides what happens to it"""
    chain, emu, xstar = chain3
    X = _near(chain, xstar, C, 3)
    X[5, 0] = -0.004
    s = _sampler(chain, X, L=L)
    assert np.isneginf(s.lp.cpu().numpy()[5]) and np.all(s.grad.cpu().numpy()[5] == 0.0)
    seen = dict(back=0)

    def each(before, info, took, dg):
        was_out = np.isinf(before["lp"])
        inside = np.all((info["x"] > chain.min) & (info["x"] < chain.max), axis=1)
        assert np.all(took[was_out & inside & ~info["escaped"]])      # finite - +inf = -inf: back inside is always accepted
        assert not np.any(took[~inside])
        seen["back"] += int(np.sum(was_out & took))

    near = _step_by_step(chain, s, 5, adapt, each=each)
    assert near <= 1
    assert s.counters()["accepted"] > 0 and seen["back"] == 1
    assert np.all(np.isfinite(s.lp.cpu().numpy()))


def test_wide_chain_127_parameters(tmp_path):
    """d = 127 (sampler_cases.wide_chain): a second pass of the lanes of k_hmc_begin / k_hmc_finish, the last normal half a pair"""
    chain = wide_chain(str(tmp_path), 127)
    s = _sampler(chain, _near(chain, wide_start(127), 8, 5, radius=0.02), L=3)
    assert s.ndim == 127
    assert _step_by_step(chain, s, 3, True) <= 1


def test_mapped_chain_71_parameters(tmp_path):
    """71 mapped parameters (sampler_cases.mapped_chain, 64 GP inputs): a box that is not the unit box"""
    chain, emu, mid = mapped_chain(tmp_path, 71)
    s = _sampler(chain, _near(chain, mid, 8, 6, radius=0.01), L=3)
    assert s.ndim == 71
    assert _step_by_step(chain, s, 3, False) <= 1


def test_walls_reflect_once_twice_and_escape(chain3):
    """chains 1e-3 from a wall, one step each at step sizes from 0.01 to 100: over the sweep the restatement sees trajectories
    with one reflection, with two or more in one drift, and escaped ones (rejected and counted), and the device agrees with it
    at every step size"""
    chain, emu, xstar = chain3
    C = 70
    X = _near(chain, xstar, C, 9)
    X[:35, 0] = chain.min[0] + 1e-3
    X[35:, 1] = chain.max[1] - 1e-3
    seen = dict(one=0, more=0, escaped=0)

    def each(before, info, took, dg):
        seen["one"] += int(np.sum((info["most_reflections"] == 1) & ~info["escaped"]))
        seen["more"] += int(np.sum((info["most_reflections"] >= 2) & ~info["escaped"]))
        seen["escaped"] += int(np.sum(info["escaped"]))
        assert not np.any(took[info["escaped"]])
        assert np.all(dg["a"][info["escaped"]] == 0.0)

    for i, eps in enumerate(np.geomspace(0.01, 100.0, 13)):
        s = _sampler(chain, X, seed=20 + i, L=1, eps=float(eps), jitter=0.0)
        _step_by_step(chain, s, 1, False, each=each)
        assert s.counters()["escaped"] == s.n_escaped
    assert seen["one"] > 0 and seen["more"] > 0 and seen["escaped"] > 0, seen


def _bits(s):
    return [s.pos.cpu().numpy(), s.lp.cpu().numpy(), s.grad.cpu().numpy(), s.state.cpu().view(s.torch.int64).numpy(),
            s.naccept.cpu().numpy()]


def test_one_call_equals_single_steps(chain3):
    """one call of 6 steps against 6 calls of one step at C = 70 with adaptation on: bit for bit, the saved samples included"""
    import torch
    chain, emu, xstar = chain3
    X = _near(chain, xstar, 70, 4)
    a, b = _sampler(chain, X, L=3), _sampler(chain, X, L=3)
    sa = torch.zeros((3, 70, 3), dtype=torch.float64, device=a.device)
    sb, la, lb = torch.zeros_like(sa), torch.zeros_like(sa[:, :, 0]), torch.zeros_like(sa[:, :, 0])
    a._advance(6, True, save=sa, lpsave=la, thin=2, count=True)           # steps 0, 2 and 4 land in slots 0, 1 and 2
    for i in range(6):
        if i % 2 == 0:
            b._advance(1, True, save=sb[i // 2:], lpsave=lb[i // 2:], thin=2, count=True)
        else:
            b._advance(1, True, count=True)
    for u, v in zip(_bits(a), _bits(b)):
        assert np.array_equal(u, v)
    assert np.array_equal(sa.cpu().numpy(), sb.cpu().numpy()) and np.array_equal(la.cpu().numpy(), lb.cpu().numpy())
    assert a.state.cpu().numpy()[4] == 6.0 and a.k == b.k == 6 and a.naccept.sum().item() > 0
    assert np.all(sa.cpu().numpy()[2] != 0.0)


def test_a_chains_bits_do_not_depend_on_the_number_of_chains(chain3):
    """chains 0 .. 7 run among 8 and among 70 chains with adaptation off: the same bits"""
    chain, emu, xstar = chain3
    X = _near(chain, xstar, 70, 4)
    a, b = _sampler(chain, X[:8], L=3), _sampler(chain, X, L=3)
    a._advance(5, False, count=True)
    b._advance(5, False, count=True)
    assert np.array_equal(a.pos.cpu().numpy(), b.pos.cpu().numpy()[:8])
    assert np.array_equal(a.lp.cpu().numpy(), b.lp.cpu().numpy()[:8])
    assert np.array_equal(a.grad.cpu().numpy(), b.grad.cpu().numpy()[:8])
    assert np.array_equal(a.naccept.cpu().numpy(), b.naccept.cpu().numpy()[:8]) and a.naccept.sum().item() > 0


def test_statistics_match_stretch_move(chain3):
    """HMCSampler (C = 256) against a long StretchSampler run on the same d = 3 chain: every mean within 5 combined Monte-Carlo
    standard errors (diagnostics() of both runs), every standard deviation within 5 standard errors from the spread of the
    per-chain values over the 256 independent chains; no trajectory escapes.  Seeds fixed."""
    from gpbayestools_hic_amd.sampler import StretchSampler
    chain, emu, xstar = chain3
    h = _sampler(chain, _near(chain, xstar, 256, 31, radius=0.03), seed=32, L=8)
    h.warmup(60)
    h.run(200)
    print("warm-up:", h.warmup_counters, "production:", h.counters(), "step size %.4g" % h.step_size, "inverse metric", h.inv_metric)
    assert h.n_escaped == 0
    st = StretchSampler(chain, 256, seed=33)
    st.run(_near(chain, xstar, 256, 34, radius=0.02), 4000)
    da, db = h.diagnostics(), st.diagnostics(discard=1000)
    zm = np.abs(da.mean - db.mean) / np.sqrt(da.mcse ** 2 + db.mcse ** 2)
    x = h._chain_dev.cpu().numpy()                                       # [nsteps, C, d]
    per_chain = np.sqrt(np.mean((x - x.reshape(-1, 3).mean(0)) ** 2, axis=0))
    se = per_chain.std(0, ddof=1) / np.sqrt(256)
    zs = np.abs(x.reshape(-1, 3).std(0) - db.std) / se
    print("HMC against the stretch move: mean z", zm, "std z", zs, "acceptance %.3f, step size %.4g, tau" % (
        h.acceptance_fraction.mean(), h.step_size), da.tau, db.tau)
    assert np.all(zm <= 5.0), zm
    assert np.all(zs <= 5.0), zs


def test_run_hmc_pickle_resume_and_shortcuts(tmp_path):
    chain, emu, xstar = _emulator(str(tmp_path), 64, 3, 8, 3)
    s = chain.run_HMC(nsteps=20, nwarmup=30, nchains=64, nleapfrog=4, nthin=2, seed=5)
    with open(chain.mcmc_path, "rb") as f:
        data = pickle.load(f)
    assert list(data) == ["chain"] and data["chain"].shape == (64, 10, 3)
    assert np.array_equal(data["chain"], chain.chain) and chain.hmc_sampler is s
    assert np.all((chain.chain > chain.min) & (chain.chain < chain.max))
    assert chain.acceptance_fraction.shape == (64,) and 0.0 <= chain.acceptance_fraction.mean() <= 1.0
    assert s.step_size > 0 and s.inv_metric.shape == (3,) and s.n_escaped >= 0 and s.n_divergent >= 0
    first = data["chain"].copy()
    s2 = chain.run_HMC(nsteps=8, nwarmup=30, nchains=64, nleapfrog=4, seed=6)
    assert chain.chain.shape == (64, 18, 3) and np.array_equal(chain.chain[:, :10], first)
    assert s2.step_size == pytest.approx(s.step_size) and np.array_equal(s2.inv_metric, s.inv_metric)
    with open(chain.mcmc_path, "rb") as f:
        assert np.array_equal(pickle.load(f)["chain"], chain.chain)
    # the stored chain is [nsteps, nchains, ndim] on the device: the analysis shortcuts read it where it lies
    assert s2.chain.shape == (64, 8, 3) and s2.lnprobability.shape == (64, 8) and s2.flatchain.shape == (512, 3)
    assert np.array_equal(s2.lnprobability[:, -1], s2.lp.cpu().numpy())
    assert np.array_equal(s2.lnprobability, chain.log_posterior(s2.flatchain).reshape(8, 64).T)
    d = s2.diagnostics()
    assert d.mean.shape == (3,) and np.all(np.isfinite(d.mean)) and np.all((d.mean > chain.min) & (d.mean < chain.max))
    m = s2.marginals(bins=8)
    assert m is not None
    with pytest.raises(ValueError, match="resuming"):
        chain.run_HMC(nsteps=4, nchains=32)


def test_refusals(tmp_path):
    from gpbayestools_hic_amd import _native as nat
    from gpbayestools_hic_amd.hmc import HMCSampler
    chain, emu, xstar = _emulator(str(tmp_path), 64, 3, 8, 3)
    for kw in (dict(nchains=0), dict(nchains=1048577), dict(nleapfrog=0), dict(nleapfrog=1025), dict(nsteps=0), dict(nwarmup=-1),
               dict(nthin=0)):
        with pytest.raises(ValueError):
            chain.run_HMC(**kw)
    for kw in (dict(jitter=1.0), dict(jitter=-0.1), dict(target_accept=0.0), dict(target_accept=1.0), dict(nleapfrog=2000)):
        with pytest.raises(ValueError):
            HMCSampler(chain, 8, **kw)
    s = HMCSampler(chain, 8, seed=1, nleapfrog=2)
    with pytest.raises(RuntimeError, match="set_state"):
        s.run(1)
    with pytest.raises(ValueError):
        s.set_state(np.zeros((7, 3)))
    s.set_state(_near(chain, xstar, 8, 1))
    before = _bits(s)
    # GPB_E_ARG of the C call itself, nothing enqueued
    engs, arr, E = chain._contexts()
    lo, hi = chain._box(s.device)

    def call(C=8, nsteps=1, step0=0, L=2, jitter=0.2, adapt=0, target=0.8, diag=None):
        return engs[0].lib.gpb_chain_hmc_run(arr, E, C, nsteps, step0, 1, L, jitter, adapt, target, nat.ptr(s.pos), nat.ptr(s.lp),
                                             nat.ptr(s.grad), nat.ptr(s.state), nat.ptr(s.minv), nat.ptr(s.msqrt), nat.ptr(lo),
                                             nat.ptr(hi), float("-inf"), chain.inside_const, None, None, 0, 0, 1, None, diag)

    dg = nat.C.byref(nat.HMCDiag())
    for kw in (dict(C=0), dict(C=1048577), dict(L=0), dict(L=1025), dict(jitter=1.0), dict(jitter=-0.5), dict(jitter=float("nan")),
               dict(step0=2 ** 32), dict(step0=2 ** 32 - 1, nsteps=2), dict(step0=2 ** 64 - 1), dict(step0=2 ** 64 - 2, nsteps=3),
               dict(nsteps=-1), dict(adapt=1, target=1.5), dict(nsteps=2, diag=dg), dict(nsteps=0, diag=dg)):
        assert call(**kw) == -1, kw
    assert call(nsteps=0) == 0
    assert all(np.array_equal(u, v) for u, v in zip(before, _bits(s)))      # (the refused calls left the state alone)
    assert call(nsteps=1, diag=dg) == 0 and call(step0=2 ** 32 - 1) == 0     # every diag output may be NULL; the last step number
    s.torch.cuda.synchronize()

    class Sharded:
        world = 2
    chain.sharding = Sharded()
    with pytest.raises(NotImplementedError, match="shard"):
        chain.run_HMC(nsteps=4, nchains=8)
    chain.sharding = None

    class Foreign:
        nobs = emu.nobs

        def predict(self, X, return_cov=True, extra_std=0.0):
            return emu.predict(X, return_cov=return_cov, extra_std=extra_std)
    chain.emuList = [Foreign()]
    with pytest.raises(NotImplementedError, match="foreign"):
        chain.run_HMC(nsteps=4, nchains=8)


def test_the_limit_of_256_parameters(tmp_path):
    """d = 256 fills the rows k_hmc_begin and k_hmc_finish keep in LDS and is accepted: steps against the restatement.  d = 257:
    HMCSampler and run_HMC raise ValueError, the C call returns GPB_E_ARG and leaves the state alone"""
    import torch
    from gpbayestools_hic_amd import _native as nat
    from gpbayestools_hic_amd.hmc import HMCSampler
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    chain = wide_chain(str(tmp_path / "a"), 256)
    s = _sampler(chain, _near(chain, wide_start(256), 8, 5, radius=0.02), L=2)
    assert s.ndim == 256
    assert _step_by_step(chain, s, 2, True) <= 1
    big = wide_chain(str(tmp_path / "b"), 257)
    assert big.ndim == 257
    with pytest.raises(ValueError, match="256 parameters"):
        HMCSampler(big, 8)
    with pytest.raises(ValueError, match="256 parameters"):
        big.run_HMC(nsteps=2, nwarmup=0, nchains=8)
    X = _near(big, wide_start(257), 8, 5, radius=0.02)
    f64 = dict(dtype=torch.float64, device="cuda:0")
    x, lpd, gd = torch.as_tensor(X, **f64), torch.full((8,), -3.0, **f64), torch.full((8, 257), 0.5, **f64)
    state, minv = torch.zeros(10, **f64), torch.full((257,), 1.0 / 12.0, **f64)
    state[0], state[3] = np.log(0.02), np.log(0.2)
    msqrt = 1.0 / torch.sqrt(minv)
    save = torch.zeros((1, 8, 257), **f64)
    keep = [t.clone() for t in (x, lpd, gd, state, save)]
    engs, arr, E = big._contexts()
    lo, hi = big._box(x.device)
    rc = engs[0].lib.gpb_chain_hmc_run(arr, E, 8, 1, 0, 1, 2, 0.2, 1, 0.8, nat.ptr(x), nat.ptr(lpd), nat.ptr(gd), nat.ptr(state),
                                       nat.ptr(minv), nat.ptr(msqrt), nat.ptr(lo), nat.ptr(hi), float("-inf"), big.inside_const,
                                       nat.ptr(save), None, 1, 0, 1, None, None)
    torch.cuda.synchronize()
    assert rc == -1
    assert all(torch.equal(u, v) for u, v in zip(keep, (x, lpd, gd, state, save)))


def test_run_hmc_reseed_switch(tmp_path, caplog):
    """reseed=False warms up without the re-seeding (other samples than the default's); a warm-up too short to separate the
    copies is not re-seeded and says so: the samples are those of reseed=False, bit for bit"""
    import logging
    import os
    chain, emu, xstar = _emulator(str(tmp_path), 64, 3, 8, 3)

    def run(**kw):
        if os.path.exists(chain.mcmc_path):
            os.remove(chain.mcmc_path)
        chain.hmc_sampler = None
        chain.run_HMC(nsteps=4, nchains=16, nleapfrog=2, seed=5, **kw)
        return chain.chain.copy()

    a, b = run(nwarmup=30), run(nwarmup=30, reseed=False)
    assert a.shape == b.shape == (16, 4, 3) and not np.array_equal(a, b)
    assert np.array_equal(run(nwarmup=30), a)
    with caplog.at_level(logging.WARNING, logger="gpbayestools_hic_amd.hmc"):
        c = run(nwarmup=18)                                   # nine steps would follow the re-seeding: ten are needed
    assert "too short to re-seed" in caplog.text
    assert np.array_equal(c, run(nwarmup=18, reseed=False))
    caplog.clear()
    with caplog.at_level(logging.WARNING, logger="gpbayestools_hic_amd.hmc"):
        run(nwarmup=19)
        run(nwarmup=0)
    assert "too short" not in caplog.text
