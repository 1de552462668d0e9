"""GPU tier of the PTLMC sampler: gpb_chain_ptlmc_run (through ptlmc.PTLMCSampler, Chain.samplerPTLMC and run_MCMC_PTLMC)
against the numpy restatement of tests/ptlmc_reference.py, fed the device's own draws."""
import functools
import os
import pickle

import numpy as np
import pytest

import ptlmc_reference as R
from sampler_cases import mapped_chain, mapped_log_posterior, wide_chain, wide_start

pytestmark = pytest.mark.gpu


def _emulator(tmp, N, d, M, P, kernel="RBF", ell=1.5, seed=0):
    """an Emulator trained at fixed hyper-parameters on synthetic data, plus a Chain over it whose experiment is the noiseless
    prediction at the truth point (5 % errors)"""
    from gpbayestools_hic_amd import synth
    from gpbayestools_hic_amd.emulator import Emulator
    from gpbayestools_hic_amd.mcmc import Chain
    os.makedirs(tmp, exist_ok=True)
    lo, hi = np.zeros(d), np.ones(d)
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


def _start(chain, xstar, T, seed, gradient, temps, radius=0.03, theta=None):
    """the start state around xstar in the unit box, or from the rows theta [T, d] given"""
    rng = np.random.default_rng(seed)
    if theta is None:
        theta = np.clip(xstar + radius * rng.standard_normal((T, chain.ndim)), 0.02, 0.98)
    if gradient:
        lp, g = chain.log_posterior(theta, return_grad=True)
        return theta, lp / temps, g / temps[:, None]
    return theta, chain.log_posterior(theta) / temps, None


def _sampler(chain, xstar, numtemps, numchain, gradient, samptunning, nsave, seed=11, maxtemp=20.0, theta=None):
    from gpbayestools_hic_amd import ptlmc
    T = numtemps + numchain
    temps = ptlmc.ladder(numtemps, numchain, maxtemp)
    theta, fval, dfval = _start(chain, xstar, T, seed, gradient, temps, theta=theta)
    covmat0, hc = ptlmc.proposal_factor(theta)
    s = ptlmc.PTLMCSampler(chain, temps, hc, covmat0, numtemps, numchain, samptunning, nsave,
                           ptlmc.TARACC_GRAD if gradient else ptlmc.TARACC_PLAIN, seed, gradient)
    s.set_state(theta, fval, dfval)
    return s, temps, hc, covmat0


def _rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))) if a.size else 0.0


def _rel_inf(a, b):
    """_rel where entries may be infinite: those are compared by equality (inf - inf must not reach _rel), the rest by _rel"""
    a, b = np.asarray(a), np.asarray(b)
    inf = np.isinf(b)
    if not np.array_equal(a[inf], b[inf]) or np.any(np.isinf(a[~inf])):
        return np.inf
    return _rel(a[~inf], b[~inf])


def _at_rows(lpf, rows):
    """lpf evaluated at the rows of `rows` wherever a row of its argument agrees with one of them to 1e-12 entry by entry
    (the bar theta itself is held to), at the argument's own row elsewhere.  The restatement's proposal and the device's
    differ in their last bits (exp, log, cos and sin of the two sides round differently), and the chain's log-posterior and
    gradient — the same device call on both sides, no part of the restated step — magnify that: an entry of the gradient
    far below its row's largest has a condition number |H| |theta| / |g| of ~1e4 with respect to theta (measured at 66 rungs:
    theta one bit apart, 1.84e-16, moved an entry of -0.0032 in a row of 0.16 by 1.5e-12 of itself).  Evaluated at the device's
    own accepted rows, value and gradient are compared at one point and the bars test the step, not that magnification."""
    def f(X):
        X = np.array(X, dtype=np.float64)
        D = np.max(np.abs(X[:, None, :] - rows[None, :, :]) / np.maximum(np.abs(X[:, None, :]), 1e-300), axis=2)
        j = np.argmin(D, axis=1)
        hit = D[np.arange(len(X)), j] <= 1e-12
        X[hit] = rows[j[hit]]
        return lpf(X)
    return f


def _step_by_step(chain, s, temps, hc, covmat0, nsteps, rel=_rel, each=None):
    """nsteps single-step calls, each checked against the restatement from the device's state before it.  rel: the comparison
    of theta / fval / dfval (_rel_inf where rungs sit outside the box); each(before, info, took): a test's own checks of a step"""
    lpf = (lambda X: chain.log_posterior(X, return_grad=True)) if s.gradient else chain.log_posterior
    temps13 = temps ** (1 / 3)
    near_ties = 0
    for _ in range(nsteps):
        before = s.state()
        k = before["k"]
        dr = R.device_draws(s.seed, k, s.T, s.d)
        acc0, swaps0 = s.naccept.cpu().numpy().copy(), s.nswap.cpu().numpy().copy()
        s.run(1)
        got = s.state()
        took = s.naccept.cpu().numpy() - acc0
        with np.errstate(invalid="ignore"):                  # (-inf - -inf of a rung outside the box)
            ref, info = R.step(before, k, dr, _at_rows(lpf, got["theta"]), temps, temps13, hc, covmat0, s.samptunning, s.taracc)
        tie = np.abs(info["delta"] - dr["logu_accept"]) < 1e-9
        assert np.array_equal(took.astype(bool)[~tie], info["accepted"][~tie]), k
        if each is not None:
            each(before, info, took)
        if np.any(tie & (took.astype(bool) != info["accepted"])):
            near_ties += 1                                   # a decision on a knife edge: compare from the next step on
            continue
        # the exchange took the same decisions at every pick (swaps per neighbour pair), so the order is the same
        assert np.array_equal(s.nswap.cpu().numpy() - swaps0, info["swaps"]), k
        assert rel(got["theta"], ref["theta"]) <= 1e-12, k
        assert rel(got["fval"], ref["fval"]) <= 1e-12, k
        if s.gradient:
            assert rel(got["dfval"], ref["dfval"]) <= 1e-12, k
        assert abs(got["tau"] - ref["tau"]) <= 1e-12 * max(abs(ref["tau"]), 1.0), k
        assert abs(got["numtimes"] - ref["numtimes"]) <= 1e-12, k
        lp = chain.log_posterior(got["theta"])
        fin = np.isfinite(lp)
        assert _rel(got["fval"][fin] * temps[fin], lp[fin]) <= 1e-14, k
        assert np.array_equal(got["fval"][~fin], lp[~fin]), k
        if k >= s.samptunning and k - s.samptunning < s.nsave:
            assert np.array_equal(s.save.cpu().numpy()[:, k - s.samptunning, :], got["theta"][s.numtemps:]), k
    return near_ties


def test_draws_match_restatement(tmp_path):
    """the debug hook's draws against the restatement: picks exact, floats within 1e-15"""
    import torch
    from gpbayestools_hic_amd import _native as nat
    from gpbayestools_hic_amd.engine import GPEngine
    with nat.debug_library():
        eng = GPEngine(0)
    for (T, d, seed, k) in [(10, 4, 7, 0), (37, 9, 2 ** 40 + 3, 123), (130, 15, 12345, 2999), (261, 127, 2 ** 35 + 9, 57)]:
        nrm = torch.empty((T, d), dtype=torch.float64, device="cuda:0")
        la = torch.empty(T, dtype=torch.float64, device="cuda:0")
        pk = torch.empty(5 * T, dtype=torch.int64, device="cuda:0")
        ls = torch.empty(5 * T, dtype=torch.float64, device="cuda:0")
        eng._ck(eng.lib.gpb_test_ptlmc_draws(eng.h, T, d, seed, k, nat.ptr(nrm), nat.ptr(la), nat.ptr(pk), nat.ptr(ls)))
        ref = R.device_draws(seed, k, T, d)
        assert np.array_equal(pk.cpu().numpy(), ref["picks"])
        assert np.all((ref["picks"] >= 1) & (ref["picks"] <= T - 1))
        assert np.max(np.abs(nrm.cpu().numpy() - ref["normals"])) <= 1e-15 * max(1.0, np.abs(ref["normals"]).max())
        assert np.max(np.abs(la.cpu().numpy() - ref["logu_accept"])) <= 1e-15 * max(1.0, np.abs(ref["logu_accept"]).max())
        assert np.max(np.abs(ls.cpu().numpy() - ref["logu_swap"])) <= 1e-15 * max(1.0, np.abs(ref["logu_swap"]).max())
    eng.close()


@pytest.mark.parametrize("gradient", [False, True])
def test_single_steps_match_restatement(tmp_path, gradient):
    """~40 single-step calls: tuning steps (k % 10 == 0), the tuning / production boundary and production steps"""
    chain, emu, xstar = _emulator(str(tmp_path), 192, 4, 8, 4)
    s, temps, hc, cov0 = _sampler(chain, xstar, 6, 4, gradient, samptunning=25, nsave=20)
    near = _step_by_step(chain, s, temps, hc, cov0, 40)
    assert near <= 2
    assert s.naccept.sum().item() > 0 and s.nswap.sum().item() > 0


@pytest.mark.parametrize("rejected", [False, True])
@pytest.mark.parametrize("gradient", [False, True])
def test_single_steps_two_emulators_one_mapped(tmp_path, gradient, rejected):
    """a chain of two emulators, the second with parameterTrafoPCA.  rejected: with the box compaction switched off
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
    s, temps, hc, cov0 = _sampler(chain, info["xstar"], 4, 4, gradient, samptunning=12, nsave=8)
    near = _step_by_step(chain, s, temps, hc, cov0, 16)
    assert near <= 2


@pytest.mark.parametrize("gradient", [False, True])
def test_one_call_equals_single_steps(tmp_path, gradient):
    chain, emu, xstar = _emulator(str(tmp_path), 192, 4, 8, 4)
    a, *_ = _sampler(chain, xstar, 6, 4, gradient, samptunning=14, nsave=16)
    b, *_ = _sampler(chain, xstar, 6, 4, gradient, samptunning=14, nsave=16)
    a.run(30)
    for _ in range(30):
        b.run(1)
    sa, sb = a.state(), b.state()
    for key in ("theta", "fval", "tau", "numtimes", "k") + (("dfval",) if gradient else ()):
        assert np.array_equal(sa[key], sb[key]), key
    for t in ("save", "naccept", "nswap"):
        assert np.array_equal(getattr(a, t).cpu().numpy(), getattr(b, t).cpu().numpy()), t


@pytest.mark.parametrize("gradient", [False, True])
def test_run_mcmc_ptlmc_end_to_end(tmp_path, gradient):
    chain, emu, xstar = _emulator(str(tmp_path), 192, 4, 8, 4)
    chain.run_MCMC_PTLMC(nsteps=40, nwalkers=4, ntemps=6, maxtemp=20, nstartparameters=200, seed=5, gradient=gradient)
    with open(chain.mcmc_path, "rb") as f:
        data = pickle.load(f)
    assert list(data) == ["chain"] and data["chain"].shape == (4, 40, 4)
    c1 = data["chain"]
    assert np.array_equal(c1, chain.chain)
    assert np.all((c1 > chain.min) & (c1 < chain.max))
    assert chain.ptlmc_sampler.gradient == gradient
    chain.run_MCMC_PTLMC(nsteps=40, nwalkers=4, ntemps=6, maxtemp=20, nstartparameters=200, seed=5, gradient=gradient)
    assert np.array_equal(chain.chain, c1)
    chain.run_MCMC_PTLMC(nsteps=40, nwalkers=4, ntemps=6, maxtemp=20, nstartparameters=200, seed=6, gradient=gradient)
    assert not np.array_equal(chain.chain, c1)


@pytest.mark.parametrize("gradient,band", [(False, (0.12, 0.40)), (True, (0.40, 0.80))])
def test_acceptance_after_tuning(tmp_path, gradient, band):
    """the tau adaptation drives the mean acceptance over the ladder towards taracc (0.25 / 0.60)"""
    chain, emu, xstar = _emulator(str(tmp_path), 192, 4, 8, 4)
    lpf = functools.partial(chain.log_posterior, return_grad=True) if gradient else chain.log_posterior
    chain.samplerPTLMC(lpf, lambda n: np.random.default_rng(3).uniform(chain.min, chain.max, (n, chain.ndim)),
                       numtemps=8, numchain=8, sampperchain=300, maxtemp=20, nstartparameters=300, seed=9)
    s = chain.ptlmc_sampler
    before = s.naccept.cpu().numpy().copy()
    s.run(200)                                               # more production steps: acceptance after tuning only
    rate = float(np.mean((s.naccept.cpu().numpy() - before) / 200.0))
    assert band[0] <= rate <= band[1], rate


def test_statistics_match_stretch_move(tmp_path):
    """d = 4: the untempered rungs' mean and standard deviation against a long device stretch-move run on the same chain"""
    chain, emu, xstar = _emulator(str(tmp_path), 192, 4, 8, 4)
    res = chain.samplerPTLMC(chain.log_posterior, lambda n: np.random.default_rng(4).uniform(chain.min, chain.max, (n, 4)),
                             numtemps=10, numchain=16, sampperchain=1500, maxtemp=20, nstartparameters=400, seed=21)
    pt = res["theta"][:, 300:, :].reshape(-1, 4)
    from gpbayestools_hic_amd.sampler import StretchSampler
    st = StretchSampler(chain, 64, seed=22)
    st.run(np.clip(xstar + 0.02 * np.random.default_rng(1).standard_normal((64, 4)), 0.01, 0.99), 3000)
    em = st.chain[:, 1000:, :].reshape(-1, 4)
    sd = em.std(0)
    dm = np.abs(pt.mean(0) - em.mean(0)) / sd
    rs = pt.std(0) / sd
    assert np.all(dm < 0.2), dm
    assert np.all((rs > 0.75) & (rs < 1.33)), rs


def test_api_branch_and_refusals(tmp_path):
    chain, emu, xstar = _emulator(str(tmp_path), 160, 4, 6, 3)
    draw = lambda n: np.random.default_rng(0).uniform(chain.min, chain.max, (n, 4))    # noqa: E731
    kw = dict(numtemps=4, numchain=4, sampperchain=5, maxtemp=10, nstartparameters=60, seed=1)
    out = chain.samplerPTLMC(functools.partial(chain.log_posterior, return_grad=True), draw, **kw)
    assert out["theta"].shape == (4, 5, 4) and chain.ptlmc_sampler.gradient
    out = chain.samplerPTLMC(functools.partial(chain.log_likelihood, finite=True), draw, **kw)
    assert not chain.ptlmc_sampler.gradient and chain.ptlmc_sampler.outside == -1e300
    with pytest.raises(TypeError, match="log_posterior"):
        chain.samplerPTLMC(lambda X: chain.log_posterior(X), draw, **kw)
    with pytest.raises(TypeError, match="log_posterior"):
        chain.samplerPTLMC(functools.partial(chain.log_posterior, finite=True), draw, **kw)
    other, *_ = _emulator(str(tmp_path / "b"), 160, 4, 6, 3)
    with pytest.raises(TypeError):
        chain.samplerPTLMC(other.log_posterior, draw, **kw)
    with pytest.raises(ValueError, match="rungs"):
        chain.samplerPTLMC(chain.log_posterior, draw, **dict(kw, numtemps=40, numchain=30, nstartparameters=60))

    class Sharded:
        world = 2
    chain.sharding = Sharded()
    with pytest.raises(NotImplementedError, match="shard"):
        chain.samplerPTLMC(chain.log_posterior, draw, **kw)
    chain.sharding = None

    class Foreign:
        nobs = emu.nobs

        def predict(self, X, return_cov=True, extra_std=0.0):
            return emu.predict(X, return_cov=return_cov, extra_std=extra_std)
    chain.emuList = [Foreign()]
    with pytest.raises(NotImplementedError, match="foreign"):
        chain.samplerPTLMC(chain.log_posterior, draw, **kw)


# ------------------------------------------------------------------ beyond one pass of the kernels' strided loops
# k_ptl_exchange draws its 5 T picks in rounds of 256 (a second round from T = 52 on) and walks the rungs 256 at a time;
# k_ptl_propose / k_ptl_accept give a parameter to each of 64 lanes (a second pass from d = 65 on).
@pytest.mark.parametrize("gradient", [False, True])
def test_default_ladder(tmp_path, gradient):
    """run_MCMC_PTLMC's default of 50 + 16 = 66 rungs: 330 picks, a full round and one of 74; a tuning step, the boundary
    and the saved samples"""
    chain, emu, xstar = _emulator(str(tmp_path), 192, 4, 8, 4)
    s, temps, hc, cov0 = _sampler(chain, xstar, 50, 16, gradient, samptunning=6, nsave=6)
    near = _step_by_step(chain, s, temps, hc, cov0, 12)
    assert near <= 2
    assert s.nswap.sum().item() > 0 and s.naccept.sum().item() > 0


def test_notebook_ladder(tmp_path):
    """100 + 30 = 130 rungs, the ladder the notebook runs: 650 picks, two full rounds and one of 138; and one call of ten
    steps against ten calls of one, bit for bit"""
    chain, emu, xstar = _emulator(str(tmp_path), 192, 4, 8, 4)
    s, temps, hc, cov0 = _sampler(chain, xstar, 100, 30, False, samptunning=4, nsave=4)
    near = _step_by_step(chain, s, temps, hc, cov0, 8)
    assert near <= 2 and s.nswap.sum().item() > 0 and s.naccept.sum().item() > 0
    a, *_ = _sampler(chain, xstar, 100, 30, False, samptunning=4, nsave=6)
    b, *_ = _sampler(chain, xstar, 100, 30, False, samptunning=4, nsave=6)
    a.run(10)
    for _ in range(10):
        b.run(1)
    sa, sb = a.state(), b.state()
    for key in ("theta", "fval", "tau", "numtimes", "k"):
        assert np.array_equal(sa[key], sb[key]), key
    for t in ("save", "naccept", "nswap"):
        assert np.array_equal(getattr(a, t).cpu().numpy(), getattr(b, t).cpu().numpy()), t


@pytest.mark.parametrize("gradient", [False, True])
def test_more_rungs_than_threads(tmp_path, gradient):
    """200 + 61 = 261 rungs: 1305 picks (five full rounds and one of 25) and a second pass of every loop over the rungs in
    the exchange's workgroup of 256"""
    chain, emu, xstar = _emulator(str(tmp_path), 192, 4, 8, 4)
    s, temps, hc, cov0 = _sampler(chain, xstar, 200, 61, gradient, samptunning=3, nsave=3)
    near = _step_by_step(chain, s, temps, hc, cov0, 6)
    assert near <= 2 and s.nswap.sum().item() > 0 and s.naccept.sum().item() > 0


def test_wide_odd_rows_plain(tmp_path):
    """127 parameters (sampler_cases.wide_chain): the lanes of k_ptl_propose and k_ptl_accept make a second pass, and the last
    normal of a row is half a pair"""
    chain = wide_chain(str(tmp_path), 127)
    s, temps, hc, cov0 = _sampler(chain, wide_start(127), 6, 4, False, samptunning=3, nsave=3)
    assert s.d == 127
    near = _step_by_step(chain, s, temps, hc, cov0, 6)
    assert near <= 2 and s.naccept.sum().item() > 0


def test_wide_odd_rows_gradient(tmp_path):
    """a real parameterTrafoPCA emulator over 71 parameters (64 GP inputs): first the chain's gradient against autograd of
    the torch restatement on eight rows at the bar of tests/test_gpu_gradient.py, then six steps of the gradient branch"""
    from test_gpu_gradient import BAR, _rowerr
    import grad_reference as G
    chain, emu, mid = mapped_chain(tmp_path, 71)
    assert chain.ndim == 71 and emu.PCA_new_design_points.shape[1] == 64
    width = chain.max - chain.min
    rng = np.random.default_rng(17)
    X = mid + 0.02 * width * rng.standard_normal((8, 71))
    lp, g = chain.log_posterior(X, return_grad=True)
    assert np.array_equal(lp, chain.log_posterior(X)) and np.all(np.isfinite(lp))
    v, gref = G.value_and_grad(mapped_log_posterior(chain, emu), X)
    print("gradient over 71 mapped parameters: worst row %.3g of the bar" % (float(np.max(_rowerr(g, gref))) / BAR))
    assert np.all(_rowerr(g, gref) <= BAR), _rowerr(g, gref)
    theta = mid + 0.01 * width * rng.standard_normal((8, 71))
    s, temps, hc, cov0 = _sampler(chain, mid, 4, 4, True, samptunning=3, nsave=3, theta=theta)
    assert s.d == 71
    near = _step_by_step(chain, s, temps, hc, cov0, 6)
    assert near <= 2 and s.naccept.sum().item() > 0


def test_rungs_outside_the_box(tmp_path):
    """two adjacent tempered rungs and one untempered rung start outside the box (fval = -inf): a proposal that lands outside
    is rejected (-inf - -inf is NaN, and NaN is not above log u), the swap test between two such rungs is NaN and does not
    swap, and every step still agrees with the restatement"""
    from gpbayestools_hic_amd import ptlmc
    chain, emu, xstar = _emulator(str(tmp_path), 192, 4, 8, 4)
    temps = ptlmc.ladder(6, 4, 20.0)
    theta, _, _ = _start(chain, xstar, 10, 11, False, temps)
    covmat0, hc = ptlmc.proposal_factor(theta)               # the proposal scale of the rows inside: steps of a few 0.01
    theta[2, 0], theta[3, 1], theta[7, 2] = 1.2, -0.004, 1.2
    fval = chain.log_posterior(theta) / temps
    assert np.array_equal(np.flatnonzero(np.isinf(fval)), [2, 3, 7]) and np.all(fval[[2, 3, 7]] < 0)
    s = ptlmc.PTLMCSampler(chain, temps, hc, covmat0, 6, 4, 3, 5, ptlmc.TARACC_PLAIN, 11, False)
    s.set_state(theta, fval)
    seen = dict(both=0)

    def each(before, info, took):
        out = ~np.all((info["thetap"] > chain.min) & (info["thetap"] < chain.max), axis=1)
        assert np.array_equal(np.isinf(info["lp"]), out)
        assert not np.any(took[out])                         # from inside or from outside: never accepted
        was_out = np.isinf(before["fval"])
        seen["both"] += int(np.sum(out & was_out))
        assert np.all(took[~out & was_out] == 1)             # finite - -inf = +inf: back inside is always accepted

    near = _step_by_step(chain, s, temps, hc, covmat0, 8, rel=_rel_inf, each=each)
    assert near <= 2
    assert seen["both"] >= 8, seen                           # the rungs 0.2 outside never come back within eight small steps
