"""
Device-resident parallel-tempered Langevin sampler: the reference's `Chain.samplerPTLMC` (surmise 0.2.1's PTLMC,
src/mcmc.py:431-676) and `run_MCMC_PTLMC` (src/mcmc.py:696-726) on this package's engine.

The pre-optimizer runs batched: the start rows are evaluated in one device batch, all T = numtemps + numchain L-BFGS-B
searches run in lock-step (emulator._batched_lbfgsb: one device evaluation of value and gradient per round for every search
still running), and the "move off the optimum" loop evaluates the candidates of every chain not yet moved in one batch per
round.  The step loop then runs in C (gpb_chain_ptlmc_run, csrc/gpb_ptlmc.hip): proposal, chain evaluation, accept test and
temperature exchange enqueued back to back, the ladder's state resident in HBM, the host involved only at the boundary
between the tuning and the production phase.

Deliberate deviations from the reference:
- random numbers: numpy's global generator is replaced by np.random.default_rng(seed) on the host (start rows through the
  caller's draw_func, the pre-optimizer's sort noise and moves) and by counter-based Philox streams keyed by the same seed
  on the device (proposals, accept tests, exchanges), so that a run is reproducible and the step loop needs no host draws;
- the pre-optimizer uses the device gradient in both branches (the reference lets scipy take finite differences when
  logpostfunc returns no gradient), and its moves draw their normals round by round for all chains still to move;
- in the gradient branch lp is treated as a column [T, 1], which is what the algorithm needs and what the reference's
  code does not do with a (lp[m], grad[m, p]) return (its `lp / temps` broadcasts to [T, T]);
- no log line every 100 steps: the loop does not come back to the host between the phase boundaries.
"""
import functools
import logging

import numpy as np

from . import _native as nat

log = logging.getLogger(__name__)

FRACTUNNING = 2.0               # tuning steps per production step (src/mcmc.py:486)
TARACC_GRAD, TARACC_PLAIN = 0.60, 0.25


def ladder(numtemps, numchain, maxtemp):
    """temps [T]: numtemps temperatures from maxtemp down, then numchain ones (src/mcmc.py:492-497)"""
    return np.concatenate((np.exp(np.linspace(np.log(maxtemp), np.log(maxtemp) / (numtemps + 1), numtemps)),
                           np.ones(numchain)))


def proposal_factor(thetac):
    """(covmat0, hc) from the start state [T, d] exactly as src/mcmc.py:604-615 forms them (np.cov receives it once)"""
    covmat0 = np.cov(thetac.T)
    if thetac.shape[1] > 1:
        covmat0 = 0.9 * covmat0 + 0.1 * np.diag(np.diag(covmat0))
        W, V = np.linalg.eigh(covmat0)
        hc = V @ np.diag(np.sqrt(W)) @ V.T
    else:
        hc = np.sqrt(covmat0).reshape(1, 1)
        covmat0 = covmat0.reshape(1, 1)
    return covmat0, hc


_ACCEPTED = ("chain.log_posterior, chain.log_likelihood, or a functools.partial of either that sets return_grad "
             "(and, for log_likelihood, finite) of the same chain")


def target_of(chain, logpostfunc):
    """the value a rung outside the prior box takes under `logpostfunc`, which must be one of this chain's log-probability
    methods (the device loop evaluates the chain itself, it cannot call back into an arbitrary function)"""
    f, kw = logpostfunc, {}
    if isinstance(f, functools.partial):
        if f.args:
            raise TypeError("samplerPTLMC: logpostfunc must be " + _ACCEPTED + "; got a partial with positional arguments")
        kw = dict(f.keywords)
        f = f.func
    if f == chain.log_posterior:
        allowed, outside = {"return_grad"}, -np.inf
    elif f == chain.log_likelihood:
        allowed = {"return_grad", "finite"}
        outside = -1e300 if kw.get("finite", False) else -np.inf
    else:
        raise TypeError("samplerPTLMC: logpostfunc must be " + _ACCEPTED + "; got %r" % (logpostfunc,))
    if set(kw) - allowed:
        raise TypeError("samplerPTLMC: logpostfunc must be " + _ACCEPTED + "; got keywords %s" % sorted(set(kw) - allowed))
    return outside


def _philox_seed(seed):
    if seed is None:
        return int(np.random.SeedSequence().generate_state(1, dtype=np.uint64)[0])
    return int(seed) & 0xFFFFFFFFFFFFFFFF


class PTLMCSampler:
    """The step loop's state in HBM and the calls of gpb_chain_ptlmc_run.  theta [T, d], fval [T] = lp / temps, dfval
    [T, d] = grad / temps (gradient branch only), tune = (tau, numtimes); `k` is the global step number (the tuning phase
    is k < samptunning, the tau update happens at its steps with k % 10 == 0, production steps save the numchain untempered
    rungs at k - samptunning)."""

    def __init__(self, chain, temps, hc, covmat0, numtemps, numchain, samptunning, nsave, taracc, seed, gradient,
                 outside=-np.inf):
        import torch
        self.torch = torch
        self.chain = chain
        self.dev = torch.device("cuda", chain.device)
        self.T, self.numtemps, self.numchain = int(numtemps) + int(numchain), int(numtemps), int(numchain)
        self.d = int(chain.ndim)
        self.samptunning, self.nsave, self.taracc = int(samptunning), int(nsave), float(taracc)
        self.seed, self.gradient, self.outside = _philox_seed(seed), bool(gradient), float(outside)
        f64 = dict(dtype=torch.float64, device=self.dev)
        temps = np.asarray(temps, dtype=np.float64)
        self.temps = torch.as_tensor(temps, **f64)
        self.temps13 = torch.as_tensor(temps ** (1 / 3), **f64)        # what the reference multiplies rho by
        self.hc = torch.as_tensor(np.ascontiguousarray(hc, dtype=np.float64), **f64)
        self.covmat0 = torch.as_tensor(np.ascontiguousarray(covmat0, dtype=np.float64), **f64)
        self.theta = torch.zeros((self.T, self.d), **f64)
        self.fval = torch.zeros(self.T, **f64)
        self.dfval = torch.zeros((self.T, self.d), **f64) if self.gradient else None
        self.tune = torch.tensor([-1.0, 0.0], **f64)
        self.save = torch.zeros((self.numchain, max(self.nsave, 1), self.d), **f64)
        self.naccept = torch.zeros(self.T, dtype=torch.int64, device=self.dev)
        self.nswap = torch.zeros(self.T - 1, dtype=torch.int64, device=self.dev)
        self.k = 0

    def set_state(self, theta, fval, dfval=None, tau=-1.0, numtimes=0.0, k=0):
        t = self.torch
        self.theta.copy_(t.as_tensor(np.ascontiguousarray(theta, dtype=np.float64)))
        self.fval.copy_(t.as_tensor(np.ascontiguousarray(np.reshape(fval, -1), dtype=np.float64)))
        if self.gradient:
            self.dfval.copy_(t.as_tensor(np.ascontiguousarray(dfval, dtype=np.float64)))
        self.tune.copy_(t.tensor([float(tau), float(numtimes)], dtype=t.float64))
        self.k = int(k)

    def state(self):
        """the resident state on the host: theta, fval, dfval (or None), tau, numtimes, k"""
        tune = self.tune.cpu().numpy()
        return dict(theta=self.theta.cpu().numpy(), fval=self.fval.cpu().numpy(),
                    dfval=None if self.dfval is None else self.dfval.cpu().numpy(), tau=float(tune[0]),
                    numtimes=float(tune[1]), k=self.k)

    def run(self, nsteps):
        """enqueue `nsteps` steps from step self.k (asynchronous: nothing waits for the device)"""
        nsteps = int(nsteps)
        if nsteps <= 0:
            return
        engs, arr, E = self.chain._contexts()
        e0 = engs[0]
        lo, hi = self.chain._box(self.dev)
        e0._ck(e0.lib.gpb_chain_ptlmc_run(
            arr, E, self.numtemps, self.numchain, nsteps, self.k, self.seed, self.samptunning, self.taracc,
            nat.ptr(self.theta), nat.ptr(self.fval), nat.ptr(self.dfval), nat.ptr(self.tune), nat.ptr(self.temps),
            nat.ptr(self.temps13), nat.ptr(self.hc), nat.ptr(self.covmat0), nat.ptr(lo), nat.ptr(hi), self.outside,
            self.chain.inside_const, nat.ptr(self.save) if self.nsave > 0 else None, self.nsave, nat.ptr(self.naccept),
            nat.ptr(self.nswap)))
        self.k += nsteps

    def acceptance_fraction(self):
        """accepted proposals per rung over the steps run so far"""
        return self.naccept.cpu().numpy() / max(self.k, 1)


def _preoptimize(chain, theta0, T, outside, rng):
    """src/mcmc.py:529-592 batched: the T best start rows (by lp plus the reference's noise), one lock-step L-BFGS-B search
    per rung on the rescaled objective, then the moves off each optimum (all rungs but the first), round by round"""
    from .emulator import _batched_lbfgsb
    d = theta0.shape[1]
    lp0 = chain._log_prob(theta0, outside)
    ord1 = np.argsort(-lp0 + (d * rng.standard_normal(size=theta0.shape[0]) ** 2))
    theta0 = theta0[ord1[0:T], :]
    thetacen = np.mean(theta0, 0)
    thetas = np.maximum(np.std(theta0, 0), 10 ** (-8) * np.std(theta0))
    boundL = np.maximum(-10 * np.ones(d), np.min((theta0 - thetacen) / thetas, 0))
    boundU = np.minimum(10 * np.ones(d), np.max((theta0 - thetacen) / thetas, 0))

    class _Scaled:                 # _batched_lbfgsb maximises .lml: the log-posterior of the rescaled rows
        @staticmethod
        def lml(x, eval_gradient=True):
            lp, g = chain._log_prob_grad(thetacen + thetas * x, outside)
            return lp, thetas * g

    x, _, hinv = _batched_lbfgsb(_Scaled, (theta0 - thetacen) / thetas, np.stack([boundL, boundU], axis=1),
                                 return_hess_inv=True)
    thetaop = thetacen + thetas * x
    l0 = -chain._log_prob(thetacen + thetas * x, outside)
    eig = [np.linalg.eigh(h @ np.eye(d)) for h in hinv]
    notmoved = np.ones(T, dtype=bool)
    notmoved[0] = False
    stepadj = np.full(T, 4.0)
    while notmoved.any():
        ids = np.flatnonzero(notmoved)
        with np.errstate(invalid="ignore"):
            r = np.stack([(eig[k][1].T * np.sqrt(eig[k][0])) @ (eig[k][1] @ rng.standard_normal(size=d)) for k in ids])
        cand = stepadj[ids, None] * r + x[ids]
        lc = -chain._log_prob(thetacen + thetas * cand, outside)
        with np.errstate(invalid="ignore"):
            ok = (lc - l0[ids]) < 3 * d
        thetaop[ids[ok]] = thetacen + thetas * cand[ok]
        notmoved[ids[ok]] = False
        bad = ids[~ok]
        stepadj[bad] /= 2
        done = bad[stepadj[bad] < 1 / 16]
        thetaop[done] = thetacen + thetas * x[done]
        notmoved[done] = False
    return thetaop


def sampler_ptlmc(chain, logpostfunc, draw_func, theta0=None, numtemps=32, numchain=16, sampperchain=400, maxtemp=30,
                  nstartparameters=1000, seed=None):
    """Chain.samplerPTLMC (see there)"""
    outside = target_of(chain, logpostfunc)
    if not chain._native():
        raise NotImplementedError("samplerPTLMC needs every emulator of the chain to be this package's Emulator (foreign "
                                  "emulators have no device derivatives and no device step loop)")
    sh = getattr(chain, "sharding", None)
    if sh is not None and getattr(sh, "world", 1) > 1:
        raise NotImplementedError("samplerPTLMC does not shard: a ladder of ~100 rungs gains nothing from several GPUs "
                                  "(chain.shard_over(None) first)")
    rng = np.random.default_rng(seed)
    if theta0 is None:
        theta0 = draw_func(nstartparameters)
    theta0 = np.array(theta0, ndmin=2, dtype=np.float64)
    if theta0.shape[0] < 10 * theta0.shape[1]:
        theta0 = np.array(draw_func(nstartparameters), ndmin=2, dtype=np.float64)
    samptunning = int(np.ceil(sampperchain * FRACTUNNING))
    T = int(numtemps) + int(numchain)
    if theta0.shape[0] < T:
        raise ValueError("samplerPTLMC: %d start rows for %d rungs (numtemps + numchain); nstartparameters must be at least "
                         "that" % (theta0.shape[0], T))
    temps = ladder(numtemps, numchain, maxtemp)
    gradient = isinstance(logpostfunc(theta0[0:2, :]), tuple)      # the reference's test of the branch (src/mcmc.py:501)
    taracc = TARACC_GRAD if gradient else TARACC_PLAIN
    log.info("Begin PTLMC pre-optimization ...")
    thetac = _preoptimize(chain, theta0, T, outside, rng)
    log.info("Initialize PTLMC starting point ...")
    if gradient:
        lp, g = chain._log_prob_grad(thetac, outside)
        fval, dfval = lp / temps, g / temps[:, None]
    else:
        fval, dfval = chain._log_prob(thetac, outside) / temps, None
    covmat0, hc = proposal_factor(thetac)
    sampler = PTLMCSampler(chain, temps, hc, covmat0, numtemps, numchain, samptunning, sampperchain, taracc, seed,
                           gradient, outside)
    sampler.set_state(thetac, fval, dfval)
    log.info("Run over all PTLMC chains and tune (%d steps) ...", samptunning)
    sampler.run(samptunning)
    log.info("PTLMC tuning done (tau %.4g); %d production steps ...", sampler.state()["tau"], sampperchain)
    sampler.run(sampperchain)
    theta = sampler.save.cpu().numpy()[:, :sampperchain, :]
    chain.ptlmc_sampler = sampler
    log.info("PTLMC done: acceptance %.3f at T = 1", float(np.mean(sampler.acceptance_fraction()[numtemps:])))
    return {"theta": theta}
