"""
Device-resident Hamiltonian Monte Carlo over many independent chains (`DESIGN.md` §30): HMCSampler drives
gpb_chain_hmc_run (csrc/gpb_hmc.hip), Chain.run_HMC wraps it with run_mcmc's pickle conventions.

Every chain runs plain HMC — a diagonal metric, `nleapfrog` leapfrog steps per trajectory, a jittered step size shared by all
chains, the hard prior box as reflecting walls — and the C chains advance in lock-step: one gpb_chain_logpost_grad of C rows
per leapfrog, nothing synchronises with the host inside a call.  The warm-up adapts the step size by dual averaging on the
mean accept probability of all chains (almost noise-free at a thousand chains, so tens of steps do) and the metric from the
variance over the chains and a window's stored steps.

The stored chain is [nsteps, nchains, ndim] in HBM, the layout every analysis call of the package reads: the accessors and
shortcuts are those of sampler.StretchSampler (sampler.StoredChainAccessors).

This is not NUTS: the trajectory length is fixed.  There is no dense metric and no sharding over several GPUs.
"""
import logging

import numpy as np

from . import _native as nat
from .sampler import StoredChainAccessors

log = logging.getLogger(__name__)

MAX_CHAINS, MAX_NDIM, MAX_LEAPFROG = 1048576, 256, 1024
STATE_SLOTS = 10                 # gpb_chain_hmc_run's state block: 5 doubles, 4 counters, one slot of the loop's own
ST_LN_EPS, ST_LN_EPS_BAR, ST_HBAR, ST_MU, ST_COUNT, ST_ACCEPTED, ST_DIVERGENT, ST_ESCAPED, ST_NAN = range(9)
SHRINK = 5.0                     # Stan's weight of the value shrunk towards, in samples


def _philox_seed(seed):
    if seed is None:
        return int(np.random.SeedSequence().generate_state(1, dtype=np.uint64)[0])
    return int(seed) & 0xFFFFFFFFFFFFFFFF


def check_arguments(nchains, ndim, nleapfrog, jitter, target_accept):
    """ValueError for what gpb_chain_hmc_run would refuse"""
    if not 1 <= int(nchains) <= MAX_CHAINS:
        raise ValueError("HMC: nchains must be 1 .. %d, got %r" % (MAX_CHAINS, nchains))
    if not 1 <= int(ndim) <= MAX_NDIM:
        raise ValueError("HMC: 1 .. %d parameters, the chain has %r" % (MAX_NDIM, ndim))
    if not 1 <= int(nleapfrog) <= MAX_LEAPFROG:
        raise ValueError("HMC: nleapfrog must be 1 .. %d, got %r" % (MAX_LEAPFROG, nleapfrog))
    if not 0.0 <= float(jitter) < 1.0:
        raise ValueError("HMC: 0 <= jitter < 1, got %r" % (jitter,))
    if not 0.0 < float(target_accept) < 1.0:
        raise ValueError("HMC: 0 < target_accept < 1, got %r" % (target_accept,))


def check_chain(chain, who):
    """the gradient path's policy: NotImplementedError for foreign emulators and for a sharded chain"""
    if not chain._native():
        raise NotImplementedError(who + " needs every emulator of the chain to be this package's Emulator (foreign emulators "
                                  "have no device derivatives and no device step loop)")
    sh = getattr(chain, "sharding", None)
    if sh is not None and getattr(sh, "world", 1) > 1:
        raise NotImplementedError(who + " does not shard over several GPUs (chain.shard_over(None) first)")


def window_lengths(nsteps, windows):
    """the warm-up's windows: lengths in the proportions 1 : 2 : 4 : ... with the last as long as the one before it (the metric
    changes at the end of every window but the last, which adapts the step size to the final metric)"""
    nsteps, windows = int(nsteps), int(windows)
    w = np.array([2.0 ** i for i in range(windows - 1)] + [2.0 ** max(windows - 2, 0)])
    edges = np.round(np.cumsum(w) / w.sum() * nsteps).astype(int)
    return [int(n) for n in np.diff(np.concatenate(([0], edges)))]


RESEED_KEEP = 8                  # the warm start keeps the best chain in RESEED_KEEP and restarts the others at copies of them


def reseed_rows(X, lp, keep=RESEED_KEEP):
    """The rows a warm start goes on from: the ceil(C / keep) rows of X [C, d] with the highest lp (ties and NaN last, by row
    number), repeated in turn until there are C again.  Independent chains started at prior draws do not all find the
    posterior's main mode — some settle in local maxima of the emulators far from the data, and independent chains, unlike
    the walkers of an ensemble, never pull each other out.  run_mcmc re-seeds its walkers at the most likely points of the
    first half of its burn-in for the same reason (src/mcmc.py:392-402).  Copies separate at their first step: every chain
    draws its own momenta."""
    X, lp = np.asarray(X, dtype=np.float64), np.asarray(lp, dtype=np.float64)
    C = X.shape[0]
    n = max(1, -(-C // int(keep)))
    order = np.argsort(-np.where(np.isnan(lp), -np.inf, lp), kind="stable")[:n]
    return X[order[np.arange(C) % n]]


RESEED_MIN_STEPS = 10            # warm-up steps that must follow a re-seeding: several autocorrelation times, so that copies separate


def warm_start(sampler, X0, nwarmup, reseed=True):
    """start at X0 and warm up for nwarmup steps; reseed: warm up for half of them, re-seed (reseed_rows), warm up for the
    rest.  A warm-up that leaves fewer than RESEED_MIN_STEPS steps behind the re-seeding is not re-seeded (a warning says so):
    production would begin from rows that are still copies of each other."""
    sampler.set_state(X0)
    nwarmup = int(nwarmup)
    n0 = nwarmup // 2
    if reseed and nwarmup - n0 < RESEED_MIN_STEPS:
        if nwarmup > 0:
            log.warning("HMC: a warm-up of %d steps is too short to re-seed the chains half way (%d steps must follow): "
                        "warming up without re-seeding", nwarmup, RESEED_MIN_STEPS)
        reseed = False
    if not reseed:
        sampler.warmup(nwarmup)
        return
    sampler.warmup(n0)
    first = sampler.warmup_counters
    sampler.set_state(reseed_rows(sampler.pos.cpu().numpy(), sampler.lp.cpu().numpy()))
    sampler.warmup(nwarmup - n0)
    sampler.warmup_counters = {k: v + first[k] for k, v in sampler.warmup_counters.items()}


class HMCSampler(StoredChainAccessors):
    """The chains' state in HBM — x [C, d], lp [C], grad [C, d], the adaptation state — and the calls of gpb_chain_hmc_run.
    `k` is the global step number, the key of the counter-based draws together with the seed and the chain's number.
    The documented start: inverse masses width^2 / 12 (the variance of the uniform prior) and step size 0.1 d^(-1/4)."""

    def __init__(self, chain, nchains, seed=None, nleapfrog=8, jitter=0.2, target_accept=0.8):
        import torch
        check_chain(chain, "HMCSampler")
        check_arguments(nchains, chain.ndim, nleapfrog, jitter, target_accept)
        self.torch = torch
        self.chain_obj = chain
        self.ndim = int(chain.ndim)
        self.nchains = self.nwalkers = int(nchains)
        self.nleapfrog, self.jitter, self.target_accept = int(nleapfrog), float(jitter), float(target_accept)
        self.seed = _philox_seed(seed)
        self.device = torch.device("cuda", chain.device)
        f64 = dict(dtype=torch.float64, device=self.device)
        C, d = self.nchains, self.ndim
        self.pos = torch.zeros((C, d), **f64)
        self.lp = torch.zeros(C, **f64)
        self.grad = torch.zeros((C, d), **f64)
        self.state = torch.zeros(STATE_SLOTS, **f64)
        self.naccept = torch.zeros(C, dtype=torch.int64, device=self.device)
        self.minv = torch.empty(d, **f64)
        self.msqrt = torch.empty(d, **f64)
        self.k = 0
        self._have_state = False
        self.warmup_counters = dict(accepted=0, divergent=0, escaped=0, nan_rows=0)
        self.set_metric((np.asarray(chain.max, dtype=np.float64) - np.asarray(chain.min, dtype=np.float64)) ** 2 / 12.0)
        self.set_step_size(0.1 * d ** -0.25)
        self.reset()

    # ------------------------------------------------------------------ state
    def reset(self):
        """drop the stored chain and the acceptance counts (the chains' state, the step size and the metric stay)"""
        self._chain_dev = None
        self._lp_dev = None
        self.iterations = 0
        self.naccept.zero_()

    def set_metric(self, inv_metric):
        """the diagonal inverse mass matrix [ndim]; the host computes 1 / sqrt of it for the momenta"""
        m = np.ascontiguousarray(inv_metric, dtype=np.float64).reshape(-1)
        if m.shape[0] != self.ndim or not np.all(np.isfinite(m)) or not np.all(m > 0.0):
            raise ValueError("HMC: the inverse metric must hold %d positive finite entries" % self.ndim)
        self.minv.copy_(self.torch.as_tensor(m))
        self.msqrt.copy_(self.torch.as_tensor(1.0 / np.sqrt(m)))

    def set_step_size(self, eps):
        """set the step size and restart the dual averaging around it (mu = ln 10 eps, Hoffman & Gelman 2014)"""
        eps = float(eps)
        if not (np.isfinite(eps) and eps > 0.0):
            raise ValueError("HMC: the step size must be positive and finite, got %r" % (eps,))
        self.state[:ST_COUNT + 1].copy_(self.torch.tensor([np.log(eps), 0.0, 0.0, np.log(10.0 * eps), 0.0],
                                                          dtype=self.torch.float64))

    def set_state(self, X):
        """start the chains at the rows of X [nchains, ndim]: their log-posterior and gradient are evaluated on the device"""
        X = np.ascontiguousarray(X, dtype=np.float64)
        if X.shape != (self.nchains, self.ndim):
            raise ValueError("HMC: the start must be [%d, %d], got %s" % (self.nchains, self.ndim, X.shape))
        self.pos.copy_(self.torch.as_tensor(X))
        engs, arr, E = self.chain_obj._contexts()
        e0 = engs[0]
        lo, hi = self.chain_obj._box(self.device)
        e0._ck(e0.lib.gpb_chain_logpost_grad(arr, E, nat.ptr(self.pos), self.nchains, nat.ptr(self.lp), nat.ptr(self.grad),
                                             nat.ptr(lo), nat.ptr(hi), float("-inf"), self.chain_obj.inside_const))
        if self.torch.isnan(self.lp).any().item():
            raise ValueError("The initial log_prob was NaN")
        self._have_state = True

    def counters(self):
        """accepted, divergent and escaped trajectories and NaN rows since the sampler was made or, as Stan reports its
        divergences, since the last warm-up ended: warmup() keeps its own in `warmup_counters` (synchronises)"""
        c = self.state.view(self.torch.int64)[ST_ACCEPTED:ST_NAN + 1].cpu().numpy()
        return dict(accepted=int(c[0]), divergent=int(c[1]), escaped=int(c[2]), nan_rows=int(c[3]))

    @property
    def step_size(self):
        return float(np.exp(self.state[ST_LN_EPS].item()))

    @property
    def inv_metric(self):
        return self.minv.cpu().numpy()

    @property
    def n_divergent(self):
        return self.counters()["divergent"]

    @property
    def n_escaped(self):
        return self.counters()["escaped"]

    # ------------------------------------------------------------------ the C call
    def _advance(self, nsteps, adapt, save=None, lpsave=None, thin=1, count=False, diag=None):
        """enqueue nsteps steps from step self.k (asynchronous); save [nsave, C, d] / lpsave [nsave, C] take every thin-th"""
        if not self._have_state:
            raise RuntimeError("HMC: no start: call set_state(X) first")
        engs, arr, E = self.chain_obj._contexts()
        e0 = engs[0]
        lo, hi = self.chain_obj._box(self.device)
        e0._ck(e0.lib.gpb_chain_hmc_run(
            arr, E, self.nchains, int(nsteps), self.k, self.seed, self.nleapfrog, self.jitter, 1 if adapt else 0,
            self.target_accept, nat.ptr(self.pos), nat.ptr(self.lp), nat.ptr(self.grad), nat.ptr(self.state), nat.ptr(self.minv),
            nat.ptr(self.msqrt), nat.ptr(lo), nat.ptr(hi), float("-inf"), self.chain_obj.inside_const, nat.ptr(save),
            nat.ptr(lpsave), 0 if save is None else save.shape[0], self.k, int(thin), nat.ptr(self.naccept) if count else None,
            None if diag is None else nat.C.byref(diag)))
        self.k += int(nsteps)

    def step_with_diagnostics(self, adapt=False):
        """one step whose draws and trajectory come back: dict of p0 [C, d], logu [C], dH [C], a [C], traj [L, C, d] and eps —
        what a restatement of the step needs to follow the device (tests/hmc_reference.py).  The step counts towards
        acceptance_fraction; it is not stored."""
        t = self.torch
        f64 = dict(dtype=t.float64, device=self.device)
        C, d, L = self.nchains, self.ndim, self.nleapfrog
        out = dict(p0=t.empty((C, d), **f64), logu=t.empty(C, **f64), dH=t.empty(C, **f64), a=t.empty(C, **f64),
                   traj=t.empty((L, C, d), **f64), eps=t.empty(1, **f64))
        dg = nat.HMCDiag(*(nat.ptr(out[n]) for n in ("p0", "logu", "dH", "a", "traj", "eps")))
        self._advance(1, adapt, count=True, diag=dg)
        self.iterations += 1
        res = {n: v.cpu().numpy() for n, v in out.items()}
        res["eps"] = float(res["eps"][0])
        return res

    # ------------------------------------------------------------------ warm-up and production
    def warmup(self, nsteps, windows=3):
        """The resident adaptation, window by window (window_lengths): inside a window every step ends with a dual-averaging
        update of the step size towards target_accept.  At a window's end the step size becomes the averaged one, eps-bar; at
        the end of every window but the last the inverse masses become the variance over the chains and the second half of
        the window's stored steps, shrunk towards the current value with Stan's weight (n var + 5 current) / (n + 5), n the
        number of chains; the averaging restarts around the new step size.  The trajectory counters restart when the warm-up
        ends (`warmup_counters` keeps the warm-up's), so that n_divergent and n_escaped speak of the production steps."""
        t = self.torch
        nsteps, windows = int(nsteps), int(windows)
        if nsteps < 0 or windows < 1:
            raise ValueError("HMC: warmup(nsteps >= 0, windows >= 1)")
        lengths = window_lengths(nsteps, windows)
        for i, n in enumerate(lengths):
            if n == 0:
                continue
            last = i == len(lengths) - 1
            store = None if last else t.empty((n, self.nchains, self.ndim), dtype=t.float64, device=self.device)
            self._advance(n, True, save=store)
            if store is not None and self.nchains > 1:
                var = store[n // 2:].reshape(-1, self.ndim).var(dim=0, unbiased=True)
                nc = float(self.nchains)
                new = (nc * var + SHRINK * self.minv) / (nc + SHRINK)
                ok = t.isfinite(new) & (new > 0.0)
                self.minv.copy_(t.where(ok, new, self.minv))
                self.msqrt.copy_(1.0 / t.sqrt(self.minv))
            eps_bar = float(np.exp(self.state[ST_LN_EPS_BAR].item()))
            self.set_step_size(eps_bar)
            log.info("HMC warm-up window %d of %d (%d steps): step size %.4g", i + 1, len(lengths), n, eps_bar)
        # the dual averaging explores step sizes up to ten times the start's in its first steps: what escapes or diverges
        # there is rejected, and is the warm-up's own business
        self.warmup_counters = self.counters()
        self.state[ST_ACCEPTED:ST_NAN + 1].zero_()

    def run(self, nsteps, thin=1):
        """`nsteps` production steps (no adaptation), every thin-th stored; returns the final positions (numpy)"""
        t = self.torch
        nsteps, thin = int(nsteps), int(thin)
        if nsteps < 0 or thin < 1:
            raise ValueError("HMC: run(nsteps >= 0, thin >= 1)")
        if nsteps > 0:
            nsave = (nsteps + thin - 1) // thin
            cd = t.empty((nsave, self.nchains, self.ndim), dtype=t.float64, device=self.device)
            ld = t.empty((nsave, self.nchains), dtype=t.float64, device=self.device)
            self._advance(nsteps, False, save=cd, lpsave=ld, thin=thin, count=True)
            self.iterations += nsteps
            self._chain_dev = cd if self._chain_dev is None else t.cat([self._chain_dev, cd], 0)
            self._lp_dev = ld if self._lp_dev is None else t.cat([self._lp_dev, ld], 0)
        return self.pos.cpu().numpy()


def run_hmc(chain, nsteps=500, nwarmup=200, nchains=1024, nleapfrog=8, nthin=1, seed=None, reseed=True):
    """Chain.run_HMC (see there)"""
    import pickle
    check_chain(chain, "run_HMC")
    check_arguments(nchains, chain.ndim, nleapfrog, 0.2, 0.8)
    nsteps, nwarmup, nchains, nthin = int(nsteps), int(nwarmup), int(nchains), int(nthin)
    if nsteps < 1 or nwarmup < 0 or nthin < 1:
        raise ValueError("run_HMC: nsteps >= 1, nwarmup >= 0 and nthin >= 1")
    chain_data = {}
    try:
        with open(chain.mcmc_path, "rb") as f:
            chain_data = pickle.load(f)
    except FileNotFoundError:
        pass
    resume = "chain" in chain_data
    if resume and chain_data["chain"].shape[0::2] != (nchains, chain.ndim):
        raise ValueError("run_HMC: %s holds a chain of shape %s; resuming needs nchains = %d"
                         % (chain.mcmc_path, chain_data["chain"].shape, chain_data["chain"].shape[0]))
    prev = getattr(chain, "hmc_sampler", None)
    sampler = HMCSampler(chain, nchains, seed=seed, nleapfrog=nleapfrog)
    if resume:
        sampler.set_state(chain_data["chain"][:, -1, :])
        sampler.k = nwarmup + chain_data["chain"].shape[1] * nthin      # (step numbers key the draws: not those of the first run)
        if prev is not None and prev.ndim == sampler.ndim and prev.nleapfrog == sampler.nleapfrog:
            sampler.set_metric(prev.inv_metric)          # the adaptation of the run that is resumed, where it is still at hand
            sampler.set_step_size(prev.step_size)
        else:
            sampler.warmup(nwarmup)
    else:
        if seed is None:
            X0 = chain.random_pos(nchains)
        else:
            X0 = np.random.default_rng([int(seed) & 0xFFFFFFFFFFFFFFFF, 1]).uniform(chain.min, chain.max, (nchains, chain.ndim))
        warm_start(sampler, X0, nwarmup, reseed=reseed)
    sampler.run(nsteps, thin=nthin)
    new = sampler.chain
    chain_data["chain"] = np.concatenate((chain_data["chain"], new), axis=1) if resume else new
    chain.chain = chain_data["chain"]
    chain.acceptance_fraction = sampler.acceptance_fraction
    chain.hmc_sampler = sampler
    c = sampler.counters()
    log.info("HMC done: acceptance %.3f, step size %.4g, %d divergent and %d escaped trajectories",
             float(np.mean(chain.acceptance_fraction)), sampler.step_size, c["divergent"], c["escaped"])
    with open(chain.mcmc_path, "wb") as f:
        pickle.dump(chain_data, f)
    return sampler
