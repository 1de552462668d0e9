"""
Device-resident tempered sequential Monte Carlo sampler with an evidence estimate: `Chain.run_SMC`.

The outer algorithm is the one pocoMC runs (adaptive tempering from the prior to the posterior, resampling, MCMC moves, a
running evidence), but this is not pocoMC: there is no normalizing flow, the moves are random-walk Metropolis steps
preconditioned by the Cholesky factor of the particle covariance, and earlier stages' particles are not reweighted at the end.

State: N particles x [N, d] in the chain's original parameters, their log-likelihoods logl [N] (bit for bit
Chain.log_likelihood(x, finite=True)) and one small device block with beta, logz, log_sigma, the effective sample size, the
counters and the flags.  The prior is the normalised uniform box.  A stage is
  reweight   beta in (beta_prev, 1] with ESS(beta) = ess_fraction * N (1 when ESS(1) suffices, else exactly 60 halvings),
             logz += logsumexp((beta - beta_prev) logl) - ln N, systematic resampling, mean / covariance / Cholesky factor
             (gpb_chain_smc_reweight);
  move       nmcmc steps x' = x + exp(log_sigma) Lc z, accepted where ln u < beta (logl' - logl), log_sigma adapted towards
             an acceptance of 0.234 after every step (gpb_chain_smc_move);
and the run stops after the moves of the stage that reached beta = 1: the particles are then equally weighted posterior
samples.  Both calls are asynchronous; the host reads the state block once per stage, which is the only synchronisation.
Random numbers: np.random.default_rng(seed) draws the start particles on the host, Philox streams keyed by the same seed
everything on the device (counters (stage, 0, 0, 8), (i, k, pair, 9), (i, k, 0, 10)): a stage's draws depend on
(seed, stage, k) only.  tests/smc_reference.py restates every piece in numpy.
"""
import logging

import numpy as np

from . import _native as nat
from .ptlmc import _philox_seed

log = logging.getLogger(__name__)

STATE_WORDS = 16                 # GPB_SMC_STATE_WORDS
OUTSIDE = -1e300                 # log_likelihood(finite=True) outside the box
MAX_D = 128
FLAG_PIVOT, FLAG_NO_WEIGHT = 1, 2


class SMCSampler:
    """The sampler's state in HBM and the calls of gpb_chain_smc_reweight / gpb_chain_smc_move.  `stage` counts the
    reweightings done, `k` the move steps of the whole run, `s` those since the last reweighting."""

    def __init__(self, chain, n_particles, ess_fraction=0.5, seed=None):
        import torch
        if not chain._native():
            raise NotImplementedError("SMC needs every emulator of the chain to be this package's Emulator (foreign emulators "
                                      "have no device step loop)")
        sh = getattr(chain, "sharding", None)
        if sh is not None and getattr(sh, "world", 1) > 1:
            raise NotImplementedError("SMC does not shard over several GPUs (chain.shard_over(None) first)")
        self.torch = torch
        self.chain = chain
        self.dev = torch.device("cuda", chain.device)
        self.N, self.d = int(n_particles), int(chain.ndim)
        self.ess_fraction = float(ess_fraction)
        self.seed = _philox_seed(seed)
        f64 = dict(dtype=torch.float64, device=self.dev)
        self.x = torch.zeros((max(self.N, 1), self.d), **f64)
        self.logl = torch.zeros(max(self.N, 1), **f64)
        self.block = torch.zeros(STATE_WORDS, **f64)
        self.Lc = torch.zeros((self.d, self.d), **f64)
        self.ancestors = torch.zeros(max(self.N, 1), dtype=torch.int64, device=self.dev)
        self.mean = torch.zeros(self.d, **f64)
        self.stage = self.k = self.s = 0

    def set_state(self, x, logl=None, beta=0.0, logz=0.0, log_sigma=None, stage=0, k=0, s=0):
        """particles [N, d] (logl: evaluated on the device when not given), the scalars, the counters zeroed"""
        t = self.torch
        self.x.copy_(t.as_tensor(np.ascontiguousarray(x, dtype=np.float64)))
        if logl is None:
            self.chain.log_prob_device(self.x, out=self.logl, outside=OUTSIDE)
        else:
            self.logl.copy_(t.as_tensor(np.ascontiguousarray(np.reshape(logl, -1), dtype=np.float64)))
        if log_sigma is None:
            log_sigma = np.log(2.38 / np.sqrt(self.d))
        blk = np.zeros(STATE_WORDS)
        blk[0:3] = float(beta), float(logz), float(log_sigma)
        self.block.copy_(t.as_tensor(blk))
        self.stage, self.k, self.s = int(stage), int(k), int(s)

    def init_uniform(self):
        """the start: uniform in the prior box from np.random.default_rng(seed), beta = 0, logz = 0"""
        ch = self.chain
        self.set_state(np.random.default_rng(self.seed).uniform(ch.min, ch.max, (self.N, self.d)))

    def read_block(self):
        """the state block on the host (one synchronisation); raises RuntimeError when a kernel has set a flag"""
        raw = self.block.cpu().numpy()
        cnt = raw.view(np.int64)
        out = dict(beta=float(raw[0]), logz=float(raw[1]), log_sigma=float(raw[2]), ess=float(raw[3]), dlogz=float(raw[4]),
                   naccept=int(cnt[10]), nan_moves=int(cnt[11]), nan_weights=int(cnt[12]), flags=int(cnt[13]))
        # the cause first: without a weight every position resamples the last particle, and that ensemble's pivot flag follows
        if out["flags"] & FLAG_NO_WEIGHT:
            raise RuntimeError("SMC: no particle has a finite log-likelihood at stage %d" % (self.stage - 1))
        if out["flags"] & FLAG_PIVOT:
            raise RuntimeError("SMC: the particle covariance is not positive definite at stage %d (a degenerate ensemble: "
                               "non-positive pivot in its Cholesky factorisation)" % (self.stage - 1))
        return out

    def state(self):
        """the resident state on the host: x, logl, the block's scalars and counters, Lc, stage, k, s"""
        out = self.read_block()
        out.update(x=self.x.cpu().numpy(), logl=self.logl.cpu().numpy(), Lc=self.Lc.cpu().numpy(), stage=self.stage, k=self.k,
                   s=self.s)
        return out

    def reweight(self):
        """enqueue one stage's reweighting, resampling and preconditioning (asynchronous)"""
        engs, arr, E = self.chain._contexts()
        e0 = engs[0]
        e0._ck(e0.lib.gpb_chain_smc_reweight(arr, E, self.N, self.stage, self.seed, self.ess_fraction, nat.ptr(self.x),
                                             nat.ptr(self.logl), nat.ptr(self.block), nat.ptr(self.Lc),
                                             nat.ptr(self.ancestors), nat.ptr(self.mean)))
        self.stage += 1
        self.s = 0

    def move(self, nsteps):
        """enqueue `nsteps` move steps from global step self.k (asynchronous)"""
        nsteps = int(nsteps)
        if nsteps <= 0:
            return
        engs, arr, E = self.chain._contexts()
        e0 = engs[0]
        lo, hi = self.chain._box(self.dev)
        e0._ck(e0.lib.gpb_chain_smc_move(arr, E, self.N, nsteps, self.k, self.s, self.seed, nat.ptr(self.x), nat.ptr(self.logl),
                                         nat.ptr(self.block), nat.ptr(self.Lc), nat.ptr(lo), nat.ptr(hi), OUTSIDE,
                                         self.chain.inside_const))
        self.k += nsteps
        self.s += nsteps

    def run(self, nmcmc=20, max_stages=200):
        """stages until beta = 1 (at most max_stages more): -> (beta ladder, acceptance rate per stage); the state block is
        read once per stage"""
        betas, rates = [], []
        acc0 = self.read_block()["naccept"]
        for _ in range(int(max_stages)):
            self.reweight()
            self.move(nmcmc)
            blk = self.read_block()
            betas.append(blk["beta"])
            rates.append((blk["naccept"] - acc0) / float(self.N * max(int(nmcmc), 1)))
            acc0 = blk["naccept"]
            log.info("SMC stage %d: beta %.6g, logz %.6g, ESS %.1f, acceptance %.3f", self.stage, blk["beta"], blk["logz"],
                     blk["ess"], rates[-1])
            if blk["beta"] >= 1.0:
                return np.array(betas), np.array(rates)
        raise RuntimeError("SMC: beta = %.6g after %d stages (max_stages)" % (betas[-1] if betas else 0.0, int(max_stages)))

    def information_gain(self, **kw):
        """InformationGain of the resident particles (divergence.py) against the uniform prior on the chain's box — after a
        resampling the particles carry equal weights; kw (k, bins, splits) as divergence.information_gain takes them"""
        from .divergence import information_gain
        kw.setdefault("names", list(getattr(self.chain, "pardict", ())) or None)
        return information_gain(self.x[:self.N], self.chain.min, self.chain.max, **kw)

    def stein_thin(self, m=100, **kw):
        """SteinThinning of the resident particles (thinning.py; Chain.stein_thin): the thinning corrects a biased sample, so
        no weights are needed"""
        return self.chain.stein_thin(self.x[:self.N], m=m, **kw)

    def ksd(self, **kw):
        """SteinDiscrepancy of the resident particles (thinning.py; Chain.ksd)"""
        return self.chain.ksd(self.x[:self.N], **kw)

    def divergence_from(self, other, **kw):
        """PosteriorComparison of the resident particles (A) against `other` (B: another SMCSampler's particles, a tensor or an
        array as divergence.posterior_divergence takes xb) on the chain's prior box"""
        from .divergence import posterior_divergence
        if isinstance(other, SMCSampler):
            other = other.x[:other.N]
        kw.setdefault("names", list(getattr(self.chain, "pardict", ())) or None)
        return posterior_divergence(self.x[:self.N], other, self.chain.min, self.chain.max, **kw)


def run_smc(chain, n_particles=4096, ess_fraction=0.5, nmcmc=20, max_stages=200, seed=None):
    """Chain.run_SMC (see there)"""
    s = SMCSampler(chain, n_particles, ess_fraction, seed)
    s.init_uniform()
    betas, rates = s.run(nmcmc, max_stages)
    st = s.state()
    n = s.N
    return {"chain": st["x"], "weights": np.full(n, 1.0 / n), "logl": st["logl"],
            "logp": np.full(n, -np.log(chain.prior_volume_)), "logz": st["logz"], "logz_err": float("nan"),
            "beta": betas, "acceptance": rates}
