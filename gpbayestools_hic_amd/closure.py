"""
Closure studies: one chain of emulators calibrated against MANY data vectors in one device-resident run.

The reference's closure test (examples/ClosureTest.ipynb; PlotMCMC.ipynb: compute_Delta_d, create_Delta_d_distribution)
replaces the experiment by the model's own output at a held-out design point, runs the whole MCMC against it and looks at
where the truth falls in the posterior.  A study over a validation set is that once per point.  Here the K calibrations are
K independent ensembles of one sampler: their proposals form one batch per half-step, the prediction of a row does not depend
on the data, and the likelihood takes a row's data terms from per-set tables (gpb_chain_like_sets, gpb_chain_logpost_sets,
gpb_chain_emcee_sets_run).  Set k's walkers are, bit for bit, those of StretchSampler(seed=seeds[k]) on a chain whose
experiment is data[k].  All sets share the chain's expdata_cov.

    ClosureSampler   the K-set counterpart of sampler.StretchSampler
    ClosureResult    what Chain.run_closure returns: the thinned chains and the summaries a closure study reports — the
                     truth's rank in each posterior, coverage, rank histogram, Delta_d per data set
"""
import logging
import pickle

import numpy as np

from . import _native as nat

log = logging.getLogger(__name__)


def closure_refusal(chain):
    """NotImplementedError with the reason when the K-set run does not serve this chain"""
    from .engine import MODE_PCA
    if not chain._native():
        raise NotImplementedError("closure runs need every emulator of the chain to be this package's Emulator (foreign "
                                  "emulators predict on the host)")
    if chain.sharding is not None and getattr(chain.sharding, "world", 1) > 1:
        raise NotImplementedError("closure runs: a chain sharded over several ranks is not supported (shard_over(None))")
    engs = [e._engine_ready() for e in chain.emuList]
    if getattr(engs[0], "_dist_world", 0) > 1:
        raise NotImplementedError("closure runs: a communicator is installed on the first emulator's engine")
    for i, g in enumerate(engs):
        if g.mode != MODE_PCA or g.P > 16:
            raise NotImplementedError("closure runs need every emulator in PCA mode with at most 16 GPs (the low-rank "
                                      "likelihood kernel): emulator %d has mode %d, %d GPs" % (i, g.mode, g.P))
    chain._prepare_blocks()
    if chain._coupled:
        raise NotImplementedError("closure runs: the experimental covariance couples different emulators (the per-set tables "
                                  "are those of the emulators' own blocks)")


def _check_data(chain, data):
    data = np.ascontiguousarray(np.atleast_2d(np.asarray(data, dtype=np.float64)))
    if data.ndim != 2 or data.shape[1] != chain.nobs or data.shape[0] < 1:
        raise ValueError("data must be [K, %d observables], got %s" % (chain.nobs, np.shape(data)))
    if not np.all(np.isfinite(data)):
        raise ValueError("data hold non-finite values")
    return data


class ClosureSampler:
    """K ensembles of `nwalkers` walkers, ensemble k calibrated against data[k] with the chain's expdata_cov.
    seeds [K] = np.random.SeedSequence(seed).generate_state(K, dtype=np.uint64): ensemble k is StretchSampler(seed=seeds[k])."""

    def __init__(self, chain, data, nwalkers, seed=None, a=2.0, randomize_split=True):
        import torch
        data = _check_data(chain, data)
        if int(nwalkers) < 2 or int(nwalkers) % 2:
            raise ValueError("nwalkers must be even")
        closure_refusal(chain)
        self.torch = torch
        self.chain_obj = chain
        self.data = data
        self.K = int(data.shape[0])
        self.ndim = int(chain.ndim)
        self.nwalkers = int(nwalkers)
        if self.nwalkers < 2 * self.ndim:
            log.warning("fewer walkers than 2*ndim")
        self.a = float(a)
        self.randomize_split = 1 if randomize_split else 0
        self.seeds = np.random.SeedSequence(seed).generate_state(self.K, dtype=np.uint64)
        self.device = torch.device("cuda", chain.device)
        self._step_counter = 0
        f64 = dict(dtype=torch.float64, device=self.device)
        self.pos = torch.empty((self.K, self.nwalkers, self.ndim), **f64)
        self.lp = torch.empty((self.K, self.nwalkers), **f64)
        self.naccept = torch.zeros((self.K, self.nwalkers), dtype=torch.int64, device=self.device)
        self._started = False
        self.reset()

    def reset(self):
        self._chain_dev = None
        self._lp_dev = None
        self.iterations = 0
        self.naccept.zero_()

    def _install(self):
        """the chain's own likelihood block (its covariance is every set's), then the per-set tables; the chain's likelihood
        state is not touched.  Before every run: another sampler, or a new experiment, may have replaced the tables."""
        ch = self.chain_obj
        closure_refusal(ch)
        engs, arr, n = ch._contexts()
        engs[0]._ck(engs[0].lib.gpb_chain_like_sets(arr, n, self.K, nat.ptr(self.data)))
        return engs[0], arr, n

    def _nan_count(self, eng):
        n = nat.c_i64(0)
        eng._ck(eng.lib.gpb_stretch_nan_count(eng.h, nat.C.byref(n), 1))
        return n.value

    def run(self, X0, nsteps, store=True):
        """Advance every ensemble `nsteps` stretch-move steps from X0 [K, nwalkers, ndim] (None: continue from the resident
        state); returns the final positions [K, nwalkers, ndim] (numpy)."""
        torch = self.torch
        nsteps = int(nsteps)
        if nsteps < 0:
            raise ValueError("nsteps >= 0")
        eng, arr, n = self._install()
        lib = eng.lib
        K, nw, d = self.K, self.nwalkers, self.ndim
        lo, hi = self.chain_obj._box(self.device)
        inside_const = self.chain_obj.inside_const
        if X0 is not None:
            X0 = np.ascontiguousarray(X0, dtype=np.float64)
            if X0.shape != (K, nw, d):
                raise ValueError("X0 must be [%d sets, %d walkers, %d parameters], got %s" % (K, nw, d, X0.shape))
            self.pos.copy_(torch.as_tensor(X0))
            eng._ck(lib.gpb_chain_logpost_sets(arr, n, nat.ptr(self.pos), K * nw, nw, nat.ptr(self.lp), nat.ptr(lo), nat.ptr(hi),
                                               float("-inf"), inside_const))
            if torch.isnan(self.lp).any().item():
                raise ValueError("The initial log_prob was NaN")
            self._started = True
        elif not self._started:
            raise ValueError("run(None, ...) continues a run: the first call needs X0")
        cd = ld = None
        if store:
            cd = torch.empty((nsteps, K, nw, d), dtype=torch.float64, device=self.device)
            ld = torch.empty((nsteps, K, nw), dtype=torch.float64, device=self.device)
        self._nan_count(eng)            # (whatever an earlier, aborted user of the context left behind is not ours)
        snap = (self.pos.clone(), self.lp.clone(), self.naccept.clone())
        eng._ck(lib.gpb_chain_emcee_sets_run(arr, n, nat.ptr(self.pos), nat.ptr(self.lp), K, nw, nsteps, nat.ptr(self.seeds),
                                             self._step_counter, self.a, self.randomize_split, nat.ptr(lo), nat.ptr(hi),
                                             float("-inf"), inside_const, nat.ptr(cd) if store else None,
                                             nat.ptr(ld) if store else None, nat.ptr(self.naccept)))
        bad = self._nan_count(eng)
        if bad:                         # as StretchSampler: back to the state in front of the call, nothing of it is kept
            self.pos.copy_(snap[0]); self.lp.copy_(snap[1]); self.naccept.copy_(snap[2])
            raise ValueError("Probability function returned NaN (%d proposal(s) within the %d steps of this run; the sampler is "
                             "back at its state before it)" % (bad, nsteps))
        self._step_counter += nsteps
        self.iterations += nsteps
        if store:
            self._chain_dev = cd if self._chain_dev is None else torch.cat([self._chain_dev, cd], 0)
            self._lp_dev = ld if self._lp_dev is None else torch.cat([self._lp_dev, ld], 0)
        return self.pos.cpu().numpy()

    @property
    def acceptance_fraction(self):
        """[K, nwalkers]"""
        return self.naccept.cpu().numpy() / max(self.iterations, 1)

    @property
    def chain(self):
        """[K, nwalkers, nsteps, ndim]: chain[k] is emcee's `sampler.chain` of set k"""
        if self._chain_dev is None:
            raise AttributeError("no stored chain: run the sampler (store=True) first")
        return self._chain_dev.permute(1, 2, 0, 3).contiguous().cpu().numpy()

    @property
    def lnprobability(self):
        """[K, nwalkers, nsteps]"""
        if self._lp_dev is None:
            raise AttributeError("no stored chain: run the sampler (store=True) first")
        return self._lp_dev.permute(1, 2, 0).contiguous().cpu().numpy()


def truth_rank(chain, truths, device=None):
    """rank [K, ndim] (int64): the number of stored samples of set k strictly below truths[k, j].  chain: numpy [K, nwalkers,
    nsteps, ndim], counted with numpy — or, with `device`, a torch tensor [nsteps, K, nwalkers, ndim] on that device, counted
    there."""
    truths = np.asarray(truths, dtype=np.float64)
    if device is not None:
        import torch
        t = torch.as_tensor(truths, device=chain.device)
        return (chain < t[None, :, None, :]).sum(dim=(0, 2)).to(torch.int64).cpu().numpy()
    chain = np.asarray(chain)
    return (chain < truths[:, None, None, :]).sum(axis=(1, 2)).astype(np.int64)


class ClosureResult:
    """chain [K, nwalkers, nstored, ndim], lnprobability [K, nwalkers, nstored], acceptance [K, nwalkers], data [K, nobs].
    With truths [K, ndim]: rank [K, ndim] (samples strictly below the truth), n_samples = nwalkers nstored, coverage(),
    rank_histogram(), and — with prior_ranges [ndim, 2] — delta [K] and delta_per_parameter [K, ndim]."""

    def __init__(self, chain, lnprobability, acceptance, data, truths=None, prior_ranges=None, names=None, rank=None,
                 device=0, chain_dev=None, seeds=None):
        self.chain = np.asarray(chain)
        self.seeds = None if seeds is None else np.asarray(seeds, dtype=np.uint64)      # [K]: ClosureSampler.seeds
        if self.chain.ndim != 4:
            raise ValueError("chain must be [K, nwalkers, nstored, ndim]")
        K, nw, ns, nd = self.chain.shape
        self.lnprobability = None if lnprobability is None else np.asarray(lnprobability)
        self.acceptance = None if acceptance is None else np.asarray(acceptance)
        self.data = None if data is None else np.asarray(data)
        self.n_samples = int(nw * ns)
        self.names = None if names is None else list(names)
        self.prior_ranges = None if prior_ranges is None else np.asarray(prior_ranges, dtype=np.float64)
        self.device = device
        self._chain_dev = chain_dev             # [nstored, K, nwalkers, ndim] on the device (not pickled), or None
        self._delta = None
        self.truths = None
        self.rank = None
        if truths is not None:
            self.truths = np.asarray(truths, dtype=np.float64)
            if self.truths.shape != (K, nd):
                raise ValueError("truths must be [%d, %d], got %s" % (K, nd, self.truths.shape))
            self.rank = truth_rank(self.chain, self.truths) if rank is None else np.asarray(rank, dtype=np.int64)
            if self.rank.shape != (K, nd):
                raise ValueError("rank must be [%d, %d]" % (K, nd))

    def _need_truths(self, who):
        if self.rank is None:
            raise ValueError("%s needs the truths" % who)

    def coverage(self, level):
        """[ndim]: the share of data sets whose central `level` credible interval (0 < level <= 1) holds the truth, decided
        from the rank alone: the truth lies inside when |rank / n_samples - 1/2| <= level / 2."""
        self._need_truths("coverage")
        level = float(level)
        if not 0.0 < level <= 1.0:
            raise ValueError("coverage: 0 < level <= 1")
        inside = np.abs(self.rank / self.n_samples - 0.5) <= 0.5 * level
        return inside.mean(axis=0)

    def rank_histogram(self, bins=10):
        """[ndim, bins] (int64): the data sets by the truth's rank, `bins` equal bins over [0, n_samples]: bin
        min(rank bins // n_samples, bins - 1).  Flat for a calibrated posterior."""
        self._need_truths("rank_histogram")
        bins = int(bins)
        if bins < 1:
            raise ValueError("rank_histogram: bins >= 1")
        b = np.minimum(self.rank * bins // self.n_samples, bins - 1)
        out = np.zeros((self.rank.shape[1], bins), dtype=np.int64)
        for j in range(self.rank.shape[1]):
            out[j] = np.bincount(b[:, j], minlength=bins)
        return out

    def _deltas(self):
        if self._delta is None:
            from .curves import closure_delta
            self._need_truths("delta")
            if self.prior_ranges is None:
                raise ValueError("delta needs prior_ranges [ndim, 2]")
            K = self.chain.shape[0]
            res = []
            for k in range(K):
                # set k's samples as [nwalkers, nstored, ndim]: a strided view of the resident chain, else the host array
                x = self._chain_dev[:, k].permute(1, 0, 2) if self._chain_dev is not None else self.chain[k]
                res.append(closure_delta(x, self.truths[k], self.prior_ranges, layout="walkers", names=self.names,
                                         device=self.device or 0))
            self._delta = (np.array([r.delta for r in res]), np.stack([r.per_parameter for r in res]))
        return self._delta

    @property
    def delta(self):
        """[K]: PlotMCMC.ipynb's Delta_d of every set (curves.closure_delta)"""
        return self._deltas()[0]

    @property
    def delta_per_parameter(self):
        """[K, ndim]"""
        return self._deltas()[1]

    def _set_samples(self, k):
        """set k's samples as [nwalkers, nstored, ndim]: a strided view of the resident chain, else the host array"""
        return self._chain_dev[:, k].permute(1, 0, 2) if self._chain_dev is not None else self.chain[k]

    def information_gain(self, k_set, discard=0, thin=1, **kw):
        """InformationGain (divergence.py) of data set k_set's samples, without the first `discard` stored steps and thinned by
        `thin`, against the uniform prior on prior_ranges; kw (k, bins, splits) as divergence.information_gain takes them"""
        from .divergence import information_gain
        if self.prior_ranges is None:
            raise ValueError("information_gain needs prior_ranges [ndim, 2]")
        kw.setdefault("names", self.names)
        kw.setdefault("device", self.device or 0)
        return information_gain(self._set_samples(int(k_set))[:, int(discard)::int(thin)], self.prior_ranges[:, 0],
                                self.prior_ranges[:, 1], layout="walkers", **kw)

    def stein_thin(self, chain, k_set, m=100, discard=0, thin=1, **kw):
        """SteinThinning (thinning.py) of data set k_set's samples, without the first `discard` stored steps and thinned by
        `thin`.  `chain`: the Chain the sets were calibrated with, holding data set k_set as its experimental data — a result
        holds arrays only, and the score is that of the chain's installed likelihood; kw as Chain.stein_thin takes them"""
        kw.setdefault("names", self.names)
        x = self._set_samples(int(k_set))[:, int(discard)::int(thin)]
        return chain.stein_thin(x.reshape(-1, x.shape[-1]), m=m, **kw)

    def ksd(self, chain, k_set, discard=0, thin=1, **kw):
        """SteinDiscrepancy (thinning.py) of data set k_set's samples; `chain` as stein_thin takes it"""
        x = self._set_samples(int(k_set))[:, int(discard)::int(thin)]
        return chain.ksd(x.reshape(-1, x.shape[-1]), **kw)

    def expected_information_gain(self, chain, k_set, discard=0, thin=1, **kw):
        """EIGResult (eig.py) over data set k_set's samples, without the first `discard` stored steps and thinned by `thin`: what a
        planned measurement is expected to add to that set's posterior.  `chain`: the Chain the sets were calibrated with (a
        result holds arrays only); kw (planned_error, groups, n_outer, seed) as Chain.expected_information_gain takes them"""
        x = self._set_samples(int(k_set))[:, int(discard)::int(thin)]
        x = x.cpu().numpy() if hasattr(x, "data_ptr") else np.asarray(x)
        return chain.expected_information_gain(np.ascontiguousarray(x).reshape(-1, x.shape[-1]), **kw)

    def divergence_between(self, k_a, k_b, discard=0, thin=1, **kw):
        """PosteriorComparison (divergence.py) of data set k_a's samples against data set k_b's on prior_ranges: do the two
        closure calibrations agree?"""
        from .divergence import posterior_divergence
        if self.prior_ranges is None:
            raise ValueError("divergence_between needs prior_ranges [ndim, 2]")
        kw.setdefault("names", self.names)
        kw.setdefault("device", self.device or 0)
        cut = (slice(None), slice(int(discard), None, int(thin)))
        return posterior_divergence(self._set_samples(int(k_a))[cut], self._set_samples(int(k_b))[cut], self.prior_ranges[:, 0],
                                    self.prior_ranges[:, 1], layout="walkers", layout_b="walkers", **kw)

    def _state(self):
        return dict(chain=self.chain, lnprobability=self.lnprobability, acceptance=self.acceptance, data=self.data,
                    truths=self.truths, prior_ranges=self.prior_ranges, names=self.names, rank=self.rank,
                    n_samples=self.n_samples, seeds=self.seeds)

    def save(self, path):
        """one pickle: a dict of the arrays (ClosureResult.load reads it back)"""
        with open(path, "wb") as f:
            pickle.dump(self._state(), f)

    @classmethod
    def load(cls, path, device=0):
        with open(path, "rb") as f:
            st = pickle.load(f)
        return cls(st["chain"], st["lnprobability"], st["acceptance"], st["data"], truths=st["truths"],
                   prior_ranges=st["prior_ranges"], names=st["names"], rank=st["rank"], device=device, seeds=st.get("seeds"))

    def write_chain(self, k, path):
        """set k's chain as the reference writes one: {"chain": [nwalkers, nstored, ndim]}, what PlotMCMC.ipynb reads"""
        k = int(k)
        if not 0 <= k < self.chain.shape[0]:
            raise ValueError("write_chain: set %d of %d" % (k, self.chain.shape[0]))
        with open(path, "wb") as f:
            pickle.dump({"chain": np.ascontiguousarray(self.chain[k])}, f)


def pseudo_data(chain, truths, noise=False, seed=None):
    """[K, nobs]: the emulators' mean at truths [K, ndim] (Chain._predict); noise=True adds one draw per set from
    expdata_cov (np.random.default_rng(seed))"""
    truths = np.atleast_2d(np.asarray(truths, dtype=np.float64))
    if truths.ndim != 2 or truths.shape[1] != chain.ndim:
        raise ValueError("truths must be [K, %d], got %s" % (chain.ndim, truths.shape))
    mean = chain._predict(truths)[0]
    if noise:
        rng = np.random.default_rng(seed)
        mean = mean + rng.multivariate_normal(np.zeros(chain.nobs), np.asarray(chain.expdata_cov, dtype=np.float64),
                                              size=truths.shape[0])
    return mean


def run_closure(chain, data, truths=None, nsteps=500, nburnsteps=None, nwalkers=None, nthin=10, seed=None):
    """Chain.run_closure (see there)"""
    if nburnsteps is None or nwalkers is None:
        raise ValueError("run_closure: nburnsteps and nwalkers must be given")
    data = _check_data(chain, data)
    K, d = data.shape[0], chain.ndim
    nsteps, nburnsteps, nwalkers, nthin = int(nsteps), int(nburnsteps), int(nwalkers), int(nthin)
    if nsteps < 1 or nburnsteps < 0 or nthin < 1:
        raise ValueError("run_closure: nsteps >= 1, nburnsteps >= 0, nthin >= 1")
    if truths is not None:
        truths = np.asarray(truths, dtype=np.float64)
        if truths.shape != (K, d):
            raise ValueError("truths must be [%d, %d], got %s" % (K, d, truths.shape))
    sampler = ClosureSampler(chain, data, nwalkers, seed=seed)
    X0 = chain.random_pos(K * nwalkers).reshape(K, nwalkers, d)
    nburn0 = nburnsteps // 2
    if nburn0 > 0:
        # run_mcmc's recipe per set (src/mcmc.py:345-426): half the burn-in, then the walkers go to the set's nwalkers most
        # likely distinct points
        sampler.run(X0, nburn0)
        lnp, ch = sampler.lnprobability, sampler.chain
        X0 = np.empty((K, nwalkers, d))
        for k in range(K):
            best = np.unique(lnp[k].reshape(-1), return_index=True)[1][-nwalkers:]
            if best.shape[0] < nwalkers:
                raise ValueError("run_closure: set %d has fewer than %d distinct points after %d burn-in steps" % (k, nwalkers, nburn0))
            X0[k] = ch[k].reshape(-1, d)[best]
        sampler.reset()
    sampler.run(X0, nburnsteps - nburn0)
    sampler.reset()
    sampler.run(None, nsteps)
    dev = sampler._chain_dev[::nthin]
    rank = truth_rank(dev, truths, device=sampler.device) if truths is not None else None
    names = list(chain.pardict) if getattr(chain, "pardict", None) else None
    return ClosureResult(sampler.chain[:, :, ::nthin], sampler.lnprobability[:, :, ::nthin], sampler.acceptance_fraction, data,
                         truths=truths, prior_ranges=np.stack([chain.min, chain.max], axis=1), names=names, rank=rank,
                         device=chain.device, chain_dev=dev, seeds=sampler.seeds)
