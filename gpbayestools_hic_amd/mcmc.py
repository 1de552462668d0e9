"""
Drop-in replacement for the reference's `src/mcmc.py` log-posterior path and emcee driver
(B2 protocol): `mvn_loglike`, `Chain` with `log_prior / log_likelihood /
log_posterior / _predict / run_mcmc / run_MCMC_PTLMC / samplerPTLMC / tempexchange / run_pocoMC /
compute_log_likelihood_for_chain`.

Every emulator prediction, covariance assembly, Cholesky and quadratic form runs in the HIP
engine.  When all emulators in `emuList` are this package's `Emulator`, a log-probability call
is E fused `gpb_loglike` block evaluations plus one box kernel; rows never leave HBM between
them.  An experimental covariance that couples different emulators (correlated systematics,
`Chain.set_systematics`) is evaluated by the coupled kernel from the same per-GP means and
variances (gpb_chain_like_set).  Foreign emulators (anything with the reference's predict protocol) go through
`_predict` on the host and the generic batched device MVN (`gpb_mvn_loglike`).
"""
import logging
import math
import os
import pickle
from pathlib import Path

import numpy as np

from .emulator import Emulator
from .engine import GPEngine
from .preprocess import parse_model_parameter_file
from .sampler import LoggingEnsembleSampler  # noqa: F401  (the reference defines it in this module)

log = logging.getLogger(__name__)

# the reference adds 2*log(extra_std + 1e-16) - extra_std/scale with extra_std == 0*X[:, -1]
# (src/mcmc.py:205,220-221 and :281,296-297): a constant inside the box
EXTRA_STD_CONST = 2.0 * math.log(1e-16)

_util_engine = None


def _utility_engine(device=0):
    global _util_engine
    if _util_engine is None:
        _util_engine = GPEngine(device)
    _util_engine._check_pid()            # created in the parent of a fork: RuntimeError before any HIP call
    return _util_engine


def mvn_loglike(y, cov):
    """Unnormalised multivariate-normal log-likelihood -1/2 y^T C^-1 y - 1/2 log det C
    (src/mcmc.py:23-65), evaluated by the device Cholesky kernel.  A covariance that is not
    positive definite raises numpy.linalg.LinAlgError (the reference's branch for this case is
    unreachable, src/mcmc.py:44-54)."""
    eng = _utility_engine()
    out = eng.mvn_loglike(np.asarray(y, float)[None, :], np.asarray(cov, float)[None, :, :])
    if eng.last_not_pd:
        raise np.linalg.LinAlgError("mvn_loglike: covariance is not positive definite")
    return float(out[0])


class Chain:
    def __init__(self, mcmc_path="./mcmc/chain.pkl", expdata_path="./exp_data.dat",
                 model_parafile="./model.dat", device=0):
        self.mcmc_path = Path(mcmc_path)
        self.mcmc_path.parent.mkdir(exist_ok=True)
        self.pardict = parse_model_parameter_file(model_parafile)
        self.ndim = len(self.pardict)
        self.label = [v[0] for v in self.pardict.values()]
        self.min = np.array([v[1] for v in self.pardict.values()])
        self.max = np.array([v[2] for v in self.pardict.values()])
        self.prior_volume_ = np.prod(self.max - self.min)
        self.expdata, self.expdata_cov = self._read_in_exp_data_pickle(expdata_path)
        self.nobs = self.expdata.shape[1]
        self.emuList = []
        self.chain = False
        self.device = device
        self._like_sig = None
        self.sharding = None                     # dist.WalkerSharding: see shard_over

    def __getstate__(self):                      # no device handles in pickles / forked workers
        st = dict(self.__dict__)
        st.pop("_box_dev", None)
        st.pop("_box_key", None)
        st["_like_sig"] = None
        st["sharding"] = None
        st.pop("_digest_cache", None)
        return st

    def __setstate__(self, st):
        self.__dict__.update(st)
        self.__dict__.setdefault("sharding", None)

    def shard_over(self, sharding):
        """Evaluate every log_posterior / log_likelihood batch in row shares over the ranks of `sharding`
        (dist.WalkerSharding; one process per GPU): rank r takes rows [r chunk, (r + 1) chunk) of the batch, one
        all-gather of the shares completes the vector on every rank.  This is the multi-GPU form of the call pocoMC makes —
        log_likelihood(X[n_active, ndim], finite=True) once per batch, src/mcmc.py:798-805 — with the sampler itself
        replicated: EVERY rank must make the same calls with the same rows, and all ranks must hold the same emulators
        (WalkerSharding.replicate).  Both are checked on EVERY call by the one all-reduce that rides in front of the batch (the
        rows' checksum and the four words of the state digest: a batch whose rows — or a replica whose model — differ between
        the ranks raises on all of them), so the sequence of collectives a rank issues never depends on what only that rank
        knows.  A row's value does not depend on the split.  `None` switches it off."""
        self.sharding = sharding
        return self

    # ------------------------------------------------------------------ inputs
    def _read_in_exp_data_pickle(self, filepath):
        """One experimental event: values and errors; covariance = diag(err^2)
        (src/mcmc.py:302-324)."""
        with open(filepath, "rb") as fp:
            data = pickle.load(fp)
        vals = np.array([data[k]["obs"][0] for k in data.keys()])
        errs = np.nan_to_num(np.abs(np.array([data[k]["obs"][1] for k in data.keys()])))
        cov = np.zeros((vals.shape[1], vals.shape[1]))
        np.fill_diagonal(cov, errs.flatten() ** 2)       # (nobs x nobs whatever the number of events, as the reference fills it)
        self._stat_errors = errs.flatten()[:cov.shape[0]].copy()      # set_systematics' default statistical errors
        return vals, cov

    def state_digest_cached(self):
        """state_digest(), recomputed only when an emulator was re-trained / re-loaded or the experiment replaced (new arrays):
        the key is rank-local, and only ever decides which VALUE this rank contributes to a check — never whether it takes part"""
        # (an emulator's fitted state by its serial number — new with every training and every __setstate__, never reused;
        # the experiment block by identity AND a content probe: id() alone can come back after an array was dropped)
        # ... the WHOLE covariance (an in-place edit off the diagonal must not leave the digest stale): its bytes up to 128
        # observables, two weighted sums over every element beyond that (a 540 x 540 block is 2.3 MB per call otherwise)
        cov = np.atleast_2d(np.asarray(self.expdata_cov, dtype=np.float64))
        if cov.size <= 128 * 128:
            cov_probe = cov.tobytes()
        else:
            w = 1.0 + np.arange(cov.shape[1], dtype=np.float64) / cov.shape[1]
            u = 1.0 + np.arange(cov.shape[0], dtype=np.float64)[::-1] / cov.shape[0]
            cov_probe = (float(cov.sum()), float(u @ cov @ w), np.diagonal(cov).tobytes())
        key = (id(self.expdata), id(self.expdata_cov), np.asarray(self.expdata).tobytes(),
               cov_probe, self.min.tobytes(), self.max.tobytes(),
               tuple((id(e), getattr(e, "_state_serial", None)) for e in self.emuList))
        if any(k[1] is None for k in key[-1]):           # a foreign emulator: no serial to trust, hash every time
            return self.state_digest()
        c = getattr(self, "_digest_cache", None)
        if c is None or c[0] != key:
            c = self._digest_cache = (key, self.state_digest())
        return c[1]

    def state_digest(self):
        """sha256 over the emulators' state digests, the experiment block and the prior box: what the ranks of a walker-
        sharded run must hold identically (dist.WalkerSharding.agree_state)."""
        import hashlib
        h = hashlib.sha256()
        for e in self.emuList:
            h.update(e.state_digest() if hasattr(e, "state_digest") else repr(type(e)).encode())
        for a in (self.expdata, self.expdata_cov, self.min, self.max):
            a = np.ascontiguousarray(a, dtype=np.float64)
            h.update(repr(a.shape).encode()); h.update(a.tobytes())
        return h.digest()

    def loadEmulator(self, emulatorPathList, adopt=True):
        """src/mcmc.py:145-150.  A pickle that holds a trained emulator of the REFERENCE (its `src.emulator.Emulator` with
        scikit-learn GPs inside: what EmulatorTraining.ipynb dumps) is taken over onto the device without retraining
        (Emulator.from_reference) unless adopt=False; anything else with the predict protocol stays a foreign emulator
        (host predictions, device likelihood)."""
        import dill
        from .emulator import Emulator
        for path in emulatorPathList:
            with open(path, "rb") as f:
                emu = dill.load(f)
            if adopt and not isinstance(emu, Emulator) and getattr(emu, "gps", None) and hasattr(emu, "scaler"):
                try:
                    emu = Emulator.from_reference(emu, device=self.device)
                    log.info("%s: a trained emulator of the reference, taken over onto device %s", path, self.device)
                except (ValueError, AttributeError, TypeError, KeyError) as e:
                    # an object that is not quite a trained reference emulator (a missing attribute, an array alpha, a GP
                    # fitted with normalize_y): it keeps the predict protocol and stays a foreign emulator, as before
                    log.info("%s: kept as a foreign emulator (%s: %s)", path, type(e).__name__, e)
            self.emuList.append(emu)
        log.info("Number of Emulators: %d", len(self.emuList))

    def set_predict_arithmetic(self, which="fp64-int8"):
        """the same choice for every drop-in emulator of the chain (Emulator.set_predict_arithmetic): "fp64-int8" (default), "fp64"
        or "int8" — foreign emulators are left alone; an emulator outside the six-plane rule keeps the fp64 kernel by itself"""
        from .emulator import Emulator
        for e in self.emuList:
            if isinstance(e, Emulator):
                e.set_predict_arithmetic(which)
        self.__dict__.pop("_digest_cache", None)
        return self

    def random_pos(self, n=1):
        return np.random.uniform(self.min, self.max, (n, self.ndim))

    @staticmethod
    def map(f, args):
        """Lets the object stand in as an emcee `pool` so that the sampler hands the whole
        half-ensemble to the log-probability function in one call (src/mcmc.py:335-342)."""
        return f(args)

    # ------------------------------------------------------------------ model prediction
    def _predict(self, X, extra_std=0.0):
        """Concatenated means and block-diagonal covariance over the emulators
        (src/mcmc.py:153-166)."""
        n = X.shape[0]
        mean = np.zeros((n, self.nobs))
        cov = np.zeros((n, self.nobs, self.nobs))
        es = extra_std * X[:, -1]
        i0 = 0
        for emu in self.emuList:
            m, c = emu.predict(X, return_cov=True, extra_std=es)
            k = m.shape[1]
            mean[:, i0:i0 + k] = m
            cov[:, i0:i0 + k, i0:i0 + k] = c
            i0 += k
        return mean, cov

    # ------------------------------------------------------------------ log-probabilities
    def log_prior(self, X):
        """log(1/volume) inside the open box, -inf outside (src/mcmc.py:169-185)."""
        X = np.array(X, ndmin=2, dtype=np.float64)
        lp = np.log(np.ones(X.shape[0]) / self.prior_volume_)
        lp[~np.all((X > self.min) & (X < self.max), axis=1)] = -np.inf
        return lp

    def _native(self):
        return len(self.emuList) > 0 and all(isinstance(e, Emulator) for e in self.emuList)

    def set_systematics(self, sources, stat=None):
        """Correlated systematic uncertainties: sources [K, nobs], row k the fully correlated one-sigma shift of source k over
        the observables of all emulators (a normalisation or luminosity uncertainty: a fraction of expdata; zero where the
        source does not act).  Sets expdata_cov = diag(stat^2) + sum_k s_k s_k^T, with stat [nobs] defaulting to the errors
        read from the experiment file (the square roots of the present diagonal).  Returns self."""
        S = np.atleast_2d(np.asarray(sources, dtype=np.float64))
        if S.ndim != 2 or S.shape[1] != self.nobs:
            raise ValueError("set_systematics: sources must be [K, %d], got %s" % (self.nobs, np.shape(sources)))
        if stat is None:                         # (a chain unpickled from before this method: the present diagonal's roots)
            stat = getattr(self, "_stat_errors", None)
            stat = np.sqrt(np.diag(self.expdata_cov)) if stat is None else stat
        stat = np.asarray(stat, dtype=np.float64).reshape(-1)
        if stat.shape[0] != self.nobs:
            raise ValueError("set_systematics: stat must hold %d errors" % self.nobs)
        cov = np.zeros((self.nobs, self.nobs))
        np.fill_diagonal(cov, stat ** 2)
        for s in S:
            cov += np.outer(s, s)
        self.expdata_cov = cov
        return self

    _coupled = False                             # expdata_cov has entries that couple different emulators ...
    _coupled_why = None                          # ... and why the device's coupled likelihood does not serve them (None: it does)

    def _prepare_blocks(self):
        """Hand every emulator its slice of the experimental data (gpb_chain_like_set).  An experimental covariance that
        couples different emulators — the reference adds whatever expdata_cov holds, src/mcmc.py:288-293 — installs the
        coupled likelihood in the first emulator's context when it applies (every emulator in PCA mode, at most 128 GPs
        and 2048 observables in all, the compacted chain call available, covariance positive definite); when it does not,
        log_posterior / log_likelihood take the generic route (_predict + the dense device MVN) and the C-driven loops
        raise NotImplementedError.  A block-diagonal covariance takes the block path as before."""
        import ctypes
        from . import _native as nat
        # (engines by their serial numbers: the id() of a closed engine can come back with the next one created; the
        # experiment's arrays and the emulators by identity, and the signature keeps them alive: the id() of a dropped
        # covariance can come back with the next one assigned, block-diagonal then, coupled now)
        prev = self._like_sig
        serials = tuple(getattr(e._engine, "serial", None) for e in self.emuList)
        if (prev is not None and prev[0] is self.expdata and prev[1] is self.expdata_cov and len(prev[2]) == len(self.emuList)
                and all(a is b for a, b in zip(prev[2], self.emuList)) and prev[3] == serials):
            return
        engs = [emu._engine_ready() for emu in self.emuList]
        nobs = sum(emu.nobs for emu in self.emuList)
        if nobs != self.nobs:
            raise ValueError("emulators provide %d observables, experiment has %d" % (nobs, self.nobs))
        cov = nat.f64(self.expdata_cov)
        yexp = nat.f64(self.expdata[0])
        if cov.shape != (nobs, nobs):
            raise ValueError("experimental covariance is %s, the emulators provide %d observables" % (cov.shape, nobs))
        mask = np.zeros(cov.shape, dtype=bool)
        i0 = 0
        for emu, eng in zip(self.emuList, engs):
            assert eng.M == emu.nobs
            mask[i0:i0 + emu.nobs, i0:i0 + emu.nobs] = True
            i0 += emu.nobs
        applies = ctypes.c_int(0)
        arr = (nat.C.c_void_p * len(engs))(*[g.h for g in engs])
        engs[0]._ck(engs[0].lib.gpb_chain_like_set(arr, len(engs), nat.ptr(yexp), nat.ptr(cov), ctypes.byref(applies)))
        self._coupled = bool(np.any(cov[~mask] != 0.0))
        self._coupled_why = None
        if self._coupled and not applies.value:
            from .engine import MODE_PCA
            ngp = sum(g.P for g in engs)
            if any(g.mode != MODE_PCA for g in engs):
                self._coupled_why = "an emulator is not in PCA mode"
            elif ngp > 128 or nobs > 2048:
                self._coupled_why = "%d GPs and %d observables exceed the limits of 128 and 2048" % (ngp, nobs)
            elif engs[0].lib.gpb_chain_supported(arr, len(engs)) != 1:
                self._coupled_why = "the emulators do not take the compacted chain call"
            else:
                self._coupled_why = ("experimental + truncation covariance is not positive definite, or an emulator's "
                                     "transform is rank deficient")
        self._like_sig = (self.expdata, self.expdata_cov, tuple(self.emuList), tuple(e._engine.serial for e in self.emuList))

    def _coupled_fallback(self):
        """True when expdata_cov couples the emulators and the device's coupled likelihood does not apply (the dense route)"""
        if not self._native():
            return False
        self._prepare_blocks()
        return self._coupled and self._coupled_why is not None

    inside_const = EXTRA_STD_CONST               # what the reference adds to every row inside the box

    def _box(self, device):
        """the prior box resident in HBM, uploaded once per device"""
        import torch
        key = (str(device), self.min.tobytes(), self.max.tobytes())
        if getattr(self, "_box_key", None) != key:
            self._box_dev = (torch.as_tensor(self.min, dtype=torch.float64, device=device),
                             torch.as_tensor(self.max, dtype=torch.float64, device=device))
            self._box_key = key
        return self._box_dev

    # False: sequence the emulators from Python (A/B tests).  The per-emulator sequence is a sum of blocks and has no coupled
    # counterpart: with a coupled experimental covariance the C chain call is always used, whatever this says.
    use_chain_call = True

    def _contexts(self):
        """(engines, ctypes array of their contexts, count) of emuList, ready for a C call that takes the chain: every
        emulator has its block of the experimental data, a fitted engine, and enqueues on torch's current stream.
        NotImplementedError when expdata_cov couples the emulators and the device's coupled likelihood does not apply: the C
        calls would evaluate another likelihood."""
        from . import _native as nat
        self._prepare_blocks()
        if self._coupled and self._coupled_why is not None:
            raise NotImplementedError("the experimental covariance couples different emulators and the device's coupled "
                                      "likelihood does not apply (%s): only log_posterior / log_likelihood evaluate it, "
                                      "through the dense route" % self._coupled_why)
        engs = [e._engine_ready() for e in self.emuList]
        for g in engs:
            g._need_data()
            g._track_stream()
        return engs, (nat.C.c_void_p * len(engs))(*[g.h for g in engs]), len(engs)

    def _chain_contexts(self):
        """(engines, ctypes array of their contexts) when the C ABI can evaluate the whole chain in one call
        (gpb_chain_logpost / gpb_chain_emcee_run: rows outside the prior box skipped, one emulator after the other on
        one stream), else None."""
        if not self._native():
            return None
        self._prepare_blocks()
        if not (self.use_chain_call or self._coupled):
            return None
        engs, arr, n = self._contexts()
        return (engs, arr) if engs[0].lib.gpb_chain_supported(arr, n) == 1 else None

    def log_prob_device(self, X_dev, out=None, outside=-np.inf, lo_dev=None, hi_dev=None):
        """Device-resident log-posterior: X_dev torch.float64 cuda [W,ndim] -> lp [W] (no host
        sync).  Used by the resident sampler; `log_posterior`/`log_likelihood` wrap it.
        The per-emulator sequence below is the Python counterpart of chain_eval (csrc/gpb_chain.hip), which the C-driven
        samplers and the gradient run; it goes through the public per-emulator calls (use_chain_call = False: the A/B path the
        tests compare the C paths against).  A change of the rule goes into both."""
        import torch
        from . import _native as nat
        self._prepare_blocks()
        if out is None:
            out = torch.empty(X_dev.shape[0], dtype=torch.float64, device=X_dev.device)
        if lo_dev is None:
            lo_dev, hi_dev = self._box(X_dev.device)
        X_dev = X_dev.contiguous()
        last = len(self.emuList) - 1
        if X_dev.shape[1] != self.ndim:
            raise ValueError("log_prob_device: X has %d columns, the chain has %d parameters" % (X_dev.shape[1], self.ndim))
        cc = self._chain_contexts()
        if cc is not None:
            engs, arr = cc
            e0 = engs[0]
            X_dev = e0._dev(X_dev, (None, self.ndim), "X")
            e0._dev(lo_dev, (self.ndim,), "lo"), e0._dev(hi_dev, (self.ndim,), "hi")
            e0._dev(out, (X_dev.shape[0],), "out")
            e0._ck(e0.lib.gpb_chain_logpost(arr, len(engs), nat.ptr(X_dev), X_dev.shape[0], nat.ptr(out), nat.ptr(lo_dev),
                                            nat.ptr(hi_dev), float(outside), EXTRA_STD_CONST))
            return out
        if self._coupled:                            # (the blocks below do not add up to a coupled likelihood)
            raise NotImplementedError("log_prob_device: the experimental covariance couples different emulators and the "
                                      "emulators do not take the compacted chain call")
        for i, emu in enumerate(self.emuList):      # all engines enqueue on torch's current stream: ordered
            eng = emu._engine_ready()
            mapped = getattr(emu, "parameterTrafoPCA_", False)
            # parameterTrafoPCA emulators see the PCA-reduced parameters (src/emulator.py:492-551): device pre-pass
            Xg = eng.param_map(X_dev) if mapped else X_dev
            if i < last or mapped:
                eng.loglike(Xg, out=out, accumulate=(i > 0), check=False)
                if i == last:                        # the prior box is over the ORIGINAL parameters
                    eng.box_finish(X_dev, lo_dev, hi_dev, outside, EXTRA_STD_CONST, out)
            else:                                    # last block: likelihood + prior box + constant, one call
                eng.logpost(X_dev, out, i > 0, lo_dev, hi_dev, outside, EXTRA_STD_CONST)
        return out

    def _log_prob(self, X, outside):
        X = np.array(X, ndmin=2, dtype=np.float64)
        # (a coupled experimental covariance that the device's coupled likelihood does not serve: the generic path below,
        # which adds the whole expdata_cov to the emulators' block-diagonal covariance as the reference does)
        if self._native() and not self._coupled_fallback():
            import torch
            dev = torch.device("cuda", self.device)
            # long inputs (a stored chain, src/mcmc.py:729-749) go through in slabs: the K*^T workspace is
            # P x N x rows doubles per emulator; a row's result does not depend on how the batch is cut
            per_row = max(8 * e._ngp * e._X_train.shape[0] for e in self.emuList)
            slab = int(min(max((8 << 30) // per_row, 1024), 1 << 17)) // 128 * 128
            sh = self.sharding if (self.sharding is not None and getattr(self.sharding, "world", 1) > 1) else None
            # sharded: all ranks must hold the same model and be handed the same rows.  ONE all-reduce of the rows' checksum
            # and the state digest's words rides in front of every batch and is read after it — every rank issues it on every
            # call, whatever it knows locally (a rank whose engines were rebuilt by replicate(), a rank that has evaluated
            # before): the collective sequences of the ranks cannot drift apart
            digest = self.state_digest_cached() if sh is not None else None

            def evaluate(Xd):
                if sh is None:
                    return self.log_prob_device(Xd, outside=outside)
                pending = sh.rows_agree_begin(Xd, digest)
                out = torch.empty(Xd.shape[0], dtype=torch.float64, device=Xd.device)
                sh.logprob(lambda Xr, o: self.log_prob_device(Xr, out=o, outside=outside), Xd, out)
                sh.rows_agree_end(pending)
                return out
            if X.shape[0] <= slab:
                Xd = torch.as_tensor(np.ascontiguousarray(X), device=dev)
                return evaluate(Xd).cpu().numpy()
            out = np.empty(X.shape[0])
            for i0 in range(0, X.shape[0], slab):
                Xd = torch.as_tensor(np.ascontiguousarray(X[i0:i0 + slab]), device=dev)
                out[i0:i0 + slab] = evaluate(Xd).cpu().numpy()
            return out
        # generic path: foreign emulators predict on the host, the MVN runs on the device
        lp = np.zeros(X.shape[0])
        inside = np.all((X > self.min) & (X < self.max), axis=1)
        lp[~inside] = outside
        if np.count_nonzero(inside) > 0:
            Xi = X[inside]
            mY, mC = self._predict(Xi, 0.0 * Xi[:, -1])
            eng = _utility_engine(self.device)
            lp[inside] += eng.mvn_loglike(mY - self.expdata, mC + self.expdata_cov)
            lp[inside] += EXTRA_STD_CONST
        return lp

    def sobol_indices(self, log_observable=False):
        """Sobol indices of every emulator of emuList over the chain's prior box (Emulator.sobol_indices with bounds = the
        chain's min / max), concatenated along the observables in emuList order: a SobolIndices with mean, variance [nobs],
        first_order, total [nobs, ndim].  NotImplementedError for foreign emulators (and what Emulator.sobol_indices refuses)."""
        from .emulator import SobolIndices
        if not self._native():
            raise NotImplementedError("sobol_indices needs every emulator of the chain to be this package's Emulator (foreign "
                                      "emulators expose no GP state to integrate)")
        bounds = np.stack([self.min, self.max], axis=1)
        parts = [e.sobol_indices(bounds, log_observable=log_observable) for e in self.emuList]
        return SobolIndices(*[np.concatenate([getattr(r, k) for r in parts], axis=0)
                              for k in ("mean", "variance", "first_order", "total")], names=list(self.pardict))

    ppd_slab_rows = None                         # most rows of one posterior_predictive slab (None: _log_prob's rule); same bits

    def _predict_slab_rows(self, override=None):
        """rows of one predict slab: _log_prob's rule (the K*^T workspace is P x N x rows doubles per emulator), or the override"""
        per_row = max(8 * e._ngp * e._X_train.shape[0] for e in self.emuList)
        slab = int(min(max((8 << 30) // per_row, 1024), 1 << 17)) // 128 * 128
        return slab if override is None else max(int(override), 1)

    def _predict_diag_slab(self, engs, X_host, Xd, esd, mu_T, var_T):
        """One slab of rows (X_host on the host, Xd the same rows on the device) through every emulator: gpb_emu_predict_diag into
        the emulator's rows of the [nobs, rows] device views mu_T, var_T — _predict's mean and np.diagonal(cov), bit for bit."""
        import torch
        r0 = 0
        for emu, eng in zip(self.emuList, engs):
            # parameterTrafoPCA emulators: the HOST map, as Emulator.predict applies it — the device pre-pass agrees with it
            # to ~1e-12, not to the bit, and these arrays are _predict's bits
            Xg = Xd
            if getattr(emu, "parameterTrafoPCA_", False):
                Xg = torch.as_tensor(np.ascontiguousarray(emu._map_parameters(X_host() if callable(X_host) else X_host)), device=Xd.device)
            eng.emu_predict_diag(Xg, extra_std=esd, out=(mu_T[r0:r0 + emu.nobs], var_T[r0:r0 + emu.nobs]))
            r0 += emu.nobs

    def _ppd_arrays(self, X, extra_std=0.0):
        """(engines, mu_T, var_T): the emulators' means and covariance diagonals at the rows X [S, ndim], observable-major
        device arrays [nobs, S] in emuList order — what _predict(X, extra_std) returns as mean and np.diagonal(cov), bit for
        bit, without the [S, nobs, nobs] array.  Slab by slab and emulator by emulator: upload (for parameterTrafoPCA emulators
        the rows mapped on the host, as predict maps them), gpb_emu_predict_diag into the emulator's rows."""
        import torch
        dev = torch.device("cuda", self.device)
        engs = [e._engine_ready() for e in self.emuList]
        for g in engs:
            g._need_data()
            g._track_stream()
        S = X.shape[0]
        if sum(e.nobs for e in self.emuList) != self.nobs:
            raise ValueError("emulators provide %d observables, experiment has %d" % (sum(e.nobs for e in self.emuList), self.nobs))
        slab = self._predict_slab_rows(self.ppd_slab_rows)
        mu_T = torch.empty((self.nobs, S), dtype=torch.float64, device=dev)
        var_T = torch.empty((self.nobs, S), dtype=torch.float64, device=dev)
        es = np.ascontiguousarray(extra_std * X[:, -1])               # as _predict forms it (src/mcmc.py:153-166)
        for i0 in range(0, S, slab):
            i1 = min(i0 + slab, S)
            Xd = torch.as_tensor(np.ascontiguousarray(X[i0:i1]), device=dev)
            esd = torch.as_tensor(es[i0:i1], device=dev)
            self._predict_diag_slab(engs, X[i0:i1], Xd, esd, mu_T[:, i0:i1], var_T[:, i0:i1])
        return engs, mu_T, var_T

    def posterior_predictive(self, samples, quantiles=(0.05, 0.16, 0.5, 0.84, 0.95), extra_std=0.0):
        """What does the posterior predict for every observable, with the emulator's own uncertainty, and where does the data
        sit in it — over ALL samples of a chain, on the device.  The posterior-predictive check of examples/ClosureTest.ipynb
        and the bands of PlotMCMC.ipynb, which take fifteen samples because `_predict` returns the [S, nobs, nobs] covariance.

        samples: [S, ndim], or a stored [nwalkers, nsteps, ndim] chain (flattened).  Rows outside the prior box are predicted
        like any other, as `_predict` does.  Per slab and emulator one predict pass writes the means and the covariance
        diagonals observable-major into one [nobs, S] device pair (gpb_emu_predict_diag); two reductions over the sample axis
        follow (gpb_ppd_summary): moments, the order statistics for np.percentile's band and the quantiles of the predictive
        mixture 1/S sum_s N(mu_s, sigma_s^2); then the mixture's CDF at the measurement with the experimental variance added.
        Closed form, nothing sampled, equal inputs give equal bits.  Returns a PosteriorPredictive.
        NotImplementedError for foreign emulators and for a chain sharded over several ranks."""
        from .emulator import PosteriorPredictive, percentile_from_order
        if not self._native():
            raise NotImplementedError("posterior_predictive needs every emulator of the chain to be this package's Emulator (foreign "
                                      "emulators expose no GP state to predict from on the device)")
        if self.sharding is not None and getattr(self.sharding, "world", 1) > 1:
            raise NotImplementedError("posterior_predictive: a chain sharded over several ranks is not supported; call it on one "
                                      "rank (shard_over(None))")
        X = np.asarray(samples, dtype=np.float64)
        if X.ndim == 3:
            X = X.reshape(-1, X.shape[-1])
        X = np.ascontiguousarray(np.atleast_2d(X))
        if X.ndim != 2 or X.shape[1] != self.ndim or X.shape[0] < 1:
            raise ValueError("posterior_predictive: samples must be [S, %d] or [nwalkers, nsteps, %d], got %s"
                             % (self.ndim, self.ndim, np.shape(samples)))
        if not np.all(np.isfinite(X)):
            raise ValueError("posterior_predictive: samples hold non-finite values")
        q = np.ascontiguousarray(np.atleast_1d(np.asarray(quantiles, dtype=np.float64)).reshape(-1))
        if q.shape[0] < 1 or q.shape[0] > GPEngine.PPD_MAX_LEVELS or not np.all((q >= 0.0) & (q <= 1.0)):
            raise ValueError("posterior_predictive: 1 to %d quantile levels in [0, 1]" % GPEngine.PPD_MAX_LEVELS)
        S = X.shape[0]
        engs, mu_T, var_T = self._ppd_arrays(X, extra_std)
        e0 = engs[0]
        out = e0.ppd_summary(mu_T, var_T, q)
        pit = e0.ppd_summary(mu_T, var_T, q, vadd=np.diag(self.expdata_cov), yobs=self.expdata[0], outputs=("pit",))["pit"]
        mom = out["moments"]
        return PosteriorPredictive(q, mom[:, 0], np.sqrt(mom[:, 1]), np.sqrt(mom[:, 2]), np.sqrt(mom[:, 1] + mom[:, 2]),
                                   np.ascontiguousarray(percentile_from_order(out["order"], q, S).T),
                                   np.ascontiguousarray(out["mixq"].T), pit, S)

    hm_slab_rows = None                          # most rows of one history_match / implausibility slab (None: _log_prob's rule); same bits

    def implausibility(self, X, kth=2, discrepancy=None, rel_discrepancy=0.0, observable_mask=None):
        """The univariate implausibility of explicit rows X [S, ndim]: I_m = |expdata_m - mean_m(x)| / sqrt(var_m(x) + V_m) with
        V = diag(expdata_cov) + discrepancy + (rel_discrepancy expdata)^2 (discrepancy, rel_discrepancy: scalars or [nobs]) and
        the observables where observable_mask is False left out.  Returns a dict of numpy arrays: "top" [kth, S] the kth largest
        per row (a row is not ruled out yet iff top[kth - 1] < cutoff), "arg" [S] the observable of the largest, "gmax" [E, S]
        the largest per emulator, "bad" the number of rows with an undefined implausibility.  Predict and reduction run on the
        device slab by slab (gpb_emu_predict_diag, gpb_hm_implausibility).  Errors as history_match."""
        from .history import chain_implausibility
        return chain_implausibility(self, X, kth, discrepancy, rel_discrepancy, observable_mask)

    def history_match(self, n_samples=1 << 20, X=None, cutoff=3.0, kth=2, discrepancy=None, rel_discrepancy=0.0, observable_mask=None,
                      bins=20, bounds=None, pairs=None, keep=100000, seed=0):
        """How much of the box do the data already rule out, which observable or data set does it, and where should the next wave
        of model runs go: history matching (history.py) with the trained emulators, BEFORE any sampling.  n_samples candidates are
        drawn uniformly in `bounds` [ndim, 2] (default the prior box) on the device (gpb_hm_uniform, keyed by `seed` and the row),
        or X [S, ndim] is judged as given (posterior draws, a design).  Slab by slab (hm_slab_rows; the workspace does not grow
        with n_samples): the predict pass of posterior_predictive, emulator by emulator, into one [nobs, slab] pair; the
        implausibility I_m = |expdata_m - mean_m| / sqrt(var_m + V_m), V = diag(expdata_cov) + discrepancy + (rel_discrepancy
        expdata)^2, masked observables (observable_mask False) left out (gpb_hm_implausibility: the kth largest, the observable
        of the largest, the largest per emulator); the maps of the kth largest over `bins` (<= 64) equal bins per parameter
        and the parameter pairs `pairs` (default all) (gpb_hm_maps).  A candidate is not ruled out yet (NROY) iff its kth largest
        implausibility is < cutoff.  Returns a HistoryMatch: NROY fraction, ruled_out_by, dataset_nroy_fraction, minimum-
        implausibility and optical-depth maps, the NROY box and the first `keep` NROY rows — candidates for propose_design —
        and .refocus() for the next wave's bounds.  Integer reductions only: equal inputs give equal results whatever the slabs.

        The measure is the UNIVARIATE one: correlations between observables in expdata_cov are ignored (history.py shows the way
        to a multivariate score).  n_bad > 0 — candidates whose implausibility is undefined — raises a RuntimeWarning.  A
        nroy_fraction of 0 means that nothing survives: look at ruled_out_by and the discrepancy; it is not an error.
        NotImplementedError for foreign emulators and a chain sharded over several ranks; ValueError for kth above the number
        of unmasked observables (or 4), wrong shapes and bounds."""
        from .history import history_match
        return history_match(self, n_samples, X, cutoff, kth, discrepancy, rel_discrepancy, observable_mask, bins, bounds, pairs, keep,
                             seed)

    def convergence(self, chain=None, discard=0, c=5, tol=50):
        """Is the chain long enough?  ChainDiagnostics (diagnostics.py) of a stored [nwalkers, nsteps, ndim] array — self.chain
        (default; read from mcmc_path when it is not in memory), a loaded pickle's, or run_MCMC_PTLMC's output — without its
        first `discard` steps: integrated autocorrelation time with emcee's automatic window, effective sample size,
        split-R-hat, mean, std and Monte-Carlo standard error per parameter, computed on the device (gpb_mcmc_diag; the
        array is uploaded in its own layout, not permuted, and read through its strides).  Never raises for a short chain:
        converged=False."""
        from .diagnostics import diagnose
        if chain is None:
            if self.chain is False:
                with open(self.mcmc_path, "rb") as f:
                    self.chain = pickle.load(f)["chain"]
            chain = self.chain
        x = np.asarray(chain, dtype=np.float64)
        if x.ndim != 3:
            raise ValueError("convergence: chain must be [nwalkers, nsteps, ndim], got %s" % (np.shape(chain),))
        discard = int(discard)
        if discard < 0 or x.shape[1] - discard < 4:
            raise ValueError("convergence: at least 4 steps must remain after discard")
        names = list(self.pardict) if len(getattr(self, "pardict", ())) == x.shape[2] else None
        return diagnose(x[:, discard:], c=c, tol=tol, layout="walkers", names=names, device=self.device or 0)

    def rank_convergence(self, chain=None, discard=0, thin=1, **kw):
        """Are the chains mixed, and are the bulk and the tails resolved?  RankDiagnostics (diagnostics.py) of a stored [nwalkers,
        nsteps, ndim] array — self.chain (default; read from mcmc_path when it is not in memory), a loaded pickle's, run_HMC's or
        run_MCMC_PTLMC's output — without its first `discard` steps and thinned by `thin`: rank-normalised split-R-hat (the larger
        of bulk and folded) with bulk-, tail-, mean- and quantile-ESS per parameter (Vehtari et al. 2021), computed on the device
        (gpb_chain_rank_diag; the array is uploaded in its own layout and read through its strides).  kw (probs, min_ess,
        rhat_max) as diagnostics.rank_diagnose takes them.  A weighted particle set (run_SMC's, pocoMC's) is refused."""
        from .diagnostics import rank_diagnose
        if kw.get("weights") is not None:
            raise ValueError("rank_convergence: ranks of weighted draws are out of scope; resample the particle set to equal weights")
        if chain is None:
            if self.chain is False:
                with open(self.mcmc_path, "rb") as f:
                    self.chain = pickle.load(f)["chain"]
            chain = self.chain
        x = np.asarray(chain, dtype=np.float64)
        if x.ndim != 3:
            raise ValueError("rank_convergence: chain must be [nwalkers, nsteps, ndim], got %s (a flat particle set has no chains to "
                             "compare)" % (np.shape(chain),))
        discard, thin = int(discard), int(thin)
        if discard < 0 or thin < 1 or (x.shape[1] - discard + thin - 1) // thin < 4:
            raise ValueError("rank_convergence: at least 4 steps must remain after discard and thin")
        names = list(self.pardict) if len(getattr(self, "pardict", ())) == x.shape[2] else None
        kw.setdefault("names", names)
        return rank_diagnose(x[:, discard::thin], thin=thin, layout="walkers", device=self.device or 0, **kw)

    def posterior_marginals(self, chain=None, discard=0, thin=1, bins=20, range=None, weights=None,
                            quantiles=(0.05, 0.16, 0.5, 0.84, 0.95), pairs=None):
        """The posterior in parameter space: PosteriorMarginals (marginals.py) of a stored [nwalkers, nsteps, ndim] array —
        self.chain (default; read from mcmc_path when it is not in memory), a loaded pickle's — without its first `discard`
        steps and thinned by `thin`, or of a flat [S, ndim] particle set with its importance `weights` (the `chain` and
        `weights` of a pocoMC / run_SMC pickle; discard and thin do not apply).  Histograms of every parameter and pair over
        `range` (default: the prior box min / max; "data": every parameter's own extent, as the notebook's hist2d(bins=20)),
        np.percentile's percentiles and the median -lower +upper intervals of PlotMCMC.ipynb, computed on the device
        (gpb_chain_marginals, gpb_ppd_summary; the array is uploaded in its own layout and read through its strides)."""
        from .marginals import marginals
        if chain is None:
            if self.chain is False:
                with open(self.mcmc_path, "rb") as f:
                    self.chain = pickle.load(f)["chain"]
            chain = self.chain
        x = np.asarray(chain, dtype=np.float64)
        if x.ndim not in (2, 3):
            raise ValueError("posterior_marginals: chain must be [nwalkers, nsteps, ndim] or [S, ndim], got %s" % (np.shape(chain),))
        names = list(self.pardict) if len(getattr(self, "pardict", ())) == x.shape[-1] else None
        if range is None and np.ndim(bins) == 0:
            if len(self.min) != x.shape[-1]:
                raise ValueError("posterior_marginals: the chain has %d parameters, the prior box %d" % (x.shape[-1], len(self.min)))
            range = np.stack([self.min, self.max], axis=1)
        kw = dict(bins=bins, range=range, pairs=pairs, quantiles=quantiles, names=names, device=self.device or 0)
        if x.ndim == 2:
            return marginals(x, weights=weights, **kw)
        if weights is not None:
            raise ValueError("posterior_marginals: weights go with a flat [S, ndim] particle set")
        discard, thin = int(discard), int(thin)
        if discard < 0 or thin < 1 or x.shape[1] - discard < 1:
            raise ValueError("posterior_marginals: discard >= 0, thin >= 1 and at least one step must remain")
        import torch
        xd = torch.as_tensor(np.require(x, requirements=["C"]), device=torch.device("cuda", self.device or 0))
        return marginals(xd[:, discard::thin], layout="walkers", **kw)

    def _stored_for_curves(self, who, chain, discard, thin, weights):
        """the chain argument of posterior_curves / closure_delta / trace_histogram: (a flat [S, ndim] numpy set, None) or (None,
        the device view [nwalkers, nsteps', ndim] of the stored array without `discard` steps, thinned by `thin`)"""
        if chain is None:
            if self.chain is False:
                with open(self.mcmc_path, "rb") as f:
                    self.chain = pickle.load(f)["chain"]
            chain = self.chain
        x = np.asarray(chain, dtype=np.float64)
        if x.ndim == 2:
            return x, None
        if x.ndim != 3:
            raise ValueError("%s: chain must be [nwalkers, nsteps, ndim] or [S, ndim], got %s" % (who, np.shape(chain)))
        if weights is not None:
            raise ValueError("%s: weights go with a flat [S, ndim] particle set" % who)
        discard, thin = int(discard), int(thin)
        if discard < 0 or thin < 1 or x.shape[1] - discard < 1:
            raise ValueError("%s: discard >= 0, thin >= 1 and at least one step must remain" % who)
        import torch
        xd = torch.as_tensor(np.require(x, requirements=["C"]), device=torch.device("cuda", self.device or 0))
        return None, xd[:, discard::thin]

    def posterior_curves(self, chain=None, discard=0, thin=1, weights=None, **kw):
        """The posterior of the functions zeta/s (T), eta/s (mu_B) and <y_loss> (y_init): PosteriorCurves (curves.py) — median
        and 68 / 95 / 99.7 % bands over ALL samples, PlotMCMC.ipynb's plot_*_posterior — of a stored [nwalkers, nsteps, ndim]
        array (self.chain by default, read from mcmc_path when it is not in memory) without its first `discard` steps and
        thinned by `thin`, or of a flat [S, ndim] particle set with its `weights`.  Selected exactly on the device without
        forming the [S, 100] arrays (gpb_chain_curves); kw (curves, columns, grid, levels, truth, return_values) as
        curves.posterior_curves takes them."""
        from .curves import posterior_curves
        flat, xd = self._stored_for_curves("posterior_curves", chain, discard, thin, weights)
        kw.setdefault("device", self.device or 0)
        if flat is not None:
            return posterior_curves(flat, weights=weights, **kw)
        return posterior_curves(xd, layout="walkers", **kw)

    def closure_delta(self, truth, chain=None, discard=0, thin=1, prior_ranges=None, weights=None, **kw):
        """The closure verdict against the true parameters `truth` [ndim]: ClosureDelta (curves.py) — PlotMCMC.ipynb's Delta_d,
        its per-sample distribution's histogram and quantiles, and every parameter's share — of the stored chain as
        posterior_curves takes it.  prior_ranges [ndim, 2]: default the prior box min / max."""
        from .curves import closure_delta
        flat, xd = self._stored_for_curves("closure_delta", chain, discard, thin, weights)
        if prior_ranges is None:
            prior_ranges = np.stack([self.min, self.max], axis=1)
        nd = (flat if flat is not None else xd).shape[-1]
        kw.setdefault("names", list(self.pardict) if len(getattr(self, "pardict", ())) == nd else None)
        kw.setdefault("device", self.device or 0)
        if flat is not None:
            return closure_delta(flat, truth, prior_ranges, weights=weights, **kw)
        return closure_delta(xd, truth, prior_ranges, layout="walkers", **kw)

    def trace_histogram(self, chain=None, discard=0, thin=1, bins=30, range=None):
        """The walkers' distribution step by step: TraceHistogram (curves.py), PlotMCMC.ipynb's plot_chain_histogram — per
        parameter np.histogram2d(step, value, bins=[nsteps, 30])'s counts — of a stored [nwalkers, nsteps, ndim] array as
        posterior_curves takes it, counted on the device (gpb_chain_trace_hist).  range: default every parameter's extent
        over the chain, as the notebook's call takes it; [ndim, 2] for fixed edges."""
        from .curves import trace_histogram
        flat, xd = self._stored_for_curves("trace_histogram", chain, discard, thin, None)
        if flat is not None:
            raise ValueError("trace_histogram: chain must be [nwalkers, nsteps, ndim] (a flat set has no steps)")
        names = list(self.pardict) if len(getattr(self, "pardict", ())) == xd.shape[-1] else None
        return trace_histogram(xd, bins=bins, range=range, layout="walkers", names=names, device=self.device or 0)

    sens_slab_rows = None                        # most rows of one sensitivity slab (None: sensitivity.slab_rows' rule); same bits

    def sensitivity(self, samples=None, discard=0, thin=1, weights=None):
        """Which data constrain which parameter: PosteriorSensitivity (sensitivity.py) over ALL rows of `samples` — [S, ndim], or
        a stored [nwalkers, nsteps, ndim] array without its first `discard` steps and thinned by `thin`; default self.chain, read
        from mcmc_path when it is not in memory; `weights` [S] go with a flat set.  The observable-by-parameter response matrix of
        examples/SensitivityAnalysis.ipynb (x_j / y_m dy_m / dx_j, there from 2 d finite-difference predictions at one design
        point) with its mean and spread over the posterior, and per emulator the Fisher information J^T C^-1 J, C = the
        emulator's predictive covariance plus its block of expdata_cov, the covariance of the likelihood.  Jacobian, covariance,
        Cholesky solve and the sums run on the device (gpb_emu_predict, gpb_emu_predict_jac, gpb_sens_accumulate); equal inputs
        give equal bits whatever the slab size.  fisher is the Gauss-Newton Hessian of the negative log-likelihood with the
        covariance frozen at each sample, not the full Gaussian Fisher matrix (the 1/2 tr(C^-1 dC C^-1 dC) term is left out).
        NotImplementedError for foreign emulators, a chain sharded over several ranks and an expdata_cov that couples
        emulators; ValueError for wrong shapes, non-finite samples, negative or all-zero weights."""
        from .sensitivity import posterior_sensitivity
        if samples is None:
            if self.chain is False:
                with open(self.mcmc_path, "rb") as f:
                    self.chain = pickle.load(f)["chain"]
            samples = self.chain
        x = np.asarray(samples, dtype=np.float64)
        if x.ndim == 3:
            if weights is not None:
                raise ValueError("sensitivity: weights go with a flat [S, ndim] sample set")
            discard, thin = int(discard), int(thin)
            if discard < 0 or thin < 1 or x.shape[1] - discard < 1:
                raise ValueError("sensitivity: discard >= 0, thin >= 1 and at least one step must remain")
            x = x[:, discard::thin].reshape(-1, x.shape[-1])
        elif x.ndim != 2:
            raise ValueError("sensitivity: samples must be [S, %d] or [nwalkers, nsteps, %d], got %s"
                             % (self.ndim, self.ndim, np.shape(samples)))
        return posterior_sensitivity(self, x, weights=weights)

    gof_slab_rows = None                         # most rows of one goodness-of-fit slab (None: gof.slab_rows' rule); same bits

    def goodness_of_fit(self, samples=None, discard=0, thin=1, weights=None, **kw):
        """Does the calibrated model describe the data, data set by data set: GoodnessOfFit (gof.py) over ALL rows of `samples` —
        [S, ndim], or a stored [nwalkers, nsteps, ndim] array without its first `discard` steps and thinned by `thin`; default
        self.chain, read from mcmc_path when it is not in memory; `weights` [S] go with a flat set.  Per emulator chi2 = dY^T C^-1
        dY with C = the emulator's predictive covariance plus its block of expdata_cov — the covariance of the likelihood, the
        two pieces mvn_loglike computes (src/mcmc.py:23-65) kept apart — its quantiles over the posterior, chi2 per degree of
        freedom (ndf = the number of observables; no parameters are subtracted, the chi2 is the posterior's, not a minimum), the
        closed-form posterior-predictive p-value, the whitened residuals and pulls per observable, the totals over the emulators
        and what the posterior would be without each data set (importance reweighting; its ess says when that has collapsed).
        Predict, Cholesky, p-values and sums run on the device (gpb_emu_predict, gpb_gof_accumulate, gpb_chi2_sf,
        gpb_gof_influence); equal inputs give equal bits whatever the slab size.  kw: quantiles, influence, return_rows, profile
        (gof.posterior_gof).  A coupled expdata_cov: per-emulator marginal checks, the total from the joint matrix, no influence.
        NotImplementedError for foreign emulators and a chain sharded over several ranks; ValueError for wrong shapes,
        non-finite samples, negative or all-zero weights, quantile levels outside [0, 1]."""
        from .gof import posterior_gof
        if samples is None:
            if self.chain is False:
                with open(self.mcmc_path, "rb") as f:
                    self.chain = pickle.load(f)["chain"]
            samples = self.chain
        x = np.asarray(samples, dtype=np.float64)
        if x.ndim == 3:
            if weights is not None:
                raise ValueError("goodness_of_fit: weights go with a flat [S, ndim] sample set")
            discard, thin = int(discard), int(thin)
            if discard < 0 or thin < 1 or x.shape[1] - discard < 1:
                raise ValueError("goodness_of_fit: discard >= 0, thin >= 1 and at least one step must remain")
            x = x[:, discard::thin].reshape(-1, x.shape[-1])
        elif x.ndim != 2:
            raise ValueError("goodness_of_fit: samples must be [S, %d] or [nwalkers, nsteps, %d], got %s"
                             % (self.ndim, self.ndim, np.shape(samples)))
        return posterior_gof(self, x, weights=weights, **kw)

    def loo(self, samples=None, discard=0, thin=1, **kw):
        """Leave-one-out predictive accuracy of the calibration: LooResult (loo.py) over ALL rows of `samples` — [S, ndim], or a
        stored [nwalkers, nsteps, ndim] array without its first `discard` steps and thinned by `thin`; default self.chain, read
        from mcmc_path when it is not in memory.  PSIS-LOO and WAIC per observable (its density given all other observables,
        from the covariance the likelihood factorises) or per data set (kw unit="dataset"), the Pareto khat that says whether
        each estimate can be trusted, the leave-one-out PIT; loo.compare(a, b) ranks two calibrations of the same data.  The
        conditionals, the Pareto fit and the sums run on the device (gpb_loo_pointwise, gpb_psis_loo); equal inputs give equal
        bits whatever the slab size (gof_slab_rows).  kw: unit, pit, return_pointwise, profile (loo.posterior_loo).  Unweighted
        draws only: weights= raises ValueError (resample the particle set).  NotImplementedError for foreign emulators, a chain
        sharded over several ranks, unit="dataset" with a coupled expdata_cov."""
        from .loo import posterior_loo
        if samples is None:
            if self.chain is False:
                with open(self.mcmc_path, "rb") as f:
                    self.chain = pickle.load(f)["chain"]
            samples = self.chain
        x = np.asarray(samples, dtype=np.float64)
        if x.ndim == 3:
            discard, thin = int(discard), int(thin)
            if discard < 0 or thin < 1 or x.shape[1] - discard < 1:
                raise ValueError("loo: discard >= 0, thin >= 1 and at least one step must remain")
            x = x[:, discard::thin].reshape(-1, x.shape[-1])
        elif x.ndim != 2:
            raise ValueError("loo: samples must be [S, %d] or [nwalkers, nsteps, %d], got %s" % (self.ndim, self.ndim, np.shape(samples)))
        return posterior_loo(self, x, **kw)

    def posterior_clusters(self, chain=None, discard=0, thin=1, n_clusters=10, n_init=10, **kw):
        """Representative parameter sets of the posterior: PosteriorClusters (clusters.py) of a stored [nwalkers, nsteps, ndim]
        array — self.chain (default; read from mcmc_path when it is not in memory), a loaded pickle's — without its first
        `discard` steps and thinned by `thin`, or of a flat [S, ndim] particle set (the `chain` of a pocoMC / run_SMC pickle,
        with kw weights=, logl= and num_samples=; discard and thin do not apply).  k-means of the standardised rows on the
        device (gpb_chain_kmeans; the array is uploaded in its own layout and read through its strides) — what
        examples/generate_posterior_clusters.py computes with scikit-learn; kw (init, seed, max_iter, tol, standardize,
        return_labels) as clusters.posterior_clusters takes them.  `.savetxt()` writes the reference's cluster_centers.txt."""
        from .clusters import posterior_clusters
        if chain is None:
            if self.chain is False:
                with open(self.mcmc_path, "rb") as f:
                    self.chain = pickle.load(f)["chain"]
            chain = self.chain
        x = np.asarray(chain, dtype=np.float64)
        if x.ndim not in (2, 3):
            raise ValueError("posterior_clusters: chain must be [nwalkers, nsteps, ndim] or [S, ndim], got %s" % (np.shape(chain),))
        kw.setdefault("names", list(self.pardict) if len(getattr(self, "pardict", ())) == x.shape[-1] else None)
        kw.setdefault("device", self.device or 0)
        if x.ndim == 2:
            return posterior_clusters(x, n_clusters, n_init, **kw)
        discard, thin = int(discard), int(thin)
        if discard < 0 or thin < 1 or x.shape[1] - discard < 1:
            raise ValueError("posterior_clusters: discard >= 0, thin >= 1 and at least one step must remain")
        import torch
        xd = torch.as_tensor(np.require(x, requirements=["C"]), device=torch.device("cuda", kw["device"]))
        return posterior_clusters(xd[:, discard::thin], n_clusters, n_init, layout="walkers", **kw)

    def _stored_for_knn(self, who, chain, discard, thin):
        """the chain argument of information_gain / posterior_divergence — None (self.chain, read from mcmc_path when it is not
        in memory), an array, a tensor or a chain pickle's path — as (samples, layout): a flat [S, ndim] set as it is, a stored
        [nwalkers, nsteps, ndim] array as the device view without its first `discard` steps, thinned by `thin`"""
        import torch
        if chain is None:
            if self.chain is False:
                with open(self.mcmc_path, "rb") as f:
                    self.chain = pickle.load(f)["chain"]
            chain = self.chain
        elif isinstance(chain, (str, os.PathLike)):
            with open(chain, "rb") as f:
                chain = pickle.load(f)["chain"]
        x = chain if hasattr(chain, "data_ptr") else np.asarray(chain, dtype=np.float64)
        if x.ndim == 2:
            return x, "steps"
        if x.ndim != 3:
            raise ValueError("%s: chain must be [nwalkers, nsteps, ndim] or [S, ndim], got %s" % (who, tuple(x.shape)))
        discard, thin = int(discard), int(thin)
        if discard < 0 or thin < 1 or x.shape[1] - discard < 1:
            raise ValueError("%s: discard >= 0, thin >= 1 and at least one step must remain" % who)
        if not hasattr(x, "data_ptr"):
            x = torch.as_tensor(np.require(x, requirements=["C"]), device=torch.device("cuda", self.device or 0))
        return x[:, discard::thin], "walkers"

    def _score_device(self, rows):
        """grad log posterior at the rows [n, ndim] (a float64 cuda tensor), as a device tensor: gpb_chain_logpost_grad in slabs
        of grad_slab_rows, nothing brought to the host.  A row's numbers are those of log_posterior(rows, return_grad=True)."""
        if not self._native():
            raise NotImplementedError("log-posterior gradients need every emulator of the chain to be this package's Emulator "
                                      "(foreign emulators have no device derivatives)")
        import torch
        from . import _native as nat
        if rows.dim() != 2 or rows.shape[1] != self.ndim:
            raise ValueError("the rows have %d columns, the chain has %d parameters" % (rows.shape[-1], self.ndim))
        dev = torch.device("cuda", self.device)
        engs, arr, nemu = self._contexts()
        e0 = engs[0]
        lo_dev, hi_dev = self._box(dev)
        per_row = max(8 * e._ngp * e._X_train.shape[0] for e in self.emuList)
        slab = int(min(max((4 << 30) // per_row, 1024), self.grad_slab_rows)) // 128 * 128
        n = int(rows.shape[0])
        grad = torch.empty((n, self.ndim), dtype=torch.float64, device=dev)
        ll = torch.empty(min(n, slab), dtype=torch.float64, device=dev)
        for i0 in range(0, n, slab):
            Xd = rows[i0:i0 + slab].contiguous()
            k = int(Xd.shape[0])
            e0._ck(e0.lib.gpb_chain_logpost_grad(arr, nemu, nat.ptr(Xd), k, nat.ptr(ll), nat.ptr(grad[i0:i0 + k]), nat.ptr(lo_dev),
                                                 nat.ptr(hi_dev), float(-np.inf), EXTRA_STD_CONST))
        return grad

    def _stein_rows(self, who, chain, discard, thin):
        """the rows [S, ndim] (a float64 cuda tensor, memory order of the chain argument) and their scores"""
        import torch
        x, _ = self._stored_for_knn(who, chain, discard, thin)
        if x.shape[-1] > 64:
            raise ValueError("%s: %d parameters, at most 64" % (who, x.shape[-1]))
        if not hasattr(x, "data_ptr"):
            x = torch.as_tensor(np.require(x, requirements=["C"]), device=torch.device("cuda", self.device or 0))
        rows = x.to(torch.float64).reshape(-1, x.shape[-1])
        return rows, self._score_device(rows)

    def stein_thin(self, chain=None, m=100, discard=0, thin=1, **kw):
        """The m parameter sets at which to run the full model again: SteinThinning (thinning.py) of a stored [nwalkers, nsteps,
        ndim] array — self.chain (default; read from mcmc_path when it is not in memory), an array, a tensor or a chain pickle's
        path — without its first `discard` steps and thinned by `thin`, or of a flat [S, ndim] set (SMC or pocoMC particles: no
        weights are needed).  Greedily the m rows whose empirical measure has the smallest kernel Stein discrepancy to the
        posterior: burn-in is dropped by itself, the points are rows of the chain, `.savetxt()` writes the format of the
        reference's cluster_centers.txt.  The scores come from gpb_chain_logpost_grad in slabs of grad_slab_rows and stay on the
        device, where the m passes run (gpb_stein_thin).  The prior box self.min / self.max is taken out by the logit
        transform; kw (preconditioner, transform) as thinning.stein_thin takes them.  ValueError for more than 64 parameters."""
        from .thinning import stein_thin
        rows, g = self._stein_rows("stein_thin", chain, discard, thin)
        kw.setdefault("names", list(self.pardict) if len(getattr(self, "pardict", ())) == rows.shape[-1] else None)
        kw.setdefault("lo", self.min)
        kw.setdefault("hi", self.max)
        return stein_thin(rows, g, m, **kw)

    def ksd(self, chain=None, discard=0, thin=1, **kw):
        """How well does a point set represent the posterior?  SteinDiscrepancy (thinning.py) of a chain as stein_thin takes it,
        or of ARBITRARY rows [S, ndim] — posterior_clusters(...).centers, a SteinThinning's points, another sampler's chain: the
        kernel Stein discrepancy needs only the rows and the score at them, so sets of any origin are compared on one scale
        (give them the same explicit preconditioner=).  n^2 pair evaluations on the device (gpb_stein_ksd); kw (preconditioner,
        transform, splits, return_rows) as thinning.ksd takes them."""
        from .thinning import ksd
        rows, g = self._stein_rows("ksd", chain, discard, thin)
        kw.setdefault("lo", self.min)
        kw.setdefault("hi", self.max)
        return ksd(rows, g, **kw)

    def information_gain(self, chain=None, discard=0, thin=1, k=8, **kw):
        """How much did the data teach us?  InformationGain (divergence.py) of a stored [nwalkers, nsteps, ndim] array —
        self.chain (default; read from mcmc_path when it is not in memory), a loaded pickle's — without its first `discard`
        steps and thinned by `thin`, or of a flat [S, ndim] set, against the uniform prior on the box self.min / self.max: the
        Kullback-Leibler divergence from prior to posterior in the whole parameter space (nearest-neighbour entropy for every k
        up to `k`, brute force on the device: gpb_chain_knn) and per parameter (histograms).  Thin by about the autocorrelation
        time: repeated rows distort the estimate (duplicate_fraction).  kw (bins, weights, splits) as
        divergence.information_gain takes them."""
        from .divergence import information_gain
        x, layout = self._stored_for_knn("information_gain", chain, discard, thin)
        if len(self.min) != x.shape[-1]:
            raise ValueError("information_gain: the chain has %d parameters, the prior box %d" % (x.shape[-1], len(self.min)))
        kw.setdefault("names", list(self.pardict) if len(getattr(self, "pardict", ())) == x.shape[-1] else None)
        kw.setdefault("device", self.device or 0)
        return information_gain(x, self.min, self.max, k=k, layout=layout, **kw)

    def posterior_divergence(self, other, chain=None, discard=0, thin=1, **kw):
        """Do two calibrations agree?  PosteriorComparison (divergence.py) of this object's chain (`chain`, discard, thin as
        information_gain takes them) against `other` — an array, a tensor or a chain pickle's path, [nwalkers, nsteps, ndim]
        (cut by the same discard and thin) or flat [S, ndim] — on the prior box self.min / self.max: D(A || B) and D(B || A) in
        the whole parameter space (gpb_chain_knn), per parameter and pair the Jensen-Shannon divergence of the histograms and the
        shift of the medians.  kw (k, bins, pairs, splits) as divergence.posterior_divergence takes them."""
        from .divergence import posterior_divergence
        xa, la = self._stored_for_knn("posterior_divergence", chain, discard, thin)
        xb, lb = self._stored_for_knn("posterior_divergence", other, discard, thin)
        if len(self.min) != xa.shape[-1] or xb.shape[-1] != xa.shape[-1]:
            raise ValueError("posterior_divergence: the chains have %d and %d parameters, the prior box %d"
                             % (xa.shape[-1], xb.shape[-1], len(self.min)))
        kw.setdefault("names", list(self.pardict) if len(getattr(self, "pardict", ())) == xa.shape[-1] else None)
        kw.setdefault("device", self.device or 0)
        return posterior_divergence(xa, xb, self.min, self.max, layout=la, layout_b=lb, **kw)

    def expected_information_gain(self, samples=None, discard=0, thin=1, weights=None, planned_error=None, groups=None,
                                  n_outer=8192, seed=None, **kw):
        """Which data set, measured to which precision, is expected to constrain the parameters most?  EIGResult (eig.py): the
        expected information gain — the mutual information between the parameters and a planned measurement, in nats — of
        every emulator's observables alone and of all together, over `samples`: [S, ndim], or a stored [nwalkers, nsteps, ndim]
        array without its first `discard` steps and thinned by `thin`; default self.chain, read from mcmc_path when it is not in
        memory; `weights` [S] go with a flat set.  The stored chain gives the gain expected on top of the present posterior;
        self.random_pos(n) gives the prior's, to set beside information_gain (what the data at hand realised).
        Identical rows are collapsed into one sample with their summed weight first.  One predict pass writes means and
        predictive variances observable-major (gpb_emu_predict_diag); n_outer measurements are simulated from samples drawn by
        weight (np.random.default_rng(seed)) with the variance var + planned_error^2 (planned_error [nobs]: default
        sqrt(diag(expdata_cov)), the errors of the data at hand), and the log-likelihood of every one under every sample goes
        through the fp64 matrix pipe with an online log-sum-exp (gpb_eig_simulate, gpb_eig_lse).  groups: default the emulators
        in emuList order ("emulator0", ...), then "all"; else a dict name -> (c0, c1) of contiguous observable ranges.
        `lower` (prior-contrastive, biased low, saturates at ln S: a warning when within 1 nat) and `upper` (leave-one-out
        nested Monte Carlo, biased high) bracket the value in expectation.  NOT solved here: the covariance is diagonal — the
        PCA truncation term and an expdata_cov that couples observables are ignored —, and the number is the gain under the
        emulator's own model of its error.
        NotImplementedError for foreign emulators and a chain sharded over several ranks; ValueError for wrong shapes,
        non-finite samples, bad weights and fewer than 2 distinct samples."""
        from .eig import chain_expected_information_gain
        return chain_expected_information_gain(self, samples, discard, thin, weights, planned_error, groups, n_outer, seed, **kw)

    def propose_design(self, n_new, candidates, reference=None, weights=None, return_scores=False, candidate_error=None):
        """Where should the next n_new model runs go, for this calibration?  Emulator.propose_design over all emulators of
        emuList at once (gpb_chain_design_run): one run yields every observable, so the pick is common — the score of a
        candidate is the sum of the emulators' scores in emuList order, each emulator seeing the points through its own
        parameter map.  Observable m weighs 1 / expdata_cov[m, m]: variance in units of the experimental variance.

        candidates [C, ndim]; those outside the open prior box are never picked.  reference [R, ndim] (default: the candidates)
        is typically a set of posterior samples, weights [R] their weights (default uniform).  Returns a DesignProposal.
        candidate_error [C, nobs of all emulators] (optional): the candidates' statistical errors, its columns split per emulator
        in emuList order (Emulator.propose_design); None: each emulator's own default.
        NotImplementedError for foreign emulators and for exp_and_cov_diagonal emulators (their design variance is that of the
        log-observable, which the experimental variance does not measure)."""
        from .emulator import DesignProposal, _design_inputs
        from .engine import design_run
        if not self._native():
            raise NotImplementedError("propose_design needs every emulator of the chain to be this package's Emulator (foreign "
                                      "emulators expose no GP state to condition)")
        if any(e.exp_and_cov_diagonal_ for e in self.emuList):
            raise NotImplementedError("propose_design: an exp_and_cov_diagonal emulator's design variance is that of the "
                                      "log-observable; the experimental variance is in the observable's units")
        import torch
        n_new, cand, ref, w = _design_inputs("propose_design", n_new, candidates, reference, weights, self.ndim)
        inside = np.all((cand > self.min) & (cand < self.max), axis=1)
        if n_new > np.count_nonzero(inside):
            raise ValueError("propose_design: n_new = %d, but only %d candidates lie inside the prior box"
                             % (n_new, np.count_nonzero(inside)))
        u = 1.0 / np.diag(self.expdata_cov)
        if u.shape[0] != sum(e.nobs for e in self.emuList):
            raise ValueError("emulators provide %d observables, experiment has %d" % (sum(e.nobs for e in self.emuList), u.shape[0]))
        dev = torch.device("cuda", self.device)
        cand_dev, ref_dev, w_dev = (torch.as_tensor(a, device=dev) for a in (cand, ref, w))
        eligible = torch.as_tensor(inside.astype(np.uint8), device=dev)
        if candidate_error is not None:
            candidate_error = np.asarray(candidate_error, dtype=np.float64)
            if candidate_error.shape != (cand.shape[0], u.shape[0]):
                raise ValueError("propose_design: candidate_error must be [%d candidates, %d observables], got %s"
                                 % (cand.shape[0], u.shape[0], candidate_error.shape))
        engs, variance0, i0 = [], 0.0, 0
        try:
            for emu in self.emuList:
                engs.append(emu._engine_ready())
                ce = None if candidate_error is None else candidate_error[:, i0:i0 + emu.nobs]
                _, v0 = emu._design_begin(cand_dev, ref_dev, w_dev, emu._design_gp_weights(u[i0:i0 + emu.nobs]),
                                          emu._design_candidate_noise(ce, cand.shape[0]))
                variance0 += v0
                i0 += emu.nobs
            picks, gain, scores = design_run(engs, n_new, eligible, return_scores)
        finally:
            for g in engs:
                g.design_end()
        return DesignProposal(cand[picks], picks, gain, variance0, scores)

    grad_slab_rows = 1 << 14                     # most rows of one gradient evaluation (a row's numbers do not depend on it)

    def _log_prob_grad(self, X, outside):
        """(lp[m], grad[m, ndim]): lp bit for bit what _log_prob gives, grad in fp64 (gpb_chain_logpost_grad); rows outside the
        prior box get a zero gradient, rows whose covariance block is not positive definite NaN in both."""
        if not self._native():
            raise NotImplementedError("log-posterior gradients need every emulator of the chain to be this package's Emulator "
                                      "(foreign emulators have no device derivatives)")
        import torch
        from . import _native as nat
        X = np.array(X, ndmin=2, dtype=np.float64)
        if X.shape[1] != self.ndim:
            raise ValueError("X has %d columns, the chain has %d parameters" % (X.shape[1], self.ndim))
        dev = torch.device("cuda", self.device)
        engs, arr, nemu = self._contexts()
        e0 = engs[0]
        lo_dev, hi_dev = self._box(dev)
        # slabs: the gradient keeps beta = K^-1 k* ([P, rows, N] doubles) per emulator besides the predict workspaces
        per_row = max(8 * e._ngp * e._X_train.shape[0] for e in self.emuList)
        slab = int(min(max((4 << 30) // per_row, 1024), self.grad_slab_rows)) // 128 * 128
        lp = np.empty(X.shape[0])
        grad = np.empty(X.shape)
        for i0 in range(0, X.shape[0], slab):
            Xd = torch.as_tensor(np.ascontiguousarray(X[i0:i0 + slab]), device=dev)
            n = Xd.shape[0]
            ll = torch.empty(n, dtype=torch.float64, device=dev)
            gd = torch.empty((n, self.ndim), dtype=torch.float64, device=dev)
            e0._ck(e0.lib.gpb_chain_logpost_grad(arr, nemu, nat.ptr(Xd), n, nat.ptr(ll), nat.ptr(gd), nat.ptr(lo_dev),
                                                 nat.ptr(hi_dev), float(outside), EXTRA_STD_CONST))
            if not self.use_chain_call:              # (the A/B switch: the value from the per-emulator sequence)
                ll = self.log_prob_device(Xd, outside=outside)
            lp[i0:i0 + n] = ll.cpu().numpy()
            grad[i0:i0 + n] = gd.cpu().numpy()
        return lp, grad

    def log_likelihood(self, X, extra_std_prior_scale=0.001, finite=False, return_grad=False):
        """src/mcmc.py:188-222 (pocoMC calls it with finite=True).  return_grad=True: (lp[m], grad[m, ndim]), the tuple the
        reference's PTLMC takes from a logpostfunc (src/mcmc.py:446-453)."""
        outside = -1e300 if finite else -np.inf
        if return_grad:
            return self._log_prob_grad(X, outside)
        return self._log_prob(X, outside)

    def log_posterior(self, X, extra_std_prior_scale=.05, return_grad=False):
        """src/mcmc.py:261-299 (the function emcee samples).  return_grad=True: (lp[m], grad[m, ndim]) — hand
        functools.partial(chain.log_posterior, return_grad=True) to a gradient-based sampler (PTLMC, src/mcmc.py:446-453)."""
        if return_grad:
            return self._log_prob_grad(X, -np.inf)
        return self._log_prob(X, -np.inf)

    def find_map(self, nstarts=32, seed=None, X0=None):
        """Maximum a posteriori search: nstarts L-BFGS-B minimisations of -log_posterior from uniform draws in the prior box
        (or from the rows of X0), run in lock-step — every round of objective calls is ONE batched device evaluation of
        value and gradient for all searches still running (emulator._batched_lbfgsb, the driver of the hyper-parameter
        searches; each search is scipy.optimize.minimize(method="L-BFGS-B", jac=True) bit for bit).  The box is open and
        L-BFGS-B evaluates on its bounds: the bounds are the box shrunk by 1e-9 (max - min).
        Returns (X_opt[n, ndim], lp_opt[n]) sorted by descending lp."""
        from .emulator import _batched_lbfgsb
        if X0 is None:
            rng = np.random.default_rng(seed)
            X0 = rng.uniform(self.min, self.max, (int(nstarts), self.ndim))
        X0 = np.array(X0, ndmin=2, dtype=np.float64)
        eps = 1e-9 * (self.max - self.min)
        bounds = np.stack([self.min + eps, self.max - eps], axis=1)
        chain = self

        class _Objective:             # the interface _batched_lbfgsb drives: maximises .lml, i.e. minimises -lp
            @staticmethod
            def lml(x, eval_gradient=True):
                return chain.log_posterior(x, return_grad=True)

        x, f = _batched_lbfgsb(_Objective, X0, bounds)
        lp = -np.asarray(f, dtype=np.float64)
        order = np.argsort(-lp, kind="stable")
        return x[order], lp[order]

    def log_likelihood_point_by_point(self, X, extra_std_prior_scale=0.001):
        """Same values as the reference's per-row loop (src/mcmc.py:225-258), in one batch."""
        return self._log_prob(np.asarray(X), -np.inf)

    def compute_log_likelihood_for_chain(self, output_path="./mcmc/log_likelihood.pkl"):
        """src/mcmc.py:729-749."""
        if self.chain is False:
            with open(self.mcmc_path, "rb") as f:
                self.chain = pickle.load(f)["chain"]
        ll = self.log_likelihood_point_by_point(self.chain.reshape(-1, self.ndim))
        ll = ll.reshape(self.chain.shape[0], self.chain.shape[1])
        with open(output_path, "wb") as f:
            pickle.dump({"log_likelihood": ll}, f)

    # ------------------------------------------------------------------ samplers
    def run_mcmc(self, nsteps=500, nburnsteps=None, nwalkers=None, status=None, nthin=10,
                 skip_initial_state_check=False, seed=None):
        """Affine-invariant ensemble sampling with the reference's schedule (src/mcmc.py:345-426):
        resume from an existing chain pickle, else two-stage burn-in with re-seeding at the
        `nwalkers` best unique log-probabilities, then production; thinned chain appended to
        `{'chain': [nwalkers, nsteps/nthin, ndim]}`.  The stretch move runs on the device
        (sampler.StretchSampler) instead of emcee.  After `shard_over(WalkerSharding())` the walkers are sharded over the
        GPUs of the group (collective: every rank calls it with the same arguments)."""
        from .sampler import StretchSampler
        # Several GPUs (chain.shard_over(WalkerSharding()), one process per GPU, every rank makes this call): the sampler runs
        # replicated and walker-sharded — rank 0's start positions, seed and chain file are everybody's (broadcast: numpy's
        # global RandomState and a file system need not agree between processes), every half-step's rows are evaluated in shares
        # with one all-gather (in-stream RCCL when the group's backend is nccl), every rank ends with the same chain, rank 0
        # writes the pickle.  The samples are those of the single-GPU run with the same seed and start, bit for bit.
        sh = self.sharding if (self.sharding is not None and getattr(self.sharding, "world", 1) > 1) else None
        root = sh is None or sh.rank == 0
        share = (lambda obj: obj) if sh is None else sh.broadcast_object
        chain_data = {}
        failed = None
        if root:
            try:
                with open(self.mcmc_path, "rb") as f:
                    chain_data = pickle.load(f)
            except FileNotFoundError:
                pass
            except Exception as e:          # an unreadable chain file: the other ranks must not wait for rank 0 in a collective
                if sh is None:
                    raise
                failed = "%s: %s" % (type(e).__name__, e)
        failed = share(failed)
        if failed:
            raise RuntimeError("run_mcmc: rank 0 could not read %s (%s)" % (self.mcmc_path, failed))
        burn = share("chain" not in chain_data)
        if nburnsteps is None or nwalkers is None:
            log.error("must specify nburnsteps and nwalkers to start chain")
            return
        if sh is not None:
            if seed is None:
                seed = int(np.random.SeedSequence().generate_state(1, dtype=np.uint64)[0])
            seed = share(int(seed))
            if sh.direct is None and sh.backend() == "nccl" and self._native():
                sh.try_direct(self.emuList[0]._engine_ready())        # collective; torch.distributed's all-gather stays otherwise
        sampler = StretchSampler(self, nwalkers, seed=seed, sharding=sh)
        if burn:
            nburn0 = nburnsteps // 2
            sampler.run(share(self.random_pos(nwalkers) if root else None), nburn0, status=status)
            flat_lp = sampler.lnprobability.reshape(-1)
            flat_x = sampler.chain.reshape(-1, self.ndim)
            X0 = flat_x[np.unique(flat_lp, return_index=True)[1][-nwalkers:]]
            sampler.reset()
            X0 = sampler.run(X0, nburnsteps - nburn0, status=status)
            sampler.reset()
        else:
            X0 = share(chain_data["chain"][:, -1, :] if root else None)
        sampler.run(X0, nsteps, status=status)
        thinned = sampler.chain[:, ::nthin, :]
        if "chain" in chain_data:
            chain_data["chain"] = np.concatenate((chain_data["chain"], thinned), axis=1)
        else:
            chain_data["chain"] = thinned
        self.chain = chain_data["chain"] if root else thinned
        self.acceptance_fraction = sampler.acceptance_fraction
        if root:
            try:
                with open(self.mcmc_path, "wb") as f:
                    pickle.dump(chain_data, f)
            except Exception as e:
                if sh is None:
                    raise
                failed = "%s: %s" % (type(e).__name__, e)
        if sh is not None:
            self.chain = share(self.chain if root else None)          # (also: nobody returns before the file is written)
            failed = share(failed)
            if failed:
                raise RuntimeError("run_mcmc: rank 0 could not write %s (%s)" % (self.mcmc_path, failed))

    def pseudo_data(self, truths, noise=False, seed=None):
        """Closure-test data: the emulators' mean at truths [K, ndim] (_predict), [K, nobs] — the model's own output in the
        experiment's place, examples/ClosureTest.ipynb.  noise=True adds one draw per set from expdata_cov
        (np.random.default_rng(seed))."""
        from .closure import pseudo_data
        return pseudo_data(self, truths, noise=noise, seed=seed)

    def run_closure(self, data, truths=None, nsteps=500, nburnsteps=None, nwalkers=None, nthin=10, seed=None):
        """A closure study in one resident run: the chain calibrated against every row of data [K, nobs] (pseudo_data) with the
        shared error model expdata_cov — K independent ensembles of `nwalkers` walkers whose proposals form one batch per
        half-step (closure.ClosureSampler; gpb_chain_like_sets, gpb_chain_emcee_sets_run).  run_mcmc's recipe per set: half the
        burn-in from random_pos, the walkers repositioned to the set's `nwalkers` most likely distinct points, the second half,
        then `nsteps` of production thinned by `nthin`.  Set k's samples are, bit for bit, those of StretchSampler(seed =
        result seeds[k]) on a chain whose experiment is data[k].  Returns a closure.ClosureResult — chain [K, nwalkers,
        nsteps / nthin, ndim], lnprobability, acceptance, data and, with truths [K, ndim], the truth's rank in every posterior,
        coverage(level), rank_histogram(bins), delta [K] and delta_per_parameter (closure_delta per set); save(path) and
        write_chain(k, path) write pickles.  Nothing is written to mcmc_path, and the chain's own experiment stays installed.
        NotImplementedError for foreign emulators, an emulator outside PCA mode or with more than 16 GPs, an expdata_cov that
        couples emulators and a sharded chain; ValueError for a data width other than nobs, truths of another shape, odd
        nwalkers, missing nburnsteps / nwalkers."""
        from .closure import run_closure
        return run_closure(self, data, truths=truths, nsteps=nsteps, nburnsteps=nburnsteps, nwalkers=nwalkers, nthin=nthin,
                           seed=seed)

    def samplerPTLMC(self, logpostfunc, draw_func, theta0=None, numtemps=32, numchain=16, sampperchain=400, maxtemp=30,
                     nstartparameters=1000, seed=None):
        """Parallel-tempered Langevin Monte Carlo (surmise 0.2.1's PTLMC as the reference carries it, src/mcmc.py:431-676),
        with the step loop resident on the device (ptlmc.PTLMCSampler, gpb_chain_ptlmc_run).  `logpostfunc` must be this
        chain's log_posterior or log_likelihood, or a functools.partial of either setting return_grad (and finite): the loop
        evaluates the chain itself.  A tuple return selects the Langevin branch (target acceptance 0.60), otherwise the
        random-walk branch (0.25).  Returns {'theta': [numchain, sampperchain, ndim]}, the untempered rungs.  `seed` keys
        np.random.default_rng for the host draws and the device's Philox streams; the deviations from the reference are
        listed in gpbayestools_hic_amd/ptlmc.py.  Raises TypeError for any other logpostfunc, ValueError when there are fewer
        start rows than rungs, NotImplementedError for foreign emulators or a sharded chain."""
        from .ptlmc import sampler_ptlmc
        return sampler_ptlmc(self, logpostfunc, draw_func, theta0=theta0, numtemps=numtemps, numchain=numchain,
                             sampperchain=sampperchain, maxtemp=maxtemp, nstartparameters=nstartparameters, seed=seed)

    def run_HMC(self, nsteps=500, nwarmup=200, nchains=1024, nleapfrog=8, nthin=1, seed=None, *, reseed=True):
        """Hamiltonian Monte Carlo over `nchains` independent chains, resident on the device (hmc.HMCSampler,
        gpb_chain_hmc_run, `DESIGN.md` §30): a diagonal metric, `nleapfrog` leapfrog steps per trajectory, the prior box as
        reflecting walls, one batched gradient of the log-posterior per leapfrog.  Resumes from the last column of an existing
        `{'chain': ...}` pickle as run_mcmc does (with the step size and metric of this object's previous run_HMC where there
        was one, after a warm-up from the resumed positions otherwise); else the chains start at random_pos (drawn from
        np.random.default_rng when a seed is given) and `nwarmup` steps adapt the step size and the metric, with the chains
        re-seeded at the most likely eighth of them half way (hmc.warm_start: independent chains do not pull each other out
        of a local maximum, and run_mcmc re-seeds its walkers for the same reason).  That discards chains that sit in genuine
        minor modes: `reseed=False` (keyword only) warms up without it, and a warm-up that would leave fewer than 10 steps
        behind the re-seeding is not re-seeded (a warning says so).  `nsteps`
        production steps thinned by `nthin` are appended to `{'chain': [nchains, nsteps / nthin, ndim]}`; sets self.chain,
        self.acceptance_fraction and self.hmc_sampler (the sampler: step_size, inv_metric, n_divergent, n_escaped, diagnostics()
        and the other shortcuts of the stretch-move sampler) and returns the sampler.  NotImplementedError for foreign emulators
        and for a sharded chain; ValueError for nchains outside 1 .. 1048576, nleapfrog outside 1 .. 1024, more than 256
        parameters, nsteps < 1, nwarmup < 0, nthin < 1 and a pickle whose chain has another shape."""
        from .hmc import run_hmc
        return run_hmc(self, nsteps=nsteps, nwarmup=nwarmup, nchains=nchains, nleapfrog=nleapfrog, nthin=nthin, seed=seed,
                       reseed=reseed)

    def tempexchange(self, lpostf, temps, iters=1):
        """The temperature exchange of surmise's PTLMC (src/mcmc.py:679-692) on the host with numpy's global generator: iters
        sweeps of len(lpostf) random neighbour picks rt in [1, T), each swapping rungs rt - 1 and rt by the parallel-tempering
        rule.  Returns the new order.  (The device loop runs the same rule on Philox draws, csrc/gpb_ptlmc.hip.)"""
        n = lpostf.shape[0]
        order = np.arange(0, n)
        for _ in range(iters):
            for rt in np.random.choice(range(1, n), n):
                dtemp = 1 / temps[rt - 1] - 1 / temps[rt]
                if (lpostf[order[rt]] - lpostf[order[rt - 1]]) * dtemp > np.log(np.random.uniform(size=1)):
                    order[rt - 1], order[rt] = order[rt], order[rt - 1]
        return order

    def run_MCMC_PTLMC(self, nsteps=500, nwalkers=16, ntemps=50, maxtemp=100, nstartparameters=1000, *, seed=None,
                       gradient=False):
        """src/mcmc.py:696-726: samplerPTLMC with numchain = nwalkers, numtemps = ntemps, sampperchain = nsteps and start rows
        drawn uniformly in the prior box; writes {'chain': [nwalkers, nsteps, ndim]} to mcmc_path and sets self.chain.
        gradient=False samples log_posterior as the reference does; gradient=True takes the Langevin branch
        (functools.partial(self.log_posterior, return_grad=True))."""
        import functools
        log.info("Starting MCMC ...")
        draws = np.random.default_rng(None if seed is None else [int(seed), 1])
        result = self.samplerPTLMC(functools.partial(self.log_posterior, return_grad=True) if gradient else self.log_posterior,
                                   lambda n: draws.uniform(self.min, self.max, (n, self.ndim)), theta0=None, numtemps=ntemps,
                                   numchain=nwalkers, sampperchain=nsteps, maxtemp=maxtemp,
                                   nstartparameters=nstartparameters, seed=seed)
        self.chain = result["theta"].reshape((nwalkers, nsteps, self.ndim))
        log.info("Writing MCMC chains to file ...")
        with open(self.mcmc_path, "wb") as f:
            pickle.dump({"chain": self.chain}, f)

    def run_pocoMC(self, n_effective=1000, n_active=250, n_prior=2000, sample="tpcn", n_max_steps=200,
                   random_state=42, n_total=5000, n_evidence=5000, pool=None, prior=None):
        """pocoMC driver with the reference's call shape and output schema (src/mcmc.py:752-819);
        the likelihood callback is this class's device-backed log_likelihood(finite=True)."""
        import pocomc
        from scipy.stats import uniform
        if pool is not None:
            # the reference hands `pool=12` to pocoMC, whose workers are FORKED copies of this Chain
            # (src/mcmc.py:775-776, 798-804; examples/RunBayesianAnalysis.ipynb:85).  Here the whole 8192-row batch is
            # one device call (vectorize=True); forked workers could not use the parent's GPU context anyway.
            log.info("run_pocoMC: pool=%r ignored — likelihood batches are already vectorised on the device", pool)
            pool = None
        if prior is None:
            prior = pocomc.Prior([uniform(self.min[i], self.max[i] - self.min[i]) for i in range(self.ndim)])
        elif self.ndim != prior.dim:
            raise ValueError("prior.dim does not match the model parameter space")
        sampler = pocomc.Sampler(prior=prior, likelihood=self.log_likelihood, likelihood_kwargs={"finite": True},
                                 n_effective=n_effective, n_active=n_active, n_prior=n_prior, sample=sample,
                                 n_max_steps=n_max_steps, random_state=random_state, vectorize=True, pool=pool)
        sampler.run(n_total=n_total, n_evidence=n_evidence)
        samples, weights, logl, logp = sampler.posterior()
        logz, logz_err = sampler.evidence()
        with open(self.mcmc_path, "wb") as f:
            pickle.dump({"chain": samples, "weights": weights, "logl": logl, "logp": logp, "logz": logz,
                         "logz_err": logz_err}, f)

    def run_SMC(self, n_particles=4096, ess_fraction=0.5, nmcmc=20, max_stages=200, seed=None):
        """A tempered sequential Monte Carlo sampler resident on the device, with an evidence estimate (smc.SMCSampler,
        gpb_chain_smc_reweight / gpb_chain_smc_move, `DESIGN.md` §12).  It runs the outer algorithm pocoMC runs — adaptive
        tempering from the uniform prior box to the posterior at an effective sample size of ess_fraction * n_particles,
        systematic resampling, nmcmc Metropolis moves per stage, a running log-evidence — but it is not pocoMC: there is no
        normalizing flow (the Cholesky factor of the particle covariance preconditions the random-walk moves) and no
        reweighting of earlier stages' particles.  The defaults are choices, not tuned values.
        Writes the six keys of the reference's pocoMC pickle (src/mcmc.py:816-819) to mcmc_path: chain [n_particles, ndim]
        (equally weighted posterior samples), weights (uniform), logl (log_likelihood(chain, finite=True), bit for bit), logp
        (-ln of the box volume), logz, and logz_err = NaN — a single run does not estimate its own error; run several seeds
        for one.  Returns the same dict plus `beta` (the ladder, ending at exactly 1.0) and `acceptance` (per stage).
        `seed` keys np.random.default_rng for the start particles and the device's Philox streams.  Raises
        NotImplementedError for foreign emulators or a sharded chain, RuntimeError when the particle covariance is not
        positive definite at a stage boundary or beta has not reached 1 after max_stages stages."""
        from .smc import run_smc
        out = run_smc(self, n_particles=n_particles, ess_fraction=ess_fraction, nmcmc=nmcmc, max_stages=max_stages, seed=seed)
        with open(self.mcmc_path, "wb") as f:
            pickle.dump({k: out[k] for k in ("chain", "weights", "logl", "logp", "logz", "logz_err")}, f)
        return out
