"""
GPEngine — thin Python handle on one gpb_ctx (include/gpbayes.h): the P independent GPs of one
emulator resident in HBM, plus its observable transform and likelihood block.
Host code only moves arguments; every number is produced by the HIP kernels.
"""
import ctypes as C
import itertools
import os

import numpy as np

from . import _native as nat

KERNEL_IDS = {"RBF": 0, "Matern": 1, "Matern15": 1, "Matern25": 2}
MODE_PCA, MODE_NO_PCA, MODE_EXPDIAG, MODE_NO_PCA_EXPDIAG = 0, 1, 2, 3


class NotPositiveDefinite(np.linalg.LinAlgError):
    pass


def _is_torch(x):
    return hasattr(x, "data_ptr") and hasattr(x, "is_cuda")


_SERIAL = itertools.count(1)

# gpb_ctx_option 51, the arithmetic of V = L^-1 K*^T: 0 the fp64 kernel, 1 six int8 digit planes where their rule admits the
# context, 2 six planes with the rule off (accuracy probes), 3 seven planes (fp64-accurate): the library's default
PREDICT_SLICED_DEFAULT = 3
_PREDICT_SLICED_ENV = {"0": 0, "fp64": 0, "1": 1, "int8": 1, "2": 2, "3": 3, "fp64-int8": 3}


def predict_sliced_from_env():
    """the option-51 value GPB_PREDICT_SLICED asks every engine of the process for ("0" / "fp64": the fp64 kernel, "1" / "int8":
    six digit planes, "2": six planes with the rule off, "3" / "fp64-int8": seven planes), None when it is unset, empty or not one
    of these (a warning says so: a typo must not fail every GPEngine() nor silently run another arithmetic than asked for)"""
    v = os.environ.get("GPB_PREDICT_SLICED", "").strip().lower()
    if not v:
        return None
    if v not in _PREDICT_SLICED_ENV:
        import warnings
        warnings.warn("GPB_PREDICT_SLICED=%r is not one of %s: ignored" % (v, sorted(_PREDICT_SLICED_ENV)), RuntimeWarning)
        return None
    return _PREDICT_SLICED_ENV[v]


class GPEngine:
    def __init__(self, device=0, stream="torch", debug=None):
        """stream: "torch" = enqueue on torch's current stream of `device` (one ordered queue
        shared with torch copies and collectives), None = private stream, or a hipStream_t.
        debug: True binds libgpbayes_debug.so (test hooks, kernel variants); None = the process default (the product library
        unless GPB_DEBUG_LIB=1 or inside _native.debug_library())."""
        self.lib = nat.load(debug)
        if self.lib.gpb_device_count() <= 0:
            raise nat.GPBError("no HIP device visible: the gfx950 kernels cannot run (no CPU fallback)")
        h = nat.VP()
        rc = self.lib.gpb_ctx_create(int(device), None, C.byref(h))
        if rc != 0:
            raise nat.GPBError(f"gpb_ctx_create failed ({rc})")
        self._pid = os.getpid()          # device state does not survive a fork: see _check_pid
        self._h = h
        self.serial = next(_SERIAL)      # which context is this? (never reused within the process, unlike id() of a freed object)
        self.device = int(device)
        self._follow_torch = stream == "torch"
        self._stream = None
        if self._follow_torch:
            self._track_stream()
        elif stream is not None:
            self._ck(self.lib.gpb_ctx_set_stream(self.h, nat.VP(int(stream))))
        self.N = self.d = self.P = self.M = 0
        self.mode = None                         # the transform's mode (set_transform)
        # option key 51 (csrc/gpb_sliced.hip): the context starts at PREDICT_SLICED_DEFAULT (seven int8 digit planes); the
        # GPB_PREDICT_SLICED environment hook gives every engine of the process another value (0: the fp64 kernel, 1: six planes)
        # — the whole test suite runs under it this way
        self.predict_sliced = PREDICT_SLICED_DEFAULT
        env = predict_sliced_from_env()
        if env is not None:
            self.tune("predict_sliced", env)

    # ------------------------------------------------------------------ plumbing
    def _ck(self, rc):
        if rc < 0:
            raise nat.GPBError(f"{self.lib.gpb_last_error(self.h).decode()} (code {rc})")
        return rc

    def _check_pid(self):
        """A process forked AFTER this engine was created inherits the handle but not a usable HIP context (the
        runtime's state does not survive fork()): the reference's pocoMC `pool=int` workers are such processes
        (src/mcmc.py:775-776, 798-804).  Raise before any HIP call is issued on the dead context."""
        if self._pid != os.getpid():
            raise RuntimeError(
                "GPEngine was created in process %d, this is process %d: the GPU context does not survive a fork. "
                "Log-probability batches are already vectorised on the device — use pool=None, or start workers with "
                "the 'spawn' method before the parent touches the GPU" % (self._pid, os.getpid()))

    @property
    def h(self):
        """the gpb_ctx handle every C-ABI call takes: handing it out is where the fork guard sits"""
        self._check_pid()
        return self._h

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self, "_pid", None) == os.getpid():       # never issue HIP calls on a context inherited by fork
                self.lib.gpb_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        self._check_pid()
        self._ck(self.lib.gpb_sync(self.h))

    def _need_data(self):
        self._check_pid()
        if self.N == 0:
            raise nat.GPBError("no GP data: call set_data / set_theta / factor first")

    def _track_stream(self):
        """stream="torch": the kernels must run on the stream torch allocates and frees the caller's tensors on.
        Called at the top of every method that takes torch tensors: if torch's current stream of this device has
        changed since the last call (`with torch.cuda.stream(s):`, a sampler on a side stream) the context is
        re-targeted onto it (gpb_ctx_set_stream drains the old stream first, so work already enqueued is ordered
        before anything that follows)."""
        self._check_pid()
        if not self._follow_torch:
            return
        import torch
        s = torch.cuda.current_stream(self.device).cuda_stream
        if s != self._stream:
            self._ck(self.lib.gpb_ctx_set_stream(self.h, nat.VP(s)))
            self._stream = s

    def _dev(self, x, shape, name, dtype="torch.float64", contiguous=True):
        """Validate a tensor whose raw pointer goes to the C ABI as DEVICE memory: a wrong device, dtype, shape
        or stride would be read by the kernels as an address (a GPU fault, not an exception).  `shape` entries
        of None are free.  Returns the tensor (made contiguous when `contiguous` is False = input may be a view)."""
        if not _is_torch(x):
            raise ValueError("%s: expected a torch tensor, got %s" % (name, type(x).__name__))
        if not x.is_cuda or x.device.index != self.device:
            raise ValueError("%s: tensor lives on %s, the engine on cuda:%d" % (name, x.device, self.device))
        if str(x.dtype) != dtype:
            raise ValueError("%s: expected %s, got %s" % (name, dtype, x.dtype))
        if x.dim() != len(shape) or any(s is not None and int(s) != int(n) for s, n in zip(shape, x.shape)):
            raise ValueError("%s: expected shape %s, got %s" % (name, tuple(shape), tuple(x.shape)))
        if not x.is_contiguous():
            if contiguous:
                raise ValueError("%s: must be contiguous" % name)
            x = x.contiguous()
        return x

    def _check_cols(self, X_dev, name="X"):
        """device inputs are used as they are: the kernels index them with the engine's d"""
        self._track_stream()
        return self._dev(X_dev, (None, self.d), name, contiguous=False)

    def _extra_std_dev(self, extra_std, W):
        """extra_std of the torch path as a device vector [W] (None = 0)"""
        if extra_std is None:
            return None
        import torch
        if _is_torch(extra_std):
            if extra_std.dim() == 0:
                extra_std = extra_std.reshape(1)
            if extra_std.numel() == 1 and W != 1:
                extra_std = extra_std.expand(W)
            return self._dev(extra_std, (W,), "extra_std", contiguous=False)
        es = np.array(np.broadcast_to(np.asarray(extra_std, dtype=np.float64).reshape(-1), (W,)))     # writable copy
        return torch.as_tensor(es, device=torch.device("cuda", self.device))

    # ------------------------------------------------------------------ GP state
    def set_point_noise(self, point_noise):
        """Per-point simulation noise of the training diagonal (gpb_gp_set_point_noise, stochastic kriging): one row of
        variances >= 0 per GP — [P, N] for set_data, a list of P arrays [N_p] for set_data_multi — or None for none.  The
        diagonal of GP p becomes c + sigma_n^2 + (alpha + s[p, i]); the context is left without a factorisation.  ValueError for a
        wrong shape; GPBError (GPB_E_ARG) for a negative or non-finite entry, the context stays as it was."""
        self._check_pid()
        if point_noise is None:
            self._ck(self.lib.gpb_gp_set_point_noise(self.h, None))
            return
        import ctypes
        rows = [nat.f64(r).reshape(-1) for r in point_noise]
        if len(rows) != self.P:
            raise ValueError("point_noise: %d rows for %d GPs" % (len(rows), self.P))
        Ns = getattr(self, "_Ns", None)
        for p, r in enumerate(rows):
            want = self.N if Ns is None else int(Ns[p])
            if r.shape[0] != want:
                raise ValueError("point_noise: row %d has %d entries for %d design points" % (p, r.shape[0], want))
        sp = (ctypes.c_void_p * self.P)(*[r.ctypes.data for r in rows])
        self._ck(self.lib.gpb_gp_set_point_noise(self.h, sp))

    def set_data(self, X, Z, kernel="RBF", alpha=0.1, point_noise=None):
        """X[N,d] design, Z[P,N] targets (one row per GP); point_noise [P,N] (optional): see set_point_noise."""
        self._check_pid()
        X, Z = nat.f64(X), nat.f64(Z)
        self.N, self.d = X.shape
        self.P = Z.shape[0]
        assert Z.shape[1] == self.N
        kid = KERNEL_IDS[kernel] if isinstance(kernel, str) else int(kernel)
        self.M, self.pmap_d_in, self.pmap_d_out = 0, -1, -1       # gpb_gp_set drops the transform, likelihood and map
        self._ck(self.lib.gpb_gp_set(self.h, self.N, self.d, self.P, nat.ptr(X), nat.ptr(Z), kid, float(alpha)))
        self._Ns = None
        if point_noise is not None:
            self.set_point_noise(point_noise)

    def set_data_multi(self, Xs, Zs, kernel="RBF", alpha=0.1, point_noise=None):
        """P GPs, each over its own design: Xs[p] [N_p, d], Zs[p] [N_p] (gpb_gp_set_multi: the GPs of several emulators or
        the restarts of a search side by side; the designs must pad to the same multiple of 64 points).  Fit-only.
        point_noise (optional): a list of P arrays [N_p], see set_point_noise."""
        self._check_pid()
        import ctypes
        Xs = [nat.f64(x) for x in Xs]
        Zs = [nat.f64(z).reshape(-1) for z in Zs]
        self.P = len(Xs)
        assert self.P >= 1 and len(Zs) == self.P
        self.d = Xs[0].shape[1]
        for x, z in zip(Xs, Zs):
            assert x.ndim == 2 and x.shape[1] == self.d and z.shape[0] == x.shape[0]
        Ns = np.array([x.shape[0] for x in Xs], dtype=np.int64)
        self.N = int(Ns.max())
        kid = KERNEL_IDS[kernel] if isinstance(kernel, str) else int(kernel)
        self.M, self.pmap_d_in, self.pmap_d_out = 0, -1, -1
        xp = (ctypes.c_void_p * self.P)(*[x.ctypes.data for x in Xs])
        zp = (ctypes.c_void_p * self.P)(*[z.ctypes.data for z in Zs])
        self._ck(self.lib.gpb_gp_set_multi(self.h, self.P, self.d, nat.ptr(Ns), xp, zp, kid, float(alpha)))
        self._Ns = Ns
        if point_noise is not None:
            self.set_point_noise(point_noise)

    def lml_subset(self, idx, theta, eval_gradient=True):
        """LML (and gradient) of the stored GPs `idx` at theta[len(idx), d+2] in one launch sequence (gpb_gp_lml_subset);
        the context is left without a factorisation."""
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        n = idx.shape[0]
        theta = nat.f64(theta).reshape(n, self.d + 2)
        val = np.empty(n)
        grad = np.empty((n, self.d + 2)) if eval_gradient else None
        info = np.zeros(n, dtype=np.int32)
        self._ck(self.lib.gpb_gp_lml_subset(self.h, n, nat.ptr(idx), nat.ptr(theta), nat.ptr(val), nat.ptr(grad), nat.ptr(info)))
        return (val, grad) if eval_gradient else val

    lml_active = lml_subset          # the name the lock-step search driver looks for (emulator._batched_lbfgsb)

    def set_theta(self, theta):
        theta = nat.f64(theta).reshape(self.P, self.d + 2)
        self._ck(self.lib.gpb_gp_set_theta(self.h, nat.ptr(theta)))
        self.theta = theta.copy()

    def factor(self, raise_on_fail=True):
        info = np.zeros(self.P, dtype=np.int32)
        rc = self._ck(self.lib.gpb_gp_factor(self.h, nat.ptr(info)))
        if rc > 0 and raise_on_fail:
            raise NotPositiveDefinite(
                f"kernel matrix of GP {int(np.flatnonzero(info)[0])} is not positive definite "
                f"(leading minor {rc}); try increasing alpha")
        return info

    def get(self, what, W=None):
        """K / L / Linv [P,N,N], alpha [P,N], "Kstar" [P,W,N] (K(X*, X) of the most recent batch of W rows), "form" [P]
        (0 = Gram form, 1 = difference form of the distances: chosen per GP from theta, gpbayes.h GPB_GET_FORM)."""
        sel = {"K": 0, "L": 1, "Linv": 2, "alpha": 3, "Kstar": 4, "form": 5}[what]
        if what == "Kstar":
            shape = (self.P, int(W), self.N)
        elif what == "form":
            shape = (self.P,)
        else:
            shape = (self.P, self.N) if what == "alpha" else (self.P, self.N, self.N)
        out = np.empty(shape)
        self._ck(self.lib.gpb_gp_get(self.h, sel, nat.ptr(out)))
        return out

    def lml(self, theta, eval_gradient=True):
        theta = nat.f64(theta).reshape(self.P, self.d + 2)
        val = np.empty(self.P)
        grad = np.empty((self.P, self.d + 2)) if eval_gradient else None
        info = np.zeros(self.P, dtype=np.int32)
        self._ck(self.lib.gpb_gp_lml(self.h, nat.ptr(theta), nat.ptr(val), nat.ptr(grad), nat.ptr(info)))
        self.theta = theta.copy()
        return (val, grad) if eval_gradient else val

    def predict(self, Xs, return_var=True):
        """per-GP mean[W,P] (and var[W,P]); numpy in -> numpy out, torch(cuda) in -> torch out."""
        self._need_data()
        if _is_torch(Xs):
            import torch
            Xs = self._check_cols(Xs, "Xs")
            W = Xs.shape[0]
            mean = torch.empty((W, self.P), dtype=torch.float64, device=Xs.device)
            var = torch.empty((W, self.P), dtype=torch.float64, device=Xs.device) if return_var else None
            self._ck(self.lib.gpb_gp_predict(self.h, nat.ptr(Xs), W, 1, nat.ptr(mean), nat.ptr(var)))
            return (mean, var) if return_var else mean
        Xs = nat.f64(Xs).reshape(-1, self.d)
        W = Xs.shape[0]
        mean = np.empty((W, self.P))
        var = np.empty((W, self.P)) if return_var else None
        self._ck(self.lib.gpb_gp_predict(self.h, nat.ptr(Xs), W, 0, nat.ptr(mean), nat.ptr(var)))
        return (mean, var) if return_var else mean

    # gpb_gp_predict_cov's own limit (csrc/gpb_api.hip, "W > 8192": the library refuses a larger batch itself; tests/
    # test_gpu_predict_cov.py::test_limits asks both for PREDICT_COV_MAX_W + 1 rows, so the two cannot drift apart unnoticed)
    PREDICT_COV_MAX_W = 8192

    def predict_cov(self, Xs):
        """per-GP mean[W,P] and full covariance cov[P,W,W] between the query points (numpy in/out)."""
        self._need_data()
        Xs = nat.f64(Xs).reshape(-1, self.d)
        W = Xs.shape[0]
        if W > self.PREDICT_COV_MAX_W:       # before P x W x W doubles of pinned memory are asked for
            raise nat.GPBError("predict_cov: W = %d > %d (the W x W covariance is for small batches)" % (W, self.PREDICT_COV_MAX_W))
        mean = np.empty((W, self.P))
        cov = nat.host_empty((self.P, W, W))
        self._ck(self.lib.gpb_gp_predict_cov(self.h, nat.ptr(Xs), W, 0, nat.ptr(mean), nat.ptr(cov)))
        return mean, cov

    def predict_grad(self, Xs, return_var=True):
        """d mean / d x [W,P,d] (and d var / d x [W,P,d]) of every GP at the rows Xs (gpb_gp_predict_grad, fp64);
        numpy in -> numpy out, torch(cuda) in -> torch out."""
        self._need_data()
        if _is_torch(Xs):
            import torch
            Xs = self._check_cols(Xs, "Xs")
            W = Xs.shape[0]
            dm = torch.empty((W, self.P, self.d), dtype=torch.float64, device=Xs.device)
            dv = torch.empty((W, self.P, self.d), dtype=torch.float64, device=Xs.device) if return_var else None
            self._ck(self.lib.gpb_gp_predict_grad(self.h, nat.ptr(Xs), W, 1, nat.ptr(dm), nat.ptr(dv)))
            return (dm, dv) if return_var else dm
        Xs = nat.f64(Xs).reshape(-1, self.d)
        W = Xs.shape[0]
        dm = nat.host_empty((W, self.P, self.d))
        dv = nat.host_empty((W, self.P, self.d)) if return_var else None
        self._ck(self.lib.gpb_gp_predict_grad(self.h, nat.ptr(Xs), W, 0, nat.ptr(dm), nat.ptr(dv)))
        return (dm, dv) if return_var else dm

    # ------------------------------------------------------------------ closed-form cross-validation
    CV_MAX_FOLD = 64

    def _cv_folds(self, folds):
        """folds (None = leave-one-out of all points, or a list of index arrays) -> (idx int32 [n] | None, fold_ptr int32
        [nf+1] | None, n, nf, kmax); ValueError for what gpb_gp_cv answers with GPB_E_ARG"""
        self._need_data()
        if folds is None:
            return None, None, self.N, self.N, 1
        folds = [np.atleast_1d(np.asarray(f)).reshape(-1) for f in folds]
        if not folds:
            raise ValueError("cross_validate: no folds")
        sizes = np.array([f.shape[0] for f in folds], dtype=np.int64)
        if sizes.min() < 1:
            raise ValueError("cross_validate: fold %d is empty" % int(np.argmin(sizes)))
        if sizes.max() > self.CV_MAX_FOLD:
            raise ValueError("cross_validate: fold %d has %d points; the closed form takes folds of 1 to %d points "
                             "(use more folds, or refit for larger hold-out sets)" % (int(np.argmax(sizes)), int(sizes.max()), self.CV_MAX_FOLD))
        flat = np.concatenate(folds)
        if not np.issubdtype(flat.dtype, np.integer):
            raise ValueError("cross_validate: folds must hold integer design-point indices")
        if flat.min() < 0 or flat.max() >= self.N:
            raise ValueError("cross_validate: design-point index outside [0, %d)" % self.N)
        if np.unique(flat).shape[0] != flat.shape[0]:
            raise ValueError("cross_validate: a design point appears in the folds twice")
        idx = np.ascontiguousarray(flat, dtype=np.int32)
        fptr = np.ascontiguousarray(np.concatenate([[0], np.cumsum(sizes)]), dtype=np.int32)
        return idx, fptr, idx.shape[0], len(folds), int(sizes.max())

    def cross_validate(self, folds=None, return_cov=False):
        """Hold-out predictions of the fitted GPs in closed form (gpb_gp_cv): for every fold F the mean and variance, at X_F, of
        the GP refitted WITHOUT the fold's points at the same theta — mean = z_F - G^-1 alpha_F, cov = G^-1 - alpha I with
        G = (Ky^-1)_FF from the resident L^-1; no refit, no N-sized factorisation.  folds: None = leave-one-out of all N points,
        or a list of arrays of distinct design-point indices, 1 to 64 points each.  Returns (mean [n_idx, P], var [n_idx, P]) in
        the order of the concatenated folds, plus with return_cov the folds' covariance blocks [P, nf, kmax, kmax] (zero-padded
        to the largest fold size kmax).  Variances are not clipped.  ValueError for empty or oversized folds, indices out of
        range or repeated."""
        idx, fptr, n, nf, kmax = self._cv_folds(folds)
        self._track_stream()
        mean, var = np.empty((n, self.P)), np.empty((n, self.P))
        cov = nat.host_empty((self.P, nf, kmax, kmax)) if return_cov else None
        self._ck(self.lib.gpb_gp_cv(self.h, nat.ptr(idx), n, nat.ptr(fptr), nf, 0, nat.ptr(mean), nat.ptr(var), nat.ptr(cov)))
        return (mean, var, cov) if return_cov else (mean, var)

    def emu_cross_validate(self, folds=None, return_cov=True):
        """cross_validate through the installed observable transform (gpb_emu_cv, extra_std = 0): mean [n_idx, M] and, with
        return_cov, cov [n_idx, M, M] — what emu_predict would give at the held-out design points after a refit without their
        fold.  Overwrites the workspace of the last predict batch (get("Kstar") is undefined afterwards)."""
        idx, fptr, n, nf, _ = self._cv_folds(folds)
        self._track_stream()
        mean = nat.host_empty((n, self.M))
        cov = nat.host_empty((n, self.M, self.M)) if return_cov else None
        self._ck(self.lib.gpb_emu_cv(self.h, nat.ptr(idx), n, nat.ptr(fptr), nf, 0, nat.ptr(mean), nat.ptr(cov)))
        return (mean, cov) if return_cov else mean

    # ------------------------------------------------------------------ closed-form Sobol indices
    def _box(self, lo, hi):
        self._need_data()
        self._track_stream()
        lo, hi = nat.f64(lo).reshape(-1), nat.f64(hi).reshape(-1)
        if lo.shape[0] != self.d or hi.shape[0] != self.d:
            raise ValueError("sobol: lo and hi need one entry per input dimension (%d)" % self.d)
        return lo, hi

    def sobol(self, lo, hi, on_device=False):
        """Closed-form integrals of the GPs' posterior means over the uniform box [lo, hi] (gpb_gp_sobol, RBF only):
        e [P] = E[m_p] and H [P, P, 2d + 1] = E[E[m_p | x_S] E[m_q | x_S]] for the subsets S = {j} (slot j), all but j (slot d + j)
        and all (slot 2d).  numpy out, or with on_device torch tensors on the engine's device (asynchronous)."""
        lo, hi = self._box(lo, hi)
        shapes = ((self.P,), (self.P, self.P, 2 * self.d + 1))
        if on_device:
            import torch
            e, H = (torch.empty(s, dtype=torch.float64, device=torch.device("cuda", self.device)) for s in shapes)
        else:
            e, H = (np.empty(s) for s in shapes)
        self._ck(self.lib.gpb_gp_sobol(self.h, nat.ptr(lo), nat.ptr(hi), 1 if on_device else 0, nat.ptr(e), nat.ptr(H)))
        return e, H

    def emu_sobol(self, lo, hi, on_device=False):
        """Sobol indices of the observables' posterior mean through the installed (linear) transform (gpb_emu_sobol): mean [M],
        variance [M], first-order indices [M, d], total indices [M, d] over the uniform box [lo, hi]; of the log-observable in
        the two exp modes.  numpy out, or with on_device torch tensors on the engine's device (asynchronous)."""
        lo, hi = self._box(lo, hi)
        if on_device:
            import torch
            dev = torch.device("cuda", self.device)
            out = [torch.empty(s, dtype=torch.float64, device=dev) for s in ((self.M,), (self.M,), (self.M, self.d), (self.M, self.d))]
        else:
            out = [np.empty(s) for s in ((self.M,), (self.M,), (self.M, self.d), (self.M, self.d))]
        self._ck(self.lib.gpb_emu_sobol(self.h, nat.ptr(lo), nat.ptr(hi), 1 if on_device else 0, *[nat.ptr(o) for o in out]))
        return tuple(out)

    def emu_main_effect(self, lo, hi, j, t):
        """Main-effect curve E[f_m | x_j = t] of the observables' posterior mean on the grid t [G] over the box [lo, hi]
        (gpb_emu_main_effect): curve [G, M], numpy out."""
        lo, hi = self._box(lo, hi)
        t = nat.f64(t).reshape(-1)
        curve = np.empty((t.shape[0], self.M))
        self._ck(self.lib.gpb_emu_main_effect(self.h, nat.ptr(lo), nat.ptr(hi), int(j), nat.ptr(t), t.shape[0], 0, nat.ptr(curve)))
        return curve

    # ------------------------------------------------------------------ variance-reduction sequential design
    def design_begin(self, candidates, reference, weights, g, candidate_noise=None):
        """Build the design workspace (gpb_design_begin): candidates [C, d], reference [R, d] and weights [R] (>= 0, sum 1) are
        torch cuda tensors in the GPs' input space (behind param_map for a parameterTrafoPCA emulator), g [P] the GPs' weights
        (host).  For every GP: S_rc = c k(x_r, x_c) - V_r^T V_c and s(c, c).  Overwrites the predict workspace; asynchronous.
        candidate_noise [P, C] (optional, host or torch cuda): see design_set_noise."""
        self._need_data()
        Xc = self._check_cols(candidates, "candidates")
        Xr = self._check_cols(reference, "reference")
        w = self._dev(weights, (Xr.shape[0],), "weights", contiguous=False)
        g = nat.f64(g).reshape(-1)
        if g.shape[0] != self.P:
            raise ValueError("design_begin: g needs one weight per GP (%d), got %d" % (self.P, g.shape[0]))
        self._ck(self.lib.gpb_design_begin(self.h, nat.ptr(Xc), Xc.shape[0], nat.ptr(Xr), Xr.shape[0], nat.ptr(w), nat.ptr(g)))
        self._design_C = int(Xc.shape[0])
        if candidate_noise is not None:
            self.design_set_noise(candidate_noise)

    def design_set_noise(self, candidate_noise):
        """The candidates' own simulation noise (gpb_design_set_noise, between design_begin and design_run): candidate_noise
        [P, C] variances >= 0 in the GPs' target units, numpy or a torch cuda tensor; candidate c is then observed with
        tau_p(c) = sigma_n^2 + (alpha + s_c[p, c]).  None: back to the training runs' tau_p.  ValueError for a wrong shape or a
        negative / non-finite entry."""
        self._need_data()
        if candidate_noise is None:
            self._ck(self.lib.gpb_design_set_noise(self.h, None))
            return
        import torch
        C = int(getattr(self, "_design_C", 0))
        if C < 1:
            self._ck(self.lib.gpb_design_set_noise(self.h, None))   # (no workspace: the library's GPB_E_STATE and its message)
            return
        if not _is_torch(candidate_noise):
            candidate_noise = torch.as_tensor(nat.f64(candidate_noise), device=torch.device("cuda", self.device))
        sc = self._dev(candidate_noise, (self.P, C), "candidate_noise")
        if not bool(torch.all(torch.isfinite(sc) & (sc >= 0.0))):
            raise ValueError("design_set_noise: candidate_noise must be finite and non-negative")
        self._ck(self.lib.gpb_design_set_noise(self.h, nat.ptr(sc)))
    def design_run(self, n_picks, eligible=None, return_scores=False):
        """The greedy loop over this engine alone (the E = 1 chain call): see design_run() of this module."""
        return design_run([self], n_picks, eligible, return_scores)

    def design_end(self):
        """Release the design workspace (gpb_design_end)."""
        self._check_pid()
        self._design_C = 0
        self._ck(self.lib.gpb_design_end(self.h))

    # ------------------------------------------------------------------ emulator transform
    def set_transform(self, mode, mu, A=None, cov_trunc=None, scale=None):
        mu = nat.f64(mu)
        self.M = mu.shape[0]
        self.mode = int(mode)
        A = None if A is None else nat.f64(A)
        cov_trunc = None if cov_trunc is None else nat.f64(cov_trunc)
        scale = None if scale is None else nat.f64(scale)
        self._ck(self.lib.gpb_emu_set_transform(self.h, int(mode), self.M, nat.ptr(A), nat.ptr(mu),
                                                nat.ptr(cov_trunc), nat.ptr(scale)))

    def emu_predict(self, Xs, return_cov=True, extra_std=None):
        self._need_data()
        if _is_torch(Xs):
            import torch
            Xs = self._check_cols(Xs, "Xs")
            W = Xs.shape[0]
            es = self._extra_std_dev(extra_std, W)       # numbers / numpy are uploaded, tensors are validated
            mean = torch.empty((W, self.M), dtype=torch.float64, device=Xs.device)
            cov = torch.empty((W, self.M, self.M), dtype=torch.float64, device=Xs.device) if return_cov else None
            self._ck(self.lib.gpb_emu_predict(self.h, nat.ptr(Xs), W, 1, nat.ptr(es), nat.ptr(mean), nat.ptr(cov)))
            return (mean, cov) if return_cov else mean
        Xs = nat.f64(Xs).reshape(-1, self.d)
        W = Xs.shape[0]
        es = None if extra_std is None else nat.f64(np.broadcast_to(np.asarray(extra_std, float).reshape(-1), (W,)))
        mean = nat.host_empty((W, self.M))
        cov = nat.host_empty((W, self.M, self.M)) if return_cov else None
        self._ck(self.lib.gpb_emu_predict(self.h, nat.ptr(Xs), W, 0, nat.ptr(es), nat.ptr(mean), nat.ptr(cov)))
        return (mean, cov) if return_cov else mean

    def emu_predict_diag(self, Xs, extra_std=None, out=None):
        """emu_predict without the [W, M, M] array, observable-major (gpb_emu_predict_diag): (mean_T [M, W], var_T [M, W]) with
        mean_T[m, w] = emu_predict's mean[w, m] and var_T[m, w] = its cov[w, m, m], bit for bit.  numpy in -> numpy out, torch(cuda)
        in -> torch out.  out (torch path): a pair of device views [M, >= W] with unit stride along the samples — the slab's
        columns of a larger [M, S] pair, e.g. (mu[:, i0:i1], var[:, i0:i1]) — written in place; their other columns stay."""
        self._need_data()
        if _is_torch(Xs):
            import torch
            Xs = self._check_cols(Xs, "Xs")
            W = Xs.shape[0]
            es = self._extra_std_dev(extra_std, W)
            if out is None:
                out = (torch.empty((self.M, W), dtype=torch.float64, device=Xs.device),
                       torch.empty((self.M, W), dtype=torch.float64, device=Xs.device))
            mean_T, var_T = out
            for name, t in (("out[0]", mean_T), ("out[1]", var_T)):
                if not _is_torch(t) or not t.is_cuda or t.device.index != self.device or str(t.dtype) != "torch.float64":
                    raise ValueError("%s: expected a torch.float64 tensor on cuda:%d" % (name, self.device))
                if t.dim() != 2 or t.shape[0] != self.M or t.shape[1] < W or (t.shape[1] > 1 and t.stride(1) != 1) \
                        or (self.M > 1 and t.stride(0) < W):
                    raise ValueError("%s: expected a [%d, >= %d] view with unit stride along the samples" % (name, self.M, W))
            ld = int(mean_T.stride(0)) if self.M > 1 else max(int(mean_T.shape[1]), W)
            if self.M > 1 and int(var_T.stride(0)) != ld:
                raise ValueError("out: the two views need the same row stride")
            if W:
                self._ck(self.lib.gpb_emu_predict_diag(self.h, nat.ptr(Xs), W, 1, nat.ptr(es), nat.ptr(mean_T), nat.ptr(var_T), ld))
            return mean_T, var_T
        if out is not None:
            raise ValueError("emu_predict_diag: out= takes device views, together with torch input")
        Xs = nat.f64(Xs).reshape(-1, self.d)
        W = Xs.shape[0]
        es = None if extra_std is None else nat.f64(np.broadcast_to(np.asarray(extra_std, float).reshape(-1), (W,)))
        mean_T, var_T = nat.host_empty((self.M, W)), nat.host_empty((self.M, W))
        if W:
            self._ck(self.lib.gpb_emu_predict_diag(self.h, nat.ptr(Xs), W, 0, nat.ptr(es), nat.ptr(mean_T), nat.ptr(var_T), W))
        return mean_T, var_T

    PPD_MAX_LEVELS = 16

    def ppd_summary(self, mu_T, var_T, q, vadd=None, yobs=None, S=None, on_device=False, outputs=None):
        """Reductions over the sample axis of observable-major device arrays (gpb_ppd_summary): mu_T, var_T (None = 0) torch cuda
        views [M, >= S] with unit stride along the samples (S: the samples to reduce, default all columns), q the levels in
        [0, 1] (at most 16).  Returns a dict with only the outputs whose inputs were given: "moments" [M, 3] (E mu, E sigma^2,
        E (mu - E mu)^2) and "order" [M, nq, 2] (the two order statistics numpy's percentile interpolates between) always;
        "mixq" [M, nq], the quantiles of the predictive mixture with tau^2 = sigma^2 + vadd, when var_T or vadd is given; "pit"
        [M], the mixture's CDF at yobs, when yobs is.  vadd, yobs: [M], numpy or torch cuda.  numpy out, or with on_device
        torch tensors (asynchronous).  outputs: the names to compute instead of that rule (the library refuses a name whose inputs
        are missing).  The engine lends its device and stream only: M is the caller's."""
        import torch
        self._track_stream()
        dev = torch.device("cuda", self.device)
        if not _is_torch(mu_T) or mu_T.dim() != 2:
            raise ValueError("mu_T: expected a two-dimensional torch tensor")
        M = int(mu_T.shape[0])
        S = int(mu_T.shape[1]) if S is None else int(S)
        ld = None
        for name, t in (("mu_T", mu_T), ("var_T", var_T)):
            if t is None:
                continue
            if not _is_torch(t) or not t.is_cuda or t.device.index != self.device or str(t.dtype) != "torch.float64":
                raise ValueError("%s: expected a torch.float64 tensor on cuda:%d" % (name, self.device))
            if t.dim() != 2 or t.shape[0] != M or t.shape[1] < S or (t.shape[1] > 1 and t.stride(1) != 1):
                raise ValueError("%s: expected a [%d, >= %d] view with unit stride along the samples" % (name, M, S))
            t_ld = int(t.stride(0)) if M > 1 else max(int(t.shape[1]), S)
            if ld is not None and t_ld != ld:
                raise ValueError("mu_T and var_T need the same row stride")
            ld = t_ld
        q = nat.f64(np.atleast_1d(np.asarray(q, dtype=np.float64))).reshape(-1)
        nq = int(q.shape[0])

        def vec(a, name):
            if a is None:
                return None
            if not _is_torch(a):
                a = torch.as_tensor(nat.f64(a).reshape(-1), device=dev)
            return self._dev(a, (M,), name, contiguous=False)
        vadd, yobs = vec(vadd, "vadd"), vec(yobs, "yobs")
        shapes = {"moments": (M, 3), "order": (M, nq, 2), "mixq": (M, nq), "pit": (M,)}
        if outputs is None:
            outputs = ["moments", "order"] + (["mixq"] if var_T is not None or vadd is not None else []) \
                + (["pit"] if yobs is not None else [])
        shapes = {k: shapes[k] for k in outputs}
        if on_device:
            out = {k: torch.empty(s, dtype=torch.float64, device=dev) for k, s in shapes.items()}
        else:
            out = {k: np.empty(s) for k, s in shapes.items()}
        self._ck(self.lib.gpb_ppd_summary(self.h, nat.ptr(mu_T), nat.ptr(var_T), M, S, ld, nat.ptr(q), nq, nat.ptr(vadd),
                                          nat.ptr(yobs), 1 if on_device else 0, nat.ptr(out.get("moments")),
                                          nat.ptr(out.get("order")), nat.ptr(out.get("mixq")), nat.ptr(out.get("pit"))))
        return out

    SENS_LDS_DOUBLES = 8064                       # GPB_SENS_LDS_DOUBLES
    SENS_MAX_M, SENS_MAX_D, SENS_CHUNK = 2048, 64, 256

    @classmethod
    def sens_path(cls, M, d):
        """"lds" when gpb_sens_accumulate keeps a row's Cw [M, M | 1] and L^-1 J [M, d] in LDS, "global" when it factorises the
        row in place in its slab of C"""
        M, d = int(M), int(d)
        return "lds" if M * (M | 1) + M * d <= cls.SENS_LDS_DOUBLES else "global"

    @staticmethod
    def sens_acc_doubles(M, d):
        """GPB_SENS_ACC_DOUBLES(M, d): sum wt | sum wt F [d, d] | sum wt R | sum wt R^2 | sum wt I [M, d] each"""
        return 1 + int(d) * int(d) + 3 * int(M) * int(d)

    def sens_accumulate(self, J, y, C, Cadd, x, wt, acc, cnt):
        """Adds the rows' Fisher matrices, response matrices and single-observable informations to running sums
        (gpb_sens_accumulate).  torch cuda tensors, contiguous: J [W, M, d], y [W, M], C [W, M, M] (DESTROYED), Cadd [M, M] or
        None, x [W, d], wt [W] or None (= 1; non-negative), acc [sens_acc_doubles(M, d)] float64 and cnt [2] int64, both zeroed
        by the caller before the first slab.  Every slab but the last must hold a multiple of 256 rows (GPBError otherwise); any
        such split leaves the bits of one call.  The engine lends its device and stream only: M and d are the caller's."""
        self._track_stream()
        J = self._dev(J, (None, None, None), "J")
        W, M, d = (int(v) for v in J.shape)
        if M < 1 or d < 1 or M > self.SENS_MAX_M or d > self.SENS_MAX_D:
            raise ValueError("sens_accumulate: need 1 <= M <= %d and 1 <= d <= %d" % (self.SENS_MAX_M, self.SENS_MAX_D))
        self._dev(y, (W, M), "y")
        self._dev(C, (W, M, M), "C")
        self._dev(x, (W, d), "x")
        if Cadd is not None:
            self._dev(Cadd, (M, M), "Cadd")
        if wt is not None:
            self._dev(wt, (W,), "wt")
        self._dev(acc, (self.sens_acc_doubles(M, d),), "acc")
        self._dev(cnt, (2,), "cnt", dtype="torch.int64")
        self._ck(self.lib.gpb_sens_accumulate(self.h, W, M, d, nat.ptr(J), nat.ptr(y), nat.ptr(C), nat.ptr(Cadd), nat.ptr(x),
                                              nat.ptr(wt), nat.ptr(acc), nat.ptr(cnt)))

    def sens_unpack(self, acc, cnt, M, d):
        """The running sums of sens_accumulate as host arrays (sums, not means): "wsum", "fisher" [d, d], "response",
        "response_sq", "obs_information" [M, d], "n_rows", "n_bad"."""
        M, d = int(M), int(d)
        a = acc.cpu().numpy() if _is_torch(acc) else np.asarray(acc, dtype=np.float64)
        c = cnt.cpu().numpy() if _is_torch(cnt) else np.asarray(cnt)
        if a.shape != (self.sens_acc_doubles(M, d),) or c.shape != (2,):
            raise ValueError("sens_unpack: acc [%d] and cnt [2] expected" % self.sens_acc_doubles(M, d))
        o = 1 + d * d
        return {"wsum": float(a[0]), "fisher": a[1:o].reshape(d, d).copy(),
                "response": a[o:o + M * d].reshape(M, d).copy(),
                "response_sq": a[o + M * d:o + 2 * M * d].reshape(M, d).copy(),
                "obs_information": a[o + 2 * M * d:o + 3 * M * d].reshape(M, d).copy(),
                "n_rows": int(c[0]), "n_bad": int(c[1])}

    GOF_LDS_DOUBLES = 8064                        # GPB_GOF_LDS_DOUBLES
    GOF_MAX_M, GOF_MAX_D, GOF_MAX_E, GOF_CHUNK = 2048, 512, 64, 256

    @classmethod
    def gof_path(cls, M):
        """"lds" when gpb_gof_accumulate keeps a row's Cw and z ([M + 1, M | 1]) in LDS, "global" when it factorises the row in
        place in its slab of C"""
        M = int(M)
        return "lds" if (M + 1) * (M | 1) <= cls.GOF_LDS_DOUBLES else "global"

    @staticmethod
    def gof_acc_doubles(M):
        """GPB_GOF_ACC_DOUBLES(M): sum wt | sum wt p | sum wt z | sum wt z^2 | sum wt pull | sum wt pull^2 [M] each"""
        return 2 + 4 * int(M)

    def gof_accumulate(self, y, C, yexp, Cadd, wt, chi2_out, ll_out, acc, cnt):
        """chi2 and log-likelihood of every row against one data set, and the running sums of the whitened residuals, the pulls
        and the predictive p-value (gpb_gof_accumulate).  torch cuda tensors: y [W, M], C [W, M, M] (DESTROYED), yexp [M], Cadd
        [M, M] or None, wt [W] or None (= 1; non-negative), chi2_out and ll_out [W] with unit stride (a slab of a row of an
        [E, S] array), acc [gof_acc_doubles(M)] float64 and cnt [2] int64, both zeroed by the caller before the first slab.
        Every slab but the last must hold a multiple of 256 rows (GPBError otherwise); any such split leaves the bits of one
        call.  The engine lends its device and stream only: M is the caller's."""
        self._track_stream()
        y = self._dev(y, (None, None), "y")
        W, M = (int(v) for v in y.shape)
        if M < 1 or M > self.GOF_MAX_M:
            raise ValueError("gof_accumulate: need 1 <= M <= %d" % self.GOF_MAX_M)
        self._dev(C, (W, M, M), "C")
        self._dev(yexp, (M,), "yexp")
        if Cadd is not None:
            self._dev(Cadd, (M, M), "Cadd")
        if wt is not None:
            self._dev(wt, (W,), "wt")
        self._dev(chi2_out, (W,), "chi2_out")
        self._dev(ll_out, (W,), "ll_out")
        self._dev(acc, (self.gof_acc_doubles(M),), "acc")
        self._dev(cnt, (2,), "cnt", dtype="torch.int64")
        self._ck(self.lib.gpb_gof_accumulate(self.h, W, M, nat.ptr(y), nat.ptr(C), nat.ptr(yexp), nat.ptr(Cadd), nat.ptr(wt),
                                             nat.ptr(chi2_out), nat.ptr(ll_out), nat.ptr(acc), nat.ptr(cnt)))

    @staticmethod
    def gof_unpack(acc, cnt, M):
        """The running sums of gof_accumulate as host arrays (sums, not means): "wsum", "p", "z", "z_sq", "pull", "pull_sq" [M],
        "n_rows", "n_bad"."""
        M = int(M)
        a = acc.cpu().numpy() if _is_torch(acc) else np.asarray(acc, dtype=np.float64)
        c = cnt.cpu().numpy() if _is_torch(cnt) else np.asarray(cnt)
        if a.shape != (2 + 4 * M,) or c.shape != (2,):
            raise ValueError("gof_unpack: acc [%d] and cnt [2] expected" % (2 + 4 * M))
        return {"wsum": float(a[0]), "p": float(a[1]), "z": a[2:2 + M].copy(), "z_sq": a[2 + M:2 + 2 * M].copy(),
                "pull": a[2 + 2 * M:2 + 3 * M].copy(), "pull_sq": a[2 + 3 * M:2 + 4 * M].copy(),
                "n_rows": int(c[0]), "n_bad": int(c[1])}

    def chi2_sf(self, x, ndf, out=None):
        """Q(ndf / 2, x / 2) per element of the torch cuda tensor x [n] (gpb_chi2_sf): the chi-square survival function; NaN in
        gives NaN out, x <= 0 gives 1.  Returns a device tensor (out, when given).  Asynchronous."""
        import torch
        self._track_stream()
        x = self._dev(x, (None,), "x", contiguous=False)
        ndf = float(ndf)
        if not (ndf > 0.0 and np.isfinite(ndf)):
            raise ValueError("chi2_sf: ndf must be finite and positive")
        if out is None:
            out = torch.empty_like(x)
        self._dev(out, (x.shape[0],), "out")
        self._ck(self.lib.gpb_chi2_sf(self.h, nat.ptr(x), int(x.shape[0]), ndf, nat.ptr(out)))
        return out

    def gof_influence(self, ll_T, x, wt=None, S=None):
        """The moments of the rows x [S, d] under the importance weights wt exp(-(ll_T[e] - min ll_T[e])) of the posterior
        without data set e (gpb_gof_influence): ll_T a torch cuda view [E, >= S] with unit stride along the rows, wt [S] or
        None.  Returns a device tensor [E, 2 + 2 d]: sum w | sum w^2 | sum w x_j | sum w x_j^2.  Rows with a NaN ll or wt == 0
        are left out.  Asynchronous; equal inputs give equal bits, and a row of the result does not depend on the others."""
        import torch
        self._track_stream()
        if not _is_torch(ll_T) or ll_T.dim() != 2:
            raise ValueError("ll_T: expected a two-dimensional torch tensor")
        E = int(ll_T.shape[0])
        S = int(ll_T.shape[1]) if S is None else int(S)
        if not ll_T.is_cuda or ll_T.device.index != self.device or str(ll_T.dtype) != "torch.float64":
            raise ValueError("ll_T: expected a torch.float64 tensor on cuda:%d" % self.device)
        if S < 1 or ll_T.shape[1] < S or (ll_T.shape[1] > 1 and ll_T.stride(1) != 1):
            raise ValueError("ll_T: expected a [%d, >= %d] view with unit stride along the rows, S >= 1" % (E, S))
        ld = int(ll_T.stride(0)) if E > 1 else max(int(ll_T.shape[1]), S)
        x = self._dev(x, (S, None), "x")
        d = int(x.shape[1])
        if E < 1 or E > self.GOF_MAX_E or d < 1 or d > self.GOF_MAX_D or ld < S:
            raise ValueError("gof_influence: need 1 <= E <= %d, 1 <= d <= %d and a row stride >= S" % (self.GOF_MAX_E, self.GOF_MAX_D))
        if wt is not None:
            self._dev(wt, (S,), "wt")
        out = torch.empty((E, 2 + 2 * d), dtype=torch.float64, device=x.device)
        self._ck(self.lib.gpb_gof_influence(self.h, nat.ptr(ll_T), E, S, ld, nat.ptr(x), d, nat.ptr(wt), nat.ptr(out)))
        return out

    PSIS_MAX_S = 1 << 24                          # GPB_PSIS_MAX_S
    LOO_COLUMNS = ("elpd_loo", "lppd", "p_waic", "khat", "ess", "n_tail", "loo_pit", "min_ll")     # GPB_LOO_*

    def loo_pointwise(self, y, C, yexp, Cadd, ll_T, zc_T, flag):
        """The leave-one-out conditionals of every observable of every row (gpb_loo_pointwise; include/gpbayes.h has the
        formulas).  torch cuda tensors: y [W, M], C [W, M, M] (DESTROYED), yexp [M], Cadd [M, M] or None; ll_T and zc_T (or None)
        views [M, W] with unit stride along the rows and one row stride (a slab of columns of an [nobs, S] array); flag [W] uint8,
        1 where the row's covariance had a non-positive pivot (its column is NaN).  Asynchronous.  The engine lends its device
        and stream only: M is the caller's."""
        self._track_stream()
        y = self._dev(y, (None, None), "y")
        W, M = (int(v) for v in y.shape)
        if M < 1 or M > self.GOF_MAX_M:
            raise ValueError("loo_pointwise: need 1 <= M <= %d" % self.GOF_MAX_M)
        self._dev(C, (W, M, M), "C")
        self._dev(yexp, (M,), "yexp")
        if Cadd is not None:
            self._dev(Cadd, (M, M), "Cadd")
        self._dev(flag, (W,), "flag", dtype="torch.uint8")
        ld = None
        for name, a in (("ll_T", ll_T), ("zc_T", zc_T)):
            if a is None:
                if name == "ll_T":
                    raise ValueError("ll_T: expected a torch tensor")
                continue
            if not _is_torch(a) or not a.is_cuda or a.device.index != self.device or str(a.dtype) != "torch.float64":
                raise ValueError("%s: expected a torch.float64 tensor on cuda:%d" % (name, self.device))
            if a.dim() != 2 or tuple(a.shape) != (M, W) or (W > 1 and a.stride(1) != 1):
                raise ValueError("%s: expected a [%d, %d] view with unit stride along the rows" % (name, M, W))
            a_ld = int(a.stride(0)) if M > 1 else W
            if a_ld < W or (ld is not None and a_ld != ld):
                raise ValueError("ll_T and zc_T need the same row stride, at least W")
            ld = a_ld
        self._ck(self.lib.gpb_loo_pointwise(self.h, W, M, nat.ptr(y), nat.ptr(C), nat.ptr(yexp), nat.ptr(Cadd), nat.ptr(ll_T),
                                            nat.ptr(zc_T), ld, nat.ptr(flag)))

    def _rows_view(self, a, name, S=None):
        """(R, S, ld) of a [R, >= S] float64 array of rows: a torch cuda view with unit stride along the samples, or a numpy array
        (made C-contiguous by the caller)"""
        if _is_torch(a):
            if a.dim() != 2 or not a.is_cuda or a.device.index != self.device or str(a.dtype) != "torch.float64":
                raise ValueError("%s: expected a two-dimensional torch.float64 tensor on cuda:%d" % (name, self.device))
            R = int(a.shape[0])
            S = int(a.shape[1]) if S is None else int(S)
            if S < 1 or a.shape[1] < S or (a.shape[1] > 1 and a.stride(1) != 1):
                raise ValueError("%s: expected a [%d, >= %d] view with unit stride along the samples, S >= 1" % (name, R, S))
            ld = int(a.stride(0)) if R > 1 else max(int(a.shape[1]), S)
            if ld < S:
                raise ValueError("%s: the row stride must be at least S" % name)
            return R, S, ld
        if a.ndim != 2 or a.shape[1] < 1:
            raise ValueError("%s: expected a [R, S] array, S >= 1" % name)
        S = int(a.shape[1]) if S is None else int(S)
        if S < 1 or S > a.shape[1]:
            raise ValueError("%s: S outside 1 .. %d" % (name, a.shape[1]))
        return int(a.shape[0]), S, int(a.shape[1])

    def psis(self, lr_T, S=None, outputs=None):
        """Pareto-smoothed importance sampling of every row of log ratios (gpb_psis; include/gpbayes.h has the procedure): lr_T
        [R, >= S], finite (the caller checks), a torch cuda view with unit stride along the samples — the results are then device
        tensors and the call is asynchronous — or a numpy array — numpy results.  Returns a dict: "khat" [R], "n_tail" [R] int64,
        "ess" [R], "log_weights" [R, S] (normalised: logsumexp of a row is 0).  outputs: the names to compute (default all).
        A row's bits depend on neither R, the row stride, the other rows nor the outputs asked for."""
        import torch
        names = ("khat", "n_tail", "ess", "log_weights")
        outputs = names if outputs is None else tuple(outputs)
        if any(k not in names for k in outputs):
            raise ValueError("outputs: names among %s" % (names,))
        on_device = _is_torch(lr_T)
        if on_device:
            self._track_stream()
        else:
            self._check_pid()
            lr_T = nat.f64(lr_T)
        R, S, ld = self._rows_view(lr_T, "lr_T", S)
        if R < 1 or S > self.PSIS_MAX_S:
            raise ValueError("psis: need R >= 1 and S <= 2^24")
        shapes = {"khat": (R,), "n_tail": (R,), "ess": (R,), "log_weights": (R, ld)}
        if on_device:
            dev = torch.device("cuda", self.device)
            out = {k: torch.empty(shapes[k], dtype=torch.int64 if k == "n_tail" else torch.float64, device=dev) for k in outputs}
        else:
            out = {k: np.empty(shapes[k], dtype=np.int64 if k == "n_tail" else np.float64) for k in outputs}
        self._ck(self.lib.gpb_psis(self.h, nat.ptr(lr_T), R, S, ld, 1 if on_device else 0, nat.ptr(out.get("khat")),
                                   nat.ptr(out.get("n_tail")), nat.ptr(out.get("ess")), nat.ptr(out.get("log_weights"))))
        if "log_weights" in out:
            out["log_weights"] = out["log_weights"][:, :S]
        return out

    def psis_loo(self, ll_T, zc_T=None, S=None):
        """PSIS-LOO and WAIC of R units from their pointwise log-likelihoods (gpb_psis_loo): ll_T [R, >= S] finite, zc_T the
        standardised conditional residuals of the same shape and row stride or None; torch cuda views (device result,
        asynchronous) or numpy arrays.  Returns [R, 8] in the order of LOO_COLUMNS."""
        import torch
        on_device = _is_torch(ll_T)
        if zc_T is not None and _is_torch(zc_T) != on_device:
            raise ValueError("ll_T and zc_T: both torch cuda tensors or both numpy arrays")
        if on_device:
            self._track_stream()
        else:
            self._check_pid()
            ll_T = nat.f64(ll_T)
            zc_T = None if zc_T is None else nat.f64(zc_T)
        R, S, ld = self._rows_view(ll_T, "ll_T", S)
        if zc_T is not None and self._rows_view(zc_T, "zc_T", S) != (R, S, ld):
            raise ValueError("zc_T: expected the shape and the row stride of ll_T")
        if R < 1 or S > self.PSIS_MAX_S:
            raise ValueError("psis_loo: need R >= 1 and S <= 2^24")
        if on_device:
            out = torch.empty((R, len(self.LOO_COLUMNS)), dtype=torch.float64, device=torch.device("cuda", self.device))
        else:
            out = np.empty((R, len(self.LOO_COLUMNS)))
        self._ck(self.lib.gpb_psis_loo(self.h, nat.ptr(ll_T), nat.ptr(zc_T), R, S, ld, 1 if on_device else 0, nat.ptr(out)))
        return out

    DIAG_NO_WINDOW = 1 << 30                      # GPB_DIAG_NO_WINDOW

    def mcmc_diag(self, x_dev, layout="steps", max_lag=None, c=5.0, on_device=False, outputs=None):
        """Convergence diagnostics of a chain that lies on the device (gpb_mcmc_diag): x_dev a torch cuda float64 tensor, layout
        "steps" = [nsteps, nwalkers, ndim] (the sampler's store) or "walkers" = [nwalkers, nsteps, ndim] (the pickles), or any
        view of either with unit stride along the parameters (chain[discard::thin]): the strides are passed, nothing is copied.
        max_lag: the largest lag of the autocorrelation function (default nsteps - 1); c: the factor of emcee's automatic window.
        Returns a dict of numpy arrays (torch tensors, asynchronously, with on_device): "rho" [ndim, max_lag + 1], "tau" [ndim],
        "window" [ndim] int32 (bit 30, DIAG_NO_WINDOW: no window inside max_lag; -1: no walker moved), "moments" [ndim, 3]
        (mean, W, B), "rhat" [ndim], "nconst" [ndim] int32.  outputs: the names to compute (default all).  The engine lends its
        device and stream only."""
        import torch
        self._track_stream()
        dev = torch.device("cuda", self.device)
        if layout not in ("steps", "walkers"):
            raise ValueError("layout: 'steps' ([nsteps, nwalkers, ndim]) or 'walkers' ([nwalkers, nsteps, ndim])")
        if not _is_torch(x_dev) or x_dev.dim() != 3:
            raise ValueError("x_dev: expected a three-dimensional torch tensor")
        if not x_dev.is_cuda or x_dev.device.index != self.device or str(x_dev.dtype) != "torch.float64":
            raise ValueError("x_dev: expected a torch.float64 tensor on cuda:%d" % self.device)
        ts, tw = (0, 1) if layout == "steps" else (1, 0)
        n, nw, d = int(x_dev.shape[ts]), int(x_dev.shape[tw]), int(x_dev.shape[2])
        if d > 1 and x_dev.stride(2) != 1:
            raise ValueError("x_dev: expected unit stride along the parameters")
        ss, ws = int(x_dev.stride(ts)), int(x_dev.stride(tw))
        # an axis of extent 1 has no meaningful stride: give it the one of a contiguous array
        if nw == 1 and layout == "steps":
            ws = d
        if n == 1 and layout == "walkers":
            ss = d
        if nw == 1 and layout == "walkers":
            ws = max(ws, ss * n)
        max_lag = n - 1 if max_lag is None else int(max_lag)
        names = ("rho", "tau", "window", "moments", "rhat", "nconst")
        outputs = names if outputs is None else tuple(outputs)
        if any(k not in names for k in outputs):
            raise ValueError("outputs: names among %s" % (names,))
        shapes = {"rho": (d, max(max_lag, 0) + 1), "tau": (d,), "window": (d,), "moments": (d, 3), "rhat": (d,), "nconst": (d,)}
        ints = ("window", "nconst")
        if on_device:
            out = {k: torch.empty(shapes[k], dtype=torch.int32 if k in ints else torch.float64, device=dev) for k in outputs}
        else:
            out = {k: np.empty(shapes[k], dtype=np.int32 if k in ints else np.float64) for k in outputs}
        self._ck(self.lib.gpb_mcmc_diag(self.h, nat.ptr(x_dev), n, nw, d, ss, ws, max_lag, float(c), 1 if on_device else 0,
                                        nat.ptr(out.get("rho")), nat.ptr(out.get("tau")), nat.ptr(out.get("window")),
                                        nat.ptr(out.get("moments")), nat.ptr(out.get("rhat")), nat.ptr(out.get("nconst"))))
        return out

    RANK_NO_BAND = 1 << 30                        # GPB_RANK_NO_BAND
    RANK_MAX_Q = 8                                # GPB_RANK_MAX_Q

    def rank_diag(self, x_dev, layout="steps", probs=(0.05, 0.95), max_lag=None, on_device=False, outputs=None):
        """Rank-normalised diagnostics of a chain that lies on the device (gpb_chain_rank_diag; include/gpbayes.h has the
        statistic): x_dev and layout as mcmc_diag takes them; probs: the levels of the quantile indicators (1 to 8, inside (0, 1));
        max_lag: the largest lag formed (default nsteps // 2 - 1, all).  Returns a dict of numpy arrays (torch tensors,
        asynchronously, with on_device), n = 2 (nsteps // 2) nwalkers, K = 2 + len(probs): "rank2" [ndim, n] int64 (twice the
        average rank of the kept draws, in (step, walker) order), "median" [ndim], "quant" [ndim, nq], "rhat" [ndim, 2] (bulk,
        folded), "ess" [ndim, K] (bulk, mean, the indicators), "stop" [ndim, K] int32 (bit 30, RANK_NO_BAND: the estimator needs
        lags beyond max_lag and ess is NaN; -1: the series never varies), "sd" [ndim].  outputs: the names to compute (default
        all but "rank2").  The engine lends its device, stream and buffer cache only."""
        import torch
        self._track_stream()
        dev = torch.device("cuda", self.device)
        n, nw, d, ss, ws = self._chain_view(x_dev, layout)
        h = n // 2
        probs = nat.f64(np.atleast_1d(np.asarray(probs, dtype=np.float64)).reshape(-1))
        nq = int(probs.shape[0])
        max_lag = h - 1 if max_lag is None else int(max_lag)
        names = ("rank2", "median", "quant", "rhat", "ess", "stop", "sd")
        outputs = names[1:] if outputs is None else tuple(outputs)
        if any(k not in names for k in outputs):
            raise ValueError("outputs: names among %s" % (names,))
        K = 2 + nq
        shapes = {"rank2": (d, 2 * h * nw), "median": (d,), "quant": (d, nq), "rhat": (d, 2), "ess": (d, K), "stop": (d, K), "sd": (d,)}
        types = {"rank2": "int64", "stop": "int32"}
        if on_device:
            out = {k: torch.empty(shapes[k], dtype=getattr(torch, types.get(k, "float64")), device=dev) for k in outputs}
        else:
            out = {k: np.empty(shapes[k], dtype=getattr(np, types.get(k, "float64"))) for k in outputs}
        self._ck(self.lib.gpb_chain_rank_diag(self.h, nat.ptr(x_dev), n, nw, d, ss, ws, nat.ptr(probs), nq, max_lag,
                                              1 if on_device else 0, *[nat.ptr(out.get(k)) for k in names]))
        return out

    MARG_MAX_BINS = 64

    def chain_marginals(self, x_dev, layout="steps", edges=None, pairs=None, weights=None, on_device=False, outputs=None):
        """Histograms of every parameter and parameter pair of a chain that lies on the device (gpb_chain_marginals): x_dev and
        layout as mcmc_diag takes them (a flat [S, ndim] particle set: x_dev[:, None, :]); edges [ndim, B + 1] the bin edges
        per parameter, B <= 64, taken as given: a value is in bin b iff e[b] <= x < e[b + 1], the last bin closed, NaN and the
        rest outside — np.histogram's and np.histogram2d's counts.  pairs [npairs, 2] (default all i < j, lexicographic);
        weights [nsteps] (numpy or torch cuda; one walker only): sample t adds rint(w_t 2^32 / max w) instead of 1.
        Returns a dict of int64 numpy arrays (torch tensors, asynchronously, with on_device): "h1" [ndim, B], "h2" [npairs, B,
        B] (h2[p, bi, bj]: pairs[p, 0] in bin bi, pairs[p, 1] in bin bj), "outside" [ndim].  outputs: the names to compute
        (default all).  Integer accumulation only: equal inputs give equal counts whatever the layout.  The engine lends its
        device and stream only."""
        import torch
        self._track_stream()
        dev = torch.device("cuda", self.device)
        if layout not in ("steps", "walkers"):
            raise ValueError("layout: 'steps' ([nsteps, nwalkers, ndim]) or 'walkers' ([nwalkers, nsteps, ndim])")
        if not _is_torch(x_dev) or x_dev.dim() != 3:
            raise ValueError("x_dev: expected a three-dimensional torch tensor")
        if not x_dev.is_cuda or x_dev.device.index != self.device or str(x_dev.dtype) != "torch.float64":
            raise ValueError("x_dev: expected a torch.float64 tensor on cuda:%d" % self.device)
        ts, tw = (0, 1) if layout == "steps" else (1, 0)
        n, nw, d = int(x_dev.shape[ts]), int(x_dev.shape[tw]), int(x_dev.shape[2])
        if d > 1 and x_dev.stride(2) != 1:
            raise ValueError("x_dev: expected unit stride along the parameters")
        ss, ws = int(x_dev.stride(ts)), int(x_dev.stride(tw))
        # an axis of extent 1 has no meaningful stride: give it the one of a contiguous array
        if nw == 1 and layout == "steps":
            ws = d
        if n == 1 and layout == "walkers":
            ss = d
        if nw == 1 and layout == "walkers":
            ws = max(ws, ss * n)
        if n == 1 and layout == "steps":
            ss = max(ss, ws * nw)
        edges = nat.f64(edges)
        if edges.ndim != 2 or edges.shape[0] != d or edges.shape[1] < 2:
            raise ValueError("edges: expected [%d, B + 1]" % d)
        B = int(edges.shape[1]) - 1
        if pairs is None:
            npairs = d * (d - 1) // 2
        else:
            pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
            npairs = int(pairs.shape[0])
        wscale = 1.0
        if weights is not None:
            if not _is_torch(weights):
                weights = torch.as_tensor(nat.f64(weights).reshape(-1), device=dev)
            weights = self._dev(weights, (n,), "weights", contiguous=False)
            wmax = float(weights.max()) if n else 0.0
            if not (wmax > 0.0) or not np.isfinite(wmax):
                raise ValueError("weights: the largest weight must be positive and finite")
            wscale = 4294967296.0 / wmax
        names = ("h1", "h2", "outside")
        outputs = names if outputs is None else tuple(outputs)
        if any(k not in names for k in outputs):
            raise ValueError("outputs: names among %s" % (names,))
        shapes = {"h1": (d, B), "h2": (npairs, B, B), "outside": (d,)}
        if on_device:
            out = {k: torch.empty(shapes[k], dtype=torch.int64, device=dev) for k in outputs}
        else:
            out = {k: np.empty(shapes[k], dtype=np.int64) for k in outputs}
        self._ck(self.lib.gpb_chain_marginals(self.h, nat.ptr(x_dev), n, nw, d, ss, ws, nat.ptr(edges), B, nat.ptr(pairs), npairs,
                                              nat.ptr(weights), wscale, 1 if on_device else 0, nat.ptr(out.get("h1")),
                                              nat.ptr(out.get("h2")), nat.ptr(out.get("outside"))))
        return out

    def _chain_view(self, x_dev, layout):
        """(nsteps, nwalkers, ndim, step stride, walker stride) of a device chain as chain_marginals takes it"""
        if layout not in ("steps", "walkers"):
            raise ValueError("layout: 'steps' ([nsteps, nwalkers, ndim]) or 'walkers' ([nwalkers, nsteps, ndim])")
        if not _is_torch(x_dev) or x_dev.dim() != 3:
            raise ValueError("x_dev: expected a three-dimensional torch tensor")
        if not x_dev.is_cuda or x_dev.device.index != self.device or str(x_dev.dtype) != "torch.float64":
            raise ValueError("x_dev: expected a torch.float64 tensor on cuda:%d" % self.device)
        ts, tw = (0, 1) if layout == "steps" else (1, 0)
        n, nw, d = int(x_dev.shape[ts]), int(x_dev.shape[tw]), int(x_dev.shape[2])
        if d > 1 and x_dev.stride(2) != 1:
            raise ValueError("x_dev: expected unit stride along the parameters")
        ss, ws = int(x_dev.stride(ts)), int(x_dev.stride(tw))
        # an axis of extent 1 has no meaningful stride: give it the one of a contiguous array
        if nw == 1 and layout == "steps":
            ws = d
        if n == 1 and layout == "walkers":
            ss = d
        if nw == 1 and layout == "walkers":
            ws = max(ws, ss * n)
        if n == 1 and layout == "steps":
            ss = max(ss, ws * nw)
        return n, nw, d, ss, ws

    CURVE_FNS = {"zeta_over_s": 0, "eta_over_s": 1, "y_loss": 2, "delta": 3}
    CURVES_MAX, CURVES_MAX_GRID = 8, 1024

    def chain_curves(self, x_dev, layout="steps", desc=None, grid=None, q=None, aux=None, values=False, on_device=False):
        """Order statistics over all samples of parametrised curves of a chain that lies on the device (gpb_chain_curves): x_dev
        and layout as chain_marginals takes them; desc [ncurves, 5] int32 rows (fn, col0 .. col3; -1 unused; CURVE_FNS), grid
        [ncurves, G], q the levels in [0, 1] (at most 16; None: no select), aux = truth [ndim] | width [ndim] for fn 3.  Sample
        s = step * nwalkers + walker in either layout.  Returns a dict: "order" [ncurves, G, nq, 2] (with q), the two order
        statistics numpy's percentile interpolates between, selected exactly WITHOUT forming the [G, S] values; "values"
        [ncurves, G, S] (values=True), the materialised curves — meant for small S and for fn 3.  numpy out, or with on_device
        torch tensors (asynchronous).  The engine lends its device, stream and buffer cache only."""
        import torch
        self._track_stream()
        dev = torch.device("cuda", self.device)
        n, nw, d, ss, ws = self._chain_view(x_dev, layout)
        S = n * nw
        desc = np.ascontiguousarray(np.asarray(desc, dtype=np.int32).reshape(-1, 5))
        ncurves = int(desc.shape[0])
        grid = nat.f64(np.asarray(grid, dtype=np.float64).reshape(ncurves, -1))
        G = int(grid.shape[1])
        aux = None if aux is None else nat.f64(np.asarray(aux, dtype=np.float64).reshape(-1))
        if aux is not None and aux.shape[0] != 2 * d:
            raise ValueError("aux: expected truth [%d] | width [%d]" % (d, d))
        nq = 0
        if q is not None:
            q = nat.f64(np.atleast_1d(np.asarray(q, dtype=np.float64))).reshape(-1)
            nq = int(q.shape[0])
        shapes = {}
        if q is not None:
            shapes["order"] = (ncurves, G, nq, 2)
        if values:
            shapes["values"] = (ncurves, G, S)
        if on_device:
            out = {k: torch.empty(s, dtype=torch.float64, device=dev) for k, s in shapes.items()}
        else:
            out = {k: np.empty(s) for k, s in shapes.items()}
        self._ck(self.lib.gpb_chain_curves(self.h, nat.ptr(x_dev), n, nw, d, ss, ws, ncurves, nat.ptr(desc), nat.ptr(aux), nat.ptr(grid),
                                           G, nat.ptr(q), nq, 1 if on_device else 0, nat.ptr(out.get("order")),
                                           nat.ptr(out.get("values")), S))
        return out

    def chain_trace_hist(self, x_dev, layout="steps", edges=None, on_device=False, outputs=None):
        """The walkers' distribution step by step (gpb_chain_trace_hist): x_dev and layout as chain_marginals takes them, edges
        [ndim, B + 1] with its bin rule, B <= 64.  Returns a dict of int64 arrays: "hist" [ndim, nsteps, B], hist[j, t, b] the
        walkers of step t with parameter j in bin b — np.histogram2d(step, value, bins=[nsteps, edges[j]]) — and "outside"
        [ndim, nsteps].  numpy out, or with on_device torch tensors (asynchronous)."""
        import torch
        self._track_stream()
        dev = torch.device("cuda", self.device)
        n, nw, d, ss, ws = self._chain_view(x_dev, layout)
        edges = nat.f64(edges)
        if edges.ndim != 2 or edges.shape[0] != d or edges.shape[1] < 2:
            raise ValueError("edges: expected [%d, B + 1]" % d)
        B = int(edges.shape[1]) - 1
        names = ("hist", "outside")
        outputs = names if outputs is None else tuple(outputs)
        if any(k not in names for k in outputs):
            raise ValueError("outputs: names among %s" % (names,))
        shapes = {"hist": (d, n, B), "outside": (d, n)}
        if on_device:
            out = {k: torch.empty(shapes[k], dtype=torch.int64, device=dev) for k in outputs}
        else:
            out = {k: np.empty(shapes[k], dtype=np.int64) for k in outputs}
        self._ck(self.lib.gpb_chain_trace_hist(self.h, nat.ptr(x_dev), n, nw, d, ss, ws, nat.ptr(edges), B, 1 if on_device else 0,
                                               nat.ptr(out.get("hist")), nat.ptr(out.get("outside"))))
        return out

    KMEANS_MAX_K, KMEANS_MAX_RESTARTS = 32, 16

    def chain_kmeans(self, x_dev, layout="steps", k=10, n_init=10, init=None, u=None, weights=None, max_iter=300, tol=1e-4,
                     standardize=True, return_labels=False):
        """Weighted k-means of the rows of a chain that lies on the device (gpb_chain_kmeans), n_init restarts in lock-step:
        x_dev and layout as chain_marginals takes them (a flat [S, ndim] particle set: x_dev[:, None, :]; ndim <= 64).  Exactly
        one of init [n_init, k, ndim] (the starting centres, in the chain's units) and u [n_init, k] (uniforms in [0, 1) that
        drive the k-means++ seeding) is given; weights [nsteps] (numpy or torch cuda, non-negative; one walker only).  The rows
        are standardised on the fly (standardize=False: taken as they are); a row with a non-finite coordinate is skipped.
        Returns a dict of numpy arrays: "centers" [n_init, k, ndim] (the chain's units), "inertia", "n_iter", "converged"
        [n_init], "size" (rows of positive weight, int64) and "wsum" [n_init, k], "mean", "scale" [ndim], "seed_index"
        [n_init, k] (int64; -1 with init), "best", "n_skipped" (ints) and, with return_labels, "labels" [S] (a torch int32
        cuda tensor: the best restart's labels in row order — the outer axis of the memory layout first —, -1 for a skipped
        row).  Integer accumulation: equal inputs give equal bits, and a restart's result does not depend on the restarts that
        share the call.  The engine lends its device and stream only."""
        import torch
        self._track_stream()
        dev = torch.device("cuda", self.device)
        if layout not in ("steps", "walkers"):
            raise ValueError("layout: 'steps' ([nsteps, nwalkers, ndim]) or 'walkers' ([nwalkers, nsteps, ndim])")
        if not _is_torch(x_dev) or x_dev.dim() != 3:
            raise ValueError("x_dev: expected a three-dimensional torch tensor")
        if not x_dev.is_cuda or x_dev.device.index != self.device or str(x_dev.dtype) != "torch.float64":
            raise ValueError("x_dev: expected a torch.float64 tensor on cuda:%d" % self.device)
        ts, tw = (0, 1) if layout == "steps" else (1, 0)
        n, nw, d = int(x_dev.shape[ts]), int(x_dev.shape[tw]), int(x_dev.shape[2])
        if d > 1 and x_dev.stride(2) != 1:
            raise ValueError("x_dev: expected unit stride along the parameters")
        ss, ws = int(x_dev.stride(ts)), int(x_dev.stride(tw))
        # an axis of extent 1 has no meaningful stride: give it the one of a contiguous array
        if nw == 1 and layout == "steps":
            ws = d
        if n == 1 and layout == "walkers":
            ss = d
        if nw == 1 and layout == "walkers":
            ws = max(ws, ss * n)
        if n == 1 and layout == "steps":
            ss = max(ss, ws * nw)
        k, R = int(k), int(n_init)
        if (init is None) == (u is None):
            raise ValueError("exactly one of init [n_init, k, ndim] and u [n_init, k]")
        if init is not None:
            init = nat.f64(init)
            if init.shape != (R, k, d):
                raise ValueError("init: expected [%d, %d, %d]" % (R, k, d))
        else:
            u = nat.f64(u)
            if u.shape != (R, k):
                raise ValueError("u: expected [%d, %d]" % (R, k))
        if weights is not None:
            if not _is_torch(weights):
                weights = torch.as_tensor(nat.f64(weights).reshape(-1), device=dev)
            weights = self._dev(weights, (n,), "weights", contiguous=False)
        Rk = (max(R, 0), max(k, 0))
        out = {"centers": np.empty(Rk + (d,)), "inertia": np.empty(Rk[0]), "n_iter": np.empty(Rk[0], dtype=np.int32),
               "converged": np.empty(Rk[0], dtype=np.int32), "size": np.empty(Rk, dtype=np.int64), "wsum": np.empty(Rk),
               "mean": np.empty(d), "scale": np.empty(d), "seed_index": np.empty(Rk, dtype=np.int64)}
        best, nskip = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int64)
        labels = torch.empty(n * nw, dtype=torch.int32, device=dev) if return_labels else None
        self._ck(self.lib.gpb_chain_kmeans(self.h, nat.ptr(x_dev), n, nw, d, ss, ws, nat.ptr(weights), k, R, int(max_iter), float(tol),
                                           1 if standardize else 0, nat.ptr(init), nat.ptr(u), nat.ptr(out["centers"]),
                                           nat.ptr(out["inertia"]), nat.ptr(out["n_iter"]), nat.ptr(out["converged"]),
                                           nat.ptr(out["size"]), nat.ptr(out["wsum"]), nat.ptr(out["mean"]), nat.ptr(out["scale"]),
                                           nat.ptr(out["seed_index"]), nat.ptr(best), nat.ptr(nskip), nat.ptr(labels)))
        out["best"], out["n_skipped"] = int(best[0]), int(nskip[0])
        if return_labels:
            out["labels"] = labels
        return out

    KNN_MAX_K = 16

    def chain_knn(self, a_dev, layout="steps", b_dev=None, layout_b=None, k=8, inv_scale=None, skip_zero=True, splits=0,
                  on_device=False, return_index=True, return_zeros=True):
        """For every row of a chain that lies on the device the k smallest squared distances to the rows of the chain itself
        (b_dev None; the row itself excluded) or of another chain b_dev (gpb_chain_knn): a_dev, b_dev and their layouts as
        chain_marginals takes them (a flat [S, ndim] set: x[:, None, :]; ndim <= 64), k <= 16.  Every coordinate is multiplied
        by inv_scale [ndim] (default ones) first; the squared distance is acc = acc + t * t over the coordinates in order, no
        fused multiply-add, which numpy reproduces bit for bit.  A row with a non-finite coordinate is skipped (r2 = inf, idx =
        -1; never a candidate); a candidate at distance 0 is counted in "zeros" and, with skip_zero, not listed.  Returns a
        dict: "r2" [nA, k] ascending, "idx" [nA, k] (int32 row numbers, outer axis of the memory layout first; equal distances
        by ascending row number; -1 where fewer than k candidates exist), "zeros" [nA] (int32), "n_skipped" (skipped rows of A,
        of B).  numpy out, or torch tensors with on_device.  splits (0: automatic) changes no output.  The engine lends its
        device, stream and buffer cache only."""
        import torch
        self._track_stream()
        dev = torch.device("cuda", self.device)
        na, nwa, d, ssa, wsa = self._chain_view(a_dev, layout)
        nA = na * nwa
        if b_dev is not None:
            nb, nwb, db, ssb, wsb = self._chain_view(b_dev, layout_b or layout)
            if db != d:
                raise ValueError("b_dev: %d parameters, a_dev has %d" % (db, d))
        else:
            nb = nwb = ssb = wsb = 0
        inv = np.ones(d) if inv_scale is None else nat.f64(np.asarray(inv_scale, dtype=np.float64).reshape(-1))
        if inv.shape[0] != d:
            raise ValueError("inv_scale: expected [%d]" % d)
        k = int(k)
        kk = max(k, 0)
        if on_device:
            out = {"r2": torch.empty((nA, kk), dtype=torch.float64, device=dev)}
            if return_index:
                out["idx"] = torch.empty((nA, kk), dtype=torch.int32, device=dev)
            if return_zeros:
                out["zeros"] = torch.empty((nA,), dtype=torch.int32, device=dev)
        else:
            out = {"r2": np.empty((nA, kk))}
            if return_index:
                out["idx"] = np.empty((nA, kk), dtype=np.int32)
            if return_zeros:
                out["zeros"] = np.empty((nA,), dtype=np.int32)
        nskip = np.zeros(2, dtype=np.int64)
        self._ck(self.lib.gpb_chain_knn(self.h, nat.ptr(a_dev), na, nwa, ssa, wsa, nat.ptr(b_dev), nb, nwb, ssb, wsb, d, nat.ptr(inv), k,
                                        1 if skip_zero else 0, int(splits), 1 if on_device else 0, nat.ptr(out["r2"]),
                                        nat.ptr(out.get("idx")), nat.ptr(out.get("zeros")), nat.ptr(nskip)))
        out["n_skipped"] = (int(nskip[0]), int(nskip[1]))
        return out

    STEIN_MAX_M, STEIN_MAX_SPLITS = 1 << 20, 64

    def _stein_inputs(self, x, g, ginv):
        """the shared arguments of stein_thin / stein_ksd: x, g float64 cuda tensors [n, d] with unit stride along d (a [::k] view
        of a longer array is fine: its row stride goes to the library), ginv [d, d] on the host"""
        for name, a in (("x", x), ("g", g)):
            if not (_is_torch(a) and a.is_cuda and a.device.index == self.device and str(a.dtype) == "torch.float64" and a.dim() == 2):
                raise ValueError("%s: a float64 tensor [n, d] on cuda:%d" % (name, self.device))
        n, d = int(x.shape[0]), int(x.shape[1])
        if tuple(g.shape) != (n, d):
            raise ValueError("g: expected the shape of x, %s" % ((n, d),))
        if d > 64:
            raise ValueError("x: %d parameters, at most 64" % d)
        for name, a in (("x", x), ("g", g)):
            if d > 1 and a.stride(1) != 1:
                raise ValueError("%s: expected unit stride along the parameters" % name)
        xs, gs = (int(a.stride(0)) if n > 1 else max(int(a.stride(0)), d) for a in (x, g))
        ginv = nat.f64(np.asarray(ginv, dtype=np.float64))
        if ginv.shape != (d, d):
            raise ValueError("ginv: expected [%d, %d]" % (d, d))
        return n, d, xs, gs, ginv

    def stein_thin(self, x, g, ginv, m, on_device=False, return_obj=False):
        """Stein thinning of the rows x [n, d] with scores g [n, d] (float64 cuda tensors; d <= 64) under the inverse
        multiquadric kernel with the preconditioner ginv = Gamma^-1 [d, d] (host, SPD): greedily the m rows whose empirical
        measure has the smallest kernel Stein discrepancy (gpb_stein_thin; the rule is in include/gpbayes.h and
        tests/stein_reference.py reproduces it bit for bit).  Returns a dict: "idx" [m] (int32 row numbers; rows may repeat; -1
        when no row can be picked), "ksd" [m] (ksd[t - 1]: the discrepancy of the first t picks), "n_skipped" (rows with a
        non-finite x, g or Gamma^-1 x: never picked, left out of every sum) and, with return_obj, "obj" [n] (the objective after
        the last update; NaN for a skipped row).  numpy out, or torch tensors with on_device.  All m iterations are enqueued
        in one call.  The engine lends its device, stream and buffer cache only."""
        import torch
        self._track_stream()
        dev = torch.device("cuda", self.device)
        n, d, xs, gs, ginv = self._stein_inputs(x, g, ginv)
        m = int(m)
        mm = min(max(m, 0), self.STEIN_MAX_M)
        if on_device:
            out = {"idx": torch.empty(mm, dtype=torch.int32, device=dev), "ksd": torch.empty(mm, dtype=torch.float64, device=dev)}
            if return_obj:
                out["obj"] = torch.empty(n, dtype=torch.float64, device=dev)
        else:
            out = {"idx": np.empty(mm, dtype=np.int32), "ksd": np.empty(mm)}
            if return_obj:
                out["obj"] = np.empty(n)
        nskip = np.zeros(1, dtype=np.int64)
        self._ck(self.lib.gpb_stein_thin(self.h, nat.ptr(x), nat.ptr(g), n, d, xs, gs, nat.ptr(ginv), m, 1 if on_device else 0,
                                         nat.ptr(out["idx"]), nat.ptr(out["ksd"]), nat.ptr(out.get("obj")), nat.ptr(nskip)))
        out["n_skipped"] = int(nskip[0])
        return out

    def stein_ksd(self, x, g, ginv, splits=0, on_device=False, return_rows=False):
        """The kernel Stein discrepancy of ALL rows x [n, d] with scores g [n, d] (as stein_thin takes them): n^2 pair
        evaluations in fp64 (gpb_stein_ksd).  Returns a dict: "ksd2" (the squared discrepancy sum_ij kp(i, j) / n_valid^2; a
        float, or a one-element tensor with on_device), "ksd" (its square root; host mode only), "n_skipped" and, with
        return_rows, "row_sum" [n] (sum_j kp(i, j); NaN for a skipped row).  The summation order is fixed by the header: splits
        (0: automatic) and the library's slabs change no bit."""
        import torch
        self._track_stream()
        dev = torch.device("cuda", self.device)
        n, d, xs, gs, ginv = self._stein_inputs(x, g, ginv)
        if on_device:
            ksd2 = torch.empty(1, dtype=torch.float64, device=dev)
            rows = torch.empty(n, dtype=torch.float64, device=dev) if return_rows else None
        else:
            ksd2 = np.empty(1)
            rows = np.empty(n) if return_rows else None
        nskip = np.zeros(1, dtype=np.int64)
        self._ck(self.lib.gpb_stein_ksd(self.h, nat.ptr(x), nat.ptr(g), n, d, xs, gs, nat.ptr(ginv), int(splits), 1 if on_device else 0,
                                        nat.ptr(rows), nat.ptr(ksd2), nat.ptr(nskip)))
        out = {"ksd2": ksd2 if on_device else float(ksd2[0]), "n_skipped": int(nskip[0])}
        if not on_device:
            out["ksd"] = float(np.sqrt(ksd2[0]))
        if return_rows:
            out["row_sum"] = rows
        return out

    EIG_MAX_M, EIG_MAX_GROUPS, EIG_MAX_SPLITS = 4096, 64, 64

    def _eig_inputs(self, mu_T, var_T, vadd, outer_idx):
        """the shared arguments of eig_simulate / eig_lse: observable-major float64 cuda tensors [M, S_in] whose rows are
        contiguous (a column slice of a wider array is fine: its stride is ld_in), vadd [M] and outer_idx [S_out] uploaded when
        they come as numpy"""
        import torch
        dev = torch.device("cuda", self.device)
        for name, a in (("mu_T", mu_T), ("var_T", var_T)):
            if a is None and name == "var_T":
                continue
            if not (hasattr(a, "data_ptr") and a.is_cuda and a.dtype == torch.float64 and a.dim() == 2 and a.stride(1) == 1):
                raise ValueError("%s: a float64 cuda tensor [M, S_in] with contiguous rows" % name)
        M, S_in = int(mu_T.shape[0]), int(mu_T.shape[1])
        ld_in = int(mu_T.stride(0)) if M > 1 else max(int(mu_T.stride(0)), S_in)
        if var_T is not None and (tuple(var_T.shape) != (M, S_in) or (M > 1 and int(var_T.stride(0)) != ld_in)):
            raise ValueError("var_T: the shape and row stride of mu_T")
        if vadd is not None:
            vadd = torch.as_tensor(np.ascontiguousarray(vadd, dtype=np.float64) if not hasattr(vadd, "data_ptr") else vadd,
                                   device=dev).contiguous()
            if tuple(vadd.shape) != (M,) or vadd.dtype != torch.float64:
                raise ValueError("vadd: float64 [%d]" % M)
        if not hasattr(outer_idx, "data_ptr"):
            outer_idx = torch.as_tensor(np.ascontiguousarray(outer_idx, dtype=np.int32), device=dev)
        outer_idx = outer_idx.contiguous()
        if outer_idx.dtype != torch.int32 or outer_idx.dim() != 1 or not outer_idx.is_cuda:
            raise ValueError("outer_idx: int32 [S_out]")
        return dev, M, S_in, ld_in, vadd, outer_idx

    def eig_simulate(self, mu_T, var_T, vadd, outer_idx, seed, out=None, return_z=False):
        """Simulated measurements for the expected information gain (gpb_eig_simulate): y[m, i] = mu[m, o_i] + sqrt(var[m, o_i] +
        vadd[m]) z[m, i] with o = outer_idx [S_out] (int32) and z ~ N(0, 1) from the Philox counter (i, m // 2, 0, tag 15) —
        keyed by the position i, so repeated indices get different noise.  mu_T, var_T: observable-major float64 cuda tensors
        [M, S_in] (var_T or vadd may be None: zeros).  Returns y_T [M, S_out] (cuda; `out`: a tensor whose first S_out columns are
        written, the others left alone), with return_z also z_T."""
        import torch
        self._track_stream()
        dev, M, S_in, ld_in, vadd, outer_idx = self._eig_inputs(mu_T, var_T, vadd, outer_idx)
        S_out = int(outer_idx.shape[0])
        y = torch.empty((M, S_out), dtype=torch.float64, device=dev) if out is None else out
        if not (y.is_cuda and y.dtype == torch.float64 and y.dim() == 2 and y.shape[0] == M and y.stride(1) == 1):
            raise ValueError("out: a float64 cuda tensor [M, >= S_out] with contiguous rows")
        ld_out = int(y.stride(0)) if M > 1 else max(int(y.stride(0)), int(y.shape[1]))
        z = torch.empty_strided(tuple(y.shape), tuple(y.stride()), dtype=torch.float64, device=dev) if return_z else None
        if z is not None:
            z.zero_()                                  # (the columns behind S_out are not written)
        self._ck(self.lib.gpb_eig_simulate(self.h, nat.ptr(mu_T), nat.ptr(var_T), nat.ptr(vadd), M, S_in, ld_in, nat.ptr(outer_idx),
                                           S_out, int(seed) & 0xFFFFFFFFFFFFFFFF, nat.ptr(y), nat.ptr(z), ld_out))
        return (y, z) if return_z else y

    def eig_lse(self, mu_T, var_T, vadd, logw, y_T, outer_idx, ranges, splits=0, on_device=False):
        """For every simulated data vector y_i (column i of y_T [M, >= S_out]) and every group g of observables
        [ranges[g, 0], ranges[g, 1]): lse_excl[g, i] = ln sum_{j != o_i} exp l_ij(g) over the inner samples and self[g, i] =
        l_{i, o_i}(g), with l_ij(g) = logw_j - sum_{m in g} [(y_im - mu_jm)^2 / s_jm + ln s_jm] / 2 and s = var_T + vadd
        (gpb_eig_lse: a matrix product on the fp64 matrix pipe with an online log-sum-exp; no S_out x S_in array exists).  mu_T,
        var_T, y_T: observable-major float64 cuda tensors; var_T, vadd, logw may be None.  Inputs must be finite with s > 0: the
        caller checks (eig.py does).  Returns (lse_excl, self), [G, S_out] each, numpy or, with on_device, torch.  splits (0:
        automatic) changes the values only within the rounding of the sum."""
        import torch
        self._track_stream()
        dev, M, S_in, ld_in, vadd, outer_idx = self._eig_inputs(mu_T, var_T, vadd, outer_idx)
        S_out = int(outer_idx.shape[0])
        if not (hasattr(y_T, "data_ptr") and y_T.is_cuda and y_T.dtype == torch.float64 and y_T.dim() == 2 and y_T.shape[0] == M
                and y_T.stride(1) == 1):
            raise ValueError("y_T: a float64 cuda tensor [M, >= S_out] with contiguous rows")
        ld_out = int(y_T.stride(0)) if M > 1 else max(int(y_T.stride(0)), int(y_T.shape[1]))
        if logw is not None:
            logw = torch.as_tensor(np.ascontiguousarray(logw, dtype=np.float64) if not hasattr(logw, "data_ptr") else logw,
                                   device=dev).contiguous()
            if tuple(logw.shape) != (S_in,) or logw.dtype != torch.float64:
                raise ValueError("logw: float64 [%d]" % S_in)
        rg = np.ascontiguousarray(np.asarray(ranges, dtype=np.int32).reshape(-1, 2))
        G = int(rg.shape[0])
        if on_device:
            lse, slf = (torch.empty((G, S_out), dtype=torch.float64, device=dev) for _ in range(2))
        else:
            lse, slf = np.empty((G, S_out)), np.empty((G, S_out))
        self._ck(self.lib.gpb_eig_lse(self.h, nat.ptr(mu_T), nat.ptr(var_T), nat.ptr(vadd), nat.ptr(logw), M, S_in, ld_in, nat.ptr(y_T),
                                      nat.ptr(outer_idx), S_out, ld_out, nat.ptr(rg), G, int(splits), 1 if on_device else 0,
                                      nat.ptr(lse), nat.ptr(slf)))
        return lse, slf

    HM_MAX_D, HM_MAX_K, HM_MAX_GROUPS = 512, 4, 64

    def _hm_rows(self, t, name, rows=None, dtype="torch.float64"):
        """a cuda view [rows, >= 1] with unit stride along its columns, as the history-matching calls read and write them; returns
        its leading dimension"""
        if not _is_torch(t) or not t.is_cuda or t.device.index != self.device or str(t.dtype) != dtype:
            raise ValueError("%s: expected a %s tensor on cuda:%d" % (name, dtype, self.device))
        if t.dim() != 2 or (rows is not None and t.shape[0] != rows) or t.shape[1] < 1 or (t.shape[1] > 1 and t.stride(1) != 1) \
                or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
            raise ValueError("%s: expected a [%s, n] view with unit stride along its columns" % (name, "rows" if rows is None else rows))
        return int(t.stride(0)) if t.shape[0] > 1 else int(t.shape[1])

    def hm_uniform(self, lo, hi, S, seed=0, row0=0, out=None):
        """Candidate rows drawn uniformly in the box [lo, hi) on the device (gpb_hm_uniform): x[r, j] = lo_j + (hi_j - lo_j) u with u
        the 53-bit uniform of the Philox counter (row0 + r, j, tag 16) — keyed by the ABSOLUTE row, so a row's bits do not depend
        on how the rows are cut into calls.  Returns a cuda tensor [S, d] (`out`: a [S, >= d] view whose first d columns are
        written)."""
        import torch
        self._track_stream()
        lo, hi = nat.f64(lo).reshape(-1), nat.f64(hi).reshape(-1)
        d, S = int(lo.shape[0]), int(S)
        if hi.shape[0] != d:
            raise ValueError("hm_uniform: lo and hi differ in length")
        if out is None:
            out = torch.empty((S, d), dtype=torch.float64, device=torch.device("cuda", self.device))
        ld = self._hm_rows(out, "out", S)
        if out.shape[1] < d:
            raise ValueError("out: expected [%d, >= %d]" % (S, d))
        self._ck(self.lib.gpb_hm_uniform(self.h, nat.ptr(lo), nat.ptr(hi), d, int(row0) & 0xFFFFFFFFFFFFFFFF, S,
                                         int(seed) & 0xFFFFFFFFFFFFFFFF, nat.ptr(out), ld))
        return out

    def hm_implausibility(self, mu_T, var_T, yexp, vadd=None, ranges=None, K=1, S=None, want_arg=True, bad=None, on_device=False):
        """The univariate implausibility of every sample under every observable (gpb_hm_implausibility): mu_T, var_T (None = 0)
        observable-major cuda views [M, >= S] as emu_predict_diag writes them, yexp, vadd (None = 0; +inf masks an observable) [M],
        numpy or torch cuda; I = |yexp - mu| / sqrt(var + vadd), 0 / +inf where the variance is not positive.  Returns a dict:
        "top" [K, S] the K (<= 4) largest per sample, "arg" [S] (int32) the observable of the largest (lowest on ties; omitted
        with want_arg=False), "gmax" [G, S] the largest over each range [m0, m1) of `ranges` (omitted without ranges), "bad" the
        int64 device counter [1] the number of samples with an undefined implausibility was ADDED to (`bad`: an earlier call's, to
        go on counting).  numpy arrays (and "bad" an int), or with on_device torch tensors without a synchronisation."""
        import torch
        self._track_stream()
        dev = torch.device("cuda", self.device)
        ld = self._hm_rows(mu_T, "mu_T")
        M = int(mu_T.shape[0])
        S = int(mu_T.shape[1]) if S is None else int(S)
        if S > mu_T.shape[1]:
            raise ValueError("S: more samples than mu_T has columns")
        if var_T is not None:
            if self._hm_rows(var_T, "var_T", M) != ld or var_T.shape[1] < S:
                raise ValueError("var_T: expected the shape and row stride of mu_T")

        def vec(a, name):
            if a is None:
                return None
            a = a if _is_torch(a) else torch.as_tensor(nat.f64(a).reshape(-1), device=dev)
            return self._dev(a, (M,), name, contiguous=False)
        yexp, vadd = vec(yexp, "yexp"), vec(vadd, "vadd")
        if yexp is None:
            raise ValueError("yexp: needed")
        rg = None if ranges is None else np.ascontiguousarray(np.asarray(ranges, dtype=np.int32).reshape(-1, 2))
        G, K = (0 if rg is None else int(rg.shape[0])), int(K)
        top = torch.empty((K, S), dtype=torch.float64, device=dev) if K > 0 else None
        arg = torch.empty((S,), dtype=torch.int32, device=dev) if want_arg else None
        gmax = torch.empty((G, S), dtype=torch.float64, device=dev) if G > 0 else None
        if bad is None:
            bad = torch.zeros((1,), dtype=torch.int64, device=dev)
        self._dev(bad, (1,), "bad", dtype="torch.int64")
        self._ck(self.lib.gpb_hm_implausibility(self.h, nat.ptr(mu_T), nat.ptr(var_T), M, S, ld, nat.ptr(yexp), nat.ptr(vadd), nat.ptr(rg),
                                                G, K, nat.ptr(top), nat.ptr(arg), nat.ptr(gmax), S, nat.ptr(bad)))
        out = {"top": top, "bad": bad}
        if want_arg:
            out["arg"] = arg
        if G > 0:
            out["gmax"] = gmax
        if on_device:
            return out
        return {k: (int(v.item()) if k == "bad" else v.cpu().numpy()) for k, v in out.items()}

    def hm_maps(self, X, score, cutoff, edges, pairs=None, into=None, outputs=("1d", "2d"), on_device=False):
        """Minimum-score and count maps of rows over the bins of every parameter and parameter pair (gpb_hm_maps): X a cuda view
        [S, >= d] with unit stride along the parameters, score [S] cuda (no NaN), edges [d, B + 1] (B <= 64; chain_marginals' bin
        rule), pairs [npairs, 2] (default all i < j).  Returns a dict with, for "1d" in outputs, "min1" (float64), "cnt1", "nroy1"
        (int64) [d, B] and, for "2d", "min2", "cnt2", "nroy2" [npairs, B, B]: per bin the smallest score, the number of rows and the
        number of rows with score < cutoff (strict); an empty bin reads +inf, 0, 0.  into: the device dict of an earlier call, to
        accumulate onto (slabs add up; integer minima and adds only, so the result does not depend on the slabs).  numpy arrays, or
        with on_device (and always with `into`) the device tensors, without a synchronisation."""
        import torch
        self._track_stream()
        dev = torch.device("cuda", self.device)
        edges = nat.f64(edges)
        if edges.ndim != 2 or edges.shape[1] < 2:
            raise ValueError("edges: expected [d, B + 1]")
        d, B = int(edges.shape[0]), int(edges.shape[1]) - 1
        row_stride = self._hm_rows(X, "X")
        S = int(X.shape[0])
        if X.shape[1] < d:
            raise ValueError("X: expected [S, >= %d]" % d)
        if S == 1:
            row_stride = max(row_stride, d)
        score = self._dev(score, (S,), "score", contiguous=False)
        if pairs is None:
            npairs = d * (d - 1) // 2
        else:
            pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
            npairs = int(pairs.shape[0])
        outputs = tuple(outputs)
        if not outputs or any(k not in ("1d", "2d") for k in outputs):
            raise ValueError("outputs: '1d' and / or '2d'")
        shapes = {"1": (d, B), "2": (npairs, B, B)}
        names = [n + o[0] for o in outputs for n in ("min", "cnt", "nroy")]
        if into is None:
            out = {k: torch.empty(shapes[k[-1]], dtype=torch.float64 if k[:3] == "min" else torch.int64, device=dev) for k in names}
        else:
            out = into
            for k in names:
                self._dev(out[k], shapes[k[-1]], "into[%r]" % k, dtype="torch.float64" if k[:3] == "min" else "torch.int64")
        self._ck(self.lib.gpb_hm_maps(self.h, nat.ptr(X), S, d, row_stride, nat.ptr(score), float(cutoff), nat.ptr(edges), B, nat.ptr(pairs),
                                      npairs, 1 if into is None else 0, *[nat.ptr(out.get(k)) for k in
                                                                          ("min1", "cnt1", "nroy1", "min2", "cnt2", "nroy2")]))
        if on_device or into is not None:
            return out
        return {k: v.cpu().numpy() for k, v in out.items()}

    MAXPRO_N, MAXPRO_D, MAXPRO_MAX_RESTARTS, MAXPRO_MAX_BLOCK =(4, 4096), (2, 64), 16, 64

    def _maxpro_shape(self, n, d):
        if not self.MAXPRO_N[0] <= n <= self.MAXPRO_N[1]:
            raise ValueError("maxpro: n = %d outside %d .. %d" % ((n,) + self.MAXPRO_N))
        if not self.MAXPRO_D[0] <= d <= self.MAXPRO_D[1]:
            raise ValueError("maxpro: d = %d outside %d .. %d" % ((d,) + self.MAXPRO_D))

    def maxpro_lhd(self, init, seed, n_stages, blocks_per_stage, block=32, temp0=0.001, cool=0.75, restart0=0, return_trace=False):
        """Maximum-projection Latin hypercubes by simulated annealing over column-wise swaps on the device (gpb_maxpro_lhd;
        DESIGN.md section 24): init [R, n, d] integer levels, every column a permutation of 0 .. n - 1 (R <= 16 independent
        restarts, 4 <= n <= 4096, 2 <= d <= 64); stage k of n_stages runs blocks_per_stage blocks of `block` proposals at the
        temperature temp0 cool^k; the draws are keyed by (seed, block, restart0 + r, slot).  Returns a dict of numpy arrays:
        "levels" [R, n, d] (int32, the best levels each restart has seen), "f_start", "f_best" [R] (f = ln sum of the pair terms;
        f_best recomputed from the levels), "lnpsi_start", "lnpsi" [R] (the MaxPro criterion), "accepted", "consumed" [R] (int64)
        and, with return_trace, "trace" [R, n_stages blocks_per_stage] (int32: per block the accepted slot, or -1).  The engine
        lends its device and stream only."""
        self._check_pid()
        init = np.asarray(init)
        if init.ndim != 3 or not np.issubdtype(init.dtype, np.integer):
            raise ValueError("init: expected integer levels [R, n, d]")
        R, n, d = (int(v) for v in init.shape)
        self._maxpro_shape(n, d)
        if not 1 <= R <= self.MAXPRO_MAX_RESTARTS:
            raise ValueError("init: %d restarts, outside 1 .. %d" % (R, self.MAXPRO_MAX_RESTARTS))
        if not 1 <= int(block) <= self.MAXPRO_MAX_BLOCK:
            raise ValueError("block = %d outside 1 .. %d" % (block, self.MAXPRO_MAX_BLOCK))
        if int(n_stages) < 1 or int(blocks_per_stage) < 1:
            raise ValueError("n_stages and blocks_per_stage must be at least 1")
        if not np.array_equal(np.sort(init, axis=1), np.broadcast_to(np.arange(n)[None, :, None], init.shape)):
            raise ValueError("init: every column must be a permutation of 0 .. n - 1")
        init = np.ascontiguousarray(init, dtype=np.int32)
        nb = int(n_stages) * int(blocks_per_stage)
        out = {"levels": np.empty((R, n, d), dtype=np.int32), "f_start": np.empty(R), "f_best": np.empty(R),
               "accepted": np.empty(R, dtype=np.int64), "consumed": np.empty(R, dtype=np.int64)}
        trace = np.empty((R, nb), dtype=np.int32) if return_trace else None
        self._ck(self.lib.gpb_maxpro_lhd(self.h, n, d, R, int(restart0), nat.ptr(init), int(seed) & 0xFFFFFFFFFFFFFFFF, int(n_stages),
                                         int(blocks_per_stage), int(block), float(temp0), float(cool), nat.ptr(out["levels"]),
                                         nat.ptr(out["f_start"]), nat.ptr(out["f_best"]), nat.ptr(out["accepted"]),
                                         nat.ptr(out["consumed"]), nat.ptr(trace)))
        const = (3.0 * d - np.log(0.5 * n * (n - 1))) / d
        out["lnpsi_start"], out["lnpsi"] = out["f_start"] / d + const, out["f_best"] / d + const
        if return_trace:
            out["trace"] = trace
        return out

    def maxpro_criterion(self, X, return_sum=False):
        """ln psi of a design X [n, d] in the unit cube (gpb_maxpro_criterion), psi = (mean over pairs of
        1 / prod_c (x_ic - x_jc)^2)^(1/d) (Joseph, Gul, Ba 2015): +inf when two rows share a coordinate.  return_sum: also the sum
        of the scaled pair terms prod_c (e^1.5 (x_ic - x_jc))^-2."""
        self._check_pid()
        X = nat.f64(X)
        if X.ndim != 2:
            raise ValueError("X: expected [n, d]")
        self._maxpro_shape(*X.shape)
        if not np.all(np.isfinite(X)):
            raise ValueError("X: must be finite")
        out = np.zeros(2)
        self._ck(self.lib.gpb_maxpro_criterion(self.h, nat.ptr(X), X.shape[0], X.shape[1], nat.ptr(out[:1]), nat.ptr(out[1:])))
        return (float(out[0]), float(out[1])) if return_sum else float(out[0])

    def maxpro_run_order(self, X, first=-1):
        """The greedy run order of a design X [n, d] (gpb_maxpro_run_order): row `first` (-1: the row nearest the cube's
        centre), then again and again the row with the smallest sum of its pair terms with the rows chosen so far, the lowest
        index at a tie.  Returns the order [n] (int32, 0-based row indices)."""
        self._check_pid()
        X = nat.f64(X)
        if X.ndim != 2:
            raise ValueError("X: expected [n, d]")
        self._maxpro_shape(*X.shape)
        if not np.all(np.isfinite(X)):
            raise ValueError("X: must be finite")
        if not -1 <= int(first) < X.shape[0]:
            raise ValueError("first = %d outside -1 .. n - 1" % first)
        order = np.empty(X.shape[0], dtype=np.int32)
        self._ck(self.lib.gpb_maxpro_run_order(self.h, nat.ptr(X), X.shape[0], X.shape[1], int(first), nat.ptr(order)))
        return order

    def emu_predict_jac(self, Xs, out=None):
        """Jacobian [W,M,d_in] of the observable-space mean (gpb_emu_predict_jac): through the transform and, when one is set,
        the parameter map (Xs then holds the original parameters, d_in columns).  numpy in -> numpy out; torch(cuda) in -> torch
        out (asynchronous), into `out` (a contiguous [W, M, d_in] device tensor) when it is given."""
        self._need_data()
        din = self.pmap_d_in if getattr(self, "pmap_d_in", -1) > 0 else self.d
        if _is_torch(Xs):
            import torch
            self._track_stream()
            Xs = self._dev(Xs, (None, din), "Xs", contiguous=False)
            W = Xs.shape[0]
            if out is None:
                out = torch.empty((W, self.M, din), dtype=torch.float64, device=Xs.device)
            else:
                self._dev(out, (W, self.M, din), "out")
            if W:
                self._ck(self.lib.gpb_emu_predict_jac(self.h, nat.ptr(Xs), W, 1, nat.ptr(out)))
            return out
        if out is not None:
            raise ValueError("emu_predict_jac: out= takes a device tensor, together with torch input")
        Xs = nat.f64(Xs).reshape(-1, din)
        W = Xs.shape[0]
        jac = nat.host_empty((W, self.M, din))
        self._ck(self.lib.gpb_emu_predict_jac(self.h, nat.ptr(Xs), W, 0, nat.ptr(jac)))
        return jac

    # ------------------------------------------------------------------ likelihood block
    def set_likelihood(self, yexp, cov_exp):
        yexp, cov_exp = nat.f64(yexp).reshape(-1), nat.f64(cov_exp)
        assert yexp.shape[0] == self.M and cov_exp.shape == (self.M, self.M)
        self._ck(self.lib.gpb_like_set(self.h, nat.ptr(yexp), nat.ptr(cov_exp)))

    def loglike(self, Xs, out=None, accumulate=False, check=True):
        """Block log-likelihood for every row of Xs.  torch(cuda) in/out stays on the device
        and is asynchronous when check=False."""
        self._need_data()
        npd = C.c_int(0)
        if _is_torch(Xs):
            import torch
            Xs = self._check_cols(Xs, "Xs")
            W = Xs.shape[0]
            if out is None:
                out = torch.empty(W, dtype=torch.float64, device=Xs.device)
                accumulate = False
            else:
                self._dev(out, (W,), "out")
            self._ck(self.lib.gpb_loglike(self.h, nat.ptr(Xs), W, 1, nat.ptr(out),
                                          1 if accumulate else 0, C.byref(npd) if check else None))
        else:
            Xs = nat.f64(Xs).reshape(-1, self.d)
            W = Xs.shape[0]
            if out is None:
                out = np.empty(W)
                accumulate = False
            self._ck(self.lib.gpb_loglike(self.h, nat.ptr(Xs), W, 0, nat.ptr(out), 1 if accumulate else 0,
                                          C.byref(npd) if check else None))
        self.last_not_pd = npd.value
        return out

    def logpost(self, X_dev, out, accumulate, lo_dev, hi_dev, outside, const):
        """Fused device log-posterior of the last emulator block: log-likelihood (+= when accumulate),
        strict prior box, constant.  Asynchronous; torch cuda tensors only."""
        self._need_data()
        self._track_stream()
        X_dev = self._dev(X_dev, (None, self.d), "X")               # contiguous: `out` rows must line up with X rows
        self._dev(lo_dev, (self.d,), "lo"), self._dev(hi_dev, (self.d,), "hi")
        self._dev(out, (X_dev.shape[0],), "out")
        self._ck(self.lib.gpb_logpost(self.h, nat.ptr(X_dev), X_dev.shape[0], nat.ptr(out), 1 if accumulate else 0,
                                      nat.ptr(lo_dev), nat.ptr(hi_dev), float(outside), float(const)))
        return out

    def mvn_loglike(self, dY, cov):
        """Batched mvn_loglike on explicit dY[W,M], cov[W,M,M] (numpy or torch cuda)."""
        npd = C.c_int(0)
        if _is_torch(dY):
            import torch
            self._track_stream()
            dY = self._dev(dY, (None, None), "dY", contiguous=False)
            W, M = dY.shape
            cov = self._dev(cov, (W, M, M), "cov", contiguous=False)
            out = torch.empty(W, dtype=torch.float64, device=dY.device)
            self._ck(self.lib.gpb_mvn_loglike(self.h, nat.ptr(dY), nat.ptr(cov), W, M, 1,
                                              nat.ptr(out), C.byref(npd)))
        else:
            dY, cov = nat.f64(dY), nat.f64(cov)
            W, M = dY.shape
            out = np.empty(W)
            self._ck(self.lib.gpb_mvn_loglike(self.h, nat.ptr(dY), nat.ptr(cov), W, M, 0, nat.ptr(out),
                                              C.byref(npd)))
        self.last_not_pd = npd.value
        return out

    def box_finish(self, X_dev, lo_dev, hi_dev, outside, const, ll_dev):
        self._track_stream()
        X_dev = self._dev(X_dev, (None, None), "X")
        W, d = X_dev.shape
        self._dev(lo_dev, (d,), "lo"), self._dev(hi_dev, (d,), "hi"), self._dev(ll_dev, (W,), "ll")
        self._ck(self.lib.gpb_box_finish(self.h, nat.ptr(X_dev), W, d, nat.ptr(lo_dev), nat.ptr(hi_dev),
                                         float(outside), float(const), nat.ptr(ll_dev)))

    # ------------------------------------------------------------------ parameterTrafoPCA input map
    def set_param_map(self, ppca, d_in):
        """Upload the fitted parameter-space PCA (param_pca.ParameterPCA) for the device pre-pass."""
        from .param_pca import IDX_BULK, IDX_SHEAR, IDX_YLOSS, T_GRID, MUB_GRID, YINIT_GRID
        grids = (T_GRID, MUB_GRID, YINIT_GRID)
        idx = (IDX_BULK, IDX_SHEAR, IDX_YLOSS)
        G = len(ppca.groups)
        maxpc = int(max(g.pca.n_components_ for g in ppca.groups))
        # column bookkeeping exactly as the reference does it on the values (delete, then append)
        cols = np.arange(d_in, dtype=np.int64)
        desc = np.full((G, 6), -1, dtype=np.int32)
        tab = np.zeros((G, 4 + maxpc, 100))
        for gi, g in enumerate(ppca.groups):
            k = int(g.pca.n_components_)
            cols = np.concatenate((np.delete(cols, idx[gi]), -1 - (gi * maxpc + np.arange(k))))
            desc[gi, 0] = gi
            desc[gi, 1:1 + len(idx[gi])] = idx[gi]
            desc[gi, 5] = k
            tab[gi, 0], tab[gi, 1], tab[gi, 2], tab[gi, 3] = grids[gi], g.scaler.mean_, g.scaler.scale_, g.pca.mean_
            tab[gi, 4:4 + k] = g.pca.components_
        col_src = np.ascontiguousarray(cols, dtype=np.int32)
        self.pmap_d_in, self.pmap_d_out = int(d_in), int(col_src.shape[0])
        self._ck(self.lib.gpb_param_map_set(self.h, self.pmap_d_in, self.pmap_d_out, nat.ptr(col_src), G,
                                            nat.ptr(np.ascontiguousarray(desc)), nat.ptr(np.ascontiguousarray(tab)),
                                            maxpc))

    def param_map(self, X_dev, out=None):
        """X_dev[W, d_in] (torch cuda f64) -> GP input [W, d_out] on the device, asynchronous."""
        import torch
        self._track_stream()
        if getattr(self, "pmap_d_in", -1) < 0:
            raise nat.GPBError("param_map before set_param_map")
        X_dev = self._dev(X_dev, (None, self.pmap_d_in), "X", contiguous=False)
        W = X_dev.shape[0]
        if out is None:
            out = torch.empty((W, self.pmap_d_out), dtype=torch.float64, device=X_dev.device)
        else:
            self._dev(out, (W, self.pmap_d_out), "out")
        self._ck(self.lib.gpb_param_map(self.h, nat.ptr(X_dev), W, nat.ptr(out)))
        return out

    # ------------------------------------------------------------------ diagnostics
    def tile_trace(self, capacity):
        """arm (capacity > 0) or disarm (0) the per-tile placement/timing trace of the predict kernel"""
        self._ck(self.lib.gpb_debug_tile_trace(self.h, int(capacity)))
        self._trace_cap = int(capacity)

    def tile_trace_read(self):
        """records[n, 8] uint32: HW_ID, XCC_ID, gp, row block, walker tile, start, end (100 MHz ticks), blockIdx"""
        rec = np.zeros((self._trace_cap, 8), dtype=np.uint32)
        n = C.c_int64(0)
        self._ck(self.lib.gpb_debug_tile_trace_read(self.h, nat.ptr(rec), self._trace_cap, C.byref(n)))
        return rec[:n.value]

    # ------------------------------------------------------------------ RCCL without torch.distributed
    def dist_available(self):
        """True when librccl loads with the entry points gpb_dist_* use (no communicator is created)"""
        return self.lib.gpb_dist_available() == 1

    def dist_uid(self):
        """128-byte ncclUniqueId (rank 0 creates it and hands it to the other ranks out of band)."""
        uid = np.zeros(128, dtype=np.uint8)
        self._ck(self.lib.gpb_dist_uid(nat.ptr(uid)))
        return uid.tobytes()

    def dist_init(self, rank, nranks, uid):
        buf = np.frombuffer(bytes(uid), dtype=np.uint8).copy()
        if buf.size != 128:
            raise ValueError("uid must be the 128 bytes of dist_uid()")
        self._ck(self.lib.gpb_dist_init(self.h, int(rank), int(nranks), nat.ptr(buf)))
        self._dist_world = int(nranks)

    def dist_allgather(self, send, recv):
        """In-stream ncclAllGather of float64 device tensors: recv[r*n:(r+1)*n] = rank r's send[:n]
        (in place when send is recv[rank*n:(rank+1)*n])."""
        self._track_stream()
        n = send.numel()
        self._dev(send, (n,), "send")
        self._dev(recv, (n * getattr(self, "_dist_world", 0),), "recv")
        self._ck(self.lib.gpb_dist_allgather(self.h, nat.VP(send.data_ptr()), nat.VP(recv.data_ptr()), n))
        return recv

    def dist_finalize(self):
        self._ck(self.lib.gpb_dist_finalize(self.h))
        self._dist_world = 0

    def test_gemm(self, A, B, mode=0, tile=128):
        A, B = nat.f64(A), nat.f64(B)
        if mode == 0:
            M, K = A.shape; N = B.shape[1]
        elif mode == 1:
            M, K = A.shape; N = B.shape[0]
        else:
            K, M = A.shape; N = B.shape[1]
        Cm = np.empty((M, N))
        self._ck(self.lib.gpb_test_gemm(self.h, M, N, K, nat.ptr(A), nat.ptr(B), nat.ptr(Cm),
                                        mode | (4 if tile == 64 else 0)))
        return Cm

    def force_tile(self, tile=0, switch_tiles=0):
        """k_predict tile: 0 = by rule, 128, 64, 32 (64 rows x 32 walkers), 65 (64 x 128) — same bits whatever the shape;
        switch_tiles > 0: the rule's switch point to 128x128 tiles (tiles per 256 CUs)."""
        self.tune("force_tile", int(tile))
        if switch_tiles > 0:
            self.tune("tile_switch", int(switch_tiles))

    def tune(self, key, value):
        """option keys of gpb_ctx_option by name (launch geometry, tile rules, test hooks; 'predict_sliced': the int8 predict kernel)"""
        k = {"xcd": 0, "chol_outer": 4, "resident": 5, "narrow_switch": 7, "mvn_wg_switch": 8, "chol_inner_tile": 9,
             "tile_priority": 10, "fuse_finalize": 11, "trtri_tile": 12, "syrk_tile": 14, "tri_skip": 17, "kcross_dot": 18,
             "kcross_chunks": 19, "kcross_wpl": 20, "mid_switch": 22, "lowrank": 23, "chol_lookahead": 25, "sim_ranks": 26,
             "compact": 27, "tile_by_live": 28, "premark": 29, "fuse_accept_propose": 30, "sim_rank": 32, "tile_switch_c": 33,
             "mid_switch_c": 34, "narrow_switch_c": 35, "balance_shards": 36, "chain_batch": 40, "force_tile": 42, "generic_mvn": 43,
             "tile_switch": 44, "chol_pair": 47, "lr_split": 49, "kinv_tile": 50, "predict_sliced": 51, "marg_ws_bytes": 52,
             "rank_ws_bytes": 53}[key]
        self._ck(self.lib.gpb_ctx_option(self.h, k, int(value)))
        if k == 51:
            self.predict_sliced = int(value)         # (what Emulator.state_digest folds in)

    @property
    def has_variants(self):
        """True for the debug build (GPB_DEBUG_LIB=1): every measured-and-rejected kernel variant behind its tune key"""
        return self.lib.gpb_debug_has_variants() == 1

    def fit_piece(self, piece):
        """measurement hook: enqueue one piece of factor() alone ('kmat', 'potrf', 'trtri', 'alpha'); call factor() afterwards"""
        self._ck(self.lib.gpb_profile_fit_piece(self.h, {"kmat": 0, "potrf": 1, "trtri": 2, "alpha": 3}[piece]))

    def force_generic_mvn(self, on=True):
        """route the block log-likelihood through the generic Cholesky kernel (what M > 64 takes) whatever M"""
        self.tune("generic_mvn", 1 if on else 0)

    def profile(self, on=True):
        self._ck(self.lib.gpb_profile_enable(self.h, 1 if on else 0))

    def profile_read(self):
        """(launches, total_ms, gp_walker_pairs) of the timed k_predict launches since the last read."""
        n, ms, u = C.c_int64(0), C.c_double(0.0), C.c_double(0.0)
        self._ck(self.lib.gpb_profile_read(self.h, C.byref(n), C.byref(ms), C.byref(u)))
        return n.value, ms.value, u.value

    def probe_fp64(self, mode):
        out = C.c_double(0.0)
        self._ck(self.lib.gpb_probe_fp64(self.h, int(mode), C.byref(out)))
        return out.value


def design_run(engines, n_picks, eligible=None, return_scores=False):
    """Greedy variance-reduction picks over the engines of a chain (gpb_chain_design_run), every one begun with design_begin on
    the same number of candidates and reference points: step t takes the eligible candidate with the largest score summed over
    the engines in order, then conditions every GP on it; enqueued as a whole, read back once.  eligible: torch uint8 cuda [C],
    updated in place (None: all).  Returns (picks [T] int32, gain [T], scores [T, C] or None) as numpy arrays; a pick of -1 says
    the eligible candidates ran out.  The run consumes the workspaces: design_begin again before another."""
    import torch
    e0 = engines[0]
    T = int(n_picks)
    Cn = int(getattr(e0, "_design_C", 0))
    for g in engines:
        g._need_data()
        g._track_stream()
    dev = torch.device("cuda", e0.device)
    if eligible is not None:
        eligible = e0._dev(eligible, (Cn,), "eligible", dtype="torch.uint8")
    arr = (C.c_void_p * len(engines))(*[g.h for g in engines])
    picks = torch.empty(max(T, 1), dtype=torch.int32, device=dev)
    gain = torch.empty(max(T, 1), dtype=torch.float64, device=dev)
    scores = torch.empty((max(T, 1), max(Cn, 1)), dtype=torch.float64, device=dev) if return_scores else None
    e0._ck(e0.lib.gpb_chain_design_run(arr, len(engines), T, nat.ptr(eligible), nat.ptr(picks), nat.ptr(gain), nat.ptr(scores)))
    return picks.cpu().numpy(), gain.cpu().numpy(), (scores.cpu().numpy() if return_scores else None)
