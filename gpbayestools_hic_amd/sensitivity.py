"""
Which data constrain which parameter: the response matrix of examples/SensitivityAnalysis.ipynb and the Fisher information of a
calibration, reduced over ALL samples of a chain on the device (gpb_sens_accumulate).

The notebook builds the observable-by-parameter matrix `(Y+ - Y-) / (2 h) * x / ((Y+ + Y-) / 2)` from 2 d finite-difference
predictions at one design point.  Here the Jacobian is the closed form of gpb_emu_predict_jac, the matrix R = x_j J_mj / y_m is
the formula's analytic limit, and it is averaged over the posterior with its spread.  R paints a 2 %-precise multiplicity and a
30 %-precise v3 the same colour; what says how much a data set constrains a parameter is J^T C^-1 J with C the covariance the
likelihood uses (src/mcmc.py:288-290: the emulator's predictive covariance plus the experiment's), per emulator and sample.

No [S, nobs, ndim] array reaches the host: per slab and emulator the mean, the covariance and the Jacobian are formed on the
device, reduced there into running sums, and only those sums are read back.
"""
import numpy as np


class PosteriorSensitivity:
    """posterior_sensitivity's result, E emulators, nobs observables in emuList order, ndim parameters:
      n_samples            rows used;  n_bad [E]: rows whose covariance block had a non-positive pivot (left out of that emulator)
      response_mean, response_std [nobs, ndim]   the notebook's matrix x_j / y_m dy_m / dx_j, its mean and spread over the rows
      obs_information [nobs, ndim]   mean of J_mj^2 / C_mm times (max_j - min_j)^2: what observable m alone knows of parameter j,
                           in units of the prior box (dimensionless)
      fisher [E, ndim, ndim]   mean of J^T C^-1 J per emulator, in parameter units;  fisher_total: their sum
      information [E, ndim]    diag(fisher_e) (max - min)^2: the table "data set x parameter"
      param_mean [ndim], param_cov [ndim, ndim]   of the rows used (weighted)
    fisher is the Gauss-Newton Hessian of the negative log-likelihood with the covariance frozen at each sample.  It is NOT the
    full Gaussian Fisher matrix: the term 1/2 tr(C^-1 dC C^-1 dC) needs the GPs' variance gradients through the observable
    transform and is left out."""

    def __init__(self, n_samples, n_bad, response_mean, response_std, obs_information, fisher, param_mean, param_cov, width,
                 names=None):
        self.n_samples, self.n_bad = int(n_samples), np.asarray(n_bad, dtype=np.int64)
        self.response_mean, self.response_std, self.obs_information = response_mean, response_std, obs_information
        self.fisher = fisher
        self.fisher_total = fisher.sum(0)
        self.width = np.asarray(width, dtype=np.float64)
        self.information = np.stack([np.diag(f) for f in fisher]) * (self.width * self.width)[None, :]
        self.param_mean, self.param_cov = param_mean, param_cov
        self.names = None if names is None else list(names)

    def forecast_cov(self):
        """inv(fisher_total): the parameter covariance the data alone would give in the Gauss-Newton approximation
        (np.linalg.LinAlgError when fisher_total is singular)"""
        F = self.fisher_total
        if not np.all(np.isfinite(F)) or np.linalg.matrix_rank(F) < F.shape[0]:
            raise np.linalg.LinAlgError("fisher_total is singular: the data leave a direction of the parameters unconstrained")
        return np.linalg.inv(F)

    def stiff_directions(self):
        """(eigenvalues descending [ndim], eigenvectors [ndim, ndim] in columns) of fisher_total in units of the prior box,
        width_i F_ij width_j: the stiffest combination of parameters first"""
        w, v = np.linalg.eigh(self.fisher_total * np.outer(self.width, self.width))
        return w[::-1].copy(), v[:, ::-1].copy()

    def __repr__(self):
        E, d = self.information.shape
        names = self.names or ["p%d" % j for j in range(d)]
        lines = ["PosteriorSensitivity(n_samples=%d, emulators=%d, nobs=%d, ndim=%d, n_bad=%s)"
                 % (self.n_samples, E, self.response_mean.shape[0], d, self.n_bad.tolist())]
        tot = self.information.sum(0)
        for j in np.argsort(-tot)[:min(d, 8)]:
            lines.append("  %-16s information %.4g  (emulator %d holds %.0f %%)"
                         % (names[j], tot[j], int(np.argmax(self.information[:, j])),
                            100.0 * self.information[:, j].max() / tot[j] if tot[j] > 0 else 0.0))
        return "\n".join(lines)


def slab_rows(chain):
    """rows of one slab: from max_e 8 (P_e N_e + M_e^2 + 2 M_e d) bytes per row by the rule of the other chain calls (at most 2^15
    rows, as Emulator.predict_jacobian: every emulator's context keeps its own gradient workspace), a multiple of 256;
    chain.sens_slab_rows overrides it (rounded down to a multiple of 256, at least 256)"""
    d = chain.ndim
    per_row = max(8 * (e._ngp * e._X_train.shape[0] + e.nobs * e.nobs + 2 * e.nobs * d) for e in chain.emuList)
    slab = int(min(max((8 << 30) // per_row, 1024), 1 << 15)) // 256 * 256
    if getattr(chain, "sens_slab_rows", None) is not None:
        slab = max(int(chain.sens_slab_rows) // 256 * 256, 256)
    return slab


def posterior_sensitivity(chain, X, weights=None, profile=None):
    """PosteriorSensitivity of the rows X [S, ndim] (weights [S]: non-negative, not all zero) for the emulators and the
    experiment of `chain`.  Slab by slab (a multiple of 256 rows), emulator by emulator in emuList order: gpb_emu_predict (mean
    and covariance on the device; the rows mapped on the host for parameterTrafoPCA emulators, as Chain._ppd_arrays maps them),
    gpb_emu_predict_jac on the original parameters, gpb_sens_accumulate with that emulator's diagonal block of expdata_cov.
    Equal inputs give equal bits, whatever the slab size.  profile: a dict that receives the milliseconds of the three phases
    ("predict", "jacobian", "accumulate" [E]), measured with events on the stream.
    NotImplementedError for foreign emulators, a chain sharded over several ranks and an expdata_cov that couples emulators
    (the blocks are then not independent); ValueError for wrong shapes, non-finite rows, negative or all-zero weights."""
    import torch
    if not chain._native():
        raise NotImplementedError("sensitivity needs every emulator of the chain to be this package's Emulator (foreign "
                                  "emulators expose no GP state to differentiate on the device)")
    if chain.sharding is not None and getattr(chain.sharding, "world", 1) > 1:
        raise NotImplementedError("sensitivity: a chain sharded over several ranks is not supported; call it on one rank "
                                  "(shard_over(None))")
    X = np.asarray(X, dtype=np.float64)
    if X.ndim != 2 or X.shape[1] != chain.ndim or X.shape[0] < 1:
        raise ValueError("sensitivity: samples must be [S, %d], got %s" % (chain.ndim, X.shape))
    if not np.all(np.isfinite(X)):
        raise ValueError("sensitivity: samples hold non-finite values")
    X = np.ascontiguousarray(X)
    S, d = X.shape
    w = None
    if weights is not None:
        w = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).reshape(-1))
        if w.shape[0] != S or not np.all(np.isfinite(w)) or np.any(w < 0.0) or not w.max() > 0.0:
            raise ValueError("sensitivity: weights [%d] finite, non-negative, not all zero" % S)
    chain._prepare_blocks()
    if chain._coupled:
        raise NotImplementedError("sensitivity: the experimental covariance couples different emulators; their blocks of the "
                                  "Fisher matrix are then not independent")
    dev = torch.device("cuda", chain.device or 0)
    engs = [e._engine_ready() for e in chain.emuList]
    for g in engs:
        g._need_data()
        g._track_stream()
    E = len(engs)
    cov_exp = np.asarray(chain.expdata_cov, dtype=np.float64)
    Ms, Cadd, acc, cnt = [], [], [], []
    r0 = 0
    for emu, g in zip(chain.emuList, engs):
        M = emu.nobs
        Ms.append(M)
        Cadd.append(torch.as_tensor(np.ascontiguousarray(cov_exp[r0:r0 + M, r0:r0 + M]), device=dev))
        acc.append(torch.zeros(g.sens_acc_doubles(M, d), dtype=torch.float64, device=dev))
        cnt.append(torch.zeros(2, dtype=torch.int64, device=dev))
        r0 += M
    slab = slab_rows(chain)
    ev = [] if profile is not None else None

    def mark():
        if ev is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record(torch.cuda.current_stream(dev))
            ev.append(e)
    for i0 in range(0, S, slab):
        i1 = min(i0 + slab, S)
        Xd = torch.as_tensor(X[i0:i1], device=dev)
        wd = None if w is None else torch.as_tensor(w[i0:i1], device=dev)
        for k, (emu, g) in enumerate(zip(chain.emuList, engs)):
            Xg = Xd
            if getattr(emu, "parameterTrafoPCA_", False):
                Xg = torch.as_tensor(np.ascontiguousarray(emu._map_parameters(X[i0:i1])), device=dev)
            mark()
            y, C = g.emu_predict(Xg, return_cov=True)
            mark()
            J = g.emu_predict_jac(Xd)
            mark()
            g.sens_accumulate(J, y, C, Cadd[k], Xd, wd, acc[k], cnt[k])
            mark()
            del y, C, J
    if ev is not None:
        torch.cuda.synchronize(dev)
        tp = np.array([ev[i].elapsed_time(ev[i + 1]) for i in range(0, len(ev), 4)])
        tj = np.array([ev[i + 1].elapsed_time(ev[i + 2]) for i in range(0, len(ev), 4)])
        ta = np.array([ev[i + 2].elapsed_time(ev[i + 3]) for i in range(0, len(ev), 4)])
        profile["predict"], profile["jacobian"] = float(tp.sum()), float(tj.sum())
        profile["accumulate"] = ta.reshape(-1, E).sum(0)
        profile["slab_rows"] = slab
    width = np.asarray(chain.max, dtype=np.float64) - np.asarray(chain.min, dtype=np.float64)
    rm, rs, oi, fi, nbad = [], [], [], [], []
    with np.errstate(all="ignore"):
        for k, g in enumerate(engs):
            u = g.sens_unpack(acc[k], cnt[k], Ms[k], d)
            ws = u["wsum"]
            mean = u["response"] / ws
            rm.append(mean)
            rs.append(np.sqrt(np.maximum(u["response_sq"] / ws - mean * mean, 0.0)))
            oi.append(u["obs_information"] / ws * (width * width)[None, :])
            fi.append(u["fisher"] / ws)
            nbad.append(u["n_bad"])
    wn = np.ones(S) if w is None else w
    pm = (X * wn[:, None]).sum(0) / wn.sum()
    Xc = X - pm
    pc = (Xc * wn[:, None]).T @ Xc / wn.sum()
    names = list(chain.pardict) if len(getattr(chain, "pardict", ())) == d else None
    return PosteriorSensitivity(S, nbad, np.concatenate(rm, 0), np.concatenate(rs, 0), np.concatenate(oi, 0), np.stack(fi), pm, pc,
                                width, names)
