"""
Convergence diagnostics of a chain on the device (gpb_mcmc_diag): emcee's `autocorr.integrated_time` — the integrated
autocorrelation time with the automatic window, averaged over the walkers — plus split-R-hat and effective sample sizes.

emcee takes one zero-padded FFT per (walker, parameter) in a Python loop; here the lag sums of all walkers of a parameter
are the diagonal sums of one banded fp64 matrix product over the walkers, on the chain where it
lies: the stretch sampler's [nsteps, nwalkers, ndim] store is read through its strides, nothing is permuted or copied.

Two deviations from emcee, both where emcee's answer is an accident: a walker that never moved is left out of its
parameter's average and counted (emcee: NaN for the whole parameter), and a chain so short that no window exists gets the
largest one (emcee: its np.argmin over an all-True mask can return window 0).

rank_diagnose / RankDiagnostics (gpb_chain_rank_diag) add the test that Stan, `posterior` and ArviZ report:
rank-normalised split-R-hat, the larger of the bulk and the folded value, with bulk-, tail-, mean- and quantile-ESS (Vehtari,
Gelman, Simpson, Carpenter, Buerkner 2021) — for many short independent chains (run_HMC) and for the tails the published
quantiles sit in.  ChainDiagnostics, diagnose and integrated_time are what they were.
"""
import logging

import numpy as np

log = logging.getLogger(__name__)

START_MAX_LAG = 1024          # first band of the search for the window; the result does not depend on it (see _run)


class AutocorrError(Exception):
    """Raised when the chain is too short for a reliable autocorrelation time; `.tau` is the estimate anyway (emcee's
    autocorr.AutocorrError)."""

    def __init__(self, tau, *args, **kwargs):
        self.tau = tau
        super().__init__(*args, **kwargs)


class ChainDiagnostics:
    """Per parameter [ndim]: tau, the integrated autocorrelation time in steps of the unthinned chain; window, the lag emcee's
    automatic window stopped at (in steps of the chain as analysed); ess = n_t n_moving / tau, the effective number of
    independent draws; rhat, split-R-hat over the 2 nwalkers half-walkers; mean; std = sqrt((h - 1) / h W + B / h), BDA3's
    estimate of the marginal posterior standard deviation; mcse = std / sqrt(ess); n_constant_walkers, walkers that never
    moved (left out of tau).  converged: tol tau <= n_t for every parameter (converged_per_parameter: each).  n_steps,
    n_walkers: the chain analysed (after discard and thin); names: the parameters' names where known."""

    def __init__(self, tau, window, ess, rhat, mean, std, mcse, n_constant_walkers, converged_per_parameter, n_steps, n_walkers,
                 tol, names=None):
        self.tau, self.window, self.ess, self.rhat, self.mean, self.std, self.mcse = tau, window, ess, rhat, mean, std, mcse
        self.n_constant_walkers = n_constant_walkers
        self.converged_per_parameter = converged_per_parameter
        self.converged = bool(np.all(converged_per_parameter))
        self.n_steps, self.n_walkers, self.tol = int(n_steps), int(n_walkers), tol
        self.names = None if names is None else list(names)

    def __repr__(self):
        names = self.names or ["p%d" % j for j in range(len(self.tau))]
        wid = max([9] + [len(str(s)) for s in names])
        lines = ["ChainDiagnostics(n_steps=%d, n_walkers=%d, converged=%s: %g tau <= n_steps)"
                 % (self.n_steps, self.n_walkers, self.converged, self.tol),
                 "  %-*s %10s %6s %10s %8s %12s %12s %10s %6s %s" % (wid, "parameter", "tau", "window", "ess", "rhat", "mean", "std",
                                                                    "mcse", "const", "ok")]
        for j, nm in enumerate(names):
            lines.append("  %-*s %10.2f %6d %10.1f %8.4f %12.5g %12.5g %10.3g %6d %s"
                         % (wid, nm, self.tau[j], self.window[j], self.ess[j], self.rhat[j], self.mean[j], self.std[j], self.mcse[j],
                            self.n_constant_walkers[j], "yes" if self.converged_per_parameter[j] else "NO"))
        return "\n".join(lines)


_engines = {}


def _engine(device):
    """an engine on `device` to lend its stream: the package's utility engine where that lives on this device (it is created on
    the first device that asked for it), else one of this module's own per device"""
    from .engine import GPEngine
    from .mcmc import _utility_engine
    device = int(device)
    eng = _utility_engine(device)
    if eng.device == device:
        return eng
    if device not in _engines:
        _engines[device] = GPEngine(device)
    _engines[device]._check_pid()
    return _engines[device]


def _run(x_dev, c, eng, layout="steps"):
    """gpb_mcmc_diag on a device chain with a band wide enough for every parameter's window: start at min(n_t - 1, 1024) lags
    and double up to n_t - 1 while a parameter reports no window.  rho's leading lags have the same bits whatever the band,
    so tau and window do not depend on where the search started: the start is a choice, not a tuned value.  Returns the
    dict of GPEngine.mcmc_diag (without rho), window without the flag bit."""
    n = int(x_dev.shape[0 if layout == "steps" else 1])
    if n < 4:
        raise ValueError("the chain needs at least 4 steps, got %d" % n)
    max_lag = min(n - 1, START_MAX_LAG)
    out = eng.mcmc_diag(x_dev, layout, max_lag, c, outputs=("tau", "window", "moments", "rhat", "nconst"))
    while max_lag < n - 1 and np.any((out["window"] >= 0) & (out["window"] & eng.DIAG_NO_WINDOW != 0)):
        max_lag = min(2 * max_lag, n - 1)
        out.update(eng.mcmc_diag(x_dev, layout, max_lag, c, outputs=("tau", "window")))
    w = out["window"]
    out["window"] = np.where(w >= 0, w & ~np.int32(eng.DIAG_NO_WINDOW), w).astype(np.int32)
    return out


def _as_device(x, device):
    import torch
    if hasattr(x, "data_ptr"):
        return x if x.dtype == torch.float64 else x.to(torch.float64)
    x = np.asarray(x, dtype=np.float64)
    if not np.all(np.isfinite(x)):
        raise ValueError("the chain holds non-finite values")
    return torch.as_tensor(np.require(x, requirements=["C", "W"]), device=torch.device("cuda", device))


def diagnose(x_dev, c=5, tol=50, thin=1, layout="steps", eng=None, names=None, device=0):
    """ChainDiagnostics of a chain [nsteps, nwalkers, ndim] (layout "steps") or [nwalkers, nsteps, ndim] ("walkers"), numpy or a
    torch cuda tensor / view; thin: the stride the view was thinned with (tau is reported in unthinned steps)."""
    x_dev = _as_device(x_dev, device)
    eng = eng or _engine(x_dev.device.index or 0)
    out = _run(x_dev, c, eng, layout)
    n, nw = (int(x_dev.shape[0]), int(x_dev.shape[1])) if layout == "steps" else (int(x_dev.shape[1]), int(x_dev.shape[0]))
    tau = out["tau"]
    h = n // 2
    W, B = out["moments"][:, 1], out["moments"][:, 2]
    std = np.sqrt((h - 1.0) / h * W + B / h)
    with np.errstate(divide="ignore", invalid="ignore"):
        ess = n * (nw - out["nconst"]) / tau
        mcse = std / np.sqrt(ess)
    return ChainDiagnostics(tau * thin, out["window"], ess, out["rhat"], out["moments"][:, 0], std, mcse, out["nconst"],
                            tol * tau <= n, n, nw, tol, names=names)


def integrated_time(x, c=5, tol=50, quiet=False, has_walkers=True, device=0):
    """emcee's autocorr.integrated_time by signature and shape rules: x [n_t], [n_t, n_w] (has_walkers=False: [n_t, n_d]) or
    [n_t, n_w, n_d], numpy or a torch cuda tensor; returns tau [n_d].  tol tau > n_t raises AutocorrError (carrying .tau), or
    with quiet=True logs a warning and returns."""
    if not hasattr(x, "data_ptr"):
        x = np.atleast_1d(np.asarray(x, dtype=np.float64))
    if x.ndim == 1:
        x = x[:, None, None]
    if x.ndim == 2:
        x = x[:, :, None] if has_walkers else x[:, None, :]
    if x.ndim != 3:
        raise ValueError("invalid dimensions")
    x_dev = _as_device(x, device)
    out = _run(x_dev, c, _engine(x_dev.device.index or 0))
    return _check(out["tau"], int(x_dev.shape[0]), tol, quiet)


def _check(tau, n_t, tol, quiet):
    flag = tol * tau > n_t
    if np.any(flag):
        msg = ("The chain is shorter than {0} times the integrated autocorrelation time for {1} parameter(s). Use this estimate "
               "with caution and run a longer chain!\n").format(tol, int(np.sum(flag)))
        msg += "N/{0} = {1:.0f};\ntau: {2}".format(tol, n_t / tol, tau)
        if not quiet:
            raise AutocorrError(tau, msg)
        log.warning(msg)
    return tau


# ---------------------------------------------------------------------------------------------------------------- rank-normalised
class RankDiagnostics:
    """Rank-normalised convergence diagnostics (Vehtari, Gelman, Simpson, Carpenter, Buerkner 2021), per parameter [ndim]:
    rhat = the larger of rhat_bulk (the rank-normalised split chains) and rhat_folded (the same of |x - median|: scale and tails);
    ess_bulk; ess_tail = the smaller of the effective sample sizes of I(x <= q_0.05) and I(x <= q_0.95); ess_mean, of x itself;
    ess_quantile [ndim, nq], of I(x <= q_p) per level of probs; mcse_mean = sd / sqrt(ess_mean); median; quantiles [ndim, nq], the
    levels' quantiles of the kept draws; sd.  converged_per_parameter: rhat < rhat_max and min(ess_bulk, ess_tail) >= min_ess
    (the paper's 1.01 and 400); converged: all of them.  n_steps, n_walkers: the chain analysed (after discard and thin; a
    middle step of an odd n_steps is dropped), n_draws = 2 (n_steps // 2) n_walkers; names: the parameters' names where known.
    thin: the stride the analysed view was thinned with, recorded only — effective sample sizes count draws, so nothing is
    rescaled by it.  An effective sample size is NaN for a series that never varies."""

    def __init__(self, rhat_bulk, rhat_folded, ess_bulk, ess_tail, ess_mean, ess_quantile, median, quantiles, sd, probs, n_steps,
                 n_walkers, min_ess=400, rhat_max=1.01, names=None, thin=1):
        self.thin = int(thin)
        self.rhat_bulk, self.rhat_folded = rhat_bulk, rhat_folded
        self.rhat = np.where(np.isnan(rhat_bulk) | np.isnan(rhat_folded), np.nan, np.maximum(rhat_bulk, rhat_folded))
        self.ess_bulk, self.ess_tail, self.ess_mean, self.ess_quantile = ess_bulk, ess_tail, ess_mean, ess_quantile
        self.median, self.quantiles, self.sd, self.probs = median, quantiles, sd, tuple(float(p) for p in probs)
        with np.errstate(divide="ignore", invalid="ignore"):
            self.mcse_mean = sd / np.sqrt(ess_mean)
            self.converged_per_parameter = (self.rhat < rhat_max) & (np.minimum(ess_bulk, ess_tail) >= min_ess)
        self.converged = bool(np.all(self.converged_per_parameter))
        self.n_steps, self.n_walkers = int(n_steps), int(n_walkers)
        self.n_draws = 2 * (self.n_steps // 2) * self.n_walkers
        self.min_ess, self.rhat_max = min_ess, rhat_max
        self.names = None if names is None else list(names)

    def __repr__(self):
        names = self.names or ["p%d" % j for j in range(len(self.rhat))]
        wid = max([9] + [len(str(s)) for s in names])
        lines = ["RankDiagnostics(n_steps=%d, n_walkers=%d, converged=%s: rhat < %g and min(ess_bulk, ess_tail) >= %g)"
                 % (self.n_steps, self.n_walkers, self.converged, self.rhat_max, self.min_ess),
                 "  %-*s %8s %8s %8s %10s %10s %10s %12s %10s %s" % (wid, "parameter", "rhat", "bulk", "folded", "ess_bulk", "ess_tail",
                                                                   "ess_mean", "median", "mcse_mean", "ok")]
        for j, nm in enumerate(names):
            lines.append("  %-*s %8.4f %8.4f %8.4f %10.1f %10.1f %10.1f %12.5g %10.3g %s"
                         % (wid, nm, self.rhat[j], self.rhat_bulk[j], self.rhat_folded[j], self.ess_bulk[j], self.ess_tail[j],
                            self.ess_mean[j], self.median[j], self.mcse_mean[j], "yes" if self.converged_per_parameter[j] else "NO"))
        return "\n".join(lines)


TAIL_PROBS = (0.05, 0.95)


def _run_rank(x_dev, probs, eng, layout="steps"):
    """gpb_chain_rank_diag on a device chain with a band wide enough for every series' estimator: start at min(h - 1, 1024) lags
    and double up to h - 1 while a series reports that it needs more.  rho-hat's leading lags have the same bits whatever the
    band, so no result depends on where the search started.  A wider band repeats the whole call, rank transform included,
    though only the Gram band, the lag sums and the scan depend on max_lag: the search starts at 1024
    lags so that this is rare."""
    n = int(x_dev.shape[0 if layout == "steps" else 1])
    if n < 4:
        raise ValueError("the chain needs at least 4 steps, got %d" % n)
    h = n // 2
    max_lag = min(h - 1, START_MAX_LAG)
    out = eng.rank_diag(x_dev, layout, probs, max_lag)
    while max_lag < h - 1 and np.any((out["stop"] >= 0) & (out["stop"] & eng.RANK_NO_BAND != 0)):
        max_lag = min(2 * max_lag, h - 1)
        out.update(eng.rank_diag(x_dev, layout, probs, max_lag, outputs=("ess", "stop")))
    return out


def rank_diagnose(x, probs=TAIL_PROBS, thin=1, layout="steps", min_ess=400, names=None, device=0, rhat_max=1.01, eng=None,
                  weights=None):
    """RankDiagnostics of a chain [nsteps, nwalkers, ndim] (layout "steps") or [nwalkers, nsteps, ndim] ("walkers"), numpy or a
    torch cuda tensor / view, computed on the device (gpb_chain_rank_diag: a radix sort per parameter for the ranks, the banded
    Gram product of diagnose for the autocovariances).  probs: the levels of ess_quantile and quantiles (with the 0.05 and 0.95 of
    ess_tail at most 8 distinct levels); thin: the stride x was ALREADY thinned with (as for diagnose: nothing is sliced here), kept in
    RankDiagnostics.thin; effective sample sizes count draws and are not rescaled by it.  A weighted particle set is refused:
    ranks of weighted draws are not defined here."""
    if weights is not None:
        raise ValueError("rank_diagnose: ranks of weighted draws are out of scope; resample the particle set to equal weights first")
    if len(getattr(x, "shape", np.shape(x))) != 3:
        raise ValueError("rank_diagnose: expected a three-dimensional chain (a flat particle set has no chains to compare)")
    probs = [float(p) for p in np.atleast_1d(probs)]
    levels = list(probs) + [p for p in TAIL_PROBS if p not in probs]
    if not probs or len(levels) > 8 or not all(0.0 < p < 1.0 for p in levels):
        raise ValueError("probs: 1 to 8 levels inside (0, 1), the 0.05 and 0.95 of ess_tail included")
    x_dev = _as_device(x, device)
    eng = eng or _engine(x_dev.device.index or 0)
    out = _run_rank(x_dev, levels, eng, layout)
    n, nw = (int(x_dev.shape[0]), int(x_dev.shape[1])) if layout == "steps" else (int(x_dev.shape[1]), int(x_dev.shape[0]))
    nq = len(probs)
    ess = out["ess"]
    tail = [2 + levels.index(p) for p in TAIL_PROBS]
    with np.errstate(invalid="ignore"):
        ess_tail = np.where(np.isnan(ess[:, tail]).any(axis=1), np.nan, np.min(ess[:, tail], axis=1))
    return RankDiagnostics(out["rhat"][:, 0], out["rhat"][:, 1], ess[:, 0], ess_tail, ess[:, 1], ess[:, 2:2 + nq], out["median"],
                           out["quant"][:, :nq], out["sd"], probs, n, nw, min_ess=min_ess, rhat_max=rhat_max, names=names, thin=thin)
