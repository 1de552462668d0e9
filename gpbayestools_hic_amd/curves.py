"""
The physics result of a calibration and its closure verdict, on the device: what examples/PlotMCMC.ipynb takes from a chain in
plot_zeta_s_posterior / plot_eta_s_posterior / plot_yloss_posterior (the posterior of the FUNCTIONS zeta/s (T), eta/s (mu_B) and
<y_loss> (y_init): median and 68 / 95 / 99.7 % bands over all samples on a 100-point grid), compute_Delta_d /
create_Delta_d_distribution (the closure metric and its per-sample distribution) and plot_chain_histogram (the walkers'
distribution step by step) — for a chain that lies in device memory (gpb_chain_curves, gpb_chain_trace_hist, DESIGN.md section
25): the sampler's [nsteps, nwalkers, ndim] store, a pickle's [nwalkers, nsteps, ndim] or a thinned view of either is read through
its strides.

The bands are np.percentile's of the notebook's [S, 100] array without that array: the two order statistics numpy interpolates
between are selected exactly from values that are evaluated again in every pass of the select and never stored; the workspace
does not grow with the number of samples.  For eta/s and y_loss the percentiles equal the notebook's bit for bit; zeta/s differs
by the two exponentials' last bits.

Weighted flat particle sets (a pocoMC / run_SMC pickle's `chain` and `weights`; 1e4 .. 1e5 rows) are evaluated on the host with
numpy and marginals.weighted_quantile, as marginals.marginals treats them.
"""
import numpy as np

from .marginals import weighted_quantile


# ---------------------------------------------------------------------------------------------------------------- host functions
# Vectorised numpy forms of the three parametrisations, every operation in the order csrc/curve_fn.h performs it; the parameters
# and the grid broadcast against each other (parameters [S, 1], grid [G] -> [S, G]).
def zeta_over_s(zeta_max, T_zeta0, sigma_plus, sigma_minus, T):
    zeta_max, T_zeta0, sigma_plus, sigma_minus, T = np.broadcast_arrays(*(np.asarray(a, dtype=np.float64) for a in
                                                                          (zeta_max, T_zeta0, sigma_plus, sigma_minus, T)))
    sigma = np.where(T < T_zeta0, sigma_minus, sigma_plus)
    dt = T - T_zeta0
    with np.errstate(all="ignore"):
        return zeta_max * np.exp(-(dt * dt) / (2.0 * (sigma * sigma)))


def eta_over_s(eta_0, eta_2, eta_4, mu_B):
    e0, e2, e4, g = np.broadcast_arrays(*(np.asarray(a, dtype=np.float64) for a in (eta_0, eta_2, eta_4, mu_B)))
    out = np.zeros(g.shape)
    out = np.where((g >= 0.0) & (g <= 0.2), e0 + (e2 - e0) * (g / 0.2), out)
    out = np.where((g > 0.2) & (g < 0.4), e2 + (e4 - e2) * ((g - 0.2) / 0.2), out)
    return np.where(g >= 0.4, e4, out)


def y_loss(yloss_2, yloss_4, yloss_6, y_init):
    y2, y4, y6, g = np.broadcast_arrays(*(np.asarray(a, dtype=np.float64) for a in (yloss_2, yloss_4, yloss_6, y_init)))
    out = np.zeros(g.shape)
    out = np.where((g >= 0.0) & (g <= 2.0), y2 * (g / 2.0), out)
    out = np.where((g > 2.0) & (g < 4.0), y2 + (y4 - y2) * ((g - 2.0) / 2.0), out)
    return np.where(g >= 4.0, y4 + (y6 - y4) * ((g - 4.0) / 2.0), out)


def closure_distance(theta, truth, width):
    """[S]: (sum_j ((theta_j - truth_j) / width_j)^2) / d per row of theta [S, d], j ascending, one add after the other"""
    theta = np.asarray(theta, dtype=np.float64)
    z = (theta - np.asarray(truth, dtype=np.float64)) / np.asarray(width, dtype=np.float64)
    z = z * z
    acc = np.zeros(theta.shape[0])
    for j in range(theta.shape[1]):
        acc = acc + z[:, j]
    return acc / float(theta.shape[1])


# name -> device function number, the reference's parameter indices, the notebook's grid, the host function
CURVES = {
    "zeta_over_s": dict(fn=0, columns=(15, 16, 17, 18), grid=np.linspace(0.0, 0.5, 100), host=zeta_over_s),
    "eta_over_s": dict(fn=1, columns=(12, 13, 14), grid=np.linspace(0.0, 0.6, 100), host=eta_over_s),
    "y_loss": dict(fn=2, columns=(2, 3, 4), grid=np.linspace(0.0, 6.2, 100), host=y_loss),
}
DEFAULT_LEVELS = (68, 95, 99.7)


def curve_on_host(name, theta, columns, grid):
    """[S, G]: curve `name` of the rows theta [S, ndim] on the grid, with numpy"""
    p = np.asarray(theta, dtype=np.float64)[:, list(columns)]
    return CURVES[name]["host"](*[p[:, i:i + 1] for i in range(p.shape[1])], np.asarray(grid, dtype=np.float64)[None, :])


class CurveBand:
    """One curve's posterior: grid [G], median [G], lower[level] / upper[level] [G] (the percentiles 50 -+ level / 2), percentiles
    [nq, G] at levels q [nq]; with a truth: truth_curve [G] and inside[level] [G] (bool: lower <= truth <= upper); values [S, G]
    when asked for."""

    def __init__(self, name, columns, grid, q, percentiles, levels, truth_curve=None, values=None):
        self.name, self.columns, self.grid, self.q, self.percentiles = name, tuple(columns), grid, q, percentiles
        self.median = percentiles[0]
        self.lower = {lv: percentiles[1 + 2 * i] for i, lv in enumerate(levels)}
        self.upper = {lv: percentiles[2 + 2 * i] for i, lv in enumerate(levels)}
        self.truth_curve = truth_curve
        self.inside = None if truth_curve is None else {lv: (self.lower[lv] <= truth_curve) & (truth_curve <= self.upper[lv])
                                                        for lv in levels}
        self.values = values


class PosteriorCurves:
    """posterior_curves' result: the CurveBand of every curve by name (res["eta_over_s"], res.curves), levels, n_samples"""

    def __init__(self, curves, levels, n_samples):
        self.curves, self.levels, self.n_samples = curves, tuple(levels), int(n_samples)

    def __getitem__(self, name):
        return self.curves[name]

    def __iter__(self):
        return iter(self.curves)

    def __repr__(self):
        lines = ["PosteriorCurves(n_samples=%d, levels=%s)" % (self.n_samples, self.levels)]
        for nm, b in self.curves.items():
            tail = "" if b.inside is None else "  truth inside: " + ", ".join(
                "%g%%: %d/%d" % (lv, int(b.inside[lv].sum()), b.grid.shape[0]) for lv in self.levels)
            lines.append("  %-12s columns %s, %d grid points on [%g, %g]%s" % (nm, list(b.columns), b.grid.shape[0], b.grid[0],
                                                                              b.grid[-1], tail))
        return "\n".join(lines)


class ClosureDelta:
    """closure_delta's result: delta = the mean closure distance (the notebook's Delta_d), quantiles (levels q) of the
    per-sample distances, hist [bins] over edges [bins + 1] = what ax.hist(distances, bins=30) counts, per_parameter [ndim] =
    the mean of ((theta_j - truth_j) / width_j)^2 (delta is their mean); values [S] when asked for."""

    def __init__(self, delta, q, quantiles, hist, edges, per_parameter, n_samples, names=None, values=None):
        self.delta, self.q, self.quantiles, self.hist, self.edges = float(delta), q, quantiles, hist, edges
        self.per_parameter, self.n_samples, self.values = per_parameter, int(n_samples), values
        self.names = None if names is None else list(names)

    def __repr__(self):
        return "ClosureDelta(delta=%.6g, n_samples=%d, quantiles %s = %s)" % (
            self.delta, self.n_samples, [float(v) for v in self.q], ["%.4g" % v for v in self.quantiles])


class TraceHistogram:
    """trace_histogram's result: hist [ndim, nsteps, B] (int64; hist[j, t, b]: the walkers of step t with parameter j in bin
    b), edges [ndim, B + 1], outside [ndim, nsteps]"""

    def __init__(self, hist, edges, outside, names=None):
        self.hist, self.edges, self.outside = hist, edges, outside
        self.names = None if names is None else list(names)


def _levels_q(levels):
    levels = tuple(float(v) for v in np.atleast_1d(levels))
    if not levels or any(not (0.0 < v <= 100.0) for v in levels):
        raise ValueError("levels: credible levels in (0, 100] per cent")
    pct = [50.0]
    for v in levels:
        pct += [50.0 - v / 2.0, 50.0 + v / 2.0]
    return levels, np.asarray(pct) / 100.0             # (np.percentile's own division)


def _view3(x, layout, device):
    from .diagnostics import _as_device
    x = _as_device(x, device)
    if x.dim() == 2:
        return x[:, None, :], "steps", True
    if x.dim() != 3:
        raise ValueError("x: [nsteps, nwalkers, ndim], [nwalkers, nsteps, ndim] or [S, ndim]")
    return x, layout, False


def _specs(curves, columns, grid, d):
    out = []
    for nm in curves:
        if nm not in CURVES:
            raise ValueError("curves: names among %s" % (sorted(CURVES),))
        cols = tuple(int(c) for c in ((columns or {}).get(nm) or CURVES[nm]["columns"]))
        if len(cols) != len(CURVES[nm]["columns"]) or any(c < 0 or c >= d for c in cols):
            raise ValueError("columns[%r]: %d indices in [0, %d)" % (nm, len(CURVES[nm]["columns"]), d))
        g = (grid or {}).get(nm)
        g = np.ascontiguousarray(CURVES[nm]["grid"] if g is None else np.asarray(g, dtype=np.float64).reshape(-1))
        if g.shape[0] < 1 or not np.all(np.isfinite(g)):
            raise ValueError("grid[%r]: at least one finite value" % nm)
        out.append((nm, cols, g))
    return out


def posterior_curves(x, curves=("zeta_over_s", "eta_over_s", "y_loss"), columns=None, grid=None, levels=DEFAULT_LEVELS, truth=None,
                     layout="steps", weights=None, return_values=False, device=0, eng=None):
    """PosteriorCurves of a chain: x numpy or a torch cuda tensor / view, [nsteps, nwalkers, ndim] (layout "steps"), [nwalkers,
    nsteps, ndim] ("walkers") or a flat [S, ndim].  curves: names of CURVES; columns / grid: dicts name -> the curve's parameter
    columns / grid (default: the reference's indices, the notebook's 100-point grids; at most 1024 points).  levels: credible
    levels in per cent, at most seven; the band of a level is [percentile 50 - level / 2, percentile 50 + level / 2],
    np.percentile's.  truth [ndim]: the true parameters of a closure test; adds truth_curve and inside[level].  return_values:
    also the [S, G] curves (sample s = step * nwalkers + walker; small chains only: that is the array the select avoids).
    weights [S] with a flat x: the host path, weighted_quantile of the host-evaluated curves, no interpolation."""
    from .diagnostics import _engine
    from .emulator import percentile_from_order
    levels, q = _levels_q(levels)
    if weights is not None:
        xh = np.asarray(x.cpu().numpy() if hasattr(x, "data_ptr") else x, dtype=np.float64)
        if xh.ndim != 2:
            raise ValueError("weights go with a flat [S, ndim] sample set")
        w = np.asarray(weights.cpu().numpy() if hasattr(weights, "data_ptr") else weights, dtype=np.float64).reshape(-1)
        S, d = xh.shape
        if w.shape[0] != S or not np.all(np.isfinite(w)) or np.any(w < 0.0) or not w.max() > 0.0:
            raise ValueError("weights: [%d] finite, non-negative, not all zero" % S)
        bands = {}
        for nm, cols, g in _specs(curves, columns, grid, d):
            vals = curve_on_host(nm, xh, cols, g)
            tc = None if truth is None else curve_on_host(nm, np.asarray(truth, dtype=np.float64)[None, :], cols, g)[0]
            bands[nm] = CurveBand(nm, cols, g, q, weighted_quantile(vals, w, q), levels, tc, vals if return_values else None)
        return PosteriorCurves(bands, levels, S)
    x3, layout, _ = _view3(x, layout, device)
    d = int(x3.shape[2])
    S = int(x3.shape[0]) * int(x3.shape[1])
    if S < 1:
        raise ValueError("x: no samples")
    eng = eng or _engine(x3.device.index or 0)
    if q.shape[0] > eng.PPD_MAX_LEVELS:
        raise ValueError("levels: at most %d" % ((eng.PPD_MAX_LEVELS - 1) // 2))
    specs = _specs(curves, columns, grid, d)
    bands = {}
    for G in sorted({g.shape[0] for _, _, g in specs}):               # one call per grid length (the default grids: one call)
        grp = [s for s in specs if s[2].shape[0] == G]
        desc = [[CURVES[nm]["fn"]] + list(cols) + [-1] * (4 - len(cols)) for nm, cols, _ in grp]
        out = eng.chain_curves(x3, layout, desc, np.stack([g for _, _, g in grp]), q, values=return_values)
        pct = percentile_from_order(out["order"], q, S)               # [ncurves, G, nq]
        for i, (nm, cols, g) in enumerate(grp):
            tc = None if truth is None else curve_on_host(nm, np.asarray(truth, dtype=np.float64)[None, :], cols, g)[0]
            bands[nm] = CurveBand(nm, cols, g, q, np.ascontiguousarray(pct[i].T), levels, tc,
                                  np.ascontiguousarray(out["values"][i].T) if return_values else None)
    return PosteriorCurves({nm: bands[nm] for nm, _, _ in specs}, levels, S)


def closure_delta(x, truth, prior_ranges, bins=30, quantiles=(0.16, 0.5, 0.84), layout="steps", weights=None, names=None,
                  return_values=False, device=0, eng=None):
    """ClosureDelta of a chain against the true parameters of a closure test: the notebook's compute_Delta_d (delta = the mean
    over the samples of (1 / d) sum_j ((theta_j - truth_j) / (max_j - min_j))^2), create_Delta_d_distribution (the per-sample
    distances) and the ax.hist(distances, bins=30) of them.  x as posterior_curves takes it; truth [ndim]; prior_ranges [ndim, 2].
    The distances are evaluated on the device (gpb_chain_curves' fn 3) into one [S] row that stays there; gpb_ppd_summary
    gives their mean and exact order statistics, gpb_chain_marginals counts them over np.linspace(min, max, bins + 1), minimum
    and maximum being the q = 0 and q = 1 order statistics.  per_parameter comes from torch on the device, one column at a time.
    weights [S] with a flat x: everything on the host with numpy."""
    from .diagnostics import _engine
    from .emulator import percentile_from_order
    truth = np.asarray(truth, dtype=np.float64).reshape(-1)
    pr = np.asarray(prior_ranges, dtype=np.float64)
    d = truth.shape[0]
    if pr.shape != (d, 2):
        raise ValueError("prior_ranges: [%d, 2]" % d)
    width = pr[:, 1] - pr[:, 0]
    if not (np.all(np.isfinite(truth)) and np.all(np.isfinite(width)) and np.all(width > 0.0)):
        raise ValueError("truth must be finite and every prior range of positive, finite width")
    qu = np.atleast_1d(np.asarray(quantiles, dtype=np.float64)).reshape(-1)
    B = int(bins)
    if weights is not None:
        xh = np.asarray(x.cpu().numpy() if hasattr(x, "data_ptr") else x, dtype=np.float64)
        if xh.ndim != 2 or xh.shape[1] != d:
            raise ValueError("weights go with a flat [S, %d] sample set" % d)
        w = np.asarray(weights.cpu().numpy() if hasattr(weights, "data_ptr") else weights, dtype=np.float64).reshape(-1)
        dist = closure_distance(xh, truth, width)
        hist, edges = np.histogram(dist, bins=B, weights=w)
        per = (((xh - truth) / width) ** 2 * w[:, None]).sum(axis=0) / w.sum()
        return ClosureDelta(np.sum(dist * w) / w.sum(), qu, weighted_quantile(dist[:, None], w, qu)[:, 0], hist, edges, per,
                            xh.shape[0], names, dist if return_values else None)
    import torch
    x3, layout, _ = _view3(x, layout, device)
    if int(x3.shape[2]) != d:
        raise ValueError("x has %d parameters, truth %d" % (int(x3.shape[2]), d))
    S = int(x3.shape[0]) * int(x3.shape[1])
    eng = eng or _engine(x3.device.index or 0)
    q_all = np.concatenate([[0.0, 1.0], qu])
    if q_all.shape[0] > eng.PPD_MAX_LEVELS:
        raise ValueError("quantiles: at most %d levels" % (eng.PPD_MAX_LEVELS - 2))
    vals = eng.chain_curves(x3, layout, [[3, -1, -1, -1, -1]], [[0.0]], None, aux=np.concatenate([truth, width]), values=True,
                            on_device=True)["values"].reshape(1, S)
    out = eng.ppd_summary(vals, None, q_all, outputs=("moments", "order"))
    lo, hi = float(out["order"][0, 0, 0]), float(out["order"][0, 1, 1])
    if lo == hi:                                           # numpy's rule for an empty range
        lo, hi = lo - 0.5, hi + 0.5
    edges = np.linspace(lo, hi, B + 1)
    hist = eng.chain_marginals(vals.reshape(S, 1, 1), "steps", edges[None, :], outputs=("h1",))["h1"][0]
    per = np.empty(d)
    for j in range(d):
        per[j] = float((((x3[:, :, j] - truth[j]) / width[j]) ** 2).mean())
    pct = percentile_from_order(out["order"], q_all, S)[0]
    return ClosureDelta(out["moments"][0, 0], qu, pct[2:], hist, edges, per, S, names,
                        vals.reshape(S).cpu().numpy() if return_values else None)


def trace_histogram(x, bins=30, range=None, layout="steps", names=None, device=0, eng=None):
    """TraceHistogram of a chain: per parameter np.histogram2d(step, value, bins=[nsteps, bins])'s counts, the walkers'
    distribution step by step (how burn-in is judged by eye).  x: [nsteps, nwalkers, ndim] (layout "steps") or [nwalkers, nsteps,
    ndim] ("walkers"), numpy or a torch cuda tensor / view.  bins, range: as marginals.marginals takes them; the default range is
    every parameter's extent over the whole chain, as histogram2d takes it."""
    from .diagnostics import _as_device, _engine
    from .marginals import _edges
    x = _as_device(x, device)
    if x.dim() != 3:
        raise ValueError("x: [nsteps, nwalkers, ndim] or [nwalkers, nsteps, ndim]")
    eng = eng or _engine(x.device.index or 0)
    edges = _edges(x, bins, range, int(x.shape[2]))
    out = eng.chain_trace_hist(x, layout, edges)
    return TraceHistogram(out["hist"], edges, out["outside"], names)
