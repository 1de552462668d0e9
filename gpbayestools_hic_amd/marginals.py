"""
The posterior in parameter space, on the device: what examples/PlotMCMC.ipynb (plot_corner_1dataset, extract_parameters) takes
from a chain — per parameter `np.percentile(samples[:, i], [16, 50, 84])` and `ax.hist(samples[:, i], bins=20, density=True)`,
per pair `ax.hist2d(samples[:, j], samples[:, i], bins=20)` — for a chain that lies in device memory, all pairs in one call
(gpb_chain_marginals): the sampler's [nsteps, nwalkers, ndim] store, a pickle's [nwalkers, nsteps, ndim]
or a thinned view of either is read through its strides, nothing is copied to the host but the counts.

The counts are np.histogram's and np.histogram2d's, integer for integer: a value is searched in the bin edges, e[b] <= x <
e[b + 1] with the last bin closed.  The percentiles are np.percentile's, bit for bit: the two order statistics come from the
exact select of gpb_ppd_summary and are interpolated by numpy's own rule (emulator.percentile_from_order).

Importance weights (a pocoMC / run_SMC particle set: `chain` and `weights` of the pickle) are honoured: every sample adds
rint(w 2^32 / max w) instead of 1, an integer, so that the weighted counts are as reproducible as the plain ones.  The
reference's notebook ignores the weights of such a set and plots another distribution.
"""
import numpy as np

DEFAULT_QUANTILES = (0.05, 0.16, 0.5, 0.84, 0.95)
_BAND = (0.16, 0.5, 0.84)


class PosteriorMarginals:
    """edges [ndim, B + 1]; hist1d [ndim, B] and hist2d [npairs, B, B] (int64; hist2d[p, bi, bj]: parameter pairs[p, 0] in bin
    bi, pairs[p, 1] in bin bj) with pairs [npairs, 2]; outside [ndim], the samples beyond the edges; n_samples; quantiles [nq]
    and percentiles [nq, ndim]; median [ndim], lower = median - p16, upper = p84 - median (the notebook's error form); names.
    With weights the counts are sums of the integer weights rint(w weight_scale) (weight_scale = 2^32 / max w, else None)."""

    def __init__(self, edges, hist1d, hist2d, pairs, outside, n_samples, quantiles, percentiles, median, lower, upper, names=None,
                 weight_scale=None):
        self.edges, self.hist1d, self.hist2d, self.pairs, self.outside = edges, hist1d, hist2d, pairs, outside
        self.n_samples = int(n_samples)
        self.quantiles, self.percentiles = quantiles, percentiles
        self.median, self.lower, self.upper = median, lower, upper
        self.names = None if names is None else list(names)
        self.weight_scale = weight_scale
        self._where = {(int(i), int(j)): p for p, (i, j) in enumerate(np.asarray(pairs).reshape(-1, 2))}

    def density1d(self):
        """[ndim, B]: counts / (total * bin width) with total = all samples of the parameter, those outside the edges included:
        `hist(density=True)` when nothing lies outside; each row integrates to the share inside."""
        total = (self.hist1d.sum(axis=1) + self.outside).astype(np.float64)
        return self.hist1d / (total[:, None] * np.diff(self.edges, axis=1))

    def pair(self, i, j):
        """the [B, B] table of parameters (i, j), rows the bins of i: looked up, transposed when it was stored as (j, i)"""
        i, j = int(i), int(j)
        if (i, j) in self._where:
            return self.hist2d[self._where[(i, j)]]
        if (j, i) in self._where:
            return self.hist2d[self._where[(j, i)]].T
        raise KeyError("pair (%d, %d) was not computed" % (i, j))

    def credible_levels(self, i, j, levels=(0.68, 0.95)):
        """Count thresholds of the highest-density regions of pair (i, j): the bins sorted by count, descending; the threshold
        of a level is the count of the first bin at which the cumulative count reaches level * total (contour the table at
        it).  Host arithmetic on the B x B table.  An empty table gives zeros."""
        c = np.sort(self.pair(i, j).reshape(-1))[::-1]
        cum = np.cumsum(c)
        levels = np.atleast_1d(np.asarray(levels, dtype=np.float64))
        if cum[-1] == 0:
            return np.zeros(levels.shape, dtype=c.dtype)
        k = np.minimum(np.searchsorted(cum, levels * float(cum[-1]), side="left"), c.shape[0] - 1)
        return c[k]

    def __repr__(self):
        d = self.hist1d.shape[0]
        names = self.names or ["p%d" % j for j in range(d)]
        wid = max([9] + [len(str(s)) for s in names])
        lines = ["PosteriorMarginals(n_samples=%d, ndim=%d, bins=%d, pairs=%d%s)"
                 % (self.n_samples, d, self.hist1d.shape[1], len(self.pairs), ", weighted" if self.weight_scale else ""),
                 "  %-*s %12s %12s %12s %s %10s" % (wid, "parameter", "median", "-lower", "+upper",
                                                   " ".join("%12s" % ("q%g" % q) for q in self.quantiles), "outside")]
        for j, nm in enumerate(names):
            lines.append("  %-*s %12.5g %12.5g %12.5g %s %10d"
                         % (wid, nm, self.median[j], self.lower[j], self.upper[j],
                            " ".join("%12.5g" % v for v in self.percentiles[:, j]), self.outside[j]))
        return "\n".join(lines)


def weighted_quantile(x, w, q):
    """[nq, ndim]: per column of x [S, ndim] the smallest sample whose cumulative normalised weight reaches q (host, numpy:
    a stable sort per column)."""
    x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64).reshape(-1)
    q = np.atleast_1d(np.asarray(q, dtype=np.float64))
    out = np.empty((q.shape[0], x.shape[1]))
    for j in range(x.shape[1]):
        o = np.argsort(x[:, j], kind="stable")
        cw = np.cumsum(w[o])
        k = np.minimum(np.searchsorted(cw, q * cw[-1], side="left"), x.shape[0] - 1)
        out[:, j] = x[o[k], j]
    return out


def _edges(x3, bins, rng, d):
    """[ndim, B + 1] from bins (an int, shared edges [B + 1] or per-parameter edges [ndim, B + 1]) and range ([ndim, 2], or
    None / "data": the minimum and maximum per parameter, taken on the device)"""
    if np.ndim(bins) > 0:
        e = np.asarray(bins, dtype=np.float64)
        if e.ndim == 1:
            e = np.broadcast_to(e, (d, e.shape[0]))
        if e.ndim != 2 or e.shape[0] != d or e.shape[1] < 2:
            raise ValueError("bins: an int, edges [B + 1] or per-parameter edges [%d, B + 1]" % d)
        return np.ascontiguousarray(e)
    B = int(bins)
    if B < 1:
        raise ValueError("bins: at least one")
    if rng is None or (isinstance(rng, str) and rng == "data"):
        lo = x3.amin(dim=(0, 1)).cpu().numpy()
        hi = x3.amax(dim=(0, 1)).cpu().numpy()
        same = lo == hi                                    # numpy's rule for an empty range (_get_outer_edges)
        lo, hi = np.where(same, lo - 0.5, lo), np.where(same, hi + 0.5, hi)
    else:
        r = np.asarray(rng, dtype=np.float64)
        if r.shape != (d, 2):
            raise ValueError("range: [%d, 2], None or 'data'" % d)
        lo, hi = r[:, 0], r[:, 1]
    return np.ascontiguousarray(np.stack([np.linspace(lo[j], hi[j], B + 1) for j in range(d)]))


def marginals(x, bins=20, range=None, pairs=None, weights=None, quantiles=DEFAULT_QUANTILES, layout="steps", names=None, device=0,
              eng=None):
    """PosteriorMarginals of a chain: x numpy or a torch cuda tensor / view, [nsteps, nwalkers, ndim] (layout "steps"),
    [nwalkers, nsteps, ndim] ("walkers") or a flat [S, ndim].  bins: an int (with range [ndim, 2], or None / "data" for the
    minimum and maximum of every parameter, as np.histogram2d(a, b, bins=20) takes them) or the edges themselves; at most 64
    bins.  pairs [npairs, 2]: default all i < j.  quantiles: at most 16 levels, counting 0.16 / 0.5 / 0.84, which are always
    computed.  weights [S] with a flat x only.  The values must be finite (a numpy input is checked; the library itself counts
    NaN and infinities as outside, but the percentiles' select takes finite input).

    Unweighted percentiles are np.percentile's bit for bit (the chain is transposed to [ndim, S] on the device and
    gpb_ppd_summary's exact select yields the two order statistics numpy interpolates).  WEIGHTED percentiles are computed on
    the HOST with numpy — weighted sets are particle sets of 1e4 .. 1e5 rows: the smallest sample whose cumulative normalised
    weight reaches q (weighted_quantile); no interpolation."""
    import torch
    from .diagnostics import _as_device, _engine
    from .emulator import percentile_from_order
    x = _as_device(x, device)
    flat = x.dim() == 2
    if flat:
        x3, layout = x[:, None, :], "steps"
    elif x.dim() == 3:
        x3 = x
    else:
        raise ValueError("x: [nsteps, nwalkers, ndim], [nwalkers, nsteps, ndim] or [S, ndim]")
    if weights is not None and not flat:
        raise ValueError("weights go with a flat [S, ndim] sample set")
    d = int(x3.shape[2])
    S = int(x3.shape[0]) * int(x3.shape[1])
    if S < 1 or d < 1:
        raise ValueError("x: no samples")
    eng = eng or _engine(x.device.index or 0)
    edges = _edges(x3, bins, range, d)
    if pairs is None:
        pairs_arr = np.array([(i, j) for i in np.arange(d) for j in np.arange(i + 1, d)], dtype=np.int32).reshape(-1, 2)
    else:
        pairs_arr = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
    q_user = np.atleast_1d(np.asarray(quantiles, dtype=np.float64)).reshape(-1)
    if not np.all((q_user >= 0.0) & (q_user <= 1.0)):
        raise ValueError("quantiles: levels in [0, 1]")
    q_all = np.concatenate([q_user, [v for v in _BAND if v not in q_user]])
    if q_all.shape[0] > eng.PPD_MAX_LEVELS:
        raise ValueError("quantiles: at most %d levels, 0.16 / 0.5 / 0.84 included" % eng.PPD_MAX_LEVELS)
    wscale = None
    if weights is not None:
        w = np.asarray(weights.cpu().numpy() if hasattr(weights, "data_ptr") else weights, dtype=np.float64).reshape(-1)
        if w.shape[0] != S or not np.all(np.isfinite(w)) or np.any(w < 0.0) or not w.max() > 0.0:
            raise ValueError("weights: [%d] finite, non-negative, not all zero" % S)
        wscale = 4294967296.0 / float(w.max())
    out = eng.chain_marginals(x3, layout, edges, pairs=None if pairs is None else pairs_arr, weights=weights)
    if weights is None:
        xt = x3.permute(2, 0, 1).reshape(d, S)                      # [ndim, S]: one row per parameter for the select
        order = eng.ppd_summary(xt.contiguous(), None, q_all, outputs=("order",))["order"]
        pct = np.ascontiguousarray(percentile_from_order(order, q_all, S).T)
        del xt
    else:
        pct = weighted_quantile(x3.reshape(S, d).cpu().numpy(), w, q_all)
    at = {v: int(np.flatnonzero(q_all == v)[0]) for v in _BAND}
    med = pct[at[0.5]]
    return PosteriorMarginals(edges, out["h1"], out["h2"], pairs_arr, out["outside"], S, q_user, pct[:q_user.shape[0]], med,
                              med - pct[at[0.16]], pct[at[0.84]] - med, names=names, weight_scale=wscale)
