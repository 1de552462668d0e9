"""
How much did the data teach us, and do two calibrations agree?  examples/PlotMCMC.ipynb overlays the posterior on the prior, and
two or three posteriors on each other (plot_corner_compare_datasets, plot_compare_posteriors_3datasets: other data sets, emcee
against pocoMC, closure set k against set k'), and leaves both questions to the eye.  The numbers for them:

  information_gain       the Kullback-Leibler divergence from the uniform prior box to the posterior, for the whole parameter
                         space (Kozachenko-Leonenko nearest-neighbour entropy) and per parameter (histograms)
  posterior_divergence   D(A || B) and D(B || A) of two sample sets in the whole space (Wang-Kulkarni-Verdu), and per parameter
                         and pair the Jensen-Shannon divergence of the histograms and the shift of the medians

The nearest-neighbour distances are brute force on the device (gpb_chain_knn): S^2 pair distances in d
dimensions, where kd-trees degenerate (d = 20) and the host takes minutes.  The chains are read where they lie, through their
strides, as marginals.marginals reads them.

What the estimators are NOT.  They are consistent, not unbiased: at finite n the estimate depends on k (every k = 1 .. kmax is
reported from one pass, so that the stability is visible) and the bias grows with the dimension.  The prior box has hard walls:
a posterior that fills much of the box loses neighbours beyond the walls and its gain is biased LOW.  Repeated rows distort them:
an MCMC chain repeats a row after every rejected move, its k-th neighbour is then nearer than the density warrants (or at
distance 0, which is not listed but moves the next ones up); `duplicate_fraction` reports the share of such rows and a warning
says to thin — by about the autocorrelation time, so that the rows are close to independent, which the estimators assume.
"""
import logging
import math
import pickle

import numpy as np

log = logging.getLogger(__name__)
LN2 = math.log(2.0)


# ---------------------------------------------------------------------------------------------------------------- host pieces
def digamma_int(n):
    """psi(n) for an integer n >= 1: -gamma + sum_{m < n} 1 / m, the asymptotic series from 64 on (below 1e-15 there)"""
    n = int(n)
    if n < 1:
        return float("nan")
    if n < 64:
        return -np.euler_gamma + float(np.sum(1.0 / np.arange(1, n)))
    x = float(n)
    return math.log(x) - 0.5 / x - 1.0 / (12 * x ** 2) + 1.0 / (120 * x ** 4) - 1.0 / (252 * x ** 6)


def log_unit_ball(d):
    """ln c_d, c_d = pi^(d/2) / Gamma(d/2 + 1): the volume of the unit ball"""
    return 0.5 * d * math.log(math.pi) - math.lgamma(0.5 * d + 1.0)


def kl_entropy(r2, d, keep=None):
    """Kozachenko-Leonenko entropy [kmax] in the scaled coordinates from the squared k-th neighbour distances r2 [n, kmax] within
    a set: psi(n) - psi(k) + ln c_d + (d / n) sum_i ln rho_k(i), rho = sqrt(r2[:, k - 1]), over the rows of keep (default all).
    nan for a k whose distances are not all finite and positive."""
    r2 = np.asarray(r2)[slice(None) if keep is None else keep]
    n, kmax = r2.shape
    out = np.full(kmax, np.nan)
    for k in range(1, kmax + 1):
        col = r2[:, k - 1]
        if n and np.all(np.isfinite(col)) and np.all(col > 0.0):
            out[k - 1] = digamma_int(n) - digamma_int(k) + log_unit_ball(d) + (d / n) * np.sum(np.log(np.sqrt(col)))
    return out


def wkv_divergence(r2_aa, r2_ab, d, m, keep=None):
    """Wang-Kulkarni-Verdu D(A || B) [kmax] in nats: (d / n) sum_i ln(nu_k(i) / rho_k(i)) + ln(m / (n - 1)), rho the k-th
    neighbour distance within A, nu from A to the m rows of B, over the rows of keep.  nan for a k whose distances are not all
    finite and positive."""
    sel = slice(None) if keep is None else keep
    rho2, nu2 = np.asarray(r2_aa)[sel], np.asarray(r2_ab)[sel]
    n, kmax = rho2.shape
    out = np.full(kmax, np.nan)
    for k in range(1, kmax + 1):
        a, b = rho2[:, k - 1], nu2[:, k - 1]
        if n > 1 and m > 0 and np.all(np.isfinite(a)) and np.all(np.isfinite(b)) and np.all(a > 0.0) and np.all(b > 0.0):
            out[k - 1] = (d / n) * np.sum(np.log(np.sqrt(b) / np.sqrt(a))) + math.log(m / (n - 1.0))
    return out


def hist_gain(counts):
    """sum_b p_b ln(p_b B) over the non-empty bins of every row of counts [..., B]: the divergence of the histogram from the
    uniform one, nats; nan for an empty row"""
    c = np.asarray(counts, dtype=np.float64)
    B = c.shape[-1]
    tot = c.sum(axis=-1, keepdims=True)
    with np.errstate(all="ignore"):
        p = c / tot
        term = np.where(c > 0, p * np.log(np.where(c > 0, p, 1.0) * B), 0.0)
    return np.where(tot[..., 0] > 0, term.sum(axis=-1), np.nan)


def hist_js(ca, cb):
    """Jensen-Shannon divergence (nats, at most ln 2) of the normalised histograms ca, cb [..., B]; nan where one is empty"""
    ca, cb = np.asarray(ca, dtype=np.float64), np.asarray(cb, dtype=np.float64)
    ta, tb = ca.sum(axis=-1, keepdims=True), cb.sum(axis=-1, keepdims=True)
    with np.errstate(all="ignore"):
        p, q = ca / ta, cb / tb
        m = 0.5 * (p + q)
        a = np.where(p > 0, p * np.log(np.where(p > 0, p, 1.0) / np.where(p > 0, m, 1.0)), 0.0)
        b = np.where(q > 0, q * np.log(np.where(q > 0, q, 1.0) / np.where(q > 0, m, 1.0)), 0.0)
    js = 0.5 * a.sum(axis=-1) + 0.5 * b.sum(axis=-1)
    return np.where((ta[..., 0] > 0) & (tb[..., 0] > 0), js, np.nan)


# ---------------------------------------------------------------------------------------------------------------- the raw call
def _device_chain(x, layout, device, what="x"):
    """(x3, layout): numpy or a torch cuda tensor, [nsteps, nwalkers, ndim] / [nwalkers, nsteps, ndim] / flat [S, ndim], as a
    three-dimensional float64 device tensor; non-finite rows are the library's to skip"""
    import torch
    if hasattr(x, "data_ptr"):
        x = x if x.dtype == torch.float64 else x.to(torch.float64)
    else:
        x = torch.as_tensor(np.require(np.asarray(x, dtype=np.float64), requirements=["C"]), device=torch.device("cuda", device))
    if x.dim() == 2:
        return x[:, None, :], "steps"
    if x.dim() != 3:
        raise ValueError("%s: [nsteps, nwalkers, ndim], [nwalkers, nsteps, ndim] or [S, ndim]" % what)
    return x, layout


def knn_distances(xa, xb=None, k=8, scale=None, layout="steps", layout_b=None, skip_zero=True, return_index=False, splits=0,
                  device=0, eng=None):
    """The raw call (gpb_chain_knn): for every row of xa the k smallest squared distances, in coordinates divided by scale
    [ndim] (default ones), to the rows of xa itself (xb None; the row itself excluded) or of xb.  xa, xb numpy arrays or torch
    cuda tensors / views, [nsteps, nwalkers, ndim] (layout "steps"), [nwalkers, nsteps, ndim] ("walkers") or flat [S, ndim];
    ndim <= 64, k <= 16.  Returns a dict of numpy arrays: "r2" [nA, k] ascending, "zeros" [nA] (candidates at distance exactly 0:
    repeated rows; with skip_zero they are not listed), "n_skipped" (rows of xa, of xb with a non-finite coordinate: r2 = inf,
    never a candidate) and, with return_index, "idx" [nA, k] (row numbers, the outer axis of the memory layout first; -1 where
    fewer than k candidates exist).  Bit for bit what tests/knn_reference.py computes in numpy; splits changes no output."""
    from .diagnostics import _engine
    a3, layout = _device_chain(xa, layout, device, "xa")
    b3 = None
    if xb is not None:
        b3, layout_b = _device_chain(xb, layout_b or layout, a3.device.index or 0, "xb")
        if b3.device != a3.device:
            raise ValueError("xa and xb live on different devices")
    d = int(a3.shape[2])
    if int(a3.shape[0]) * int(a3.shape[1]) < 1 or d < 1:
        raise ValueError("xa: no samples")
    sc = np.ones(d) if scale is None else np.asarray(scale, dtype=np.float64).reshape(-1)
    if sc.shape[0] != d or not np.all(np.isfinite(sc)) or not np.all(sc > 0.0):
        raise ValueError("scale: [%d] finite and positive" % d)
    eng = eng or _engine(a3.device.index or 0)
    return eng.chain_knn(a3, layout, b3, layout_b, k=k, inv_scale=1.0 / sc, skip_zero=skip_zero, splits=splits,
                         return_index=return_index)


def _no_weights(weights, who):
    if weights is not None:
        raise ValueError("%s: the nearest-neighbour estimators take unweighted samples; resample the particle set by its weights "
                         "first (k=0 gives the histogram numbers alone, which honour the weights)" % who)


def _box(lo, hi, d):
    lo, hi = np.asarray(lo, dtype=np.float64).reshape(-1), np.asarray(hi, dtype=np.float64).reshape(-1)
    if lo.shape[0] != d or hi.shape[0] != d or not np.all(np.isfinite(lo)) or not np.all(np.isfinite(hi)) or not np.all(hi > lo):
        raise ValueError("lo, hi: [%d] finite, hi > lo" % d)
    return lo, hi


def _keep(out, n):
    """the rows that were not skipped as queries (a skipped row: r2 = inf and zeros = 0), None: all.  Where rows without any
    candidate make that ambiguous, all rows are kept and every k is nan."""
    if not out["n_skipped"][0]:
        return None
    keep = np.isfinite(out["r2"][:, 0]) | (out["zeros"] > 0)
    return keep if n - int(keep.sum()) == out["n_skipped"][0] else None


def _warn_duplicates(frac, who):
    if frac > 0.0:
        log.warning("%s: %.1f%% of the rows have an exact copy in the set (rejected moves repeat a row); the nearest-neighbour "
                    "estimators assume independent samples — thin the chain by about its autocorrelation time", who, 100.0 * frac)


# ---------------------------------------------------------------------------------------------------------------- information gain
class InformationGain:
    """Of a posterior sample against the uniform prior on the box [lo, hi].  Whole space, for k = 1 .. kmax (index k - 1):
    entropy [kmax] of the sample in box units (the prior's is 0), gain_nats = -entropy, gain_bits.  Per parameter: gain_1d_nats,
    gain_1d_bits [ndim] from the `bins`-bin histograms.  duplicate_fraction: the share of rows with an exact copy in the set;
    n_samples, n_skipped (rows with a non-finite coordinate, left out), r2 [n_samples, kmax] the squared k-th neighbour distances
    in box units, scale = hi - lo, names.  log_density(k), densest: see there.  Without nearest neighbours (k = 0) the whole-space
    fields are empty."""

    def __init__(self, entropy, gain_1d_nats, r2, zeros, n_samples, n_skipped, scale, bins, names=None):
        self.entropy = entropy
        self.gain_nats = -entropy
        self.gain_bits = self.gain_nats / LN2
        self.gain_1d_nats = gain_1d_nats
        self.gain_1d_bits = gain_1d_nats / LN2
        self.r2, self.zeros = r2, zeros
        self.n_samples, self.n_skipped = int(n_samples), int(n_skipped)
        self.scale, self.bins = scale, int(bins)
        self.kmax = int(entropy.shape[0])
        self.names = None if names is None else list(names)
        self.duplicate_fraction = float(np.mean(zeros > 0)) if zeros is not None and zeros.shape[0] else 0.0

    def _valid(self):
        return np.isfinite(self.r2[:, 0]) if self.kmax else np.zeros(0, dtype=bool)

    def log_density(self, k=None):
        """[n_samples]: the k-th neighbour estimate of the log posterior density at every row, in the chain's own units: ln k -
        ln(n - 1) - ln c_d - (d / 2) ln r2_k(i) - sum_j ln scale_j (k default kmax; nan for a skipped row)"""
        k = self.kmax if k is None else int(k)
        if not 1 <= k <= self.kmax:
            raise ValueError("k: 1 .. %d" % self.kmax)
        d, n = self.scale.shape[0], int(self._valid().sum())
        with np.errstate(all="ignore"):
            out = (math.log(k) - math.log(n - 1.0) - log_unit_ball(d) - 0.5 * d * np.log(self.r2[:, k - 1])
                   - float(np.sum(np.log(self.scale))))
        return np.where(self._valid(), out, np.nan)

    @property
    def densest(self):
        """the row with the smallest kmax-th neighbour distance: the densest sample of the chain"""
        if not self.kmax or not self.r2.shape[0]:
            return -1
        return int(np.argmin(self.r2[:, self.kmax - 1]))

    def __repr__(self):
        d = self.gain_1d_nats.shape[0]
        names = self.names or ["p%d" % j for j in range(d)]
        wid = max([9] + [len(str(s)) for s in names])
        lines = ["InformationGain(n_samples=%d, ndim=%d, kmax=%d, bins=%d%s%s)"
                 % (self.n_samples, d, self.kmax, self.bins, ", skipped=%d" % self.n_skipped if self.n_skipped else "",
                    ", duplicates=%.3g" % self.duplicate_fraction if self.duplicate_fraction else "")]
        if self.kmax:
            lines.append("  %-*s %s" % (wid, "k", " ".join("%10d" % (k + 1) for k in range(self.kmax))))
            lines.append("  %-*s %s" % (wid, "gain/nats", " ".join("%10.4f" % v for v in self.gain_nats)))
            lines.append("  %-*s %s" % (wid, "gain/bits", " ".join("%10.4f" % v for v in self.gain_bits)))
        lines.append("  %-*s %12s %12s" % (wid, "parameter", "gain/nats", "gain/bits"))
        for j, nm in enumerate(names):
            lines.append("  %-*s %12.5g %12.5g" % (wid, nm, self.gain_1d_nats[j], self.gain_1d_bits[j]))
        return "\n".join(lines)


def information_gain(x, lo, hi, k=8, bins=20, weights=None, layout="steps", splits=0, names=None, device=0, eng=None):
    """InformationGain of the sample x — numpy or a torch cuda tensor / view, [nsteps, nwalkers, ndim] (layout "steps"),
    [nwalkers, nsteps, ndim] ("walkers") or flat [S, ndim] — against the uniform prior on the box [lo, hi].  The coordinates are
    divided by hi - lo: the prior is then the unit cube, of entropy 0, and the gain is minus the Kozachenko-Leonenko entropy of
    the sample, reported for every k = 1 .. k from one pass over the pairs (gpb_chain_knn).  Per parameter the divergence of the
    `bins`-bin histogram over [lo, hi] (gpb_chain_marginals' counts) from the uniform one.  weights [S] (a flat particle set)
    enter the histograms as in marginals.marginals; the nearest-neighbour part raises ValueError for them (k=0: histograms
    only).  Thin an MCMC chain first: see the module's notes."""
    from .diagnostics import _engine
    from .marginals import _edges
    x3, layout = _device_chain(x, layout, device)
    d = int(x3.shape[2])
    S = int(x3.shape[0]) * int(x3.shape[1])
    if S < 1 or d < 1:
        raise ValueError("x: no samples")
    lo, hi = _box(lo, hi, d)
    k = int(k)
    if k:
        _no_weights(weights, "information_gain")
    if weights is not None and int(x3.shape[1]) != 1:
        raise ValueError("weights go with a flat [S, ndim] sample set")
    eng = eng or _engine(x3.device.index or 0)
    scale = hi - lo
    edges = _edges(x3, int(bins), np.stack([lo, hi], axis=1), d)
    h1 = eng.chain_marginals(x3, layout, edges, weights=weights, outputs=("h1",))["h1"]
    g1 = hist_gain(h1)
    if not k:
        return InformationGain(np.zeros(0), g1, np.zeros((S, 0)), None, S, 0, scale, bins, names)
    out = eng.chain_knn(x3, layout, k=k, inv_scale=1.0 / scale, skip_zero=True, splits=splits, return_index=False)
    r2, zeros = out["r2"], out["zeros"]
    keep = _keep(out, S)
    res = InformationGain(kl_entropy(r2, d, keep), g1, r2, zeros, S, out["n_skipped"][0], scale, bins, names)
    _warn_duplicates(res.duplicate_fraction, "information_gain")
    return res


# ---------------------------------------------------------------------------------------------------------------- two posteriors
class PosteriorComparison:
    """Of two sample sets A and B on the box [lo, hi].  Whole space, for k = 1 .. kmax (index k - 1), nats: kl_ab = D(A || B),
    kl_ba = D(B || A), symmetric = kl_ab + kl_ba.  Per parameter: js_1d [ndim], the Jensen-Shannon divergence of the histograms
    (nats, at most ln 2), and shift [ndim] = (median_a - median_b) / sqrt(sigma_a^2 + sigma_b^2) with sigma = (p84 - p16) / 2; per
    pair js_2d [npairs] with pairs [npairs, 2].  duplicate_fraction_a, _b; n_a, n_b, n_skipped (a pair); names."""

    def __init__(self, kl_ab, kl_ba, js_1d, js_2d, pairs, shift, dup_a, dup_b, n_a, n_b, n_skipped, bins, names=None):
        self.kl_ab, self.kl_ba, self.symmetric = kl_ab, kl_ba, kl_ab + kl_ba
        self.js_1d, self.js_2d, self.pairs, self.shift = js_1d, js_2d, pairs, shift
        self.duplicate_fraction_a, self.duplicate_fraction_b = float(dup_a), float(dup_b)
        self.n_a, self.n_b, self.n_skipped, self.bins = int(n_a), int(n_b), tuple(n_skipped), int(bins)
        self.kmax = int(kl_ab.shape[0])
        self.names = None if names is None else list(names)

    def __repr__(self):
        d = self.js_1d.shape[0]
        names = self.names or ["p%d" % j for j in range(d)]
        wid = max([9] + [len(str(s)) for s in names])
        lines = ["PosteriorComparison(n_a=%d, n_b=%d, ndim=%d, kmax=%d, bins=%d, pairs=%d)"
                 % (self.n_a, self.n_b, d, self.kmax, self.bins, len(self.pairs))]
        if self.kmax:
            lines.append("  %-*s %s" % (wid, "k", " ".join("%10d" % (k + 1) for k in range(self.kmax))))
            lines.append("  %-*s %s" % (wid, "D(A||B)", " ".join("%10.4f" % v for v in self.kl_ab)))
            lines.append("  %-*s %s" % (wid, "D(B||A)", " ".join("%10.4f" % v for v in self.kl_ba)))
        lines.append("  %-*s %12s %12s" % (wid, "parameter", "JS/nats", "shift"))
        for j, nm in enumerate(names):
            lines.append("  %-*s %12.5g %12.5g" % (wid, nm, self.js_1d[j], self.shift[j]))
        return "\n".join(lines)


def posterior_divergence(xa, xb, lo, hi, k=8, bins=20, pairs=None, weights_a=None, weights_b=None, layout="steps", layout_b=None,
                         splits=0, names=None, device=0, eng=None):
    """PosteriorComparison of the sample sets xa and xb (each as information_gain takes x; layout_b defaults to layout).  Four
    gpb_chain_knn calls — within A, A to B, within B, B to A, in coordinates divided by hi - lo — give D(A || B) and D(B || A)
    for every k = 1 .. k; two gpb_chain_marginals calls on shared edges (`bins` bins over [lo, hi]) give the histograms.
    weights_a, weights_b enter the histograms and the percentiles as in marginals.marginals; the nearest-neighbour part raises
    ValueError for them (k=0: histograms only)."""
    from .diagnostics import _engine
    from .marginals import marginals
    a3, layout = _device_chain(xa, layout, device, "xa")
    b3, layout_b = _device_chain(xb, layout_b or layout, a3.device.index or 0, "xb")
    d = int(a3.shape[2])
    if int(b3.shape[2]) != d:
        raise ValueError("xb: %d parameters, xa has %d" % (int(b3.shape[2]), d))
    nA, nB = int(a3.shape[0]) * int(a3.shape[1]), int(b3.shape[0]) * int(b3.shape[1])
    if nA < 1 or nB < 1:
        raise ValueError("xa, xb: no samples")
    lo, hi = _box(lo, hi, d)
    k = int(k)
    if k:
        _no_weights(weights_a, "posterior_divergence")
        _no_weights(weights_b, "posterior_divergence")
    eng = eng or _engine(a3.device.index or 0)
    band = (0.16, 0.5, 0.84)
    rng = np.stack([lo, hi], axis=1)
    ma = marginals(a3[:, 0, :] if weights_a is not None else a3, bins=int(bins), range=rng, pairs=pairs, weights=weights_a,
                   quantiles=band, layout=layout, eng=eng)
    mb = marginals(b3[:, 0, :] if weights_b is not None else b3, bins=int(bins), range=rng, pairs=pairs, weights=weights_b,
                   quantiles=band, layout=layout_b, eng=eng)
    js1 = hist_js(ma.hist1d, mb.hist1d)
    npairs = ma.hist2d.shape[0]
    js2 = hist_js(ma.hist2d.reshape(npairs, -1), mb.hist2d.reshape(npairs, -1)) if npairs else np.zeros(0)
    sa, sb = 0.5 * (ma.percentiles[2] - ma.percentiles[0]), 0.5 * (mb.percentiles[2] - mb.percentiles[0])
    with np.errstate(all="ignore"):
        shift = (ma.percentiles[1] - mb.percentiles[1]) / np.sqrt(sa * sa + sb * sb)
    if not k:
        e = np.zeros(0)
        return PosteriorComparison(e, e, js1, js2, ma.pairs, shift, 0.0, 0.0, nA, nB, (0, 0), bins, names)
    inv = 1.0 / (hi - lo)
    kw = dict(k=k, inv_scale=inv, skip_zero=True, splits=splits, return_index=False)
    aa, ab = eng.chain_knn(a3, layout, **kw), eng.chain_knn(a3, layout, b3, layout_b, **kw)
    bb, ba = eng.chain_knn(b3, layout_b, **kw), eng.chain_knn(b3, layout_b, a3, layout, **kw)
    sk_a, sk_b = aa["n_skipped"][0], bb["n_skipped"][0]
    kl_ab = wkv_divergence(aa["r2"], ab["r2"], d, nB - sk_b, _keep(aa, nA))
    kl_ba = wkv_divergence(bb["r2"], ba["r2"], d, nA - sk_a, _keep(bb, nB))
    res = PosteriorComparison(kl_ab, kl_ba, js1, js2, ma.pairs, shift, np.mean(aa["zeros"] > 0), np.mean(bb["zeros"] > 0), nA, nB,
                              (sk_a, sk_b), bins, names)
    _warn_duplicates(max(res.duplicate_fraction_a, res.duplicate_fraction_b), "posterior_divergence")
    return res


def load_chain(path):
    """the `chain` of a chain pickle (run_mcmc's [nwalkers, nsteps, ndim], a pocoMC / run_SMC particle set [S, ndim])"""
    with open(path, "rb") as f:
        return np.asarray(pickle.load(f)["chain"], dtype=np.float64)
