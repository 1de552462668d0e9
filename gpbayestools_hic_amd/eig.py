"""
Which data set, measured to which precision, is expected to constrain the parameters most?  The package can say what the data
taught after the fact (Chain.information_gain: the realised Kullback-Leibler divergence; Chain.sensitivity: a local Fisher matrix;
goodness_of_fit(...).influence: the posterior without a data set).  The question asked BEFORE the next measurement is the expected
information gain of a measurement y about the parameters theta, the mutual information

    EIG = E_{theta, y | theta} [ ln p(y | theta) - ln p(y) ],        p(y) = E_{theta'} p(y | theta')

which is non-local, unlike Fisher, and defined for the prior as well as for a current posterior.  It is estimated by nested Monte
Carlo over the samples already held: simulated measurements y_i = mu(theta_{o_i}) + noise for S_out draws o_i from the sample
set, and the diagonal Gaussian log-likelihood of every y_i under every one of the S_in samples — S_out S_in M terms and a
log-sum-exp per row, on the device (gpb_eig_simulate, gpb_eig_lse), for every group of observables at once
(every emulator of a chain alone, then all together).  Two estimates bracket the value in expectation:

    lower   the prior-contrastive bound (InfoNCE): the simulating sample stays in the inner sum.  Biased LOW, and it cannot
            exceed ln S_in: it SATURATES there — a warning says so when lower > ln(S_in) - 1, and only more samples help.
    upper   the leave-one-out nested Monte Carlo estimate: the simulating sample is taken out of the inner sum.  Biased HIGH.

What the number is NOT.  The likelihood is the DIAGONAL one: variances var + planned_var per observable; the PCA truncation term
of the emulators and an expdata_cov that couples observables are ignored.  It is the EIG under the emulator's own model of its
error: the predictive variance counts as noise of the measurement.  stderr is the standard error of the outer mean only.
"""
import logging
import math

import numpy as np

log = logging.getLogger(__name__)
CHUNK = 256


def tree_sum(x):
    """sum over the first axis by the project's fixed tree: chunks of 256 rows, each halved eight times (row r + row r + h), the
    chunk sums added in order.  The shape of the tree depends on nothing but the number of rows."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    nch = max((n + CHUNK - 1) // CHUNK, 1)
    pad = np.zeros((nch * CHUNK,) + x.shape[1:])
    pad[:n] = x
    c = pad.reshape((nch, CHUNK) + x.shape[1:])
    h = CHUNK // 2
    while h >= 1:
        c = c[:, :h] + c[:, h:2 * h]
        h //= 2
    out = c[0, 0].copy() if c.ndim > 2 else np.float64(c[0, 0])
    for k in range(1, nch):
        out = out + c[k, 0]
    return out


def estimates(lse_excl, self_ll, w, outer_idx):
    """The two estimates per outer row from the library's outputs [G, S_out], the inner weights w [S_in] and the outer indices:
    with ll = self - ln w_o, the simulating sample's own log-likelihood (self carries ln w_o so that logaddexp(lse_excl, self) is
    the whole weighted sum), L = ll - [logaddexp(lse_excl, self) - ln W] (every row <= ln(W / w_o)) and U = ll - [lse_excl -
    ln(W - w_o)], W = sum w.  A sample of integer weight k counts as k identical rows, all of which leave the sum with it.
    Returns (L, U, lower, upper, stderr): [G, S_out] twice, then the means over the rows (tree_sum) and the standard error of
    the outer mean, the larger of the two estimates' (a single inner sample leaves U undefined: that of L)."""
    lse_excl, self_ll = np.asarray(lse_excl, dtype=np.float64), np.asarray(self_ll, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    W = tree_sum(w)
    wo = w[np.asarray(outer_idx)]
    with np.errstate(divide="ignore", invalid="ignore"):
        num = self_ll - np.log(wo)[None, :]                        # ln p(y_i | theta_o): self carries ln w_o for the sum below
        L = num - (np.logaddexp(lse_excl, self_ll) - math.log(W))
        U = num - (lse_excl - np.log(W - wo)[None, :])
    n = L.shape[1]
    lower, upper = tree_sum(L.T) / n, tree_sum(U.T) / n
    lower, upper = np.atleast_1d(lower), np.atleast_1d(upper)

    def se(R, mean):
        with np.errstate(invalid="ignore"):
            return np.sqrt(np.atleast_1d(tree_sum(((R - mean[:, None]) ** 2).T)) / max(n - 1, 1) / n)
    se_l, se_u = se(L, lower), se(U, upper)
    return L, U, lower, upper, np.where(np.isfinite(se_u), np.maximum(se_l, se_u), se_l)


class EIGResult:
    """Expected information gain per group of observables, nats.  names [G]; lower, upper, stderr [G]; n_inner (distinct inner
    samples), n_outer, ln_n_inner (where `lower` saturates); per_row = (L, U), [G, n_outer] each; ranges [G, 2] (observables);
    weights [n_inner] and outer_idx [n_outer] as used."""

    def __init__(self, names, ranges, lower, upper, stderr, n_inner, n_outer, per_row, weights, outer_idx):
        self.names, self.ranges = list(names), np.asarray(ranges)
        self.lower, self.upper, self.stderr = lower, upper, stderr
        self.n_inner, self.n_outer, self.ln_n_inner = int(n_inner), int(n_outer), math.log(n_inner)
        self.per_row, self.weights, self.outer_idx = per_row, weights, outer_idx

    @property
    def saturated(self):
        """[G] bool: lower > ln(n_inner) - 1 — the bound is near its ceiling and says little; use more samples"""
        return self.lower > self.ln_n_inner - 1.0

    def table(self):
        """one line per group: observables, lower, upper, stderr; '*' marks a saturated lower bound"""
        wn = max([len(str(n)) for n in self.names] + [5])
        lines = ["%-*s %9s %10s %10s %10s" % (wn, "group", "nobs", "lower", "upper", "stderr")]
        for g, name in enumerate(self.names):
            lines.append("%-*s %9d %10.4f %10.4f %10.4f%s" % (wn, name, self.ranges[g, 1] - self.ranges[g, 0], self.lower[g],
                                                              self.upper[g], self.stderr[g], " *" if self.saturated[g] else ""))
        lines.append("ln(n_inner) = %.4f (n_inner %d, n_outer %d); * lower bound saturated" % (self.ln_n_inner, self.n_inner,
                                                                                             self.n_outer))
        return "\n".join(lines)

    def __repr__(self):
        return "EIGResult(%s)" % ", ".join("%s: %.3f..%.3f" % (n, lo, up) for n, lo, up in zip(self.names, self.lower, self.upper))


def _groups(groups, M):
    """(names, ranges [G, 2]) from None (the whole range), a dict name -> (c0, c1) or a list of (c0, c1) / (name, c0, c1)"""
    if groups is None:
        return ["all"], np.array([[0, M]], dtype=np.int32)
    items = list(groups.items()) if isinstance(groups, dict) else list(groups)
    names, rg = [], []
    for k, it in enumerate(items):
        if isinstance(groups, dict):
            name, (c0, c1) = it
        elif len(it) == 3:
            name, c0, c1 = it
        else:
            name, (c0, c1) = "group%d" % k, it
        names.append(str(name))
        rg.append((int(c0), int(c1)))
    rg = np.asarray(rg, dtype=np.int32).reshape(-1, 2)
    if not 1 <= rg.shape[0] <= 64:
        raise ValueError("expected_information_gain: 1 to 64 groups")
    if np.any(rg[:, 0] < 0) or np.any(rg[:, 1] > M) or np.any(rg[:, 0] >= rg[:, 1]):
        raise ValueError("expected_information_gain: every group a non-empty range inside [0, %d)" % M)
    return names, rg


def _eig_device(eng, mu_T, var_T, vadd, w, names, ranges, n_outer, seed, splits=0):
    """the device part: mu_T, var_T [M, S] cuda tensors, vadd [M] and w [S] numpy, all checked"""
    S = int(mu_T.shape[1])
    n_outer = int(n_outer)
    if n_outer < 1:
        raise ValueError("expected_information_gain: n_outer >= 1")
    rng = np.random.default_rng(seed)
    oidx = rng.choice(S, n_outer, p=w / w.sum()).astype(np.int32)
    sim_seed = int(rng.integers(0, 2 ** 63))
    y_T = eng.eig_simulate(mu_T, var_T, vadd, oidx, sim_seed)
    lse, slf = eng.eig_lse(mu_T, var_T, vadd, np.log(w), y_T, oidx, ranges, splits=splits)
    L, U, lower, upper, stderr = estimates(lse, slf, w, oidx)
    res = EIGResult(names, ranges, lower, upper, stderr, S, n_outer, (L, U), w, oidx)
    if np.any(res.saturated):
        log.warning("expected_information_gain: the lower bound of %s is within 1 nat of ln(n_inner) = %.2f, where it saturates: "
                    "use more samples", [n for n, s in zip(names, res.saturated) if s], res.ln_n_inner)
    return res


def expected_information_gain(mean, var, planned_var, groups=None, weights=None, n_outer=8192, seed=None, device=0, eng=None,
                              splits=0):
    """EIGResult of planned measurements from plain arrays: mean, var [S, M] the model's prediction and its own variance at S
    samples of the parameters (var None: zeros), planned_var [M] the planned experimental variance; var + planned_var must be
    positive.  groups: None (all observables), a dict name -> (c0, c1) or a list of (c0, c1): contiguous observable ranges, at
    most 64.  weights [S] > 0: the counts of repeated rows of an MCMC chain or importance weights.  The n_outer simulating
    samples are drawn with np.random.default_rng(seed).choice(S, n_outer, p=w / sum w), with replacement; the noise is keyed by
    the same generator's next integer.  ValueError for wrong shapes, non-finite inputs, non-positive variances or weights and
    fewer than 2 samples."""
    import torch
    mean = np.asarray(mean, dtype=np.float64)
    if mean.ndim != 2 or mean.shape[0] < 2 or not 1 <= mean.shape[1] <= 4096:
        raise ValueError("expected_information_gain: mean must be [S >= 2, 1 <= M <= 4096], got %s" % (mean.shape,))
    S, M = mean.shape
    pv = np.array(np.broadcast_to(np.asarray(planned_var, dtype=np.float64), (M,)))                 # (a writable copy)
    if var is not None:
        var = np.asarray(var, dtype=np.float64)
        if var.shape != (S, M):
            raise ValueError("expected_information_gain: var must be [%d, %d]" % (S, M))
    w = np.ones(S) if weights is None else np.ascontiguousarray(np.asarray(weights, dtype=np.float64).reshape(-1))
    if w.shape[0] != S or not np.all(np.isfinite(w)) or not np.all(w > 0.0):
        raise ValueError("expected_information_gain: weights [%d], finite and positive" % S)
    s = pv[None, :] + (0.0 if var is None else var)
    if not (np.all(np.isfinite(mean)) and np.all(np.isfinite(s)) and np.all(s > 0.0)):
        raise ValueError("expected_information_gain: means and variances must be finite, var + planned_var positive")
    names, ranges = _groups(groups, M)
    if eng is None:
        from .diagnostics import _engine
        eng = _engine(device)
    dev = torch.device("cuda", eng.device)
    mu_T = torch.as_tensor(np.ascontiguousarray(mean.T), device=dev)
    var_T = None if var is None else torch.as_tensor(np.ascontiguousarray(var.T), device=dev)
    return _eig_device(eng, mu_T, var_T, pv, w, names, ranges, n_outer, seed, splits)


def chain_expected_information_gain(chain, samples=None, discard=0, thin=1, weights=None, planned_error=None, groups=None,
                                    n_outer=8192, seed=None, splits=0):
    """Chain.expected_information_gain (mcmc.py carries the documentation)"""
    import pickle
    import torch
    if not chain._native():
        raise NotImplementedError("expected_information_gain needs every emulator of the chain to be this package's Emulator "
                                  "(foreign emulators expose no GP state to predict from on the device)")
    if chain.sharding is not None and getattr(chain.sharding, "world", 1) > 1:
        raise NotImplementedError("expected_information_gain: a chain sharded over several ranks is not supported; call it on one "
                                  "rank (shard_over(None))")
    if samples is None:
        if chain.chain is False:
            with open(chain.mcmc_path, "rb") as f:
                chain.chain = pickle.load(f)["chain"]
        samples = chain.chain
    x = np.asarray(samples.cpu() if hasattr(samples, "data_ptr") else samples, dtype=np.float64)
    if x.ndim == 3:
        if weights is not None:
            raise ValueError("expected_information_gain: weights go with a flat [S, ndim] sample set")
        discard, thin = int(discard), int(thin)
        if discard < 0 or thin < 1 or x.shape[1] - discard < 1:
            raise ValueError("expected_information_gain: discard >= 0, thin >= 1 and at least one step must remain")
        x = x[:, discard::thin].reshape(-1, x.shape[-1])
    if x.ndim != 2 or x.shape[1] != chain.ndim:
        raise ValueError("expected_information_gain: samples must be [S, %d] or [nwalkers, nsteps, %d], got %s"
                         % (chain.ndim, chain.ndim, np.shape(samples)))
    if not np.all(np.isfinite(x)):
        raise ValueError("expected_information_gain: samples hold non-finite values")
    w = np.ones(x.shape[0]) if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1)
    if w.shape[0] != x.shape[0] or not np.all(np.isfinite(w)) or np.any(w < 0.0) or not np.any(w > 0.0):
        raise ValueError("expected_information_gain: weights [%d], finite, not negative, not all zero" % x.shape[0])
    x, w = x[w > 0.0], w[w > 0.0]
    # identical rows (an MCMC chain repeats a row after every rejected move) become ONE inner sample with their summed weight:
    # left apart, a row's twin would stay in the sum that leaves the row out
    ux, inv = np.unique(x, axis=0, return_inverse=True)
    uw = np.bincount(np.asarray(inv).reshape(-1), weights=w, minlength=ux.shape[0])
    if ux.shape[0] < 2:
        raise ValueError("expected_information_gain: fewer than 2 distinct samples")
    nobs = chain.nobs
    if planned_error is None:
        pv = np.diag(np.asarray(chain.expdata_cov, dtype=np.float64)).copy()
    else:
        pe = np.asarray(planned_error, dtype=np.float64).reshape(-1)
        if pe.shape[0] != nobs:
            raise ValueError("expected_information_gain: planned_error must be [%d]" % nobs)
        pv = pe * pe
    if not np.all(np.isfinite(pv)) or np.any(pv < 0.0):
        raise ValueError("expected_information_gain: the planned errors must be finite")
    if groups is None:
        names, rg, r0 = [], [], 0
        for k, emu in enumerate(chain.emuList):
            names.append("emulator%d" % k)
            rg.append((r0, r0 + emu.nobs))
            r0 += emu.nobs
        names.append("all")
        rg.append((0, nobs))
        groups = list(zip(names, [r[0] for r in rg], [r[1] for r in rg]))
    names, ranges = _groups(groups, nobs)
    engs, mu_T, var_T = chain._ppd_arrays(np.ascontiguousarray(ux))
    s_min = float((var_T + torch.as_tensor(pv, device=var_T.device)[:, None]).min())
    if not (bool(torch.isfinite(mu_T).all()) and bool(torch.isfinite(var_T).all()) and s_min > 0.0):
        raise ValueError("expected_information_gain: the predictions are not finite, or a variance plus its planned variance is "
                         "not positive")
    return _eig_device(engs[0], mu_T, var_T, pv, uw, names, ranges, n_outer, seed, splits)
