"""float64 numpy model of the expected-information-gain kernels (csrc/gpb_eig.hip: gpb_eig_simulate, gpb_eig_lse) and of the rule
in include/gpbayes.h.  Arrays are sample-major here: mu, s [S_in, M] (s = var + vadd, the variances of the likelihood), y
[S_out, M], logw [S_in], oidx [S_out] (the inner sample every outer row was simulated from), ranges [G, 2].

  direct      l_ij(g) = logw_j - sum_{m in g} [(y_im - mu_jm)^2 / s_jm + ln s_jm] / 2 term by term, scipy's logsumexp over j != o_i
  gemm_form   the same through the centred operands the device multiplies: l_ij = sum_m (q_im t_jm + l_im u_jm) + b_gj
  lse_bound   the tolerance of the GPU tier, from the operands: the forward error of a 2 M_g-term dot product plus a few ulps
  device_z    the draws of gpb_eig_simulate restated through oracle.stretch_oracle's Philox
The estimates built from (lse_excl, self) are the package's own host code (gpbayestools_hic_amd.eig.estimates): numpy only."""
import numpy as np
from scipy.special import logsumexp

from oracle.stretch_oracle import philox4x32_10, u01

EPS = 2.0 ** -52
TAG_EIG = 15
ROWS = 64                  # outer rows per block of the [rows, S_in, M_g] work arrays


def _key(seed):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return (seed & 0xFFFFFFFF, seed >> 32)


def device_z(seed, S_out, M):
    """z [S_out, M] as gpb_eig_simulate draws it: normal_pair of the counter (i, p, 0, 15) for the observables 2p, 2p + 1"""
    npair = (M + 1) // 2
    c = np.repeat(np.arange(S_out, dtype=np.uint64), npair)
    k = np.tile(np.arange(npair, dtype=np.uint64), S_out)
    x, y, z, w = philox4x32_10(_key(seed), (c, k, 0, TAG_EIG))
    u1, u2 = u01(x, y), u01(z, w)
    rad = np.sqrt(-2.0 * np.log(1.0 - u1))
    a = (2.0 * np.pi) * u2
    return np.ascontiguousarray(np.stack([rad * np.cos(a), rad * np.sin(a)], axis=1).reshape(S_out, 2 * npair)[:, :M])


def simulate(mu, s, oidx, z):
    """y = mu_o + sqrt(s_o) z, two roundings"""
    return mu[oidx] + np.sqrt(s[oidx]) * z


def _logw(logw, S_in):
    return np.zeros(S_in) if logw is None else np.asarray(logw, dtype=np.float64)


def direct(mu, s, logw, y, oidx, ranges):
    """(lse_excl, self) [G, S_out] term by term"""
    S_in, S_out = mu.shape[0], y.shape[0]
    lw = _logw(logw, S_in)
    ranges = np.asarray(ranges).reshape(-1, 2)
    lse, slf = np.empty((len(ranges), S_out)), np.empty((len(ranges), S_out))
    lns = np.log(s)
    for g, (c0, c1) in enumerate(ranges):
        for i0 in range(0, S_out, ROWS):
            i1 = min(i0 + ROWS, S_out)
            d = y[i0:i1, None, c0:c1] - mu[None, :, c0:c1]
            ell = lw[None, :] - 0.5 * np.sum(d * d / s[None, :, c0:c1] + lns[None, :, c0:c1], axis=2)
            rows = np.arange(i1 - i0)
            slf[g, i0:i1] = ell[rows, oidx[i0:i1]]
            ell[rows, oidx[i0:i1]] = -np.inf
            with np.errstate(divide="ignore"):
                lse[g, i0:i1] = logsumexp(ell, axis=1) if S_in > 1 else -np.inf
    return lse, slf


def operands(mu, s, y):
    """the centred operands: c [M], t, u [S_in, M], q, l [S_out, M]"""
    c = mu.mean(axis=0)
    t = 1.0 / s
    return c, t, (mu - c) * t, -0.5 * (y - c) ** 2, y - c


def bias(mu, s, logw, c, t, ranges):
    """b [G, S_in]"""
    lw = _logw(logw, mu.shape[0])
    term = (mu - c) ** 2 * t + np.log(s)
    return np.stack([lw - 0.5 * term[:, c0:c1].sum(axis=1) for c0, c1 in np.asarray(ranges).reshape(-1, 2)])


def gemm_form(mu, s, logw, y, oidx, ranges):
    """lse_excl [G, S_out] through the operand form, and mag [G, S_out] = max_j (sum_k |a_ik b_jk| + |b_gj|) for lse_bound"""
    S_in, S_out = mu.shape[0], y.shape[0]
    c, t, u, q, l = operands(mu, s, y)
    ranges = np.asarray(ranges).reshape(-1, 2)
    b = bias(mu, s, logw, c, t, ranges)
    lse, mag = np.empty((len(ranges), S_out)), np.empty((len(ranges), S_out))
    rows = np.arange(S_out)
    for g, (c0, c1) in enumerate(ranges):
        ell = q[:, c0:c1] @ t[:, c0:c1].T + l[:, c0:c1] @ u[:, c0:c1].T + b[g][None, :]
        mag[g] = np.max(np.abs(q[:, c0:c1]) @ np.abs(t[:, c0:c1]).T + np.abs(l[:, c0:c1]) @ np.abs(u[:, c0:c1]).T
                        + np.abs(b[g])[None, :], axis=1)
        ell[rows, oidx] = -np.inf
        with np.errstate(divide="ignore"):
            lse[g] = logsumexp(ell, axis=1) if S_in > 1 else -np.inf
    return lse, mag


def lse_bound(mag, model, ranges):
    """(2 M_g + 64) 2^-52 (mag + |model| + 1) [G, S_out]; inf where the model is -inf (compare those entries for equality)"""
    ranges = np.asarray(ranges).reshape(-1, 2)
    Mg = (ranges[:, 1] - ranges[:, 0]).astype(np.float64)
    return (2.0 * Mg + 64.0)[:, None] * EPS * (mag + np.abs(model) + 1.0)


def self_bound(mu, s, logw, y, oidx, ranges):
    """(M_g + 8) 2^-52 (sum |terms| + 1) [G, S_out], the terms of self: ln w, (y - mu)^2 / (2 s), ln(s) / 2 of every observable"""
    lw = _logw(logw, mu.shape[0])
    d = y - mu[oidx]
    term = 0.5 * d * d / s[oidx] + 0.5 * np.abs(np.log(s[oidx]))
    ranges = np.asarray(ranges).reshape(-1, 2)
    tot = np.stack([np.abs(lw[oidx]) + term[:, c0:c1].sum(axis=1) for c0, c1 in ranges])
    return ((ranges[:, 1] - ranges[:, 0]) + 8.0)[:, None] * EPS * (tot + 1.0)


def linear_gaussian(S_in, S_out, seed):
    """theta ~ N(0, I_4), mu = theta A with 6 observables and fixed variances: the exact EIG is ln det(I + A diag(1 / s) A^T) / 2.
    Returns (mu, s, y, oidx, exact)."""
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(4, 6))
    svec = rng.uniform(0.5, 2.0, size=6)
    theta = rng.normal(size=(S_in, 4))
    mu = theta @ A
    s = np.broadcast_to(svec, mu.shape).copy()
    oidx = rng.choice(S_in, S_out).astype(np.int32)
    y = simulate(mu, s, oidx, rng.normal(size=(S_out, 6)))
    exact = 0.5 * np.linalg.slogdet(np.eye(4) + (A / svec) @ A.T)[1]
    return mu, s, y, oidx, exact
