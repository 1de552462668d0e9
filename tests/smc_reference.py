"""float64 numpy restatement of the tempered SMC sampler of csrc/gpb_smc.hip (Chain.run_SMC): reweighting with the bisection
for the next beta, systematic resampling, the preconditioner, one move step and the driver, with every random number an
input, plus an independent restatement of the device's Philox draws (oracle.stretch_oracle), a model of the reweighting
kernel's chunked scan (device_scan) and the injected-weights recipe both test tiers use (injected_logl).

The likelihood is any callable X [n, d] -> logl [n] that returns OUTSIDE (or less) for rows outside the prior box.  Draws come
either from numpy (`NumpyDraws`) or from the device's counters (`PhiloxDraws`, what gpb_test_smc_draws reports)."""
import numpy as np

from oracle.stretch_oracle import philox4x32_10, u01

TAG_RESAMPLE, TAG_NORMAL, TAG_ACCEPT = 8, 9, 10
BISECT = 60
TARGET_ACC = 0.234
OUTSIDE = -1e300
POS_MAX = 1.0 - 2.0 ** -53
RW_THREADS = 1024                # threads of k_smc_reweight's one workgroup


def _key(seed):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return (seed & 0xFFFFFFFF, seed >> 32)


def device_draws(seed, stage, k, N, d):
    """what gpb_chain_smc_reweight draws at stage `stage` and gpb_chain_smc_move at global step k"""
    npair = (d + 1) // 2
    c = np.repeat(np.arange(N, dtype=np.uint64), npair)
    j = np.tile(np.arange(npair, dtype=np.uint64), N)
    x, y, z, w = philox4x32_10(_key(seed), (c, k, j, TAG_NORMAL))
    u1, u2 = u01(x, y), u01(z, w)
    rad = np.sqrt(-2.0 * np.log(1.0 - u1))
    a = (2.0 * np.pi) * u2
    normals = np.stack([rad * np.cos(a), rad * np.sin(a)], axis=1).reshape(N, 2 * npair)[:, :d]
    x, y, _, _ = philox4x32_10(_key(seed), (np.arange(N, dtype=np.uint64), k, 0, TAG_ACCEPT))
    with np.errstate(divide="ignore"):
        logu_accept = np.log(u01(x, y))
    x, y, _, _ = philox4x32_10(_key(seed), (stage, 0, 0, TAG_RESAMPLE))
    return dict(normals=np.ascontiguousarray(normals), logu_accept=logu_accept, u_resample=float(u01(x, y)))


class PhiloxDraws:
    def __init__(self, seed, N, d):
        self.seed, self.N, self.d = seed, N, d

    def resample(self, stage):
        return device_draws(self.seed, stage, 0, 2, 1)["u_resample"]

    def move(self, k):
        dr = device_draws(self.seed, 0, k, self.N, self.d)
        return dr["normals"], dr["logu_accept"]


class NumpyDraws:
    def __init__(self, rng, N, d):
        self.rng, self.N, self.d = rng, N, d

    def resample(self, stage):
        return float(self.rng.uniform())

    def move(self, k):
        return self.rng.standard_normal((self.N, self.d)), np.log(self.rng.uniform(size=self.N))


def weights(logl, db):
    """w = exp(db (logl - max logl)), 0 for NaN -> (w, max)"""
    mx = np.nanmax(logl)
    with np.errstate(invalid="ignore"):
        w = np.exp(db * (logl - mx))
    return np.where(np.isnan(logl), 0.0, w), mx


def ess(logl, db):
    w, _ = weights(logl, db)
    s1, s2 = np.sum(w), np.sum(w * w)
    return (s1 * s1) / s2


def reweight(logl, beta_prev, ess_fraction):
    """-> dict(beta, dlogz, w (unnormalised), ess, nan_weights)"""
    target = ess_fraction * len(logl)
    beta = 1.0
    if not ess(logl, 1.0 - beta_prev) >= target:
        lo, hi = beta_prev, 1.0
        for _ in range(BISECT):
            mid = 0.5 * (lo + hi)
            if ess(logl, mid - beta_prev) > target:
                lo = mid
            else:
                hi = mid
        beta = hi
    db = beta - beta_prev
    w, mx = weights(logl, db)
    s1 = np.sum(w)
    dlogz = (db * mx + np.log(s1)) - np.log(float(len(logl)))
    return dict(beta=beta, dlogz=dlogz, w=w, ess=(s1 * s1) / np.sum(w * w), nan_weights=int(np.sum(np.isnan(logl))))


def device_scan(w, threads=RW_THREADS):
    """the inclusive normalised scan as k_smc_reweight forms it: thread t of `threads` owns the contiguous chunk
    [t C, (t + 1) C) with C = ceil(N / threads) (the last owner's chunk may be short, the threads behind it own nothing) and
    sums it in index order; the chunks' bases are one sequential pass over the chunk totals; every entry is base + local sum,
    divided by the pass's own total"""
    N = len(w)
    C = -(-N // threads)
    padded = np.zeros(threads * C)
    padded[:N] = w                                             # (an entry nobody owns adds an exact zero)
    local = np.cumsum(padded.reshape(threads, C), axis=1)
    ends = np.cumsum(local[:, -1])
    base = np.concatenate(([0.0], ends[:-1]))
    return ((base[:, None] + local) / ends[-1]).reshape(-1)[:N]


def resample(w, u, scan=None):
    """systematic resampling -> (ancestors [N], cum [N] inclusive normalised, positions [N]); scan: the normalised scan
    of the weights (np.cumsum divided by its last entry when not given, device_scan for the kernel's)"""
    N = len(w)
    if scan is None:
        cum = np.cumsum(w)
        cum = cum / cum[-1]
    else:
        cum = scan(w)
    pos = np.minimum((u + np.arange(N, dtype=np.float64)) / float(N), POS_MAX)
    return np.searchsorted(cum, pos, side="right"), cum, pos


def knife_edges(anc, cum, pos, tol=1e-12):
    """the positions within tol of the scan entry that decides their ancestor (cum[anc] above, cum[anc - 1] below): there a
    scan that differs in its last bits may pick the neighbour"""
    N = len(cum)
    return np.minimum(np.abs(cum[np.minimum(anc, N - 1)] - pos),
                      np.abs(np.where(anc > 0, cum[np.maximum(anc - 1, 0)], -1.0) - pos)) < tol


INJECTED_SIZES = (1027, 2051, 4096, 16389)


def injected_logl(N, threads=RW_THREADS):
    """log-likelihoods with runs of zero weights and NaNs where the reweighting's chunked scan could trip:
    4 standard_normal - 30, then -inf at the front, -1e300 (exp underflows to 0) at the end, five NaNs across the boundary
    between chunks 4 and 5 (C = ceil(N / threads)), one NaN in the middle and two -inf at a third: six NaN weights"""
    C = -(-N // threads)
    logl = 4.0 * np.random.default_rng(N).standard_normal(N) - 30.0
    logl[0:3] = -np.inf
    logl[N - 2:] = -1e300
    logl[5 * C - 2:5 * C + 3] = np.nan
    logl[N // 2] = np.nan
    logl[N // 3:N // 3 + 2] = -np.inf
    return logl


def precondition(x):
    """-> (mean, covariance / N, lower Cholesky factor or None when a pivot is non-positive)"""
    N = x.shape[0]
    mean = x[0] + np.sum(x - x[0], axis=0) / float(N)
    D = x - mean
    cov = (D.T @ D) / float(N)
    try:
        if not np.all(np.diag(cov) > 0):
            raise np.linalg.LinAlgError
        Lc = np.linalg.cholesky(cov)
    except np.linalg.LinAlgError:
        Lc = None
    return mean, cov, Lc


def propose(x, log_sigma, Lc, normals):
    """x + exp(log_sigma) Lc z, each entry summed over j in index order"""
    s = np.zeros_like(x)
    for j in range(x.shape[1]):
        s = s + Lc[:, j][None, :] * normals[:, j:j + 1]
    return x + np.exp(log_sigma) * s


def move_step(x, logl, beta, log_sigma, Lc, s, normals, logu, loglike):
    """one Metropolis step, s its index within the stage -> (x, logl, log_sigma, info)"""
    xp = propose(x, log_sigma, Lc, normals)
    lp = loglike(xp)
    with np.errstate(invalid="ignore"):
        delta = beta * (lp - logl)
        take = ~np.isnan(lp) & (lp > OUTSIDE) & (logu < delta)
    x, logl = x.copy(), logl.copy()
    x[take] = xp[take]
    logl[take] = lp[take]
    log_sigma = log_sigma + (np.sum(take) / float(len(logl)) - TARGET_ACC) / (s + 1.0)
    return x, logl, log_sigma, dict(accepted=take, delta=delta, xp=xp, lp=lp, nan=int(np.sum(np.isnan(lp))))


def stage(state, draws, loglike, ess_fraction, nmcmc):
    """one stage (reweight, resample, precondition, nmcmc moves) from state = dict(x, logl, beta, logz, log_sigma, stage, k)"""
    rw = reweight(state["logl"], state["beta"], ess_fraction)
    anc, _, _ = resample(rw["w"], draws.resample(state["stage"]))
    x, logl = state["x"][anc], state["logl"][anc]
    _, _, Lc = precondition(x)
    if Lc is None:
        raise RuntimeError("the particle covariance is not positive definite")
    ls, k, nacc = state["log_sigma"], state["k"], 0
    for s in range(nmcmc):
        z, lu = draws.move(k)
        x, logl, ls, info = move_step(x, logl, rw["beta"], ls, Lc, s, z, lu, loglike)
        nacc += int(np.sum(info["accepted"]))
        k += 1
    return dict(x=x, logl=logl, beta=rw["beta"], logz=state["logz"] + rw["dlogz"], log_sigma=ls, stage=state["stage"] + 1,
                k=k), nacc / float(len(logl) * max(nmcmc, 1))


def run(loglike, lo, hi, n_particles, ess_fraction=0.5, nmcmc=20, max_stages=200, seed=0, draws="numpy"):
    """the driver of Chain.run_SMC: -> dict(x, logl, logz, beta (ladder), acceptance)"""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    d = len(lo)
    rng = np.random.default_rng(seed)
    x = rng.uniform(lo, hi, (n_particles, d))
    dr = NumpyDraws(rng, n_particles, d) if draws == "numpy" else PhiloxDraws(seed, n_particles, d)
    state = dict(x=x, logl=loglike(x), beta=0.0, logz=0.0, log_sigma=np.log(2.38 / np.sqrt(d)), stage=0, k=0)
    betas, rates = [], []
    while state["beta"] < 1.0:
        if state["stage"] >= max_stages:
            raise RuntimeError("beta = %g after %d stages" % (state["beta"], max_stages))
        state, rate = stage(state, dr, loglike, ess_fraction, nmcmc)
        betas.append(state["beta"])
        rates.append(rate)
    return dict(x=state["x"], logl=state["logl"], logz=state["logz"], beta=np.array(betas), acceptance=np.array(rates))


def gaussian_box_loglike(m, s, lo, hi):
    """a normalised isotropic Gaussian of width s centred at m, OUTSIDE for rows outside the open box"""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)

    def f(X):
        X = np.atleast_2d(X)
        ll = -0.5 * np.sum(((X - m) / s) ** 2, axis=1) - X.shape[1] * np.log(s * np.sqrt(2.0 * np.pi))
        ll[~np.all((X > lo) & (X < hi), axis=1)] = OUTSIDE
        return ll
    return f
