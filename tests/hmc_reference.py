"""float64 numpy restatement of one step of the HMC loop of csrc/gpb_hmc.hip and of the dual-averaging update, operation for
operation in the order of csrc/hmc_step.h (sums over the parameters in index order, no fused multiply-adds), with every random
number an input, plus an independent restatement of the device's Philox draws (oracle.stretch_oracle).

A step's draws are a dict: p0 [C, d] (the initial momenta, z * msqrt), logu [C] (the accept test's ln u) and eps (the step's
step size).  device_draws regenerates them from (seed, k); a test on the device feeds the step the device's own
(HMCSampler.step_with_diagnostics), so that the transcendental functions of the two sides do not enter the comparison."""
import numpy as np

from oracle.stretch_oracle import philox4x32_10, u01

TAG_MOM, TAG_EPS, TAG_ACC = 12, 13, 14
MAX_REFLECT = 8
DA_GAMMA, DA_T0, DA_KAPPA = 0.05, 10.0, 0.75
DIVERGENT = 1000.0
A_SCALE = 4294967296.0


def _key(seed):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return (seed & 0xFFFFFFFF, seed >> 32)


def device_draws(seed, k, C, d, chains=None):
    """what gpb_chain_hmc_run draws at global step k for the chains numbered `chains` (default 0 .. C - 1): z [C, d] (N(0, 1)),
    u_eps (the jitter's uniform) and logu [C]"""
    chains = np.arange(C, dtype=np.uint64) if chains is None else np.asarray(chains, dtype=np.uint64)
    npair = (d + 1) // 2
    c = np.repeat(chains, npair)
    j = np.tile(np.arange(npair, dtype=np.uint64), len(chains))
    x, y, z, w = philox4x32_10(_key(seed), (c, k, j, TAG_MOM))
    u1, u2 = u01(x, y), u01(z, w)
    rad = np.sqrt(-2.0 * np.log(1.0 - u1))
    a = (2.0 * np.pi) * u2
    normals = np.stack([rad * np.cos(a), rad * np.sin(a)], axis=1).reshape(len(chains), 2 * npair)[:, :d]
    x, y, _, _ = philox4x32_10(_key(seed), (0, k, 0, TAG_EPS))
    u_eps = float(u01(x, y))
    x, y, _, _ = philox4x32_10(_key(seed), (chains, k, 0, TAG_ACC))
    with np.errstate(divide="ignore"):
        logu = np.log(u01(x, y))
    return dict(z=np.ascontiguousarray(normals), u_eps=u_eps, logu=logu)


# ------------------------------------------------------------------ csrc/hmc_step.h
def kick(p, h, g):
    with np.errstate(invalid="ignore"):
        return p + h * g


def drift(x, p, eps, minv, lo, hi):
    """-> (x, p, reflections per coordinate, escaped per coordinate); NaN coordinates compare false and are left alone"""
    with np.errstate(invalid="ignore"):
        x = x + eps * (minv * p)
        p = np.array(p, dtype=np.float64)
        n = np.zeros(np.shape(x), dtype=np.int64)
        for _ in range(MAX_REFLECT):
            below = x < lo
            above = ~below & (x > hi)
            x = np.where(below, lo + (lo - x), np.where(above, hi - (x - hi), x))
            p = np.where(below | above, -p, p)
            n = n + (below | above)
        return x, p, n, (x < lo) | (x > hi)


def kinetic(p, minv):
    p = np.atleast_2d(p)
    s = np.zeros(p.shape[0])
    for j in range(p.shape[1]):
        s = s + (p[:, j] * p[:, j]) * minv[j]
    return 0.5 * s


def step_size(ln_eps, jitter, u):
    return np.exp(ln_eps) * (1.0 + jitter * (2.0 * u - 1.0))


def accept_prob(dH):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.where(np.isnan(dH), 0.0, np.minimum(np.exp(-dH), 1.0))


def a_mean(a):
    """the mean accept probability as the device forms it: an integer sum of the a_c in units of 2^-32"""
    total = int(np.sum((np.asarray(a) * A_SCALE).astype(np.uint64), dtype=np.uint64))
    return (float(total) / A_SCALE) / float(len(a))


def dual_average(st, a_mean_, delta):
    """Hoffman & Gelman (2014), algorithm 5, on st = [ln eps, ln eps-bar, H-bar, mu, count] -> the new five"""
    t = st[4] + 1.0
    w = 1.0 / (t + DA_T0)
    hbar = (1.0 - w) * st[2] + w * (delta - a_mean_)
    le = st[3] - (np.sqrt(t) / DA_GAMMA) * hbar
    eta = t ** (-DA_KAPPA)
    return np.array([le, eta * le + (1.0 - eta) * st[1], hbar, st[3], t])


def start_state(eps):
    return np.array([np.log(eps), 0.0, 0.0, np.log(10.0 * eps), 0.0])


# ------------------------------------------------------------------ one step
def trajectory(x, p, g, eps, minv, lo, hi, L, logpost_grad):
    """L leapfrog steps from (x, p) with the gradient g at x -> (x, p, lp, grad at the end, escaped [C], the drifts of a chain
    that reflected at a wall, the positions after each drift [L, C, d], the most reflections of one coordinate in one drift [C])"""
    h = eps / 2.0
    escaped = np.zeros(x.shape[0], dtype=bool)
    nrefl, traj, lp, most = 0, [], None, np.zeros(x.shape[0], dtype=np.int64)
    for l in range(L):
        p = kick(p, h, g)
        x, p, n, esc = drift(x, p, eps, minv, lo, hi)
        escaped |= np.any(esc, axis=1)
        nrefl += int(np.sum(np.any(n > 0, axis=1)))
        most = np.maximum(most, np.max(n, axis=1))
        traj.append(x)
        lp, g = logpost_grad(x, l)
        p = kick(p, h, g)
    return x, p, lp, g, escaped, nrefl, np.array(traj), most


def step(state, draws, logpost_grad, minv, lo, hi, L):
    """one step from state = dict(x [C, d], lp [C], grad [C, d]); draws = dict(p0, logu, eps); logpost_grad(X, l) -> (lp, grad)
    at the positions X after the l-th drift (l lets a test evaluate at the device's own points).  Returns the new state and a
    dict of what happened."""
    x0, lp0, g0 = state["x"], state["lp"], state["grad"]
    p0 = np.array(draws["p0"], dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        H0 = -lp0 + kinetic(p0, minv)
        x, p, lp, g, escaped, nrefl, traj, most = trajectory(x0, p0, g0, draws["eps"], minv, lo, hi, L, logpost_grad)
        H1 = -lp + kinetic(p, minv)
        dH = H1 - H0
        take = (draws["logu"] < -dH) & ~escaped
        a = np.where(escaped, 0.0, accept_prob(dH))
        divergent = (dH > DIVERGENT) | np.isnan(dH)
    new = dict(x=np.where(take[:, None], x, x0), lp=np.where(take, lp, lp0), grad=np.where(take[:, None], g, g0))
    return new, dict(H0=H0, H1=H1, dH=dH, a=a, accepted=take, escaped=escaped, divergent=divergent, nan_rows=np.isnan(lp),
                     traj=traj, reflected_drifts=nrefl, most_reflections=most, p=p, x=x)


# ------------------------------------------------------------------ analytic targets and a host loop over them
def boxed_gaussian(mean, sigma, lo, hi):
    """(X, l) -> (lp, grad) of a product of Gaussians truncated by the open box: -inf and a zero gradient outside it, as
    gpb_chain_logpost_grad reports rows outside"""
    mean, sigma = np.asarray(mean, dtype=np.float64), np.asarray(sigma, dtype=np.float64)

    def f(X, l=0):
        with np.errstate(invalid="ignore"):
            inside = np.all((X > lo) & (X < hi), axis=1)
        z = (X - mean) / sigma
        lp = np.where(inside, -0.5 * np.sum(z * z, axis=1), -np.inf)
        return lp, np.where(inside[:, None], -z / sigma, 0.0)
    return f


def run(target, X0, nsteps, L, minv, lo, hi, rng, ln_state, jitter=0.2, adapt=False, delta=0.8, keep=False):
    """nsteps steps of all chains with numpy's generator for the draws -> (state, ln_state, per-step mean accept probability,
    stored x [nsteps, C, d] if keep, the drifts (of one chain, one leapfrog) that reflected, drifts in all, escaped trajectories)"""
    lp, g = target(X0)
    state = dict(x=np.array(X0, dtype=np.float64), lp=lp, grad=g)
    msqrt = 1.0 / np.sqrt(minv)
    C, d = X0.shape
    acc, stored, nrefl, nesc = [], [], 0, 0
    for _ in range(nsteps):
        draws = dict(p0=rng.standard_normal((C, d)) * msqrt, logu=np.log(rng.uniform(size=C)),
                     eps=step_size(ln_state[0], jitter, rng.uniform()))
        state, info = step(state, draws, target, minv, lo, hi, L)
        acc.append(a_mean(info["a"]))
        nrefl += info["reflected_drifts"]
        nesc += int(np.sum(info["escaped"]))
        if adapt:
            ln_state = dual_average(ln_state, acc[-1], delta)
        if keep:
            stored.append(state["x"])
    return state, ln_state, np.array(acc), (np.array(stored) if keep else None), nrefl, nsteps * L * C, nesc
