"""float64 numpy restatement of one step of the PTLMC loop (src/mcmc.py:623-670, tempexchange 679-692) in the order of
operations of csrc/gpb_ptlmc.hip (sums over the parameters in index order, no fused multiply-adds), with every random number
an input, plus an independent restatement of the device's Philox draws (oracle.stretch_oracle).

A step's draws are a dict: normals [T, d] (rvalo), logu_accept [T], picks [5T] (the exchange's rt, in the order the serial
lane takes them) and logu_swap [5T].  The reference's own draws fit the same slots: np.random.normal(0, 1, (T, d)), the log of
np.random.uniform(size=T), and for each of the five sweeps np.random.choice(range(1, T), T) with one log-uniform per pick."""
import numpy as np

from oracle.stretch_oracle import philox4x32_10, u01

TAG_NORMAL, TAG_ACCEPT, TAG_SWAP = 2, 3, 4
ITERS = 5
SQRT2 = np.sqrt(2)


def _key(seed):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return (seed & 0xFFFFFFFF, seed >> 32)


def device_draws(seed, k, T, d):
    """what gpb_chain_ptlmc_run draws at global step k (and gpb_test_ptlmc_draws reports)"""
    npair = (d + 1) // 2
    c = np.repeat(np.arange(T, dtype=np.uint64), npair)
    j = np.tile(np.arange(npair, dtype=np.uint64), T)
    x, y, z, w = philox4x32_10(_key(seed), (c, k, j, TAG_NORMAL))
    u1, u2 = u01(x, y), u01(z, w)
    rad = np.sqrt(-2.0 * np.log(1.0 - u1))
    a = (2.0 * np.pi) * u2
    normals = np.stack([rad * np.cos(a), rad * np.sin(a)], axis=1).reshape(T, 2 * npair)[:, :d]
    x, y, _, _ = philox4x32_10(_key(seed), (np.arange(T, dtype=np.uint64), k, 0, TAG_ACCEPT))
    with np.errstate(divide="ignore"):
        logu_accept = np.log(u01(x, y))
    i = np.arange(ITERS * T, dtype=np.uint64)
    x, y, z, _ = philox4x32_10(_key(seed), (i, k, 0, TAG_SWAP))
    picks = (1 + ((x.astype(np.uint64) * np.uint64(T - 1)) >> np.uint64(32))).astype(np.int64)
    with np.errstate(divide="ignore"):
        logu_swap = np.log(u01(y, z))
    return dict(normals=np.ascontiguousarray(normals), logu_accept=logu_accept, picks=picks, logu_swap=logu_swap)


def rho(tau):
    e = np.exp(2.0 * tau)
    return 2.0 * (1.0 + (e - 1.0) / (e + 1.0))


def _rowmat(A, B):
    """A [T, d] @ B [d, d], each entry summed over j in index order"""
    s = np.zeros((A.shape[0], B.shape[1]))
    for j in range(A.shape[1]):
        s = s + A[:, j:j + 1] * B[j][None, :]
    return s


def propose(theta, dfval, tau, temps13, hc, covmat0, normals):
    adj = rho(tau) * temps13
    x = theta + (SQRT2 * adj)[:, None] * _rowmat(normals, hc)
    if dfval is not None:
        x = x + (adj * adj)[:, None] * _rowmat(dfval, covmat0)
    return x


def accept(theta, fval, dfval, thetap, lp, grad, normals, tau, temps, temps13, hc, logu_accept):
    """-> (theta, fval, dfval, accepted flags [T], fvalp - fval + qadj [T]) after the Metropolis-Hastings test of every rung"""
    fvalp = lp / temps
    qadj = np.zeros(len(temps))
    if dfval is not None:
        dsum = dfval + grad / temps[:, None]
        t2 = ((rho(tau) * temps13) / 2.0)[:, None] * _rowmat(dsum, hc)
        s1, s2 = np.zeros(len(temps)), np.zeros(len(temps))
        for i in range(hc.shape[0]):
            term1 = normals[:, i] / SQRT2
            s1 = s1 + term1 * t2[:, i]
            s2 = s2 + t2[:, i] * t2[:, i]
        qadj = -(2.0 * s1 + s2)
    with np.errstate(invalid="ignore"):
        delta = (fvalp - fval) + qadj
        take = logu_accept < delta
    theta, fval = theta.copy(), fval.copy()
    theta[take] = thetap[take]
    fval[take] = fvalp[take]
    if dfval is not None:
        dfval = dfval.copy()
        dfval[take] = (grad / temps[:, None])[take]
    return theta, fval, dfval, take, delta


def exchange_order(fvaln, temps, picks, logu_swap, counts=None):
    """tempexchange with the picks and log-uniforms given: the order after all of them (counts [T - 1], optional: swaps
    between rungs rt - 1 and rt are added at rt - 1)"""
    order = np.arange(len(temps))
    for rt, lu in zip(picks, logu_swap):
        rt = int(rt)
        if (fvaln[order[rt]] - fvaln[order[rt - 1]]) * (1.0 / temps[rt - 1] - 1.0 / temps[rt]) > lu:
            order[rt - 1], order[rt] = order[rt], order[rt - 1]
            if counts is not None:
                counts[rt - 1] += 1
    return order


def exchange(theta, fval, dfval, temps, picks, logu_swap, counts=None):
    fvaln = fval * temps
    order = exchange_order(fvaln, temps, picks, logu_swap, counts)
    dfo = None if dfval is None else (1.0 / temps)[:, None] * (temps[:, None] * dfval)[order]
    return theta[order], fvaln[order] / temps, dfo, order


def tune(tau, numtimes, naccepted, T, k, samptunning, taracc):
    numtimes = numtimes + naccepted / T
    if k < samptunning and k % 10 == 0:
        tau = tau + 1.0 / np.sqrt(1.0 + k / 10.0) * ((numtimes / 10.0) - taracc)
        numtimes = 0.0
    return tau, numtimes


def step(state, k, draws, logpost, temps, temps13, hc, covmat0, samptunning, taracc):
    """one step from state = dict(theta, fval, dfval (None: no gradient), tau, numtimes); logpost(X) -> lp or (lp, grad).
    Returns the new state and a dict of what happened (accepted flags, order, proposal)."""
    th, fv, df, tau, nt = state["theta"], state["fval"], state["dfval"], state["tau"], state["numtimes"]
    thetap = propose(th, df, tau, temps13, hc, covmat0, draws["normals"])
    out = logpost(thetap)
    lp, grad = out if isinstance(out, tuple) else (out, None)
    th, fv, df, take, delta = accept(th, fv, df, thetap, lp, grad, draws["normals"], tau, temps, temps13, hc, draws["logu_accept"])
    swaps = np.zeros(len(temps) - 1, dtype=np.int64)
    th, fv, df, order = exchange(th, fv, df, temps, draws["picks"], draws["logu_swap"], swaps)
    tau, nt = tune(tau, nt, int(np.sum(take)), len(temps), k, samptunning, taracc)
    return dict(theta=th, fval=fv, dfval=df, tau=tau, numtimes=nt), dict(accepted=take, order=order, swaps=swaps,
                                                                          thetap=thetap, lp=lp, delta=delta)


def gaussian_target(mean, prec, gradient):
    """the fixed Gaussian targets of tests/golden/g12_ptlmc.npz: lp = -1/2 (x - mean)^T prec (x - mean); with gradient the
    (lp[m, 1], grad[m, p]) form the reference's gradient branch works with (lp a column)"""
    def lp(X):
        D = X - mean
        return -0.5 * np.sum((D @ prec) * D, axis=1)

    if not gradient:
        return lp

    def lpg(X, return_grad=True):
        X = np.array(X, ndmin=2)
        v = lp(X)[:, None]
        return (v, -(X - mean) @ prec) if return_grad else v
    return lpg


def replay(start, steps, lpf, temps, hc, covmat0, numtemps, samptunning, sampperchain, taracc, gradient):
    """the whole step loop from the start state [T, d] with recorded draws (a list of draws dicts): the saved theta
    [numchain, sampperchain, d] (src/mcmc.py:616-670 restated)"""
    out = lpf(start)
    if gradient:
        lp, g = out
        state = dict(theta=start.copy(), fval=np.reshape(lp, -1) / temps, dfval=g / temps[:, None], tau=-1.0, numtimes=0.0)
        f = lambda X: (np.reshape(lpf(X)[0], -1), lpf(X)[1])          # noqa: E731
    else:
        state = dict(theta=start.copy(), fval=out / temps, dfval=None, tau=-1.0, numtimes=0.0)
        f = lpf
    save = np.zeros((len(temps) - numtemps, sampperchain, start.shape[1]))
    temps13 = temps ** (1 / 3)
    for k, dr in enumerate(steps):
        state, _ = step(state, k, dr, f, temps, temps13, hc, covmat0, samptunning, taracc)
        if k >= samptunning:
            save[:, k - samptunning, :] = state["theta"][numtemps:]
    return save
