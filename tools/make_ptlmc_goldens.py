#!/usr/bin/env python3
"""
Generate tests/golden/g12_ptlmc.npz by RUNNING THE REFERENCE's PTLMC sampler (Chain.samplerPTLMC and Chain.tempexchange,
src/mcmc.py:431-692) on small fixed Gaussian targets, in both branches.

    python tools/make_ptlmc_goldens.py          # needs /root/reference (as tools/make_goldens.py does)

Every draw the reference takes from numpy's global generator (np.random.normal / uniform / choice / standard_normal) is
recorded, and np.cov's argument — the start state of the step loop after the pre-optimizer, src/mcmc.py:604 — is captured,
so that tests/test_ptlmc_reference.py can replay the step loop with tests/ptlmc_reference.py and compare the saved samples.
The gradient branch's target returns lp as a column [m, 1] (the form its code works with).  Only arrays are written.
"""
import os
import sys
import tempfile
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
OUT = os.path.join(REPO, "tests", "golden")
REF = "/root/reference"

sys.dont_write_bytecode = True
os.environ["WORKDIR"] = tempfile.mkdtemp(prefix="gpb_ref_work_")
os.environ.setdefault("LOGLEVEL", "warning")
sys.path.insert(0, REF)

import ptlmc_reference as P  # noqa: E402

SETTINGS = dict(numtemps=4, numchain=4, sampperchain=12, maxtemp=10.0, nstartparameters=60)


def _import_reference():
    emcee = types.ModuleType("emcee")            # imported at module level, not used by the sampler (stand-ins)
    emcee.EnsembleSampler = type("EnsembleSampler", (), {})
    sys.modules.setdefault("emcee", emcee)
    sys.modules.setdefault("pocomc", types.ModuleType("pocomc"))
    from src import mcmc
    return mcmc


class _Recorder:
    """wraps numpy's global draws; `calls` holds (name, value) in order; np.cov's first argument is kept"""

    def __init__(self):
        self.calls, self.cov_arg = [], None
        self.orig = {n: getattr(np.random, n) for n in ("normal", "uniform", "choice", "standard_normal")}
        self.orig_cov = np.cov

    def __enter__(self):
        for n, f in self.orig.items():
            def w(*a, _f=f, _n=n, **k):
                v = _f(*a, **k)
                self.calls.append((_n, np.array(v, copy=True)))
                return v
            setattr(np.random, n, w)

        def cov(m, *a, **k):
            if self.cov_arg is None:
                self.cov_arg = (np.array(m, copy=True), len(self.calls))
            return self.orig_cov(m, *a, **k)
        np.cov = cov
        return self

    def __exit__(self, *exc):
        for n, f in self.orig.items():
            setattr(np.random, n, f)
        np.cov = self.orig_cov
        return False


def _steps(calls, T, d, K):
    """the draws of the step loop, per step: normals, accept uniforms, 5 x (picks, T swap uniforms)"""
    it = iter(calls)
    normals, ua, picks, us = [], [], [], []
    for _ in range(K):
        n, v = next(it); assert n == "normal" and v.shape == (T, d)
        normals.append(v)
        n, v = next(it); assert n == "uniform" and v.shape == (T,)
        ua.append(v)
        pk, u = [], []
        for _ in range(5):
            n, v = next(it); assert n == "choice"
            for rt in v:
                n, w = next(it); assert n == "uniform"
                pk.append(int(rt)); u.append(float(w[0]))
        picks.append(pk); us.append(u)
    assert next(it, None) is None
    return np.array(normals), np.array(ua), np.array(picks, dtype=np.int64), np.array(us)


def run_branch(mcmc, gradient, seed):
    d = 3
    rng = np.random.default_rng(seed)
    mean = rng.uniform(-0.5, 0.5, d)
    A = rng.standard_normal((d, d))
    prec = A @ A.T + d * np.eye(d)
    lpf = P.gaussian_target(mean, prec, gradient)
    chain = mcmc.Chain.__new__(mcmc.Chain)
    np.random.seed(seed)
    draw = lambda n: np.random.uniform(-2.0, 2.0, (n, d))           # noqa: E731
    with _Recorder() as rec:
        out = chain.samplerPTLMC(lpf, draw, **SETTINGS)
    start, ncall = rec.cov_arg
    T = SETTINGS["numtemps"] + SETTINGS["numchain"]
    K = int(np.ceil(SETTINGS["sampperchain"] * 2.0)) + SETTINGS["sampperchain"]
    normals, ua, picks, us = _steps(rec.calls[ncall:], T, d, K)
    p = "grad_" if gradient else "plain_"
    return {p + "mean": mean, p + "prec": prec, p + "start": start.T.copy(), p + "normals": normals, p + "u_accept": ua,
            p + "picks": picks, p + "u_swap": us, p + "theta": out["theta"]}


def tempexchange_cases(mcmc):
    chain = mcmc.Chain.__new__(mcmc.Chain)
    rng = np.random.default_rng(77)
    res = {}
    for i, (T, iters) in enumerate([(6, 1), (9, 5), (16, 3)]):
        lpostf = rng.normal(-5.0, 3.0, (T, 1))
        temps = np.array(np.concatenate((np.exp(np.linspace(np.log(20.0), np.log(20.0) / (T // 2 + 1), T // 2)),
                                         np.ones(T - T // 2))), ndmin=2).T
        np.random.seed(1000 + i)
        res["tx%d_lpostf" % i], res["tx%d_temps" % i] = lpostf, temps
        res["tx%d_iters" % i], res["tx%d_seed" % i] = np.array(iters), np.array(1000 + i)
        res["tx%d_order" % i] = chain.tempexchange(lpostf, temps, iters=iters)
    return res


def main():
    mcmc = _import_reference()
    out = {k: np.array(v) for k, v in SETTINGS.items()}
    out.update(run_branch(mcmc, False, 5))
    out.update(run_branch(mcmc, True, 6))
    out.update(tempexchange_cases(mcmc))
    path = os.path.join(OUT, "g12_ptlmc.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
