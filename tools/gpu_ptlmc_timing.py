"""PTLMC step loop (gpb_chain_ptlmc_run) per step, both branches, against one evaluation of the ladder's rows (gpb_chain_logpost /
gpb_chain_logpost_grad), at the analysis notebook's shape (nine synthetic N = 1000 emulators, ntemps 30 + nwalkers 100 = 130
rungs) and at cfg 3; plus the wall time of the batched pre-optimizer from nstartparameters rows.
Prints one line per case and a JSON summary line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _ms(fn, reps=3):
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts))


def case(name, chain, xstar, numtemps, numchain, nsteps, nstart, preopt):
    import torch
    from gpbayestools_hic_amd import ptlmc
    T = numtemps + numchain
    temps = ptlmc.ladder(numtemps, numchain, 100.0)
    rng = np.random.default_rng(0)
    theta = np.clip(xstar + 0.03 * rng.standard_normal((T, chain.ndim)), 0.02, 0.98)
    covmat0, hc = ptlmc.proposal_factor(theta)
    Xd = torch.as_tensor(theta, device="cuda:0")
    out = []
    for grad in (False, True):
        if grad:
            lp, g = chain.log_posterior(theta, return_grad=True)
            fval, dfval = lp / temps, g / temps[:, None]
            t_eval = _ms(lambda: chain._log_prob_grad(theta, -np.inf))
        else:
            fval, dfval = chain.log_posterior(theta) / temps, None
            t_eval = _ms(lambda: chain.log_prob_device(Xd))
        s = ptlmc.PTLMCSampler(chain, temps, hc, covmat0, numtemps, numchain, 2 * nsteps, nsteps, 0.6 if grad else 0.25, 1,
                               grad)
        s.set_state(theta, fval, dfval)
        t_run = _ms(lambda: s.run(nsteps)) / nsteps
        r = dict(case=name, branch="grad" if grad else "plain", rungs=T, ms_per_step=round(t_run, 4),
                 eval_ms=round(t_eval, 4))
        print("%-12s %-5s rungs %4d   %.4f ms/step   one evaluation of the rungs %.4f ms%s" %
              (name, r["branch"], T, t_run, t_eval, " (host round trip included)" if grad else ""))
        out.append(r)
    if preopt:                  # (the same in both branches: the searches take the device gradient either way)
        X0 = np.random.default_rng(1).uniform(chain.min, chain.max, (nstart, chain.ndim))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ptlmc._preoptimize(chain, X0, T, -np.inf, np.random.default_rng(2))
        t = time.perf_counter() - t0
        print("%-12s pre-optimizer from %d rows, %d searches: %.2f s" % (name, nstart, T, t))
        out.append(dict(case=name, preoptimizer_s=round(t, 2), rows=nstart, searches=T))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--only", default="", help="comma list of cases (notebook, cfg3)")
    a = ap.parse_args()
    from gpbayestools_hic_amd.workload import build_chain, build_multi_chain
    only = set(a.only.split(",")) if a.only else {"notebook", "cfg3"}
    res = []
    if "notebook" in only:
        chain, emus, info = build_multi_chain([(1000, 60, 10, "RBF")] * 9, 15)
        res += case("notebook", chain, info["xstar"], 30, 100, a.steps, 7000, True)
    if "cfg3" in only:
        chain, emu, info = build_chain(3)
        res += case("cfg3", chain, info["xstar"], 30, 100, a.steps, 7000, False)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
