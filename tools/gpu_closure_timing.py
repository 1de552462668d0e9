#!/usr/bin/env python3
"""A closure study on the nine-emulator chain of tools/gpu_multi_emulator.py (N = 1000 design points, 20 parameters, 540
observables) on one MI355X: K = 40 and K = 200 data sets x 100 walkers as ONE resident run (closure.ClosureSampler,
gpb_chain_emcee_sets_run) against the same sets run one after the other through StretchSampler (gpb_chain_emcee_run with the
set's data installed as the experiment: what a closure study cost before).  Both in one process, alternating round by round
after a warm-up, in ms per step of ALL K ensembles.  Installing a set's data as the experiment is outside the timed region of
the sequential side; the one-run side's time includes ClosureSampler.run's own installation of the K sets' tables (once per
run of `steps` steps).  The walkers of both sides are compared bit for bit.

    python tools/gpu_closure_timing.py [N] [--out=profiles/closure_timing.txt] [--sets=40,200] [--steps=20] [--rounds=3]
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpbayestools_hic_amd import StretchSampler  # noqa: E402
from gpbayestools_hic_amd.closure import ClosureSampler  # noqa: E402
from gpbayestools_hic_amd.workload import build_multi_chain  # noqa: E402


def main():
    import torch
    N = int(sys.argv[1]) if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else 1000
    opt = dict(a[2:].split("=", 1) for a in sys.argv[1:] if a.startswith("--") and "=" in a)
    out_path = opt.get("out", os.path.join("profiles", "closure_timing.txt"))
    sets = [int(v) for v in opt.get("sets", "40,200").split(",")]
    steps, rounds = int(opt.get("steps", 20)), int(opt.get("rounds", 3))
    d, nw = 20, 100
    specs = [(N, 60, 6 + i % 3, ("RBF", "Matern25", "RBF")[i % 3]) for i in range(9)]
    chain, emus, info = build_multi_chain(specs, d)
    expdata0 = chain.expdata
    lines = ["closure timing: nine emulators, N = %d, d = %d, %d observables, %d GPs; %d walkers per set, %d steps per timed run, "
             "%d alternating rounds (median)" % (N, d, chain.nobs, sum(s[2] for s in specs), nw, steps, rounds)]
    for K in sets:
        rng = np.random.default_rng(K)
        truths = rng.uniform(0.3, 0.7, (K, d))
        data = np.ascontiguousarray(chain.pseudo_data(truths, noise=True, seed=K))
        X0 = np.clip(truths[:, None, :] + 0.01 * rng.standard_normal((K, nw, d)), 0.01, 0.99)      # a burnt-in start
        cs = ClosureSampler(chain, data, nw, seed=1)
        cs.run(X0, 3, store=False)                                         # warm-up: workspaces, tables
        seq = []
        for k in range(K):                                                 # warm-up of the sequential side: same seeds, same starts
            chain.expdata = data[k][None, :].copy()
            s = StretchSampler(chain, nw, seed=int(cs.seeds[k]))
            s.run(X0[k], 3, status=10 ** 9, store=False)
            seq.append(s)
        t_sets, t_seq = [], []
        for _ in range(rounds):
            chain.expdata = expdata0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last = cs.run(None, steps, store=False)
            torch.cuda.synchronize()
            t_sets.append((time.perf_counter() - t0) / steps * 1e3)
            total, same = 0.0, True
            for k, s in enumerate(seq):
                chain.expdata = data[k][None, :].copy()
                chain._prepare_blocks()                                    # (installing the set's data: not timed)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                lk = s.run(None, steps, status=10 ** 9, store=False)
                torch.cuda.synchronize()
                total += time.perf_counter() - t0
                same = same and np.array_equal(lk, last[k])
            t_seq.append(total / steps * 1e3)
        chain.expdata = expdata0
        row = {"K": K, "walkers_per_set": nw, "rows_per_half_step": K * nw // 2, "sets_ms_per_step": round(float(np.median(t_sets)), 3),
               "sequential_ms_per_step": round(float(np.median(t_seq)), 3),
               "ratio": round(float(np.median(t_seq) / np.median(t_sets)), 2), "same_walkers": bool(same),
               "acceptance": round(float(cs.acceptance_fraction.mean()), 3),
               "sets_rounds": [round(v, 3) for v in t_sets], "sequential_rounds": [round(v, 3) for v in t_seq]}
        print(json.dumps(row), flush=True)
        lines.append("K = %3d sets x %d walkers (%5d rows a half-step): one run %8.3f ms/step, one after the other %8.3f ms/step "
                     "(%.3f per set), ratio %.2f; same walkers: %s; rounds %s | %s"
                     % (K, nw, K * nw // 2, row["sets_ms_per_step"], row["sequential_ms_per_step"],
                        row["sequential_ms_per_step"] / K, row["ratio"], same, row["sets_rounds"], row["sequential_rounds"]))
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
