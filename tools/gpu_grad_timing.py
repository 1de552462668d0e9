"""Value-only against value + gradient of the log-posterior on the same rows (gpb_chain_logpost vs gpb_chain_logpost_grad, device
tensors, no host copies), at cfg 3, cfg 4 and the nine-emulator chain; Emulator.predict_jacobian at cfg 2.
Median of --reps timed calls after two warm-up calls.  Prints one line per case and a JSON summary line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _median_ms(fn, reps):
    import torch
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts))


def chain_case(name, chain, X, reps):
    import torch
    from gpbayestools_hic_amd import _native as nat
    from gpbayestools_hic_amd.mcmc import EXTRA_STD_CONST
    Xd = torch.as_tensor(X, device="cuda:0")
    W, nd = X.shape
    ll = torch.empty(W, dtype=torch.float64, device="cuda:0")
    g = torch.empty((W, nd), dtype=torch.float64, device="cuda:0")
    chain._prepare_blocks()
    engs = [e._engine_ready() for e in chain.emuList]
    arr = (nat.C.c_void_p * len(engs))(*[e.h for e in engs])
    lo, hi = chain._box(Xd.device)
    e0 = engs[0]
    t_val = _median_ms(lambda: chain.log_prob_device(Xd, out=ll), reps)
    t_grad = _median_ms(lambda: e0._ck(e0.lib.gpb_chain_logpost_grad(arr, len(engs), nat.ptr(Xd), W, nat.ptr(ll), nat.ptr(g),
                                                                     nat.ptr(lo), nat.ptr(hi), -np.inf, EXTRA_STD_CONST)), reps)
    r = dict(case=name, rows=W, value_ms=round(t_val, 3), value_grad_ms=round(t_grad, 3), ratio=round(t_grad / t_val, 2))
    print("%-16s rows %5d   value %8.3f ms   value+grad %8.3f ms   ratio %.2f" % (name, W, t_val, t_grad, t_grad / t_val))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default="", help="comma list of cases (cfg3, cfg4, nine, jac2)")
    a = ap.parse_args()
    from gpbayestools_hic_amd import synth
    from gpbayestools_hic_amd.workload import build_chain, build_multi_chain
    only = set(a.only.split(",")) if a.only else {"cfg3", "cfg4", "nine", "jac2"}
    out = []
    for cfg in (3, 4):
        if "cfg%d" % cfg not in only:
            continue
        chain, emu, info = build_chain(cfg)
        X = synth.walkers_ball(info["W"], info["xstar"], radius=0.05)
        out.append(chain_case("cfg%d" % cfg, chain, X, a.reps))
    if "nine" in only:
        specs = [(1024, 60, 10, "RBF")] * 9
        chain, emus, info = build_multi_chain(specs, 15)
        X = synth.walkers_ball(2048, info["xstar"], radius=0.05)
        out.append(chain_case("nine x cfg3", chain, X, a.reps))
    if "jac2" in only:
        chain, emu, info = build_chain(2)
        X = synth.walkers(info["W"], info["d"])
        t_pred = _median_ms(lambda: emu.predict(X, return_cov=False), a.reps)
        t_jac = _median_ms(lambda: emu.predict_jacobian(X), a.reps)
        out.append(dict(case="cfg2 jacobian", rows=len(X), predict_ms=round(t_pred, 3), jacobian_ms=round(t_jac, 3)))
        print("%-16s rows %5d   predict %8.3f ms   predict_jacobian %8.3f ms (host in / out)" % ("cfg2", len(X), t_pred, t_jac))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
