"""Closed-form cross-validation against the only other route to the same numbers, on one context (device outputs, no host copies
of results): gpb_gp_cv leave-one-out, gpb_gp_cv with folds of 64, gpb_gp_factor, and one fold by refit (gpb_gp_set on the
remaining rows + gpb_gp_set_theta + gpb_gp_factor + gpb_gp_predict of the fold) multiplied by the fold count.
N = 1000 and 2048, P = 10, d = 8, RBF at the timing theta.  Median of --reps (>= 10) timed calls after two warm-up calls, host
clock around a call that ends in a device synchronise.  Prints one line per case and a JSON summary line."""
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
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def case(N, P, d, reps):
    import torch
    from gpbayestools_hic_amd import GPEngine, synth
    from gpbayestools_hic_amd import _native as nat
    X = synth.lhs(N, d, 31)
    rng = np.random.default_rng(32)
    Z = np.ascontiguousarray((np.sin(X @ rng.standard_normal((d, P))) + 0.1 * rng.standard_normal((N, P))).T)
    th = synth.fixed_theta(d, P)
    eng = GPEngine(0)
    eng.set_data(X, Z, "RBF", 0.1)
    eng.set_theta(th)
    eng.factor()
    dev = torch.device("cuda", 0)
    mean = torch.empty((N, P), dtype=torch.float64, device=dev)
    var = torch.empty((N, P), dtype=torch.float64, device=dev)
    folds = [np.arange(i, min(i + 64, N)) for i in range(0, N, 64)]
    idx = np.ascontiguousarray(np.concatenate(folds), dtype=np.int32)
    fptr = np.ascontiguousarray(np.concatenate([[0], np.cumsum([len(f) for f in folds])]), dtype=np.int32)
    nf = len(folds)
    cov = torch.empty((P, nf, 64, 64), dtype=torch.float64, device=dev)
    ck, lib, h = eng._ck, eng.lib, eng.h
    t_loo = _median_ms(lambda: ck(lib.gpb_gp_cv(h, None, N, None, N, 1, nat.ptr(mean), nat.ptr(var), None)), reps)
    t_f64 = _median_ms(lambda: ck(lib.gpb_gp_cv(h, nat.ptr(idx), N, nat.ptr(fptr), nf, 1, nat.ptr(mean), nat.ptr(var), None)), reps)
    t_f64c = _median_ms(lambda: ck(lib.gpb_gp_cv(h, nat.ptr(idx), N, nat.ptr(fptr), nf, 1, nat.ptr(mean), nat.ptr(var), nat.ptr(cov))), reps)
    t_fac = _median_ms(lambda: eng.factor(), reps)
    # the parent's route, one fold: a context over the remaining rows, factored, predicting the fold
    keep = np.setdiff1d(np.arange(N), folds[0])
    Xk, Zk, Xf = np.ascontiguousarray(X[keep]), np.ascontiguousarray(Z[:, keep]), np.ascontiguousarray(X[folds[0]])
    ref = GPEngine(0)

    def refit():
        ref.set_data(Xk, Zk, "RBF", 0.1)
        ref.set_theta(th)
        ref.factor()
        ref.predict(Xf)
    t_ref = _median_ms(refit, reps)
    ref.close()
    eng.close()
    r = dict(N=N, P=P, d=d, reps=reps, loo_ms=round(t_loo[0], 3), loo_min_max=[round(t_loo[1], 3), round(t_loo[2], 3)],
             folds64_ms=round(t_f64[0], 3), folds64_cov_ms=round(t_f64c[0], 3), nfolds64=nf, factor_ms=round(t_fac[0], 3),
             refit_one_fold_ms=round(t_ref[0], 3), refit_all_folds64_ms=round(t_ref[0] * nf, 1),
             refit_loo_ms=round(t_ref[0] * N, 1))
    print("N %5d P %3d   gpb_gp_cv leave-one-out %8.3f ms (%.3f - %.3f)   %d folds of 64 %8.3f ms (with blocks %8.3f)   "
          "gpb_gp_factor %8.3f ms   refit route: one fold %8.3f ms, x %d folds = %.1f ms, x N (leave-one-out) = %.1f ms"
          % (N, P, t_loo[0], t_loo[1], t_loo[2], nf, t_f64[0], t_f64c[0], t_fac[0], t_ref[0], nf, t_ref[0] * nf, t_ref[0] * N))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sizes", default="1000,2048")
    a = ap.parse_args()
    if a.reps < 10:
        ap.error("--reps must be at least 10")
    out = [case(int(n), 10, 8, a.reps) for n in a.sizes.split(",")]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
