"""Chain.loo timed on the nine-emulator chain of the benchmark (nine emulators of 1000 design points over 20 parameters, 540
observables) at S = --samples (default 1e5) posterior samples drawn in a small ball around the truth point, for both units:
  * the whole call (median of --reps calls after one untimed call, wall clock with a device synchronisation);
  * its phases from events on the stream: gpb_emu_predict, the pointwise kernel (gpb_loo_pointwise per observable,
    gpb_gof_accumulate per data set — the same rows, so the two stand side by side) and gpb_psis_loo;
  * the PSIS pass as a fraction of the HBM bandwidth (--hbm-gbs, default 8000): the kernel reads every row nine times and the
    standardised residuals once;
  * the numpy model of tests/psis_reference.py: loo_pointwise on --host-rows rows and psis_loo on --host-units units, each
    extrapolated linearly and divided by 16 (sixteen threads, taken to scale perfectly: rows and units are independent).
Prints one line per measurement and a JSON summary line; --out FILE also writes them to a file."""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PSIS_READS = 9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=100000)
    ap.add_argument("--host-rows", type=int, default=500)
    ap.add_argument("--host-units", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("gpu_loo_timing: no GPU (a timing needs one)")
    import psis_reference as R
    from gpbayestools_hic_amd import synth
    from gpbayestools_hic_amd.gof import posterior_gof
    from gpbayestools_hic_amd.loo import posterior_loo
    from gpbayestools_hic_amd.workload import build_multi_chain
    warnings.simplefilter("ignore")
    specs = [(1000, 60, 6 + i % 3, ("RBF", "Matern25", "RBF")[i % 3]) for i in range(9)]
    chain, emus, info = build_multi_chain(specs, 20)
    S = a.samples
    X = synth.walkers_ball(S, info["xstar"], 0.02)
    lines = ["chain: 9 emulators, %d observables, 20 parameters; S = %d rows" % (chain.nobs, S)]
    summary = dict(samples=S)
    res = {}
    for unit in ("observable", "dataset"):
        res[unit] = chain.loo(X, unit=unit, return_pointwise=unit == "observable")       # untimed: allocations at full size
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            chain.loo(X, unit=unit)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        total = float(np.median(ts))
        profs = []
        for _ in range(a.reps):
            p = {}
            posterior_loo(chain, X, unit=unit, profile=p)
            profs.append(p)
        pred, pw, ps = (float(np.median([p[k] for p in profs])) for k in ("predict", "pointwise", "psis"))
        n_units = res[unit].n_units
        nbytes = 8.0 * n_units * S * (PSIS_READS + (1 if unit == "observable" else 0))
        lines.append("Chain.loo(unit=%s): %.1f ms (median of %d, spread %.1f %%); phases, slabs of %d rows: gpb_emu_predict %.1f ms, "
                     "%s %.1f ms, gpb_psis_loo %.2f ms over %d units = %.0f GB/s, %.1f %% of %.0f GB/s (the row read %d times%s)"
                     % (unit, 1e3 * total, a.reps, 100.0 * (max(ts) - min(ts)) / total, profs[0]["slab_rows"], pred,
                        "gpb_loo_pointwise" if unit == "observable" else "gpb_gof_accumulate", pw, ps, n_units, nbytes / ps / 1e6,
                        100.0 * nbytes / ps / 1e6 / a.hbm_gbs, a.hbm_gbs, PSIS_READS,
                        ", the residuals once" if unit == "observable" else ""))
        summary[unit] = dict(total_ms=1e3 * total, predict_ms=pred, pointwise_ms=pw, psis_ms=ps, psis_gbs=nbytes / ps / 1e6)
    p = {}
    posterior_gof(chain, X, influence=False, profile=p)
    lines.append("the pointwise kernel beside gpb_gof_accumulate on the same rows (M = 60, LDS path): %.1f ms against %.1f ms, %.2f times"
                 % (summary["observable"]["pointwise_ms"], p["accumulate"], summary["observable"]["pointwise_ms"] / p["accumulate"]))
    summary["gof_accumulate_ms"] = p["accumulate"]
    lines.append(repr(res["observable"]))
    lines.append(repr(res["dataset"]))

    # the numpy model on subsets
    n = min(a.host_rows, S)
    t0 = time.perf_counter()
    r0 = 0
    for emu in emus:
        M = emu.nobs
        y, C = emu.predict(X[:n], return_cov=True)
        R.loo_pointwise(y, C, chain.expdata[0][r0:r0 + M], chain.expdata_cov[r0:r0 + M, r0:r0 + M])
        r0 += M
    host_pw = (time.perf_counter() - t0) / n * S
    ll, zc = res["observable"].pointwise["ll"], res["observable"].pointwise["zc"]
    u = min(a.host_units, ll.shape[0])
    t0 = time.perf_counter()
    R.psis_loo(ll[:u], zc[:u])
    host_ps = (time.perf_counter() - t0) / u * ll.shape[0]
    dev = summary["observable"]["total_ms"] / 1e3
    lines.append("numpy model, unit=observable: predict to the host and np.linalg.inv per row on %d rows, extrapolated to S: %.1f s; "
                 "psis_loo on %d units, extrapolated to %d: %.1f s; on sixteen threads %.1f s, %.0f times the device call"
                 % (n, host_pw, u, ll.shape[0], host_ps, (host_pw + host_ps) / 16, (host_pw + host_ps) / 16 / dev))
    summary.update(host_rows=n, host_units=u, host_pointwise_s=host_pw, host_psis_s=host_ps)
    lines.append(json.dumps(summary))
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
