"""Chain.goodness_of_fit timed on the nine-emulator chain of the benchmark (nine emulators of 1000 design points over 20
parameters, 540 observables) at S = --samples (default 1e5) posterior samples drawn in a small ball around the truth point:
  * the whole call (median of --reps calls after one untimed call, wall clock with a device synchronisation);
  * its phases: gpb_emu_predict and gpb_gof_accumulate from events on the stream, and the summary (gpb_ppd_summary, the totals,
    gpb_chi2_sf, gpb_gof_influence and their read-backs) by the wall clock;
  * the numpy route — Emulator.predict to the host, then per row scipy cho_factor / cho_solve and scipy.special.gammaincc — on
    --host-rows (default 2000) of those rows, extrapolated linearly to S.
Prints one line per measurement and a JSON summary line; --out FILE also writes them to a file."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=100000)
    ap.add_argument("--host-rows", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    import scipy.linalg
    import scipy.special
    import torch
    if not torch.cuda.is_available():
        sys.exit("gpu_gof_timing: no GPU (a timing needs one)")
    from gpbayestools_hic_amd import synth
    from gpbayestools_hic_amd.gof import posterior_gof
    from gpbayestools_hic_amd.workload import build_multi_chain
    specs = [(1000, 60, 6 + i % 3, ("RBF", "Matern25", "RBF")[i % 3]) for i in range(9)]
    chain, emus, info = build_multi_chain(specs, 20)
    S = a.samples
    X = synth.walkers_ball(S, info["xstar"], 0.02)
    lines = ["chain: 9 emulators, %d observables, 20 parameters; S = %d rows" % (chain.nobs, S)]
    res = chain.goodness_of_fit(X)                       # untimed: allocations at full slab size
    torch.cuda.synchronize()
    ts = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        res = chain.goodness_of_fit(X)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    total = float(np.median(ts))
    lines.append("Chain.goodness_of_fit: %.1f ms (median of %d, spread %.1f %%), %.2f us per row; n_bad %s"
                 % (1e3 * total, a.reps, 100.0 * (max(ts) - min(ts)) / total, 1e6 * total / S, res.n_bad.tolist()))
    profs = []
    for _ in range(a.reps):
        p = {}
        posterior_gof(chain, X, profile=p)
        profs.append(p)
    pred, acc, summ = (float(np.median([p[k] for p in profs])) for k in ("predict", "accumulate", "summary"))
    lines.append("phases, slabs of %d rows: gpb_emu_predict %.1f ms, gpb_gof_accumulate %.1f ms (nine emulators, M = 60, LDS path; "
                 "events on the stream), summary %.1f ms (quantiles, totals, p-values, influence and their read-backs; wall clock)"
                 % (profs[0]["slab_rows"], pred, acc, summ))
    lines.append(repr(res))

    # the numpy route on a subset
    n = min(a.host_rows, S)
    Xh = X[:n]
    t0 = time.perf_counter()
    r0 = 0
    chi2 = np.zeros((n, len(emus)))
    for k, emu in enumerate(emus):
        M = emu.nobs
        y, C = emu.predict(Xh, return_cov=True)
        C = C + chain.expdata_cov[r0:r0 + M, r0:r0 + M][None]
        dy = y - chain.expdata[0][r0:r0 + M]
        for w in range(n):
            cf = scipy.linalg.cho_factor(C[w], lower=True)
            chi2[w, k] = dy[w] @ scipy.linalg.cho_solve(cf, dy[w])
        _ = scipy.special.gammaincc(M / 2.0, chi2[:, k] / 2.0).mean(), np.percentile(chi2[:, k], [5, 16, 50, 84, 95])
        r0 += M
    host = time.perf_counter() - t0
    lines.append("numpy route (predict to the host, per-row cho_factor / cho_solve, gammaincc) on %d rows: %.2f s = %.1f us per row; "
                 "extrapolated to S: %.1f s, %.0f times the device call" % (n, host, 1e6 * host / n, host / n * S, host / n * S / total))
    summary = dict(samples=S, total_ms=1e3 * total, predict_ms=pred, accumulate_ms=acc, summary_ms=summ, host_rows=n, host_s=host,
                   host_extrapolated_s=host / n * S)
    lines.append(json.dumps(summary))
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
