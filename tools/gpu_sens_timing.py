"""Chain.sensitivity timed on the nine-emulator chain of the benchmark (nine emulators of 1000 design points over 20 parameters,
540 observables) at S = --samples (default 1e5) posterior samples drawn in a small ball around the truth point:
  * the whole call (median of --reps calls after one untimed call, wall clock with a device synchronisation);
  * its pieces from events on the stream: gpb_emu_predict, gpb_emu_predict_jac, and gpb_sens_accumulate per emulator;
  * the device memory a first call takes: the drop of the device's free memory (mem_get_info) from before the first call to after
    it, which counts torch's cached blocks AND the library's own workspaces (every emulator context's predict, gradient and
    sens_ws buffers), and beside it the peak of torch's tensors alone;
  * the numpy route — Emulator.predict_jacobian + Emulator.predict to the host, then a per-row scipy cho_factor / cho_solve loop —
    on --host-rows (default 2000) of those rows, extrapolated linearly to S.
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
    import torch
    if not torch.cuda.is_available():
        sys.exit("gpu_sens_timing: no GPU (a timing needs one)")
    from gpbayestools_hic_amd import synth
    from gpbayestools_hic_amd.sensitivity import posterior_sensitivity
    from gpbayestools_hic_amd.workload import build_multi_chain
    specs = [(1000, 60, 6 + i % 3, ("RBF", "Matern25", "RBF")[i % 3]) for i in range(9)]
    chain, emus, info = build_multi_chain(specs, 20)
    S = a.samples
    X = synth.walkers_ball(S, info["xstar"], 0.02)
    lines = ["chain: 9 emulators, %d observables, 20 parameters; S = %d rows" % (chain.nobs, S)]

    chain.sensitivity(X[:256])                           # the emulators' resident state and first launches, before the memory reading
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free0 = torch.cuda.mem_get_info()[0]
    torch.cuda.reset_peak_memory_stats()
    res = chain.sensitivity(X)                           # untimed: allocations at full slab size
    torch.cuda.synchronize()
    taken = free0 - torch.cuda.mem_get_info()[0]
    peak_first = torch.cuda.max_memory_allocated()
    ts = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        res = chain.sensitivity(X)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    total = float(np.median(ts))
    peak = peak_first
    lines.append("Chain.sensitivity: %.1f ms (median of %d, spread %.1f %%), %.2f us per row; n_bad %s"
                 % (1e3 * total, a.reps, 100.0 * (max(ts) - min(ts)) / total, 1e6 * total / S, res.n_bad.tolist()))
    lines.append("device memory taken by the call (drop of free memory: torch's blocks and the library's workspaces of all nine "
                 "contexts): %.1f MB; of it torch tensors (rows, mean, covariance, Jacobian) at their peak: %.1f MB"
                 % (taken / 2 ** 20, peak / 2 ** 20))
    profs = []
    for _ in range(a.reps):
        p = {}
        posterior_sensitivity(chain, X, profile=p)
        profs.append(p)
    pred = float(np.median([p["predict"] for p in profs]))
    jac = float(np.median([p["jacobian"] for p in profs]))
    accs = np.median(np.stack([p["accumulate"] for p in profs]), axis=0)
    lines.append("events on the stream, slabs of %d rows: gpb_emu_predict %.1f ms, gpb_emu_predict_jac %.1f ms, gpb_sens_accumulate "
                 "%.1f ms (%.0f %% of the three)" % (profs[0]["slab_rows"], pred, jac, accs.sum(),
                                                      100.0 * accs.sum() / (pred + jac + accs.sum())))
    lines.append("gpb_sens_accumulate per emulator (M = 60, d = 20, LDS path): " + ", ".join("%.1f" % v for v in accs) + " ms")

    # the numpy route on a subset
    n = min(a.host_rows, S)
    Xh = X[:n]
    t0 = time.perf_counter()
    r0 = 0
    Fh = np.zeros((len(emus), 20, 20))
    for k, emu in enumerate(emus):
        M = emu.nobs
        J = emu.predict_jacobian(Xh)
        y, C = emu.predict(Xh, return_cov=True)
        C = C + chain.expdata_cov[r0:r0 + M, r0:r0 + M][None]
        for w in range(n):
            cf = scipy.linalg.cho_factor(C[w], lower=True)
            Fh[k] += J[w].T @ scipy.linalg.cho_solve(cf, J[w])
        _ = (Xh[:, None, :] * J / y[:, :, None]).mean(0)
        r0 += M
    host = time.perf_counter() - t0
    lines.append("numpy route (predict_jacobian + predict to the host, per-row cho_solve) on %d rows: %.2f s = %.1f us per row; "
                 "extrapolated to S: %.1f s, %.0f times the device call" % (n, host, 1e6 * host / n, host / n * S, host / n * S / total))
    summary = dict(samples=S, total_ms=1e3 * total, predict_ms=pred, jacobian_ms=jac, accumulate_ms=[float(v) for v in accs],
                   taken_mb=taken / 2 ** 20, torch_peak_mb=peak / 2 ** 20, host_rows=n, host_s=host, host_extrapolated_s=host / n * S)
    lines.append(json.dumps(summary))
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
