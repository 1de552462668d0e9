"""gpb_mcmc_diag timed at the shape of a production chain (default nsteps = 2000, nwalkers = 4096, ndim = 20 — cfg 4's ensemble) on
an AR(1) chain generated on the device, with max_lag = 1024 and max_lag = nsteps - 1, against the host route: the device-to-host
copy the host needs plus the numpy restatement of emcee's integrated_time (tests/acf_reference.py: one FFT per walker and
parameter in a Python loop) on the same array.  Device times: HIP events around asynchronous calls (on_device outputs), median of
--reps after --warmup untimed calls.  The pack + statistics kernels are timed alone (outputs = moments), the band product with its
lag sums and scan is the difference; its rate counts the algorithmic flops of the band, 2 * 64 * 64 * nwalkers per block.  For
kernel times proper run it under `rocprofv3 --kernel-trace --stats -- python tools/gpu_diag_timing.py --reps 3 --no-host`.
Prints one line per measurement and a JSON summary line; --out FILE also writes them to a file."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FP64_MATRIX_PEAK = 78.6e12        # the figure k_predict's 0.83 is quoted against


def _events(fn, reps, warmup):
    """(median ms, relative spread) by device events"""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    med = float(np.median(ts))
    return med, float((max(ts) - min(ts)) / med)


def band_blocks(n, max_lag):
    nb = (n + 63) // 64
    nd = min((max_lag + 63) // 64, nb - 1) + 1
    return sum(nb - D for D in range(nd))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nsteps", type=int, default=2000)
    ap.add_argument("--nwalkers", type=int, default=4096)
    ap.add_argument("--ndim", type=int, default=20)
    ap.add_argument("--phi", type=float, default=0.8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("gpu_diag_timing: no GPU (a timing needs one)")
    from gpbayestools_hic_amd import GPEngine
    n, nw, d = a.nsteps, a.nwalkers, a.ndim
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    x = torch.empty((n, nw, d), dtype=torch.float64, device=dev)
    e = torch.randn((n, nw, d), dtype=torch.float64, device=dev, generator=g)
    x[0] = e[0]
    for t in range(1, n):
        x[t] = a.phi * x[t - 1] + (1.0 - a.phi ** 2) ** 0.5 * e[t]
    del e
    eng = GPEngine(0)
    r = dict(tool="gpu_diag_timing", nsteps=n, nwalkers=nw, ndim=d, phi=a.phi, reps=a.reps, warmup=a.warmup)
    pack_ms, pack_sp = _events(lambda: eng.mcmc_diag(x, "steps", 0, 5.0, on_device=True, outputs=("moments",)), a.reps, a.warmup)
    r.update(pack_stats_ms=pack_ms, pack_stats_spread=pack_sp)
    print("pack + statistics alone: %.3f ms (spread %.1f %%) = %.0f GB/s of chain read three times and Y written once"
          % (pack_ms, 100 * pack_sp, 4 * 8.0 * n * nw * d / pack_ms / 1e6))
    res = {}
    for name, L in (("lag1024", min(1024, n - 1)), ("full", n - 1)):
        ms, sp = _events(lambda: eng.mcmc_diag(x, "steps", L, 5.0, on_device=True), a.reps, a.warmup)
        res[name] = eng.mcmc_diag(x, "steps", L, 5.0)
        blocks = band_blocks(n, L)
        flops = 2.0 * 64 * 64 * nw * blocks * d
        band_ms = ms - pack_ms
        tf = flops / band_ms / 1e9
        r[name] = dict(max_lag=L, ms=ms, spread=sp, band_blocks_per_parameter=blocks, band_tflop=flops / 1e12,
                       band_ms_by_difference=band_ms, band_tflops=tf, band_fraction_of_fp64_matrix_peak=tf * 1e12 / FP64_MATRIX_PEAK)
        print("max_lag %d: %.3f ms (spread %.1f %%); band product + lag sums + scan by difference %.3f ms for %.3f Tflop = %.1f TF/s "
              "= %.2f of the fp64 matrix peak" % (L, ms, 100 * sp, band_ms, flops / 1e12, tf, tf * 1e12 / FP64_MATRIX_PEAK))
    same = bool(np.array_equal(res["lag1024"]["tau"], res["full"]["tau"]) and np.array_equal(res["lag1024"]["window"], res["full"]["window"]))
    r.update(tau=[float(v) for v in res["full"]["tau"]], window_max=int(res["full"]["window"].max()), band_independent=same)
    print("tau %.3f .. %.3f (AR(1) value %.3f), largest window %d; tau and window equal for both bands: %s"
          % (min(r["tau"]), max(r["tau"]), (1 + a.phi) / (1 - a.phi), r["window_max"], same))
    if not a.no_host:
        import acf_reference as R
        t0 = time.perf_counter()
        xh = x.cpu().numpy()
        t_copy = time.perf_counter() - t0
        t0 = time.perf_counter()
        ref = R.integrated_time(xh, 5.0)
        t_host = time.perf_counter() - t0
        err = float(np.max(np.abs(res["full"]["rho"] - ref["rho"])))
        r.update(host_copy_s=t_copy, host_numpy_s=t_host, host_rho_max_abs_diff=err,
                 host_window_equal=bool(np.array_equal(res["full"]["window"], ref["window"])),
                 speedup_full=(t_copy + t_host) / (r["full"]["ms"] * 1e-3), speedup_lag1024=(t_copy + t_host) / (r["lag1024"]["ms"] * 1e-3))
        print("host route: copy %.3f s + numpy FFT loop %.2f s; device full band %.0fx, max_lag 1024 %.0fx; rho max |diff| %.2e, windows "
              "equal: %s" % (t_copy, t_host, r["speedup_full"], r["speedup_lag1024"], err, r["host_window_equal"]))
    line = json.dumps(r)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
