"""gpb_chain_rank_diag timed at the shape of a production chain (default nsteps = 2000, nwalkers = 4096, ndim = 20 — cfg 4's ensemble)
on an MH-like AR(1) chain generated on the device (tools/gpu_diag_timing.py's generator; every step repeats the previous value with
probability 1/2, so half the values are ties), against the host route: the device-to-host copy plus the numpy / scipy model of
tests/rank_reference.py (rankdata twice, one FFT per split chain and series) on --host-params parameters of the same array, scaled
to all of them and stated as such.  Device times: HIP events around asynchronous calls (on_device outputs), median of --reps after
--warmup untimed calls: the whole call, and the rank transform alone (outputs = median: one sort per parameter).  The sort's rate
counts the algorithmic traffic of the passes that ran, 12 bytes read and 12 bytes written per key and pass (the counting kernel's
second read of the keys is not counted); the passes that ran are found on the host from the keys' bytes.  --trace runs the tool
once more as a child under `rocprofv3 --kernel-trace` (a run of its own, one call) and adds the per-kernel times, summed
from the trace's records.
Prints one line per measurement and a JSON summary line; --out FILE also writes all of it to a file."""
import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


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


def passes_that_run(col):
    """digits (of eight) of the order-preserving keys of a device column that are not shared by all keys"""
    import torch
    u = (col + 0.0).contiguous().view(torch.int64).reshape(-1)
    key = torch.where(u < 0, ~u, u | torch.iinfo(torch.int64).min)
    return sum(int(((key >> (8 * p)) & 255).min() != ((key >> (8 * p)) & 255).max()) for p in range(8))


def trace(args):
    """the per-kernel table of one call, from a child of this tool under rocprofv3"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "-o", "run", "--", sys.executable,
               os.path.abspath(__file__), "--child", "--nsteps", str(args.nsteps), "--nwalkers", str(args.nwalkers), "--ndim",
               str(args.ndim), "--phi", str(args.phi)]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=args.trace_timeout)
        except subprocess.TimeoutExpired:
            sys.exit("gpu_rank_diag_timing: the traced child ran into its limit of %d s; nothing more is started" % args.trace_timeout)
        if r.returncode != 0:           # (a child that failed, faulted or aborted: this process does not go on to open the GPU)
            sys.exit("gpu_rank_diag_timing: the traced child failed (%d), nothing more is started: %s"
                     % (r.returncode, r.stdout.decode()[-400:]))
        files = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            say("rocprofv3 wrote no kernel_trace.csv: %s" % [os.path.relpath(p, tmp) for p in glob.glob(os.path.join(tmp, "**", "*"), recursive=True)])
            return None
        with open(files[0]) as fh:
            rows = list(csv.DictReader(fh))
    # the trace's own records, summed here by kernel (the tool's summary cuts the names of kernels in an unnamed namespace)
    agg = {}
    for row in rows:
        name = row.get("Kernel_Name", "")
        if not any(k in name for k in ("k_rank", "k_rsort", "k_diag_gram")):
            continue
        short = re.search(r"k_(rank|rsort|diag)_[a-z0-9_]+", name).group(0)      # (names arrive as gpb::(anonymous namespace)::k_...(...))
        t = agg.setdefault(short, [0, 0.0])
        t[0] += 1
        t[1] += (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e6
    table = [dict(kernel=k, calls=v[0], total_ms=v[1], mean_us=1e3 * v[1] / v[0]) for k, v in agg.items()]
    table.sort(key=lambda t: -t["total_ms"])
    say("per kernel, one call with every output but rank2 (rocprofv3 --kernel-trace, a run of its own):")
    for t in table:
        say("  %-18s %6d calls %10.3f ms in all %10.1f us each" % (t["kernel"], t["calls"], t["total_ms"], t["mean_us"]))
    return table


def make_chain(n, nw, d, phi):
    import torch
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    x = torch.empty((n, nw, d), dtype=torch.float64, device=dev)
    x[0] = torch.randn((nw, d), dtype=torch.float64, device=dev, generator=g)
    for t in range(1, n):
        e = torch.randn((nw, d), dtype=torch.float64, device=dev, generator=g)
        stay = torch.rand((nw, d), dtype=torch.float64, device=dev, generator=g) < 0.5
        x[t] = torch.where(stay, x[t - 1], phi * x[t - 1] + (1.0 - phi ** 2) ** 0.5 * e)
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nsteps", type=int, default=2000)
    ap.add_argument("--nwalkers", type=int, default=4096)
    ap.add_argument("--ndim", type=int, default=20)
    ap.add_argument("--phi", type=float, default=0.8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-params", type=int, default=1)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--trace-timeout", type=int, default=240, help="seconds the traced child may take")
    ap.add_argument("--child", action="store_true", help="one call and nothing else (what --trace profiles)")
    ap.add_argument("--out")
    a = ap.parse_args()
    table = trace(a) if a.trace and not a.child else None       # (before this process opens the GPU)
    import torch
    if not torch.cuda.is_available():
        sys.exit("gpu_rank_diag_timing: no GPU (a timing needs one)")
    from gpbayestools_hic_amd import GPEngine
    n, nw, d = a.nsteps, a.nwalkers, a.ndim
    h = n // 2
    nk = 2 * h * nw
    x = make_chain(n, nw, d, a.phi)
    eng = GPEngine(0)
    if a.child:
        eng.rank_diag(x, "steps", on_device=True)
        torch.cuda.synchronize()
        return
    r = dict(tool="gpu_rank_diag_timing", nsteps=n, nwalkers=nw, ndim=d, phi=a.phi, reps=a.reps, warmup=a.warmup, kept_draws=nk)
    ms, sp = _events(lambda: eng.rank_diag(x, "steps", on_device=True), a.reps, a.warmup)
    r.update(all_ms=ms, all_spread=sp)
    say("every output but rank2, max_lag = %d: %.2f ms (spread %.1f %%) for %d parameters of %d kept draws" % (h - 1, ms, 100 * sp, d, nk))
    ms1, sp1 = _events(lambda: eng.rank_diag(x, "steps", on_device=True, outputs=("median",)), a.reps, a.warmup)
    passes = sum(passes_that_run(x[:, :, j]) for j in range(d))
    traffic = 24.0 * nk * passes
    r.update(sort_ms=ms1, sort_spread=sp1, sort_passes=passes, sort_traffic_gb=traffic / 1e9, sort_gb_per_s=traffic / ms1 / 1e6)
    say("the rank transform's sort alone (outputs = median: gather + %d of %d passes + order statistics): %.2f ms (spread %.1f %%) = "
        "%.0f GB/s of the passes' algorithmic traffic (%.2f GB: 12 B read + 12 B written per key and pass)"
        % (passes, 8 * d, ms1, 100 * sp1, traffic / ms1 / 1e6, traffic / 1e9))
    out = eng.rank_diag(x, "steps")
    r.update(rhat_max=float(np.max(out["rhat"])), ess_bulk=[float(v) for v in out["ess"][:, 0]], stop_max=int(out["stop"].max()))
    say("largest R-hat %.4f, bulk-ESS %.0f .. %.0f, largest stop %d" % (r["rhat_max"], min(r["ess_bulk"]), max(r["ess_bulk"]), r["stop_max"]))
    if not a.no_host:
        import rank_reference as M
        hp = max(1, min(a.host_params, d))
        t0 = time.perf_counter()
        xh = x.cpu().numpy()
        t_copy = time.perf_counter() - t0
        t0 = time.perf_counter()
        ref = M.rank_diag(xh[:, :, :hp])
        t_host = time.perf_counter() - t0
        same = bool(np.array_equal(ref["stop"], out["stop"][:hp]) and np.array_equal(ref["median"], out["median"][:hp])
                    and np.array_equal(ref["quant"], out["quant"][:hp]))
        err = float(np.max(np.abs(out["ess"][:hp] - ref["ess"]) / ref["ess"]))
        r.update(host_copy_s=t_copy, host_model_s=t_host, host_params=hp, host_model_s_scaled_to_all=t_host * d / hp,
                 host_exact_outputs_equal=same, host_ess_max_rel_diff=err)
        say("host route: copy of the whole chain %.3f s + numpy / scipy model %.2f s for %d of %d parameters = %.1f s scaled to all "
            "(not run on all); median, quantiles and stop equal: %s, ESS max relative difference %.2e"
            % (t_copy, t_host, hp, d, t_host * d / hp, same, err))
    if table is not None:
        r["kernels"] = table
    line = json.dumps(r)
    say(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
