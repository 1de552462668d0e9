"""SMC sampler (gpb_chain_smc_reweight / gpb_chain_smc_move) per move step and per reweight call at N = 4096 and 8192
particles, for the analysis notebook's shape (nine synthetic N = 1000 emulators) and cfg 5, against the same algorithm driven
from Python on the public calls: one Chain.log_likelihood(X, finite=True) per step plus numpy for the rest
(tests/smc_reference.py) — what a pocoMC-style host sampler costs here.  The share of a resident step that is the chain
evaluation comes from timing gpb_chain_logpost alone on the same rows.
--trace: run a few move steps only (the program of a `rocprofv3 --kernel-trace --stats -- python tools/gpu_smc_timing.py
--trace ...` run, whose kernel count divided by the steps gives the launches per step; --launches does that by itself in a
fresh child process).  Prints one line per case and a JSON summary line; --out FILE
also writes the results to a file."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _ms(fn, reps=5, window_ms=20.0):
    """(median, spread) of the milliseconds per call over `reps` timed windows; a window repeats the call until it holds at
    least window_ms of work (counted in a first pass), so that the host clock and the synchronisation are a small part of it;
    spread = (max - min) / median of the windows"""
    import torch
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    once = 1e3 * (time.perf_counter() - t0)
    n = int(min(max(np.ceil(window_ms / max(once, 1e-3)), 1), 1000))
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0) / n)
    med = float(np.median(ts))
    return med, float((max(ts) - min(ts)) / med)


def _chain(name):
    from gpbayestools_hic_amd.workload import build_chain, build_multi_chain
    if name == "notebook":
        chain, _, info = build_multi_chain([(1000, 60, 10, "RBF")] * 9, 15)
    else:
        chain, _, info = build_chain(5)
    return chain


def _sampler(chain, N):
    from gpbayestools_hic_amd.smc import SMCSampler
    s = SMCSampler(chain, N, 0.5, 1)
    s.init_uniform()
    s.reweight()
    s.read_block()
    return s


def case(name, chain, N, steps):
    import smc_reference as R
    s = _sampler(chain, N)
    (t_move, sp_move) = _ms(lambda: s.move(steps))
    t_move /= steps
    t_eval, sp_eval = _ms(lambda: chain.log_prob_device(s.x, outside=-1e300))
    # (a reweighting of particles that the last one resampled: the same kernels and sizes, beta moves on towards 1)
    t_rw, sp_rw = _ms(s.reweight)
    # the host-driven comparison: the restatement's step on numpy draws, one log_likelihood call per step
    st = s.state()
    rng = np.random.default_rng(0)
    f = lambda X: chain.log_likelihood(X, finite=True)          # noqa: E731

    def host_step():
        R.move_step(st["x"], st["logl"], st["beta"], st["log_sigma"], st["Lc"], 0, rng.standard_normal((N, s.d)),
                    np.log(rng.uniform(size=N)), f)
    t_host, sp_host = _ms(host_step)
    t_host_rw, sp_host_rw = _ms(lambda: (R.resample(R.reweight(st["logl"], 0.0, 0.5)["w"], 0.5), R.precondition(st["x"])))
    r = dict(case=name, particles=N, d=s.d, ms_per_move_step=round(t_move, 4), eval_ms=round(t_eval, 4),
             eval_share=round(t_eval / t_move, 3), ms_per_reweight=round(t_rw, 4), host_ms_per_move_step=round(t_host, 4),
             host_ms_per_reweight=round(t_host_rw, 4),
             spread=dict(move=round(sp_move, 3), eval=round(sp_eval, 3), reweight=round(sp_rw, 3), host_move=round(sp_host, 3),
                         host_reweight=round(sp_host_rw, 3)))
    print("%-9s N %5d d %3d   resident %.4f ms/step (spread %.0f %%; evaluation alone %.4f ms = %.0f %%, spread %.0f %%), "
          "reweight %.4f ms (spread %.0f %%)   |   host-driven %.4f ms/step (spread %.0f %%), reweight %.4f ms (spread %.0f %%)"
          % (name, N, s.d, t_move, 100 * sp_move, t_eval, 100 * t_eval / t_move, 100 * sp_eval, t_rw, 100 * sp_rw, t_host,
             100 * sp_host, t_host_rw, 100 * sp_host_rw))
    return r


def launches(name, N, steps):
    """kernel launches per move step from a rocprofv3 kernel trace of a fresh child process"""
    out = tempfile.mkdtemp(prefix="gpb_smc_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable,
           os.path.abspath(__file__), "--trace", "--only", name, "--particles", str(N), "--steps", str(steps)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    if r.returncode != 0:
        raise RuntimeError("rocprofv3 failed:\n" + r.stdout.decode()[-2000:])
    rows = []
    for fn in glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True):
        with open(fn) as f:
            rows += list(csv.DictReader(f))
    # the window: every launch from the first proposal of the last `steps` steps to the last accept
    srt = sorted(rows, key=lambda q: int(q["Start_Timestamp"]))
    prop = [i for i, row in enumerate(srt) if "k_smc_propose" in row["Kernel_Name"]]
    last = max(i for i, row in enumerate(srt) if "k_smc_accept" in row["Kernel_Name"])
    first = prop[-steps]
    return (last - first + 1) / float(steps), len(prop)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--only", default="", help="comma list of cases (notebook, cfg5)")
    ap.add_argument("--particles", default="4096,8192")
    ap.add_argument("--trace", action="store_true", help="a few move steps only (the program of a kernel-trace run)")
    ap.add_argument("--launches", action="store_true", help="count launches per step with rocprofv3 in a child process")
    ap.add_argument("--out", default="", help="also write the lines to this file (the profile to keep)")
    a = ap.parse_args()
    only = a.only.split(",") if a.only else ["notebook", "cfg5"]
    Ns = [int(v) for v in a.particles.split(",")]
    if a.trace:
        import torch
        chain = _chain(only[0])
        s = _sampler(chain, Ns[0])
        s.move(a.steps)
        torch.cuda.synchronize()
        s.move(a.steps)
        torch.cuda.synchronize()
        return
    res = []
    for name in only:
        chain = _chain(name)
        for N in Ns:
            r = case(name, chain, N, a.steps)
            res.append(r)
    if a.launches:
        for name in only:
            per, _ = launches(name, Ns[0], 5)
            print("%-9s N %5d   %.1f launches per move step (kernel trace)" % (name, Ns[0], per))
            res.append(dict(case=name, particles=Ns[0], launches_per_step=round(per, 1)))
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write("tools/gpu_smc_timing.py --steps %d --particles %s%s\n" % (a.steps, a.particles, " --launches" if a.launches else ""))
            f.write("median of 5 windows of >= 20 ms each, spread = (max - min) / median\n")
            f.write("\n".join(json.dumps(r) for r in res) + "\n")


if __name__ == "__main__":
    main()
