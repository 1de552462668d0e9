"""Sequential design (gpb_design_begin, gpb_chain_design_run) timed by HIP events at cfg 4's shape (N = 2048, d = 20, P = 10,
C = R = 4096): the set-up (cross kernels, V = L^-1 K*^T twice, the S_rc product, the diagonal) and the time per pick, from the
difference of a long and a short run.  Next to them the arithmetic floors: 2 P Np R C flop for the S_rc product, and per pick one
read of S_rc (8 P Rp Cp bytes; the pending downdate writes it back as well) plus one of V_c (8 P Np Cp bytes).
Prints one line and a JSON summary line; --out FILE also writes them to a file."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _event_ms(fn, reps):
    """median and spread of fn's milliseconds between two events on the current stream"""
    import torch
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="2048,20,10,4096,4096", help="N,d,P,C,R")
    ap.add_argument("--picks", type=int, default=17, help="picks of the long run (the short one takes 1)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("gpu_design_timing: no GPU (a timing needs one)")
    import design_reference as R
    from gpbayestools_hic_amd import GPEngine
    from gpbayestools_hic_amd.engine import design_run
    N, d, P, C, Rn = (int(v) for v in args.shape.split(","))
    c = R.make_case(N, d, P, C, Rn, 3, "RBF", 1.5)
    eng = GPEngine(0)
    eng.set_data(c["X"], c["Z"], "RBF", R.ALPHA)
    eng.set_theta(c["theta"])
    eng.factor()
    Xc, Xr, w = (torch.as_tensor(c[k], device="cuda:0") for k in ("Xc", "Xr", "w"))
    begin = lambda: eng.design_begin(Xc, Xr, w, c["g"])
    begin()                                              # (the first call sizes the workspaces)
    design_run([eng], args.picks)
    t_begin, s_begin = _event_ms(begin, args.reps)
    runs = {}
    for T in (1, args.picks):
        ts = []
        for _ in range(args.reps):
            begin()
            ts.append(_event_ms(lambda: design_run([eng], T), 1)[0])
        runs[T] = float(np.median(ts))
    eng.design_end()
    eng.close()
    per_pick = (runs[args.picks] - runs[1]) / (args.picks - 1)
    Np, Cp, Rp = -(-N // 64) * 64, -(-C // 128) * 128, -(-Rn // 128) * 128
    gflop = 2.0 * P * Np * Rn * C / 1e9
    gb_s, gb_v = 8.0 * P * Rp * Cp / 1e9, 8.0 * P * Np * Cp / 1e9
    r = dict(tool="gpu_design_timing", N=N, d=d, P=P, C=C, R=Rn, begin_ms=t_begin, begin_spread=s_begin, run1_ms=runs[1],
             runT_ms=runs[args.picks], picks=args.picks, per_pick_ms=per_pick, gemm_gflop=gflop, s_rc_gb=gb_s, v_c_gb=gb_v,
             stream_gb_per_s=(2 * gb_s + gb_v) / per_pick * 1e3)
    lines = ["N=%d d=%d P=%d C=%d R=%d: set-up %.2f ms (spread %.1f %%; the S_rc product alone is %.0f GF), first pick %.3f ms, "
             "each further pick %.3f ms (S_rc %.2f GB read and written back, V_c %.2f GB read: %.0f GB/s)"
             % (N, d, P, C, Rn, t_begin, 100 * s_begin, gflop, runs[1], per_pick, gb_s, gb_v, r["stream_gb_per_s"]), json.dumps(r)]
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
