"""design.maxpro_design timed with its default schedule at the reference's design sizes, (npoints, ndim) = (500, 15) and
(1000, 20) by default: the wall time of the whole call (starts drawn on the host, the annealing of all restarts on the device,
the run order), the proposals consumed per second over all restarts, and ln psi of every restart's start and result.  Beside
it the host model of tests/maxpro_reference.py on the CPU of the same host at the same shapes and temperatures, one restart over
a shortened budget (--host-blocks blocks per stage): its proposals per second.  R's MaxPro package, which the reference calls,
is not available to time.  The tool ends itself after --timeout seconds.  No threshold is asserted.  Prints one line per
measurement and a JSON summary line; --out FILE also writes them to a file."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="500x15,1000x20")
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--host-blocks", type=int, default=8)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--timeout", type=int, default=300, help="seconds after which the tool gives up (0: no limit)")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.timeout > 0:                                                # its own limit: a run that hangs ends here, not at the caller's
        import signal
        signal.signal(signal.SIGALRM, lambda *_: sys.exit("gpu_maxpro_timing: gave up after %d s" % a.timeout))
        signal.alarm(a.timeout)
    import torch
    if not torch.cuda.is_available():
        sys.exit("gpu_maxpro_timing: no GPU (a timing needs one)")
    from gpbayestools_hic_amd import GPEngine
    from gpbayestools_hic_amd import design as D
    eng = GPEngine(0)
    lines, results = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    D.maxpro_design(16, 3, 1, eng=eng)                               # (warm-up: the library, the kernels)
    for shape in a.shapes.split(","):
        n, d = (int(v) for v in shape.split("x"))
        cfg = dict(D.DEFAULTS)
        bps = max(1, -(-cfg["proposals_per_cell"] * n * d // (cfg["block"] * cfg["n_stages"])))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = D.maxpro_design(n, d, a.seed, eng=eng)
        wall = time.perf_counter() - t0
        cons, acc = int(res.consumed.sum()), int(res.accepted.sum())
        r = dict(npoints=n, ndim=d, schedule=dict(cfg, blocks_per_stage=bps), wall_s=wall, consumed=cons, accepted=acc,
                 proposals_per_s=cons / wall, lnpsi_start=[float(v) for v in res.lnpsi_start], lnpsi=[float(v) for v in res.lnpsi],
                 best=int(res.best))
        say("%d x %d, %d restarts, %d stages x %d blocks of %d, temp %g x %g^k: %.3f s for the whole call; %d proposals consumed "
            "(%d accepted) = %.3g per second; ln psi %s -> %s, best restart %d"
            % (n, d, cfg["n_restarts"], cfg["n_stages"], bps, cfg["block"], cfg["temp0"], cfg["cool"], wall, cons, acc, cons / wall,
               ["%.4f" % v for v in res.lnpsi_start], ["%.4f" % v for v in res.lnpsi], res.best))
        if not a.no_host:
            import maxpro_reference as M
            start = M.random_starts(a.seed, 1, n, d)[0]
            t0 = time.perf_counter()
            m = M.anneal(start, a.seed, 0, cfg["n_stages"], a.host_blocks, cfg["block"], cfg["temp0"], cfg["cool"])
            host = time.perf_counter() - t0
            r["host_model"] = dict(blocks_per_stage=a.host_blocks, wall_s=host, consumed=int(m["consumed"]),
                                   proposals_per_s=m["consumed"] / host, cpus=os.cpu_count())
            say("    the host model (numpy, one restart, %d blocks per stage): %d proposals in %.2f s = %.3g per second; the device "
                "call: %.0f times that" % (a.host_blocks, m["consumed"], host, m["consumed"] / host, cons / wall / (m["consumed"] / host)))
        results.append(r)
    say(json.dumps(dict(tool="gpu_maxpro_timing", seed=a.seed, results=results)))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
