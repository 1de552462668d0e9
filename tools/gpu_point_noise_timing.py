"""Fit at fixed theta (gpb_gp_factor) and the K build alone at the shapes of bench.py --full's fit_fixed_theta lines (N = 1024 /
2048 / 4096, P = 10), without and with a per-point noise array installed (gpb_gp_set_point_noise): one JSON line per process.

    python tools/gpu_point_noise_timing.py [--noise] [--lib PATH]

--lib PATH times another build of libgpbayes.so (e.g. the parent commit's, which has no gpb_gp_set_point_noise: --noise is
refused with it).  For an A/B comparison alternate the two libraries in fresh processes (DESIGN.md section 16,
profiles/r15_point_noise_fit_timing.txt).  Host clock around groups of synchronised calls, median of three groups, after a
50 ms pre-heat."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

NEW_ENTRY_POINTS = ("gpb_gp_set_point_noise", "gpb_design_set_noise")


def timed(fn, reps, sync):
    fn(); sync()
    t = time.perf_counter()
    while time.perf_counter() - t < 0.05:
        fn()
    sync()
    groups = []
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        sync()
        groups.append((time.perf_counter() - t0) / reps)
    return sorted(groups)[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--noise", action="store_true", help="install a log-uniform [1e-4, 0.3] noise array before the fit")
    ap.add_argument("--lib", default=None, help="path of another libgpbayes.so to time")
    args = ap.parse_args()
    from gpbayestools_hic_amd import _native
    if args.lib:
        import ctypes
        _native.LIB_PATHS[False] = os.path.abspath(args.lib)
        probe = ctypes.CDLL(_native.LIB_PATHS[False])
        for name in NEW_ENTRY_POINTS:
            if not hasattr(probe, name):
                if args.noise:
                    sys.exit("%s has no %s: --noise needs a library with it" % (args.lib, name))
                _native.BOUNDARY.pop(name, None)
    from gpbayestools_hic_amd import GPEngine, synth
    out = {"lib": args.lib or "product", "noise": bool(args.noise)}
    for cfg in (2, 4, 5):
        c = synth.CONFIGS[cfg]
        N, d, P = c["N"], c["d"], c["P"]
        eng = GPEngine(0)
        eng.set_data(synth.lhs(N, d), np.random.default_rng(1).standard_normal((P, N)), c["kernel"], 0.1)
        if args.noise:
            eng.set_point_noise(np.exp(np.random.default_rng(2).uniform(np.log(1e-4), np.log(0.3), size=(P, N))))
        eng.set_theta(synth.fixed_theta(d, P))
        eng.factor()
        out["fit_ms_N%d" % N] = timed(eng.factor, 5, eng.sync) * 1e3
        out["kmat_ms_N%d" % N] = timed(lambda: eng.fit_piece("kmat"), 20, eng.sync) * 1e3
        eng.factor()
        eng.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
