"""gpb_chain_curves timed at the shape of a production chain (default nsteps = 2000, nwalkers = 4096, ndim = 20 — the shape
gpb_chain_marginals and gpb_mcmc_diag are timed at): the three default curves (zeta/s, eta/s, y_loss on their 100-point grids) at
the seven levels of the median and the 68 / 95 / 99.7 % bands, layout "steps", on a synthetic chain generated on the device (uniform
over a box: a broad posterior; and a Gaussian of 1 / 50 of the box: a converged one, whose keys share their leading digits).
  fused          gpb_chain_curves(order): the select that evaluates the curves again in every pass and stores none of them
  materialising  what the library's other pieces allow: per curve a [100, S] array built row by row with torch (the same
                 arithmetic, nothing fused), then gpb_ppd_summary(order) on it
  memory         device memory each route takes while it runs: the drop of the device's free memory (hipMemGetInfo) from before the
                 first call to the lowest value seen after a call, the arrays the route holds included; for the fused route first at a
                 tenth of the steps, then at all of them — the workspace does not grow with S
  trace, delta   gpb_chain_trace_hist (B = 30) and curves.closure_delta on the same chain
Device times: HIP events around asynchronous calls (on_device outputs), median of --reps after --warmup untimed calls.  Prints
one line per measurement and a JSON summary line; --out FILE also writes them to a file."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def _free():
    import torch
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def _torch_row(fn, p, g):
    """one grid point's values [S] with torch, the operations of csrc/curve_fn.h one by one"""
    import torch
    if fn == 0:
        s = torch.where(g < p[1], p[3], p[2])
        dt = g - p[1]
        return p[0] * torch.exp(-(dt * dt) / (2.0 * (s * s)))
    if fn == 1:
        if 0.0 <= g <= 0.2:
            return p[0] + (p[1] - p[0]) * (g / 0.2)
        if 0.2 < g < 0.4:
            return p[1] + (p[2] - p[1]) * ((g - 0.2) / 0.2)
        return p[2].clone()
    if 0.0 <= g <= 2.0:
        return p[0] * (g / 2.0)
    if 2.0 < g < 4.0:
        return p[0] + (p[1] - p[0]) * ((g - 2.0) / 2.0)
    return p[1] + (p[2] - p[1]) * ((g - 4.0) / 2.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nsteps", type=int, default=2000)
    ap.add_argument("--nwalkers", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-materialise", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("gpu_curves_timing: no GPU (a timing needs one)")
    from gpbayestools_hic_amd import GPEngine
    from gpbayestools_hic_amd import curves as C
    n, nw, d = a.nsteps, a.nwalkers, 20
    S = n * nw
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    eng = GPEngine(0)
    names = ("zeta_over_s", "eta_over_s", "y_loss")
    desc = [[C.CURVES[nm]["fn"]] + list(C.CURVES[nm]["columns"]) + [-1] * (4 - len(C.CURVES[nm]["columns"])) for nm in names]
    grid = np.stack([C.CURVES[nm]["grid"] for nm in names])
    _, q = C._levels_q(C.DEFAULT_LEVELS)
    lo, hi = np.full(d, 0.05), np.full(d, 0.45)
    hi[2:5] = 2.5
    lo_t, hi_t = torch.as_tensor(lo, device=dev), torch.as_tensor(hi, device=dev)
    r = dict(tool="gpu_curves_timing", nsteps=n, nwalkers=nw, ndim=d, samples=S, curves=len(names), grid=int(grid.shape[1]),
             levels=int(q.shape[0]), reps=a.reps, warmup=a.warmup, chains={})
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    R, nr = grid.size, 2 * q.shape[0]
    ws_bytes = 8 * (R + 3 * R * nr) + 4 * (R * nr * 256 + R * nr + R + 5 * len(names))
    r["workspace_bytes_by_layout"] = ws_bytes
    say("workspace by its layout (grid, prefixes, ranks, digit tables): %.2f MB for %d rows x %d ranks, whatever S" % (ws_bytes / 1e6, R, nr))
    for kind in ("broad", "concentrated"):
        if kind == "broad":
            x = lo_t + (hi_t - lo_t) * torch.rand((n, nw, d), dtype=torch.float64, device=dev, generator=gen)
        else:
            x = 0.5 * (lo_t + hi_t) + (hi_t - lo_t) / 50.0 * torch.randn((n, nw, d), dtype=torch.float64, device=dev, generator=gen)
        c = {}
        if kind == "broad":
            # memory of the fused route: a fresh call at a tenth of the steps sizes the workspace, the whole chain adds nothing
            f0 = _free()
            eng.chain_curves(x[: max(n // 10, 1)], "steps", desc, grid, q, on_device=True)
            f1 = _free()
            out = eng.chain_curves(x, "steps", desc, grid, q, on_device=True)
            f2 = _free()
            del out
            c["fused_memory_bytes_tenth"], c["fused_memory_bytes_full"] = f0 - f1, f0 - f2
            say("fused route, device memory taken: %.2f MB at S = %d, %.2f MB at S = %d (the chain itself: %.0f MB)"
                % ((f0 - f1) / 1e6, max(n // 10, 1) * nw, (f0 - f2) / 1e6, S, 8.0 * S * d / 1e6))
        c["floor_sum_ms"], _ = _events(lambda: x.sum(), a.reps, a.warmup)
        fused = lambda: eng.chain_curves(x, "steps", desc, grid, q, on_device=True)                 # noqa: E731
        c["fused_ms"], c["fused_spread"] = _events(fused, a.reps, a.warmup)
        evals = 8.0 * S * grid.size
        say("%s chain: x.sum() %.3f ms; fused select of %d curves x %d grid points x %d levels over %d samples: %.2f ms (spread %.1f %%) "
            "= %.1f curve evaluations per ns" % (kind, c["floor_sum_ms"], len(names), grid.shape[1], q.shape[0], S, c["fused_ms"],
                                                  100 * c["fused_spread"], evals / (c["fused_ms"] * 1e6)))
        order = eng.chain_curves(x, "steps", desc, grid, q)["order"]
        c["trace_hist_ms"], _ = _events(lambda: eng.chain_trace_hist(x, "steps", np.stack([np.linspace(lo[j], hi[j], 31) for j in range(d)]),
                                                                     on_device=True), a.reps, a.warmup)
        say("%s chain: trace histogram [20, %d, 30]: %.3f ms" % (kind, n, c["trace_hist_ms"]))
        if kind == "broad":
            import time
            truth = 0.5 * (lo + hi) + 0.01
            C.closure_delta(x, truth, np.stack([lo, hi], axis=1))
            t0 = time.perf_counter()
            cd = C.closure_delta(x, truth, np.stack([lo, hi], axis=1))
            c["closure_delta_s"] = time.perf_counter() - t0
            say("broad chain: closure_delta (distances, mean, quantiles, histogram, per-parameter shares): %.3f s wall, delta = %.6g"
                % (c["closure_delta_s"], cd.delta))
        if not a.no_materialise:
            f0 = _free()
            low = f0
            tb, ts_, equal = 0.0, 0.0, True
            for ci, nm in enumerate(names):
                cols = C.CURVES[nm]["columns"]
                p = [x[:, :, col].reshape(S) for col in cols]
                vals = torch.empty((grid.shape[1], S), dtype=torch.float64, device=dev)

                def build():
                    for gi in range(grid.shape[1]):
                        vals[gi] = _torch_row(desc[ci][0], p, float(grid[ci, gi]))
                ms_b, _ = _events(build, max(a.reps // 2, 1), 1)
                ms_s, _ = _events(lambda: eng.ppd_summary(vals, None, q, on_device=True, outputs=("order",)), max(a.reps // 2, 1), 1)
                low = min(low, _free())
                got = eng.ppd_summary(vals, None, q, outputs=("order",))["order"]
                same = bool(np.array_equal(got, order[ci])) if desc[ci][0] != 0 else bool(np.allclose(got, order[ci], rtol=2.0 ** -49, atol=1e-300))
                equal &= same
                tb, ts_ = tb + ms_b, ts_ + ms_s
                say("%s chain, materialising route, %s: build [%d, %d] %.1f ms + gpb_ppd_summary(order) %.1f ms; order statistics %s the fused ones"
                    % (kind, nm, grid.shape[1], S, ms_b, ms_s, ("equal" if desc[ci][0] else "within 2^-49 of") if same else "DIFFER from"))
                del vals, p
            torch.cuda.empty_cache()
            c.update(materialise_build_ms=tb, materialise_select_ms=ts_, materialise_ms=tb + ts_, materialise_memory_bytes=f0 - low,
                     materialise_agrees=equal, fused_speedup=(tb + ts_) / c["fused_ms"])
            say("%s chain: materialising route %.1f ms (build %.1f + select %.1f), %.0f MB of device memory at its peak (one curve at a time); "
                "fused %.2f ms: %.1fx" % (kind, tb + ts_, tb, ts_, (f0 - low) / 1e6, c["fused_ms"], c["fused_speedup"]))
        r["chains"][kind] = c
        del x
        torch.cuda.empty_cache()
    line = json.dumps(r)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n" + line + "\n")


if __name__ == "__main__":
    main()
