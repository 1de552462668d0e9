"""gpb_chain_marginals timed at the shape of a production chain (default nsteps = 2000, nwalkers = 4096, ndim = 20 — cfg 4's
ensemble), all 190 pairs, layout "steps", B = 20 and B = 64, on two synthetic chains generated on the device: a broad one (uniform
over 1.2 of the box, so that some samples fall outside) and a concentrated one (a Gaussian of width 1 / 50 of the box around its
centre: what a converged posterior looks like, most samples in a few bins — the case in which the LDS atomics of a wave meet).
Device times: HIP events around asynchronous calls (on_device outputs), median of --reps after --warmup untimed calls.
  coding pass   outputs = h1, outside: the chain read once, searched, counted (no code bytes written)
  both passes   outputs = h2: the coding pass with its code bytes written + the pair pass; the pair pass is the difference to the
                coding pass (which then lacks the byte stores: an upper bound of the pair pass)
  floor         x.sum(): a plain device read of the same view
  percentiles   the transpose to [ndim, S] + gpb_ppd_summary's select for five levels
against the host route on the same machine's CPUs: the device-to-host copy, 190 np.histogram2d calls, 20 np.histogram calls and 20
np.percentile calls (--host-steps N times the host route on the first N steps only and scales it; default all).  For kernel times
proper run it under `rocprofv3 --kernel-trace --stats -- python tools/gpu_marginals_timing.py --reps 3 --no-host`.
Prints one line per measurement and a JSON summary line; --out FILE also writes them to a file."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

QS = (0.05, 0.16, 0.5, 0.84, 0.95)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nsteps", type=int, default=2000)
    ap.add_argument("--nwalkers", type=int, default=4096)
    ap.add_argument("--ndim", type=int, default=20)
    ap.add_argument("--bins", type=int, nargs="+", default=[20, 64])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--host-steps", type=int, default=0)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("gpu_marginals_timing: no GPU (a timing needs one)")
    from gpbayestools_hic_amd import GPEngine
    from gpbayestools_hic_amd.emulator import percentile_from_order
    n, nw, d = a.nsteps, a.nwalkers, a.ndim
    S = n * nw
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    eng = GPEngine(0)
    lo, hi = -np.ones(d), np.ones(d) + 0.1 * np.arange(d)
    r = dict(tool="gpu_marginals_timing", nsteps=n, nwalkers=nw, ndim=d, pairs=d * (d - 1) // 2, reps=a.reps, warmup=a.warmup, chains={})
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    mid_t = torch.as_tensor(0.5 * (lo + hi), device=dev)
    half_t = torch.as_tensor(0.5 * (hi - lo), device=dev)
    for kind in ("broad", "concentrated"):
        if kind == "broad":
            x = (torch.rand((n, nw, d), dtype=torch.float64, device=dev, generator=g) * 2.0 - 1.0) * (1.2 * half_t) + mid_t
        else:
            x = torch.randn((n, nw, d), dtype=torch.float64, device=dev, generator=g) * (2.0 * half_t / 50.0) + mid_t
        c = {}
        c["floor_sum_ms"], _ = _events(lambda: x.sum(), a.reps, a.warmup)
        say("%s chain: x.sum() %.3f ms = %.0f GB/s" % (kind, c["floor_sum_ms"], 8.0 * S * d / c["floor_sum_ms"] / 1e6))

        def pct():
            xt = x.permute(2, 0, 1).reshape(d, S).contiguous()
            return eng.ppd_summary(xt, None, QS, on_device=True, outputs=("order",))
        c["percentiles_ms"], c["percentiles_spread"] = _events(pct, max(a.reps // 2, 1), 1)
        say("%s chain: percentiles (transpose + select of %d levels) %.3f ms" % (kind, len(QS), c["percentiles_ms"]))
        for B in a.bins:
            edges = np.stack([np.linspace(lo[j], hi[j], B + 1) for j in range(d)])
            code_ms, code_sp = _events(lambda: eng.chain_marginals(x, "steps", edges, on_device=True, outputs=("h1", "outside")),
                                       a.reps, a.warmup)
            h2_ms, h2_sp = _events(lambda: eng.chain_marginals(x, "steps", edges, on_device=True, outputs=("h2",)), a.reps, a.warmup)
            all_ms, all_sp = _events(lambda: eng.chain_marginals(x, "steps", edges, on_device=True), a.reps, a.warmup)
            out = eng.chain_marginals(x, "steps", edges)
            occupied = float(np.count_nonzero(out["h2"])) / out["h2"].size
            c["B%d" % B] = dict(code_ms=code_ms, code_spread=code_sp, h2_ms=h2_ms, h2_spread=h2_sp, pairs_ms_by_difference=h2_ms - code_ms,
                                all_ms=all_ms, all_spread=all_sp, code_gbs=8.0 * S * d / code_ms / 1e6,
                                pair_updates_per_ns=S * (d * (d - 1) // 2) / ((h2_ms - code_ms) * 1e6),
                                device_route_ms=all_ms + c["percentiles_ms"], occupied_bin_share=occupied,
                                outside_share=float(out["outside"].sum()) / (S * d))
            say("%s chain, B = %d: coding pass %.3f ms (spread %.1f %%, %.0f GB/s of chain); h2 alone %.3f ms (%.1f %%) -> pair pass by "
                "difference %.3f ms = %.1f (sample, pair) updates per ns; all outputs %.3f ms (%.1f %%); %.3f of the 2-D bins occupied, "
                "%.4f of the values outside" % (kind, B, code_ms, 100 * code_sp, c["B%d" % B]["code_gbs"], h2_ms, 100 * h2_sp,
                                                 h2_ms - code_ms, c["B%d" % B]["pair_updates_per_ns"], all_ms, 100 * all_sp, occupied,
                                                 c["B%d" % B]["outside_share"]))
        if not a.no_host:
            hs = a.host_steps if 0 < a.host_steps < n else n
            scale = n / float(hs)
            t0 = time.perf_counter()
            xh = x.cpu().numpy()
            t_copy = time.perf_counter() - t0
            flat = xh[:hs].reshape(-1, d)
            B = a.bins[0]
            edges = np.stack([np.linspace(lo[j], hi[j], B + 1) for j in range(d)])
            out = eng.chain_marginals(x[:hs], "steps", edges)
            t0 = time.perf_counter()
            ok, p = True, 0
            for i in range(d):
                for j in range(i + 1, d):
                    ok &= bool(np.array_equal(np.histogram2d(flat[:, i], flat[:, j], bins=[edges[i], edges[j]])[0].astype(np.int64),
                                              out["h2"][p]))
                    p += 1
            t_h2 = time.perf_counter() - t0
            t0 = time.perf_counter()
            for j in range(d):
                ok &= bool(np.array_equal(np.histogram(flat[:, j], bins=edges[j])[0], out["h1"][j]))
            t_h1 = time.perf_counter() - t0
            t0 = time.perf_counter()
            ref = np.stack([np.percentile(flat[:, j], [100 * q for q in QS]) for j in range(d)], axis=1)
            t_pct = time.perf_counter() - t0
            xt = x[:hs].permute(2, 0, 1).reshape(d, -1).contiguous()
            mine = percentile_from_order(eng.ppd_summary(xt, None, QS, outputs=("order",))["order"], QS, flat.shape[0]).T
            ok_pct = bool(np.array_equal(mine, ref))
            host_s = t_copy + scale * (t_h2 + t_h1 + t_pct)
            c.update(host_steps=hs, host_copy_s=t_copy, host_hist2d_s=scale * t_h2, host_hist1d_s=scale * t_h1, host_percentile_s=scale * t_pct,
                     host_route_s=host_s, host_counts_equal=ok, host_percentiles_equal=ok_pct,
                     speedup={"B%d" % b: host_s / (c["B%d" % b]["device_route_ms"] * 1e-3) for b in a.bins})
            say("%s chain, host route (B = %d, %d of %d steps%s): copy %.3f s + %d histogram2d %.2f s + %d histogram %.2f s + %d percentile "
                "%.2f s = %.2f s; counts equal: %s, percentiles equal: %s; device route (all outputs + percentiles) %s"
                % (kind, B, hs, n, ", scaled" if hs < n else "", t_copy, d * (d - 1) // 2, scale * t_h2, d, scale * t_h1, d, scale * t_pct,
                   host_s, ok, ok_pct, ", ".join("B = %d: %.1f ms, %.0fx" % (b, c["B%d" % b]["device_route_ms"], c["speedup"]["B%d" % b])
                                                 for b in a.bins)))
        r["chains"][kind] = c
        del x
    r["concentrated_to_broad"] = {"B%d" % b: dict(code=r["chains"]["concentrated"]["B%d" % b]["code_ms"] / r["chains"]["broad"]["B%d" % b]["code_ms"],
                                                  pairs=r["chains"]["concentrated"]["B%d" % b]["pairs_ms_by_difference"]
                                                  / r["chains"]["broad"]["B%d" % b]["pairs_ms_by_difference"]) for b in a.bins}
    say("concentrated : broad — " + "; ".join("B = %d: coding pass %.2f, pair pass %.2f" % (b, v["code"], v["pairs"])
                                              for b, v in ((b, r["concentrated_to_broad"]["B%d" % b]) for b in a.bins)))
    line = json.dumps(r)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n" + line + "\n")


if __name__ == "__main__":
    main()
