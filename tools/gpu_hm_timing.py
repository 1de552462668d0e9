"""Chain.history_match timed on the nine-emulator chain of the benchmark (nine emulators of 1000 design points over 20 parameters,
540 observables) at --samples (default 1e6) candidates, B = 20 bins, all 190 parameter pairs:
  * the whole call (median of --reps calls after one untimed call, wall clock with a device synchronisation);
  * on ONE slab of candidates, from events on the stream (median of --reps): the predict pass (gpb_emu_predict_diag, emulator by
    emulator), gpb_hm_implausibility (top 2, the arg and the nine group maxima) and gpb_hm_maps, scaled to all slabs;
  * beside gpb_hm_implausibility, in the same run, a torch device copy of the same mu_T / var_T slab: the kernel reads 16 M S
    bytes and writes almost nothing, the copy moves twice that;
  * beside gpb_hm_maps, gpb_chain_marginals on the same rows, same edges, all pairs: the same passes without the 64-bit minimum
    and the second counter;
  * the numpy model of tests/hm_reference.py on --host-rows rows (the predictions taken from the device, so the model's share is
    implausibility and maps only), EXTRAPOLATED linearly to all candidates and divided by 16 (sixteen threads, taken to scale
    perfectly: rows are independent).
Prints one line per measurement and a JSON summary line; --out FILE also writes them to a file."""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _events(fn, reps, warmup=1):
    import torch
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), (max(ts) - min(ts)) / max(float(np.median(ts)), 1e-12)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1000000)
    ap.add_argument("--host-rows", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("gpu_hm_timing: no GPU (a timing needs one)")
    import hm_reference as R
    from gpbayestools_hic_amd.workload import build_multi_chain
    warnings.simplefilter("ignore")
    specs = [(1000, 60, 6 + i % 3, ("RBF", "Matern25", "RBF")[i % 3]) for i in range(9)]
    chain, emus, info = build_multi_chain(specs, 20)
    S, B, d, M = a.samples, 20, chain.ndim, chain.nobs
    dev = torch.device("cuda", chain.device)
    lines = ["chain: 9 emulators, %d observables, %d parameters; %d candidates, B = %d, %d pairs" % (M, d, S, B, d * (d - 1) // 2)]
    hm = chain.history_match(n_samples=S, bins=B, seed=1)                     # untimed: allocations at full size
    torch.cuda.synchronize()
    ts = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        hm = chain.history_match(n_samples=S, bins=B, seed=1)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    total = float(np.median(ts))
    lines.append("Chain.history_match: %.1f ms (median of %d, spread %.1f %%); %r" % (1e3 * total, a.reps, 100 * (max(ts) - min(ts)) / total, hm))

    # one slab, phase by phase
    slab = min(chain._predict_slab_rows(chain.hm_slab_rows), S)
    nslabs = S / slab
    engs = [e._engine_ready() for e in chain.emuList]
    e0 = engs[0]
    Xd = e0.hm_uniform(chain.min, chain.max, slab, seed=1)
    mu_T = torch.empty((M, slab), dtype=torch.float64, device=dev)
    var_T = torch.empty_like(mu_T)
    esd = torch.zeros((slab,), dtype=torch.float64, device=dev)
    yexp = torch.as_tensor(np.ascontiguousarray(chain.expdata[0]), device=dev)
    vadd = torch.as_tensor(np.ascontiguousarray(np.diagonal(chain.expdata_cov)), device=dev)
    ranges = np.array([(60 * i, 60 * i + 60) for i in range(9)], dtype=np.int32)
    edges = hm.edges
    t_uni, _ = _events(lambda: e0.hm_uniform(chain.min, chain.max, slab, seed=1, out=Xd), a.reps)
    t_pred, sp_pred = _events(lambda: chain._predict_diag_slab(engs, None, Xd, esd, mu_T, var_T), a.reps)
    r = e0.hm_implausibility(mu_T, var_T, yexp, vadd, ranges, 2, on_device=True)
    t_imp, sp_imp = _events(lambda: e0.hm_implausibility(mu_T, var_T, yexp, vadd, ranges, 2, bad=r["bad"], on_device=True), a.reps)
    t_imp0, _ = _events(lambda: e0.hm_implausibility(mu_T, var_T, yexp, vadd, None, 2, want_arg=False, bad=r["bad"], on_device=True), a.reps)
    mu2, var2 = torch.empty_like(mu_T), torch.empty_like(var_T)

    def copy():
        mu2.copy_(mu_T)
        var2.copy_(var_T)
    t_copy, sp_copy = _events(copy, a.reps)
    score = r["top"][1].contiguous()
    t_maps, sp_maps = _events(lambda: e0.hm_maps(Xd, score, 3.0, edges, on_device=True), a.reps)
    t_maps1, _ = _events(lambda: e0.hm_maps(Xd, score, 3.0, edges, outputs=("1d",), on_device=True), a.reps)
    x3 = Xd[:, None, :]
    t_marg, sp_marg = _events(lambda: e0.chain_marginals(x3, "steps", edges, on_device=True), a.reps)
    nbytes = 16.0 * M * slab
    lines.append("one slab of %d rows (%.2f slabs in all), events on the stream, median of %d:" % (slab, nslabs, a.reps))
    lines.append("  gpb_hm_uniform %.3f ms" % t_uni)
    lines.append("  predict (gpb_emu_predict_diag x 9) %.2f ms (spread %.1f %%) -> %.1f ms for all candidates" % (t_pred, 100 * sp_pred, t_pred * nslabs))
    lines.append("  gpb_hm_implausibility (K = 2, arg, 9 groups) %.3f ms (spread %.1f %%) = %.0f GB/s of its %.0f MB read -> %.2f ms for all; "
                 "without arg and groups %.3f ms" % (t_imp, 100 * sp_imp, nbytes / t_imp / 1e6, nbytes / 1e6, t_imp * nslabs, t_imp0))
    lines.append("  torch copy of the same mu_T, var_T slab (reads and writes %.0f MB each) %.3f ms (spread %.1f %%) = %.0f GB/s moved; "
                 "kernel / copy = %.2f" % (nbytes / 1e6, t_copy, 100 * sp_copy, 2 * nbytes / t_copy / 1e6, t_imp / t_copy))
    lines.append("  gpb_hm_maps (1-D and 190 pairs) %.3f ms (spread %.1f %%) -> %.2f ms for all; 1-D only %.3f ms" % (t_maps, 100 * sp_maps, t_maps * nslabs, t_maps1))
    lines.append("  gpb_chain_marginals on the same rows and edges %.3f ms (spread %.1f %%); gpb_hm_maps / gpb_chain_marginals = %.2f"
                 % (t_marg, 100 * sp_marg, t_maps / t_marg))
    summary = dict(samples=S, slab=slab, total_ms=1e3 * total, uniform_ms=t_uni, predict_ms=t_pred, implausibility_ms=t_imp,
                   implausibility_plain_ms=t_imp0, copy_ms=t_copy, maps_ms=t_maps, maps_1d_ms=t_maps1, marginals_ms=t_marg,
                   implausibility_gbs=nbytes / t_imp / 1e6, nroy_fraction=hm.nroy_fraction)

    # the numpy model on a subset of the slab's rows
    n = min(a.host_rows, slab)
    Xh, mu_h, var_h = Xd[:n].cpu().numpy(), mu_T[:, :n].cpu().numpy(), var_T[:, :n].cpu().numpy()
    t0 = time.perf_counter()
    ref = R.implausibility(mu_h, var_h, chain.expdata[0], np.diagonal(chain.expdata_cov), ranges, 2)
    t_hi = time.perf_counter() - t0
    t0 = time.perf_counter()
    R.maps(Xh, ref["top"][1], 3.0, edges)
    t_hm = time.perf_counter() - t0
    same = np.array_equal(ref["top"], r["top"][:, :n].cpu().numpy())
    lines.append("numpy model on %d rows (predictions from the device), EXTRAPOLATED to %d candidates: implausibility %.1f s, maps %.1f s; on "
                 "sixteen threads %.2f s against the device's %.1f ms for the same two steps; top-2 equal to the device's bit for bit: %s"
                 % (n, S, t_hi / n * S, t_hm / n * S, (t_hi + t_hm) / n * S / 16, (t_imp + t_maps) * nslabs, same))
    summary.update(host_rows=n, host_implausibility_s=t_hi / n * S, host_maps_s=t_hm / n * S)
    lines.append(json.dumps(summary))
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
