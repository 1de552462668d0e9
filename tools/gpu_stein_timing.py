"""gpb_stein_thin and gpb_stein_ksd timed on the nine-emulator chain (nine synthetic N = 1000 emulators, 540 observables, 20
parameters): a stretch-move run of 1024 walkers, --burn steps thrown away and 100 stored = 102400 rows, their scores from
gpb_chain_logpost_grad, everything in the logit space of the prior box with the "sclmed" preconditioner of those rows.
  (a) thinning     the call at m = --m, wall clock around the synchronising call with the results left on the device, median of
                   --reps after a warm-up, per iteration; the same iteration restated in torch device operations (argmin, the
                   four sums by broadcasting, the update of obj), timed over 100 iterations; and one device copy of the three
                   packed arrays (x, b, g) for comparison: an iteration reads them once.
  (b) full KSD     the call, median of --reps; 11 operations per coordinate pair (3 subtractions, 4 multiplications, 4 additions
                   — nothing is fused) over n^2 d pairs, as a share of the 78.6 TF/s fp64 vector peak, which counts a fused
                   multiply-add as two operations.  The call's time stands for the kernel's (the other kernels touch n numbers).
  (c) the model    tests/stein_reference.py (numpy): the row sums of a subset of rows against all columns on --workers threads,
                   EXTRAPOLATED linearly to all rows; three thinning iterations on all rows.
  (d) the scores   Chain._score_device over all rows, once after a warm-up of one slab.
  (e) the use      with ONE preconditioner (the chain's) for every set: the KSD of the stretch chain, of Chain.stein_thin's picks
                   (m = 32 and 100), of posterior_clusters' 32 centres (the most gpb_chain_kmeans takes), of 32 and 100 equally
                   spaced rows, and of an HMC chain of 1024 chains with the stretch run's wall time as its budget (at least 100 warm-up +
                   100 steps: the line says when that minimum exceeds the budget).
No threshold is asserted.  Prints one line per measurement and a JSON summary line; --out FILE also writes them to a file."""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK_FP64_VECTOR = 78.6e12


def _wall(fn, reps):
    import torch
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts)), float((max(ts) - min(ts)) / np.median(ts)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=int, default=1024)
    ap.add_argument("--burn", type=int, default=400)
    ap.add_argument("--stored", type=int, default=100)
    ap.add_argument("--m", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--model-rows", type=int, default=512)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-hmc", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("gpu_stein_timing: no GPU (a timing needs one)")
    from gpbayestools_hic_amd import thinning as T
    from gpbayestools_hic_amd.sampler import StretchSampler
    from gpbayestools_hic_amd.workload import build_multi_chain
    lines, r = [], dict(tool="gpu_stein_timing", walkers=a.walkers, burn=a.burn, stored=a.stored, m=a.m, reps=a.reps)

    def say(s):
        print(s, flush=True)
        lines.append(s)
    chain, emus, info = build_multi_chain([(1000, 60, 10, "RBF")] * 9, 20)
    d, lo, hi = chain.ndim, np.asarray(chain.min), np.asarray(chain.max)
    rng = np.random.default_rng(0)
    start = np.clip(info["xstar"] + 0.03 * rng.standard_normal((a.walkers, d)), lo + 0.02, hi - 0.02)
    s = StretchSampler(chain, a.walkers, seed=1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    X = s.run(start, a.burn, store=False)
    s.reset()
    s.run(X, a.stored)
    torch.cuda.synchronize()
    t_stretch = time.perf_counter() - t0
    rows = s._chain_dev.reshape(-1, d)
    n = int(rows.shape[0])
    eng = emus[0]._engine_ready()
    say("nine-emulator chain, %s: stretch move, %d walkers, %d burn-in + %d stored steps in %.2f s: %d rows of %d parameters"
        % (torch.cuda.get_device_name(0), a.walkers, a.burn, a.stored, t_stretch, n, d))

    # (d) the scores
    chain._score_device(rows[:1024])
    t_score, _, g = _wall(lambda: chain._score_device(rows), 1)
    r["score"] = dict(ms=t_score, rows=n)
    say("(d) scores: gpb_chain_logpost_grad over %d rows in slabs of %d: %.1f ms" % (n, chain.grad_slab_rows, t_score))

    _, z, gz, gamma, ginv, _ = T.prepare(rows, g, "sclmed", lo, hi, "logit")
    tr = float(np.trace(ginv))
    say("logit space, preconditioner sclmed: Gamma = %.4g I" % gamma[0, 0])

    # (a) thinning
    eng.stein_thin(z, gz, ginv, 8, on_device=True)
    t_thin, sp, out = _wall(lambda: eng.stein_thin(z, gz, ginv, a.m, on_device=True), a.reps)
    Gi = torch.as_tensor(ginv, device=z.device)
    Xp, Bp, Gp = z.contiguous(), (z @ Gi.T).contiguous(), gz.contiguous()
    obj0 = tr + (Gp * Gp).sum(1)

    def torch_iters(k):
        obj = obj0.clone()
        for _ in range(k):
            p = torch.argmin(obj)
            h = Bp - Bp[p]
            q = 1.0 + ((Xp - Xp[p]) * h).sum(1)
            t1, t3, t4 = (h * h).sum(1), ((Gp - Gp[p]) * h).sum(1), (Gp * Gp[p]).sum(1)
            i1 = 1.0 / q.sqrt()
            i2 = 1.0 / q
            i3 = i1 * i2
            obj += 2.0 * ((-3.0 * t1) * (i3 * i2) + (tr + t3) * i3 + t4 * i1)
        return obj
    torch_iters(5)
    t_torch, sp_t, _ = _wall(lambda: torch_iters(100), a.reps)
    t_copy, _, _ = _wall(lambda: [Xp.clone(), Bp.clone(), Gp.clone()], 20)
    r["thin"] = dict(call_ms=t_thin, spread=sp, us_per_iteration=1e3 * t_thin / a.m, torch_us_per_iteration=1e3 * t_torch / 100,
                     torch_spread=sp_t, copy_us=1e3 * t_copy, n_skipped=out["n_skipped"], ksd_last=float(out["ksd"][-1]))
    say("(a) thinning: gpb_stein_thin, m = %d: %.2f ms (spread %.1f %%) = %.1f us per iteration (the prepare kernel and the read-back "
        "included); the same iteration in torch device operations %.1f us (spread %.1f %%, %.1f x); one device copy of the three "
        "packed arrays (%.1f MB) %.1f us" % (a.m, t_thin, 100 * sp, 1e3 * t_thin / a.m, 1e3 * t_torch / 100, 100 * sp_t,
                                             t_torch / 100 / (t_thin / a.m), 3 * n * d * 8 / 1e6, 1e3 * t_copy))

    # (b) the full discrepancy
    eng.stein_ksd(z, gz, ginv, on_device=True)
    t_ksd, sp, full = _wall(lambda: eng.stein_ksd(z, gz, ginv, on_device=True), a.reps)
    ops = 11.0 * n * n * d
    ksd_all = float(full["ksd2"][0]) ** 0.5
    r["ksd"] = dict(call_ms=t_ksd, spread=sp, ops_per_s=ops / (t_ksd * 1e-3), share_of_fp64_vector_peak=ops / (t_ksd * 1e-3) / PEAK_FP64_VECTOR,
                    ksd=ksd_all)
    say("(b) full KSD: gpb_stein_ksd of %d rows: %.1f ms (spread %.1f %%): %.3g coordinate pairs, 11 operations each = %.2f T operations/s "
        "= %.3f of the 78.6 TF/s fp64 vector peak (gpb_chain_knn: 0.246)"
        % (n, t_ksd, 100 * sp, ops / 11.0, ops / (t_ksd * 1e-3) / 1e12, r["ksd"]["share_of_fp64_vector_peak"]))

    # (c) the numpy model
    if not a.no_host:
        import stein_reference as R
        zh, gh = z.cpu().numpy(), gz.cpu().numpy()
        sub = np.arange(a.model_rows)
        per = max(1, a.model_rows // a.workers)
        t0 = time.perf_counter()
        with ThreadPoolExecutor(a.workers) as ex:
            parts = list(ex.map(lambda i0: R.row_sums(zh, gh, ginv, rows=sub[i0:i0 + per], block=32), range(0, a.model_rows, per)))
        t_model = time.perf_counter() - t0
        same = bool(np.array_equal(np.concatenate(parts), eng.stein_ksd(z, gz, ginv, return_rows=True)["row_sum"][:a.model_rows]))
        t0 = time.perf_counter()
        mt = R.thin(zh, gh, ginv, 3)
        t_mthin = (time.perf_counter() - t0) / 3
        same_t = bool(np.array_equal(mt["idx"], out["idx"][:3].cpu().numpy()))
        r["model"] = dict(rows_timed=a.model_rows, seconds=t_model, extrapolated_s=t_model * n / a.model_rows, workers=a.workers,
                          thin_iteration_s=t_mthin, row_sums_equal=same, picks_equal=same_t)
        say("(c) numpy model, %d threads: row sums of %d rows against all columns %.1f s -> EXTRAPOLATED linearly to %.0f s for all %d rows "
            "(%.0f x the device call); one thinning iteration %.3f s (%.0f x); the device's row sums and first picks are the model's: %s, %s"
            % (a.workers, a.model_rows, t_model, t_model * n / a.model_rows, n, t_model * n / a.model_rows / (t_ksd * 1e-3), t_mthin,
               t_mthin / (1e-3 * t_thin / a.m), same, same_t))

    # (e) the use
    th = chain.stein_thin(rows, m=100, preconditioner=gamma)
    cl = chain.posterior_clusters(rows.cpu().numpy(), n_clusters=32, n_init=4)
    e = dict(stretch_chain=ksd_all, thin_32=float(th.ksd[31]), thin_100=float(th.ksd[-1]),
             clusters_32=chain.ksd(cl.centers, preconditioner=gamma).ksd,
             spaced_32=chain.ksd(rows[::n // 32][:32], preconditioner=gamma).ksd,
             spaced_100=chain.ksd(rows[::n // 100][:100], preconditioner=gamma).ksd, thin_n_skipped=th.n_skipped)
    say("(e) KSD with the chain's preconditioner: the stretch chain (all %d rows) %.4f; Chain.stein_thin's picks %.4f (m = 32) and %.4f "
        "(m = 100); posterior_clusters' 32 centres %.4f; equally spaced rows %.4f (32) and %.4f (100)"
        % (n, ksd_all, e["thin_32"], e["thin_100"], e["clusters_32"], e["spaced_32"], e["spaced_100"]))
    if not a.no_hmc:
        from gpbayestools_hic_amd.hmc import HMCSampler
        h = HMCSampler(chain, a.walkers, seed=1)
        h.set_state(start)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h.warmup(100)
        torch.cuda.synchronize()
        t_warm = time.perf_counter() - t0
        nrun = max(a.stored, int((t_stretch - t_warm) / (t_warm / 100.0)))
        thin = max(1, nrun // a.stored)
        t0 = time.perf_counter()
        h.run(nrun, thin=thin)
        torch.cuda.synchronize()
        t_hmc = t_warm + time.perf_counter() - t0
        hrows = h._chain_dev[-a.stored:].reshape(-1, d)
        e.update(hmc_chain=chain.ksd(hrows, preconditioner=gamma, return_rows=False).ksd, hmc_seconds=t_hmc, stretch_seconds=t_stretch,
                 hmc_steps=nrun, hmc_thin=thin)
        say("    an HMC chain of %d chains with the stretch run's wall time as its budget and a minimum of 100 warm-up + %d steps (%d "
            "steps, every %d-th stored, %.2f s against the stretch run's %.2f s%s): KSD of its %d rows %.4f"
            % (a.walkers, a.stored, nrun, thin, t_hmc, t_stretch, "" if t_hmc <= 1.2 * t_stretch else ": the minimum exceeds the budget, NOT equal cost",
               hrows.shape[0], e["hmc_chain"]))
    r["use"] = e
    line = json.dumps(r)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n" + line + "\n")


if __name__ == "__main__":
    main()
