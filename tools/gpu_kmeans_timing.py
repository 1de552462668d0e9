"""gpb_chain_kmeans timed at the shape of a production chain (default nsteps = 2000, nwalkers = 4096, ndim = 20 — the shape
gpb_mcmc_diag and gpb_chain_marginals are timed at), k = 10 clusters, n_init = 10 restarts in lock-step, layout "steps", on a
synthetic chain generated on the device (a mixture of 2 k Gaussians, every column with its own offset and scale).
  floor          one device copy of the chain (x.clone(), HIP events, median of --reps): what a streaming pass costs at least
  Lloyd pass     the call stopped after 1 and after 1 + --iters iterations from the same given centres (tol = 0; wall clock
                 around the synchronising call, median of --reps): the difference / --iters is one iteration of all restarts
                 together — an assignment pass and the centre update; as a multiple of the floor
  whole call     seeded (k-means++ from u, 10 passes) and run to convergence (max_iter = 300, tol = 1e-4): once
  sklearn        KMeans(init=C0_r, n_init=1, algorithm="lloyd") for every restart's starting centres on the host's CPUs, on the
                 first --sk-rows rows of the standardised chain (default 200 000; --sk-full: also on all rows)
No threshold is asserted.  Prints one line per measurement and a JSON summary line; --out FILE also writes them to a file."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    ap.add_argument("--nsteps", type=int, default=2000)
    ap.add_argument("--nwalkers", type=int, default=4096)
    ap.add_argument("--ndim", type=int, default=20)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--n-init", type=int, default=10)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sk-rows", type=int, default=200000)
    ap.add_argument("--sk-full", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("gpu_kmeans_timing: no GPU (a timing needs one)")
    from gpbayestools_hic_amd import GPEngine
    n, nw, d, k, R = a.nsteps, a.nwalkers, a.ndim, a.k, a.n_init
    S = n * nw
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    rng = np.random.default_rng(5)
    eng = GPEngine(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    modes = torch.as_tensor(2.0 * rng.standard_normal((2 * k, d)), device=dev)
    x = torch.randn((n, nw, d), dtype=torch.float64, device=dev, generator=g)
    x += modes[torch.randint(0, 2 * k, (n, nw), device=dev, generator=g)]
    x = x * torch.as_tensor(np.exp(rng.uniform(-2.0, 2.0, d)), device=dev) + torch.as_tensor(rng.uniform(-5.0, 5.0, d), device=dev)
    r = dict(tool="gpu_kmeans_timing", nsteps=n, nwalkers=nw, ndim=d, k=k, n_init=R, iters=a.iters, reps=a.reps)

    for _ in range(2):
        x.clone()
    torch.cuda.synchronize()
    ts = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        x.clone()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    r["floor_copy_ms"] = float(np.median(ts))
    say("floor: one device copy of the chain (%.2f GB read + written) %.3f ms = %.0f GB/s read"
        % (8e-9 * S * d, r["floor_copy_ms"], 8.0 * S * d / r["floor_copy_ms"] / 1e6))

    rows = x.reshape(S, d)[torch.as_tensor(rng.choice(S, R * k, replace=False), device=dev)].cpu().numpy()
    init = rows.reshape(R, k, d)
    eng.chain_kmeans(x, "steps", k, R, init=init, max_iter=1, tol=0.0)                                      # (warm-up: the workspace)
    t1, s1, o1 = _wall(lambda: eng.chain_kmeans(x, "steps", k, R, init=init, max_iter=1, tol=0.0), a.reps)
    t2, s2, o2 = _wall(lambda: eng.chain_kmeans(x, "steps", k, R, init=init, max_iter=1 + a.iters, tol=0.0), a.reps)
    full = bool(np.all(o2["n_iter"] == 1 + a.iters))
    r.update(call_1_iter_ms=t1, call_1_iter_spread=s1, call_n_iter_ms=t2, call_n_iter_spread=s2, all_restarts_ran_every_iteration=full,
             lloyd_iter_ms=(t2 - t1) / a.iters, lloyd_iter_over_floor=(t2 - t1) / a.iters / r["floor_copy_ms"])
    say("Lloyd: call with max_iter = 1 %.2f ms (spread %.1f %%), with max_iter = %d %.2f ms (%.1f %%), every restart ran every "
        "iteration: %s -> one iteration of all %d restarts %.3f ms = %.1f x the floor (%.1f centre distances per ns)"
        % (t1, 100 * s1, 1 + a.iters, t2, 100 * s2, full, R, r["lloyd_iter_ms"], r["lloyd_iter_over_floor"],
           S * R * k / (r["lloyd_iter_ms"] * 1e6)))

    u = np.random.default_rng(42).random((R, k))
    tw, _, ow = _wall(lambda: eng.chain_kmeans(x, "steps", k, R, u=u, max_iter=300, tol=1e-4), 1)
    r.update(whole_call_ms=tw, whole_call_n_iter=ow["n_iter"].tolist(), whole_call_converged=ow["converged"].tolist(),
             whole_call_best=ow["best"], whole_call_inertia=ow["inertia"].tolist())
    say("whole call: k-means++ seeding from u + Lloyd to convergence (max_iter = 300, tol = 1e-4): %.1f ms; n_iter %s, converged %s, "
        "best restart %d" % (tw, ow["n_iter"].tolist(), ow["converged"].tolist(), ow["best"]))

    if not a.no_host:
        try:
            from sklearn.cluster import KMeans
        except Exception as e:                      # the measurement is then absent, and says so
            say("sklearn: not importable on this machine (%s): no host time" % type(e).__name__)
            KMeans = None
        if KMeans is not None:
            mean, scale = o1["mean"], o1["scale"]
            C0 = (init - mean) / scale
            for nrows in [min(a.sk_rows, S)] + ([S] if a.sk_full and a.sk_rows < S else []):
                z = (x.reshape(S, d)[:nrows].cpu().numpy() - mean) / scale
                t0 = time.perf_counter()
                its = []
                for c0 in C0:
                    its.append(int(KMeans(n_clusters=k, init=c0, n_init=1, algorithm="lloyd", tol=1e-4, max_iter=300).fit(z).n_iter_))
                th = time.perf_counter() - t0
                td, _, od = _wall(lambda: eng.chain_kmeans(x.reshape(S, d)[:nrows][:, None, :], "steps", k, R, init=init, max_iter=300,
                                                           tol=1e-4, standardize=True), 1)
                r["sklearn_%d" % nrows] = dict(rows=nrows, host_s=th, host_n_iter=its, device_ms=td, device_n_iter=od["n_iter"].tolist(),
                                               cpus=os.cpu_count())
                say("sklearn, %d rows, the %d restarts one after the other from the same centres: %.2f s (n_iter %s); the device call "
                    "on the same rows %.1f ms (n_iter %s; its own moments, so the iterations need not agree)"
                    % (nrows, R, th, its, td, od["n_iter"].tolist()))
    line = json.dumps(r)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n" + line + "\n")


if __name__ == "__main__":
    main()
