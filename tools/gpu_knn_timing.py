"""gpb_chain_knn timed at the shape of a production chain (default nsteps = 2000, nwalkers = 4096, ndim = 20 — the shape
gpb_mcmc_diag, gpb_chain_marginals and gpb_chain_kmeans are timed at) thinned to about 10^5 rows, read as the strided view
chain[::thin] where it lies, kmax = 8, on synthetic chains generated on the device (a Gaussian posterior inside the unit box,
every column with its own width; the second chain shifted by 0.3 of the width).
  the call       self mode (the neighbours of every row within the chain) and cross mode (in the second chain): wall clock around
                 the synchronising call with the results left on the device, median of --reps after a warm-up.  The call is the
                 scaled copies, the main kernel over all nA nB pairs and the merge of the partial lists.
  the rate       3 operations (a subtraction, a multiplication, an addition — nothing is fused) per coordinate pair, nA nB d pairs,
                 over the call's time, as a share of the 78.6 TF/s fp64 vector peak, which counts a fused multiply-add as two
                 operations: a stream of unfused operations can reach half of it.  The call's time stands for the kernel's: the
                 scaled copies and the merge touch nA (d + splits kmax) numbers, the main kernel nA nB d.
  the host       scipy.spatial.cKDTree on the same scaled rows: the tree built on all rows, query(k) timed on as many rows as
                 finish in about --host-seconds, with --workers threads, and EXTRAPOLATED linearly to all rows.
  the estimate   information_gain and posterior_divergence on the same views, whole (histograms included), once each.
No threshold is asserted.  Prints one line per measurement and a JSON summary line; --out FILE also writes them to a file."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

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
    ap.add_argument("--nsteps", type=int, default=2000)
    ap.add_argument("--nwalkers", type=int, default=4096)
    ap.add_argument("--ndim", type=int, default=20)
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-seconds", type=float, default=60.0)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("gpu_knn_timing: no GPU (a timing needs one)")
    from gpbayestools_hic_amd import GPEngine, divergence
    n, nw, d, k = a.nsteps, a.nwalkers, a.ndim, a.k
    thin = max(1, int(round(n * nw / float(a.rows))))
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    rng = np.random.default_rng(5)
    eng = GPEngine(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    width = torch.as_tensor(0.02 * np.exp(rng.uniform(-1.0, 1.0, d)), device=dev)
    xa = 0.5 + width * torch.randn((n, nw, d), dtype=torch.float64, device=dev, generator=g)
    xb = 0.5 + width * (0.3 + torch.randn((n, nw, d), dtype=torch.float64, device=dev, generator=g))
    va, vb = xa[::thin], xb[::thin]
    nA = int(va.shape[0]) * nw
    lo, hi = np.zeros(d), np.ones(d)
    inv = 1.0 / (hi - lo)
    r = dict(tool="gpu_knn_timing", nsteps=n, nwalkers=nw, ndim=d, thin=thin, rows=nA, k=k, reps=a.reps)
    say("chain [%d, %d, %d] read as chain[::%d]: %d rows of %d parameters, kmax = %d" % (n, nw, d, thin, nA, d, k))

    ops = 3.0 * nA * nA * d
    for name, b in (("self", None), ("cross", vb)):
        kw = dict(k=k, inv_scale=inv, on_device=True, return_index=False)
        eng.chain_knn(va, "steps", b, "steps", **kw)                                                   # (warm-up: the workspace)
        t, s, out = _wall(lambda: eng.chain_knn(va, "steps", b, "steps", **kw), a.reps)
        dup = float((out["zeros"] > 0).double().mean())
        r[name] = dict(call_ms=t, spread=s, ops_per_s=ops / (t * 1e-3), share_of_fp64_vector_peak=ops / (t * 1e-3) / PEAK_FP64_VECTOR,
                       n_skipped=list(out["n_skipped"]), duplicate_fraction=dup)
        say("%s mode: the call %.2f ms (spread %.1f %%): %.3g coordinate pairs, 3 operations each = %.2f T operations/s = %.3f of the "
            "78.6 TF/s fp64 vector peak (%.3f of the half of it that unfused operations can reach)"
            % (name, t, 100 * s, ops / 3.0, ops / (t * 1e-3) / 1e12, r[name]["share_of_fp64_vector_peak"],
               2.0 * r[name]["share_of_fp64_vector_peak"]))

    t, _, ig = _wall(lambda: divergence.information_gain(va, lo, hi, k=k, eng=eng), 1)
    r["information_gain"] = dict(ms=t, gain_nats=ig.gain_nats.tolist(), gain_1d_nats_sum=float(ig.gain_1d_nats.sum()))
    say("information_gain on the view, whole (histograms, the results copied to the host, the host sums): %.1f ms; gain for k = 1 .. %d: "
        "%s nats; the sum of the per-parameter gains %.3f nats" % (t, k, " ".join("%.3f" % v for v in ig.gain_nats), ig.gain_1d_nats.sum()))
    t, _, pc = _wall(lambda: divergence.posterior_divergence(va, vb, lo, hi, k=k, eng=eng), 1)
    r["posterior_divergence"] = dict(ms=t, kl_ab=pc.kl_ab.tolist(), kl_ba=pc.kl_ba.tolist(), exact_kl=0.5 * d * 0.09)
    say("posterior_divergence of the two views, whole (four neighbour calls, all pair histograms, percentiles): %.1f ms; D(A||B) for "
        "k = 1 .. %d: %s nats (the closed form for these two Gaussians: %.3f)" % (t, k, " ".join("%.3f" % v for v in pc.kl_ab), 0.5 * d * 0.09))

    if not a.no_host:
        try:
            from scipy.spatial import cKDTree
        except Exception as e:                      # the measurement is then absent, and says so
            say("scipy: not importable on this machine (%s): no host time" % type(e).__name__)
            cKDTree = None
        if cKDTree is not None:
            za = va.reshape(nA, d).cpu().numpy() * inv
            zb = vb.reshape(nA, d).cpu().numpy() * inv
            dev_self = eng.chain_knn(va, "steps", k=k, inv_scale=inv)
            for name, zt, kk in (("self", za, k + 1), ("cross", zb, k)):
                t0 = time.perf_counter()
                tree = cKDTree(zt)
                tb = time.perf_counter() - t0
                done, tq, chunk = 0, 0.0, 100
                budget = 0.5 * a.host_seconds
                while done < nA and tq < budget:
                    q = za[done:done + chunk]
                    t0 = time.perf_counter()
                    dist, idx = tree.query(q, k=kk, workers=a.workers)
                    tq += time.perf_counter() - t0
                    if name == "self" and done == 0:          # the same neighbours as the device's, on the first rows
                        same = bool(np.array_equal(idx[:, 1:], dev_self["idx"][:chunk]))
                        r["host_neighbours_agree"] = same
                    done += q.shape[0]
                    chunk = min(2 * chunk, 20000)
                total = tb + tq * nA / done
                r["ckdtree_" + name] = dict(rows_timed=done, build_s=tb, query_s=tq, extrapolated_s=total, workers=a.workers,
                                            extrapolated=done < nA)
                say("cKDTree, %s mode: tree of %d rows built in %.2f s; query(k = %d, workers = %d) of %d rows %.2f s -> %s %.1f s for "
                    "all %d rows (%.0f x the device call)"
                    % (name, nA, tb, kk, a.workers, done, tq, "EXTRAPOLATED linearly to" if done < nA else "measured:", total, nA,
                       total / (r[name]["call_ms"] * 1e-3)))
            say("the device's neighbours of the first rows are cKDTree's: %s" % r.get("host_neighbours_agree"))
    line = json.dumps(r)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n" + line + "\n")


if __name__ == "__main__":
    main()
