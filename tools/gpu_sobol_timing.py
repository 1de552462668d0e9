"""Closed-form Sobol indices (gpb_emu_sobol) timed at cfg 4's shape (N = 2048, d = 20, P = 10, M = 64) and at the shape of one emulator
of the nine-emulator analysis (N = 1000, d = 15, P = 7, M = 60), against
  * a Saltelli Monte-Carlo estimate with --base (default 1e5) base samples on the existing predict path: (d + 2) batches of
    emu_predict, the estimators of Saltelli et al. 2010 (first order) and Jansen 1999 (total), reduced on the device; its time and
    its largest deviation from the closed form;
  * the numpy model (tests/sobol_reference.py) at N = 256, d = 20, P = 2, with the device's time on the same shape.
Prints one line per case and a JSON summary line; --out FILE also writes them to a file."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _ms(fn, reps=5, window_ms=50.0):
    """(median, spread) of the milliseconds per call over `reps` windows of at least window_ms of work each"""
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


def _engine(N, d, P, M, seed):
    import sobol_reference as R
    from gpbayestools_hic_amd import GPEngine
    X, Z, theta, lo, hi = R.make_case(N, d, P, seed)
    rng = np.random.default_rng(seed + 50)
    A, mu = rng.standard_normal((P, M)), rng.standard_normal(M)
    eng = GPEngine(0)
    eng.set_data(X, Z, "RBF", R.ALPHA)
    eng.set_theta(theta)
    eng.factor()
    eng.set_transform(0, mu, A=A, cov_trunc=np.zeros((M, M)))
    return eng, X, theta, lo, hi, A, mu


def saltelli(eng, lo, hi, n, seed=0):
    """(first [M, d], total [M, d], seconds) from n base samples: (d + 2) n predictions"""
    import torch
    dev = torch.device("cuda", eng.device)
    g = torch.Generator(device=dev).manual_seed(seed)
    d = eng.d
    lo_t, w_t = torch.as_tensor(lo, device=dev), torch.as_tensor(hi - lo, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    Am = lo_t + w_t * torch.rand((n, d), generator=g, device=dev, dtype=torch.float64)
    Bm = lo_t + w_t * torch.rand((n, d), generator=g, device=dev, dtype=torch.float64)
    def predict(Xm, slab=16384):       # (K*^T of a batch is P x N doubles per row)
        return torch.cat([eng.emu_predict(Xm[i:i + slab], return_cov=False) for i in range(0, n, slab)])

    fA, fB = predict(Am), predict(Bm)
    V = torch.cat([fA, fB]).var(dim=0)
    first, total = [], []
    for j in range(d):
        Cm = Am.clone()
        Cm[:, j] = Bm[:, j]
        fC = predict(Cm)
        first.append((fB * (fC - fA)).mean(dim=0) / V)
        total.append(0.5 * ((fA - fC) ** 2).mean(dim=0) / V)
    first, total = torch.stack(first, dim=1).cpu().numpy(), torch.stack(total, dim=1).cpu().numpy()
    return first, total, time.perf_counter() - t0


def case(name, N, d, P, M, base):
    import torch
    eng, X, theta, lo, hi, A, mu = _engine(N, d, P, M, 3)
    ms, spread = _ms(lambda: eng.emu_sobol(lo, hi, on_device=True))
    mean, var, first, total = eng.emu_sobol(lo, hi)
    saltelli(eng, lo, hi, 1024)                                  # warm the predict path's shapes
    f_mc, t_mc, sec = saltelli(eng, lo, hi, base)
    torch.cuda.synchronize()
    eng.close()
    pairs = P * (P + 1) / 2 * N * N * d                          # pair terms with p <= q (the p = q blocks do half of theirs)
    r = dict(case=name, N=N, d=d, P=P, M=M, sobol_ms=ms, spread=spread, pair_terms=pairs, gterms_per_s=pairs / ms / 1e6,
             saltelli_base=base, saltelli_predictions=(d + 2) * base, saltelli_s=sec,
             saltelli_first_maxdev=float(np.abs(f_mc - first).max()), saltelli_total_maxdev=float(np.abs(t_mc - total).max()),
             first_sum_range=[float(first.sum(axis=1).min()), float(first.sum(axis=1).max())])
    print("%-9s N=%d d=%d P=%d M=%d: gpb_emu_sobol %.3f ms (spread %.1f %%), %.2f G pair terms/s; Saltelli %d x %d predictions "
          "%.2f s, max |first - closed form| %.2e, max |total - closed form| %.2e"
          % (name, N, d, P, M, ms, 100 * spread, r["gterms_per_s"], d + 2, base, sec, r["saltelli_first_maxdev"],
             r["saltelli_total_maxdev"]))
    return r


def numpy_case():
    import sobol_reference as R
    N, d, P, M = 256, 20, 2, 8
    eng, X, theta, lo, hi, A, mu = _engine(N, d, P, M, 5)
    ms, spread = _ms(lambda: eng.emu_sobol(lo, hi, on_device=True))
    alpha = eng.get("alpha")
    e_d, H_d = eng.sobol(lo, hi)
    eng.close()
    t0 = time.perf_counter()
    e, H, Ue, UH = R.gp_integrals(X, alpha, np.exp(theta[:, 0]), np.exp(theta[:, 1:d + 1]), lo, hi)
    sec = time.perf_counter() - t0
    ratio = float((np.abs(H_d - H) / (R.bar_factor(N, d) * UH)).max())
    print("numpy     N=%d d=%d P=%d: model %.2f s, device %.3f ms (spread %.1f %%), device / model within %.3g of the bar"
          % (N, d, P, sec, ms, 100 * spread, ratio))
    return dict(case="numpy", N=N, d=d, P=P, numpy_s=sec, sobol_ms=ms, spread=spread, ratio_to_bar=ratio)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base", type=int, default=100000)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("gpu_sobol_timing: no GPU (a timing needs one)")
    res = [case("cfg4", 2048, 20, 10, 64, a.base), case("notebook", 1000, 15, 7, 60, a.base), numpy_case()]
    line = json.dumps(dict(tool="gpu_sobol_timing", results=res))
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
