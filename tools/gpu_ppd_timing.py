"""Chain.posterior_predictive timed on the nine-emulator chain of the benchmark (nine emulators of 1000 design points over 20
parameters, 540 observables) at S = --samples (default 1e5) posterior samples drawn in a small ball around the truth point, against
  * the host route: Chain._predict (means and the [S, nobs, nobs] covariance on the host) followed by np.percentile of the means,
    at the largest S whose covariance array fits --host-gb (default 4) gigabytes — the prediction time of posterior_predictive is
    quoted against this, per sample;
  * its own pieces: the predict pass into the [nobs, S] device pair (Chain._ppd_arrays) and the two gpb_ppd_summary calls, apart.
Prints one line per measurement and a JSON summary line; --out FILE also writes them to a file."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed(fn, reps):
    """(median seconds, relative spread, last result) over reps calls after one untimed call"""
    import torch
    res = fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    med = float(np.median(ts))
    return med, float((max(ts) - min(ts)) / med), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=100000)
    ap.add_argument("--host-gb", type=float, default=4.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("gpu_ppd_timing: no GPU (a timing needs one)")
    from gpbayestools_hic_amd import synth
    from gpbayestools_hic_amd.workload import build_multi_chain
    specs = [(1000, 60, 6 + i % 3, ("RBF", "Matern25", "RBF")[i % 3]) for i in range(9)]
    chain, emus, info = build_multi_chain(specs, 20)
    S, nobs = a.samples, chain.nobs
    X = synth.walkers_ball(S, info["xstar"], 0.02)
    q = (0.05, 0.16, 0.5, 0.84, 0.95)

    t_all, sp_all, pp = _timed(lambda: chain.posterior_predictive(X, q), a.reps)
    t_pred, sp_pred, arrs = _timed(lambda: chain._ppd_arrays(X), a.reps)
    engs, mu_T, var_T = arrs
    e0 = engs[0]
    qa = np.asarray(q)
    vexp, yobs = np.diag(chain.expdata_cov), chain.expdata[0]
    t_sum, sp_sum, _ = _timed(lambda: e0.ppd_summary(mu_T, var_T, qa), a.reps)
    t_pit, sp_pit, _ = _timed(lambda: e0.ppd_summary(mu_T, var_T, qa, vadd=vexp, yobs=yobs, outputs=("pit",)), a.reps)
    parts = {}
    for k in ("moments", "order", "mixq"):
        parts[k] = _timed(lambda: e0.ppd_summary(mu_T, var_T, qa, outputs=(k,)), a.reps)[0]

    S_host = int(min(S, max(a.host_gb * 2 ** 30 // (8 * nobs * nobs), 16)))
    Xh = X[:S_host]

    def host():
        mean, cov = chain._predict(Xh)
        return np.percentile(mean, 100.0 * qa, axis=0), cov.shape
    t_host, sp_host, (band_h, _) = _timed(host, 1)
    pph = chain.posterior_predictive(Xh, q)
    same = bool(np.array_equal(pph.band, band_h))

    r = dict(tool="gpu_ppd_timing", emulators=9, observables=nobs, samples=S, quantiles=list(q),
             posterior_predictive_s=t_all, spread=sp_all, predict_pass_s=t_pred, predict_pass_spread=sp_pred,
             summary_s=t_sum, summary_spread=sp_sum, pit_s=t_pit, pit_spread=sp_pit,
             summary_parts_s=parts, host_samples=S_host, host_predict_percentile_s=t_host,
             host_cov_gb=8.0 * S_host * nobs * nobs / 2 ** 30, host_us_per_sample=1e6 * t_host / S_host,
             device_us_per_sample=1e6 * t_all / S, device_predict_us_per_sample=1e6 * t_pred / S,
             band_equals_host_percentile=same, pit_range=[float(pp.pit.min()), float(pp.pit.max())])
    print("posterior_predictive S=%d, %d observables: %.3f s (spread %.1f %%) = predict pass %.3f s + summary %.3f s + PIT %.3f s"
          % (S, nobs, t_all, 100 * sp_all, t_pred, t_sum, t_pit))
    print("summary pieces alone: moments %.4f s, order statistics %.4f s, mixture quantiles %.4f s"
          % (parts["moments"], parts["order"], parts["mixq"]))
    print("host route _predict + np.percentile at S=%d (covariance %.2f GB): %.3f s = %.1f us per sample; device %.2f us per sample "
          "(predict pass alone %.2f); bands equal: %s" % (S_host, r["host_cov_gb"], t_host, r["host_us_per_sample"],
                                                         r["device_us_per_sample"], r["device_predict_us_per_sample"], same))
    line = json.dumps(r)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
