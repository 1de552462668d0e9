"""gpb_eig_simulate and gpb_eig_lse timed on the nine-emulator chain of bench.py's extras (nine emulators, N = 1000 each, 63 GPs, 540
observables, 20 parameters: tools/gpu_multi_chain_profile.py), default 10^5 inner samples drawn from the prior box, 8192 simulated
measurements, ten groups of observables (every emulator's 60, then all 540).
  the predict pass  Chain._ppd_arrays on all inner samples, once: what Chain.expected_information_gain pays before the estimator.
  the calls         wall clock around the synchronising calls with the results left on the device, median of --reps after a
                    warm-up.  gpb_eig_lse is the check of the indices, the centres, the two operand panels, the bias, the main
                    kernel and the merge; the per-kernel split needs a kernel trace, a run of its own:
                        rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/gpu_eig_timing.py --no-host
                        python tools/kernel_trace_summary.py DIR/*/run_kernel_trace.csv
  the rate          2 S_out S_in 2 sum_g M_g flops (the matrix product alone: the exponentials are not counted) over the call's
                    time, as a share of the 78.6 TF/s fp64 matrix peak.
  the whole         Chain.expected_information_gain on the same samples, once (unique rows, predict pass, draws, calls, host sums).
  the host          tests/eig_reference.py on --workers threads: `direct` (term by term, one outer row per thread at a time) and
                    `gemm_form` (BLAS) on a subset of the outer rows, EXTRAPOLATED linearly to all of them; the device's values on
                    those rows against the model, in units of the GPU tier's bound.
No threshold is asserted.  Prints one line per measurement and a JSON summary line; --out FILE also writes them to a file."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK_FP64_MATRIX = 78.6e12


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
    ap.add_argument("--inner", type=int, default=100000)
    ap.add_argument("--outer", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--host-rows", type=int, default=16, help="outer rows of the term-by-term host route")
    ap.add_argument("--host-gemm-rows", type=int, default=512, help="outer rows of the BLAS host route")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("gpu_eig_timing: no GPU (a timing needs one)")
    from gpbayestools_hic_amd import synth
    from gpbayestools_hic_amd.workload import build_multi_chain
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    d, S, So = 20, a.inner, a.outer
    specs = [(1000, 60, 6 + i % 3, ("RBF", "Matern25", "RBF")[i % 3]) for i in range(9)]
    chain, emus, info = build_multi_chain(specs, d)
    X = synth.walkers(S, d, seed=41)
    M = chain.nobs
    ranges, r0 = [], 0
    for e in emus:
        ranges.append((r0, r0 + e.nobs))
        r0 += e.nobs
    ranges.append((0, M))
    ranges = np.asarray(ranges, dtype=np.int32)
    sumM = int((ranges[:, 1] - ranges[:, 0]).sum())
    r = dict(tool="gpu_eig_timing", inner=S, outer=So, observables=M, groups=len(ranges), sum_Mg=sumM, reps=a.reps)
    say("nine-emulator chain: %d observables, %d groups (sum of M_g = %d); %d inner samples from the prior box, %d simulated measurements"
        % (M, len(ranges), sumM, S, So))

    chain._ppd_arrays(X[:4096])                                                       # (warm-up: kernels, workspaces)
    t, _, (engs, mu_T, var_T) = _wall(lambda: chain._ppd_arrays(X), 1)
    r["predict_pass_ms"] = t
    say("the predict pass (means and predictive variances of all inner samples, observable-major): %.1f ms" % t)
    eng = engs[0]
    pv = np.diag(chain.expdata_cov).copy()
    rng = np.random.default_rng(7)
    oidx = torch.as_tensor(rng.choice(S, So).astype(np.int32), device=mu_T.device)
    pvd = torch.as_tensor(pv, device=mu_T.device)
    y_T = eng.eig_simulate(mu_T, var_T, pvd, oidx, 5)
    t, s, y_T = _wall(lambda: eng.eig_simulate(mu_T, var_T, pvd, oidx, 5), a.reps)
    r["simulate"] = dict(call_ms=t, spread=s)
    say("gpb_eig_simulate: the call %.3f ms (spread %.1f %%)" % (t, 100 * s))
    flops = 2.0 * So * S * 2.0 * sumM
    for splits in (0,):
        eng.eig_lse(mu_T, var_T, pvd, None, y_T, oidx, ranges, splits=splits, on_device=True)
        t, s, out = _wall(lambda: eng.eig_lse(mu_T, var_T, pvd, None, y_T, oidx, ranges, splits=splits, on_device=True), a.reps)
        r["lse"] = dict(call_ms=t, spread=s, flops=flops, flops_per_s=flops / (t * 1e-3),
                        share_of_fp64_matrix_peak=flops / (t * 1e-3) / PEAK_FP64_MATRIX)
        say("gpb_eig_lse (index check, centres, panels, bias, main kernel, merge): the call %.2f ms (spread %.1f %%): %.3g flops of the "
            "matrix product = %.2f TF/s = %.3f of the 78.6 TF/s fp64 matrix peak by the CALL's time"
            % (t, 100 * s, flops, flops / (t * 1e-3) / 1e12, r["lse"]["share_of_fp64_matrix_peak"]))
    # one group alone: what the whole range costs, what one data set costs
    for name, rg in (("all 540 observables alone", ranges[-1:]), ("one data set of 60 alone", ranges[:1])):
        eng.eig_lse(mu_T, var_T, pvd, None, y_T, oidx, rg, on_device=True)
        t, s, _ = _wall(lambda: eng.eig_lse(mu_T, var_T, pvd, None, y_T, oidx, rg, on_device=True), a.reps)
        f1 = 2.0 * So * S * 2.0 * float(rg[0, 1] - rg[0, 0])
        r["lse_" + name.split()[0]] = dict(call_ms=t, spread=s, share_of_fp64_matrix_peak=f1 / (t * 1e-3) / PEAK_FP64_MATRIX)
        say("gpb_eig_lse, %s: the call %.2f ms (spread %.1f %%), %.3f of the matrix peak by the call's time"
            % (name, t, 100 * s, f1 / (t * 1e-3) / PEAK_FP64_MATRIX))
    lse_dev, slf_dev = (o.cpu().numpy() for o in out)

    t, _, res = _wall(lambda: chain.expected_information_gain(X, n_outer=So, seed=3), 1)
    r["chain_call"] = dict(ms=t, lower=res.lower.tolist(), upper=res.upper.tolist(), stderr=res.stderr.tolist(),
                           ln_n_inner=res.ln_n_inner)
    say("Chain.expected_information_gain on the same samples, whole (unique rows, predict pass, draws, both calls, host sums): %.1f ms"
        % t)
    for ln in res.table().split("\n"):
        say("    " + ln)

    if not a.no_host:
        import eig_reference as R
        from concurrent.futures import ThreadPoolExecutor
        mu = mu_T.cpu().numpy().T.copy()
        sv = var_T.cpu().numpy().T + pv[None, :]
        y = y_T.cpu().numpy().T.copy()
        oi = oidx.cpu().numpy()
        nrow = min(a.host_rows, So)
        R.ROWS = 1

        def one(i):
            return R.direct(mu, sv, None, y[i:i + 1], oi[i:i + 1], ranges)
        t0 = time.perf_counter()
        with ThreadPoolExecutor(a.workers) as ex:
            parts = list(ex.map(one, range(nrow)))
        td = time.perf_counter() - t0
        mlse = np.concatenate([p[0] for p in parts], axis=1)
        mslf = np.concatenate([p[1] for p in parts], axis=1)
        ng = min(a.host_gemm_rows, So)
        t0 = time.perf_counter()
        glse, mag = R.gemm_form(mu, sv, None, y[:ng], oi[:ng], ranges)
        tg = time.perf_counter() - t0
        err = np.abs(lse_dev[:, :nrow] - mlse) / R.lse_bound(mag[:, :nrow], mlse, ranges)
        errs = np.abs(slf_dev[:, :nrow] - mslf) / R.self_bound(mu, sv, None, y[:nrow], oi[:nrow], ranges)
        r["host"] = dict(direct_rows=nrow, direct_s=td, direct_extrapolated_s=td * So / nrow, gemm_rows=ng, gemm_s=tg,
                         gemm_extrapolated_s=tg * So / ng, workers=a.workers, lse_error_over_bound=float(err.max()),
                         self_error_over_bound=float(errs.max()))
        say("numpy, term by term (eig_reference.direct, %d threads): %d outer rows in %.2f s -> EXTRAPOLATED linearly to %.0f s for all "
            "%d rows (%.0f x the device call)" % (a.workers, nrow, td, td * So / nrow, So, td * So / nrow / (r["lse"]["call_ms"] * 1e-3)))
        say("numpy, operand form through BLAS (eig_reference.gemm_form, with its magnitudes): %d outer rows in %.2f s -> EXTRAPOLATED "
            "linearly to %.0f s for all %d rows (%.0f x the device call)"
            % (ng, tg, tg * So / ng, So, tg * So / ng / (r["lse"]["call_ms"] * 1e-3)))
        say("the device against the term-by-term model on those %d rows, all groups: lse_excl error / bound %.3g, self error / bound %.3g"
            % (nrow, err.max(), errs.max()))
    line = json.dumps(r)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n" + line + "\n")


if __name__ == "__main__":
    main()
