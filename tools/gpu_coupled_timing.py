"""What a coupled experimental covariance costs per step: the benchmark's nine-emulator chain (63 GPs, 540 observables, nine
synthetic N = 1000 designs over 20 parameters, built as bench.py builds it), 4096 walkers, burnt-in ensemble.
  (i)   ms/step of gpb_chain_emcee_run with the experiment file's diagonal covariance (the block path)
  (ii)  ms/step with covariance (a): diag(sigma^2) + 0.03 |y_exp| over all observables + 0.05 |y_exp| over the middle half
        (Chain.set_systematics) — the coupled kernel in place of the nine low-rank blocks
  (iii) one 2048-row batch through the dense route (Chain._predict + gpb_mvn_loglike on the 540 x 540 matrices), in slabs
Each ms/step is the median of --reps blocks of --steps steps behind an untimed pre-heat.  Also the coupled kernel alone:
gpb_chain_logpost on 2048 rows with and without the coupling.  Prints one line per figure and a JSON summary; --out FILE writes
the text lines to a file."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _step_ms(chain, X0, nw, steps, reps):
    import torch
    from gpbayestools_hic_amd import StretchSampler
    heat = StretchSampler(chain, nw, seed=6)
    heat.run(X0, 40, status=10 ** 9, store=False)
    del heat
    s = StretchSampler(chain, nw, seed=5)
    assert s._resident_engine() is not None
    s.run(X0, 3, status=10 ** 9, store=False)
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.run(None, steps, status=10 ** 9, store=False)
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0) / steps)
    acc = float(s.naccept.sum().item()) / (nw * (3 + steps * reps))
    return float(np.median(ts)), float((max(ts) - min(ts)) / np.median(ts)), acc


def _call_ms(fn, reps=7):
    import torch
    fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--walkers", type=int, default=4096)
    ap.add_argument("--dense-rows", type=int, default=2048)
    ap.add_argument("--out")
    ap.add_argument("--trace", choices=["diag", "coupled"],
                    help="only 43 + --steps steps with this covariance: the program of a `rocprofv3 --kernel-trace --stats` run")
    a = ap.parse_args()
    import torch
    from gpbayestools_hic_amd import synth
    from gpbayestools_hic_amd.workload import build_multi_chain
    specs = [(1000, 60, 6 + i % 3, ("RBF", "Matern25", "RBF")[i % 3]) for i in range(9)]
    chain, emus, info = build_multi_chain(specs, 20)
    nw = a.walkers
    X0 = synth.walkers_ball(nw, info["xstar"], 1e-8)
    y = np.abs(info["yexp"])
    n = len(y)
    s2 = np.zeros(n)
    s2[n // 4:3 * n // 4] = 0.05 * y[n // 4:3 * n // 4]
    sources = np.stack([0.03 * y, s2])
    diag_cov = chain.expdata_cov
    dev = torch.device("cuda", chain.device)
    Xb = torch.as_tensor(synth.walkers_ball(a.dense_rows, info["xstar"], 1e-3), device=dev)
    lines, res = [], {}
    if a.trace:
        if a.trace == "coupled":
            chain.set_systematics(sources)
        print("%s: %.3f ms/step" % (a.trace, _step_ms(chain, X0, nw, a.steps, 1)[0]))
        return

    def say(key, value, text):
        res[key] = value
        lines.append(text)
        print(text, flush=True)

    ms, spread, acc = _step_ms(chain, X0, nw, a.steps, a.reps)
    say("diag_ms_per_step", ms, "(i)   diagonal covariance (block path):   %8.3f ms/step  (spread %.1f %%, acceptance %.2f; median of %d x %d steps)"
        % (ms, 100 * spread, acc, a.reps, a.steps))
    k_diag = _call_ms(lambda: chain.log_prob_device(Xb))
    say("diag_logpost_2048_ms", k_diag, "      gpb_chain_logpost, %d rows, block path:   %8.3f ms" % (a.dense_rows, k_diag))

    t0 = time.perf_counter()
    chain.set_systematics(sources)
    chain._prepare_blocks()
    setup_s = time.perf_counter() - t0
    assert chain._coupled and chain._coupled_why is None
    say("setup_s", setup_s, "      gpb_chain_like_set (host set-up, once per experiment):   %8.3f s" % setup_s)
    ms2, spread2, acc2 = _step_ms(chain, X0, nw, a.steps, a.reps)
    say("coupled_ms_per_step", ms2, "(ii)  covariance (a) (coupled kernel):      %8.3f ms/step  (spread %.1f %%, acceptance %.2f)"
        % (ms2, 100 * spread2, acc2))
    k_cpl = _call_ms(lambda: chain.log_prob_device(Xb))
    say("coupled_logpost_2048_ms", k_cpl, "      gpb_chain_logpost, %d rows, coupled:      %8.3f ms" % (a.dense_rows, k_cpl))

    # the dense route: _predict's [rows, 540, 540] covariances + the device MVN, in slabs that fit the host
    from gpbayestools_hic_amd.mcmc import _utility_engine
    Xh = Xb.cpu().numpy()
    eng = _utility_engine(chain.device)

    def dense():
        out = np.empty(len(Xh))
        for i0 in range(0, len(Xh), 256):
            mY, mC = chain._predict(Xh[i0:i0 + 256], 0.0)
            out[i0:i0 + 256] = eng.mvn_loglike(mY - chain.expdata, mC + chain.expdata_cov)
        return out
    t0 = time.perf_counter()
    ref = dense()
    dense_ms = 1e3 * (time.perf_counter() - t0)
    got = chain.log_prob_device(Xb).cpu().numpy() - chain.inside_const
    say("dense_2048_ms", dense_ms, "(iii) dense route, one batch of %d rows:   %8.1f ms  (coupled kernel against it: %.2e relative)"
        % (a.dense_rows, dense_ms, float(np.max(np.abs(got - ref) / np.abs(ref)))))
    chain.expdata_cov = diag_cov
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
