"""HMC step loop (gpb_chain_hmc_run) on the nine-emulator chain (nine synthetic N = 1000 emulators, 540 observables, 20
parameters): ms per step and per leapfrog at C = 1024 and 4096 (L = 8) with the share of gpb_chain_logpost_grad, the effective
samples per second of the worst parameter (diagnostics() after warm-up) against StretchSampler at 4096 walkers on the same chain
and build over three seeds, and the warm-up a sampler started from prior draws needs until split-R-hat < 1.01.

    python tools/gpu_hmc_timing.py --out profiles/hmc_timing.txt --history profiles/HISTORY.md
        every section: writes the file as it goes (the command line is its first line) and appends an entry to the history
    python tools/gpu_hmc_timing.py --launches 5
        five steps at C = 1024 and nothing else: the program of a kernel trace (a run of its own, no counters in it)
    python tools/gpu_hmc_timing.py --summarise-trace kernel_trace.csv --out profiles/hmc_timing.txt --history profiles/HISTORY.md
        launches per step from that trace's CSV, appended to the file and to the history entry

Timing follows the package's other tools: a warm call, then the median of repeated synchronised runs (wall clock around
enqueue + synchronize; the loop never comes back to the host inside a call).  Each section has a wall-clock budget and says so
when it stops early."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

L = 8


def _sync_ms(fn, reps=3):
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts)), float(min(ts)), float(max(ts))


HISTORY_TITLE = "## Round 27 — Hamiltonian Monte Carlo over many chains: the gradient gets its batch"


def history(path, rows):
    """append table rows (what, outcome) to the tool's entry in profiles/HISTORY.md, which is begun if it is not there"""
    if not path or not rows:
        return
    text = open(path).read() if os.path.exists(path) else ""
    with open(path, "a") as f:
        if HISTORY_TITLE not in text:
            f.write("\n\n\n%s\n\n| what | outcome | evidence |\n|---|---|---|\n" % HISTORY_TITLE)
        for what, outcome in rows:
            f.write("| %s | %s | `profiles/hmc_timing.txt` |\n" % (what, outcome))


class Report:
    def __init__(self, path, append=False):
        self.path, self.rows = path, []
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)) or ".", exist_ok=True)
            open(path, "a" if append else "w").close()
        self.line("$ python tools/gpu_hmc_timing.py " + " ".join(sys.argv[1:]))

    def line(self, text="", **row):
        print(text, flush=True)
        if self.path:
            with open(self.path, "a") as f:
                f.write(text + "\n")
        if row:
            self.rows.append(row)


def _near(chain, xstar, C, seed, radius=0.03):
    rng = np.random.default_rng(seed)
    return np.clip(xstar + radius * rng.standard_normal((C, chain.ndim)), chain.min + 0.02, chain.max - 0.02)


def _prior(chain, C, seed):
    return np.random.default_rng(seed).uniform(chain.min, chain.max, (C, chain.ndim))


def step_cost(rep, chain, xstar, C, steps):
    import torch
    from gpbayestools_hic_amd import _native as nat
    from gpbayestools_hic_amd.hmc import HMCSampler
    s = HMCSampler(chain, C, seed=1, nleapfrog=L)
    s.set_state(_near(chain, xstar, C, 0))
    s.warmup(30)
    torch.cuda.synchronize()
    t_step = _sync_ms(lambda: s._advance(steps, False))
    engs, arr, E = chain._contexts()
    lo, hi = chain._box(s.device)
    lp, g = torch.empty_like(s.lp), torch.empty_like(s.grad)

    def grad():        # the resident call the loop makes once per leapfrog
        engs[0]._ck(engs[0].lib.gpb_chain_logpost_grad(arr, E, nat.ptr(s.pos), C, nat.ptr(lp), nat.ptr(g), nat.ptr(lo), nat.ptr(hi),
                                                       float("-inf"), chain.inside_const))
    t_grad = _sync_ms(lambda: [grad() for _ in range(L)], reps=5)
    per_step, per_grad = t_step[0] / steps, t_grad[0] / L
    rep.line("C = %5d  L = %d   %.3f ms/step (min %.3f, max %.3f over 3 runs of %d steps)   %.3f ms/leapfrog   "
             "gpb_chain_logpost_grad of %d rows %.3f ms: %.1f %% of a step   step size %.4g"
             % (C, L, per_step, t_step[1] / steps, t_step[2] / steps, steps, per_step / L, C, per_grad,
                100.0 * L * per_grad / per_step, s.step_size),
             section="step_cost", C=C, ms_per_step=per_step, ms_per_leapfrog=per_step / L, grad_ms=per_grad,
             grad_share=L * per_grad / per_step)
    return per_step


def ess_hmc(rep, chain, xstar, C, seed, nwarm, nsteps):
    import torch
    from gpbayestools_hic_amd.hmc import HMCSampler
    s = HMCSampler(chain, C, seed=seed, nleapfrog=L)
    s.set_state(_near(chain, xstar, C, 100 + seed))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s.warmup(nwarm)
    torch.cuda.synchronize()
    t_warm = time.perf_counter() - t0
    t0 = time.perf_counter()
    s.run(nsteps)
    torch.cuda.synchronize()
    t_run = time.perf_counter() - t0
    d = s.diagnostics()
    ess = float(np.min(d.ess))
    rep.line("HMC      C = %5d seed %d: %d steps in %.2f s (warm-up of %d steps %.2f s); worst ESS %.0f, tau %.2f .. %.2f, "
             "R-hat <= %.4f, acceptance %.3f, step size %.4g, %d divergent, %d escaped -> %.0f ESS/s"
             % (C, seed, nsteps, t_run, nwarm, t_warm, ess, float(np.min(d.tau)), float(np.max(d.tau)), float(np.max(d.rhat)),
                float(s.acceptance_fraction.mean()), s.step_size, s.n_divergent, s.n_escaped, ess / t_run),
             section="ess", sampler="hmc", C=C, seed=seed, ess=ess, seconds=t_run, ess_per_s=ess / t_run,
             converged=bool(d.converged))
    return ess / t_run


def ess_stretch(rep, chain, xstar, W, seed, nburn, nsteps):
    import torch
    from gpbayestools_hic_amd.sampler import StretchSampler
    s = StretchSampler(chain, W, seed=seed)
    X = s.run(_near(chain, xstar, W, 200 + seed), nburn, store=False)
    s.reset()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s.run(X, nsteps)
    torch.cuda.synchronize()
    t_run = time.perf_counter() - t0
    d = s.diagnostics()
    ess = float(np.min(d.ess))
    rep.line("stretch  W = %5d seed %d: %d steps in %.2f s (after %d burn-in steps); worst ESS %.0f, tau %.1f .. %.1f%s, "
             "R-hat <= %.4f, acceptance %.3f -> %.0f ESS/s"
             % (W, seed, nsteps, t_run, nburn, ess, float(np.min(d.tau)), float(np.max(d.tau)),
                "" if d.converged else " (the run is shorter than %g tau: the estimate is not converged)" % d.tol,
                float(np.max(d.rhat)), float(s.acceptance_fraction.mean()), ess / t_run),
             section="ess", sampler="stretch", C=W, seed=seed, ess=ess, seconds=t_run, ess_per_s=ess / t_run,
             converged=bool(d.converged))
    return ess / t_run


def warmup_to_rhat(rep, chain, which, n, grid, budget_s):
    """from prior draws: W warm-up steps, then split-R-hat over the W steps that follow; the first W of the grid below 1.01.
    hmc: Chain.run_HMC's start (hmc.warm_start, the chains re-seeded half way); hmc-plain: HMCSampler.warmup alone"""
    import torch
    from gpbayestools_hic_amd.hmc import HMCSampler, warm_start
    from gpbayestools_hic_amd.sampler import StretchSampler
    t_start, prev, last = time.perf_counter(), 0, float("nan")
    for W in grid:
        if time.perf_counter() - t_start > budget_s:
            rep.line("%-8s split-R-hat < 1.01 not reached by %d warm-up steps within this section's %d s"
                     % (which, prev, budget_s), section="rhat", sampler=which, steps=None, last_rhat=last, last_steps=prev)
            return
        if which in ("hmc", "hmc-plain"):
            s = HMCSampler(chain, n, seed=7, nleapfrog=L)
            if which == "hmc":
                warm_start(s, _prior(chain, n, 8), W)             # run_HMC's start: re-seeded half way
            else:
                s.set_state(_prior(chain, n, 8))
                s.warmup(W)
            s.run(W)
        else:
            s = StretchSampler(chain, n, seed=7)
            X = s.run(_prior(chain, n, 8), W, store=False)
            s.reset()
            s.run(X, W)
        torch.cuda.synchronize()
        r = last = float(np.max(s.diagnostics().rhat))
        rep.line("%-8s %5d warm-up steps from prior draws, split-R-hat over the next %d: %.4f" % (which, W, W, r))
        prev = W
        if r < 1.01:
            rep.line("%-8s split-R-hat < 1.01 after %d warm-up steps (grid %s)" % (which, W, list(grid)),
                     section="rhat", sampler=which, steps=W)
            return
    rep.line("%-8s split-R-hat < 1.01 not reached by %d warm-up steps" % (which, grid[-1]), section="rhat", sampler=which,
             steps=None, last_rhat=last, last_steps=grid[-1])


def summarise_trace(path):
    """launches per HMC step from a kernel trace's CSV: the dispatches from the first k_hmc_eps to the last k_hmc_finish (or
    k_hmc_adapt), divided by the number of k_hmc_finish among them"""
    with open(path) as f:
        rows = list(csv.DictReader(f))
    col = next(c for c in rows[0] if c.lower().replace("_", "") == "kernelname")
    start = next((c for c in rows[0] if c.lower().replace("_", "") in ("starttimestamp", "beginns")), None)
    if start:
        rows.sort(key=lambda r: int(r[start]))
    names = [r[col] for r in rows]
    first = next(i for i, n in enumerate(names) if "k_hmc_eps" in n)
    last = max(i for i, n in enumerate(names) if "k_hmc_finish" in n or "k_hmc_adapt" in n)
    span = names[first:last + 1]
    steps = sum("k_hmc_finish" in n for n in span)
    own = sum("k_hmc_" in n for n in span)
    return ("%d dispatches in %d steps: %.1f launches per step, %.1f of them this loop's own kernels, %.1f per gradient call "
            "(L = %d)" % (len(span), steps, len(span) / steps, own / steps, (len(span) - own) / steps / L, L))


def history_rows(a, rows):
    """the history entry of a full run, from the report's rows"""
    by = lambda sec, **kw: [r for r in rows if r.get("section") == sec and all(r.get(k) == v for k, v in kw.items())]   # noqa: E731
    out = []
    cost = by("step_cost")
    if cost:
        out.append(("`gpb_chain_hmc_run` on nine N = 1000 emulators, 20 parameters, L = %d" % L,
                    "; ".join("C = %d: %.1f ms/step, %.2f ms/leapfrog, `gpb_chain_logpost_grad` %.1f %% of a step"
                              % (r["C"], r["ms_per_step"], r["ms_per_leapfrog"], 100 * r["grad_share"]) for r in cost)))
    es = by("ess_summary")
    if es:
        h, st = es[0]["hmc"], es[0]["stretch"]
        out.append(("worst-parameter effective samples per second, three seeds: HMC at C = %d (%d warm-up, %d production steps) "
                    "against `StretchSampler` at 4096 walkers (%d burn-in, %d production steps)"
                    % (a.ess_chains, a.hmc_warmup, a.hmc_steps, a.stretch_burn, a.stretch_steps),
                    "HMC %.0f … %.0f (median %.0f), stretch move %.0f … %.0f (median %.0f): ratio of the medians %.2f%s"
                    % (min(h), max(h), np.median(h), min(st), max(st), np.median(st), np.median(h) / np.median(st),
                       "" if all(r["converged"] for r in by("ess", sampler="stretch")) else
                       "; the stretch runs are shorter than 50 τ, their estimate is not converged")))
    rh = by("rhat")
    if rh:
        names = {"hmc": "HMC, `run_HMC`'s re-seeded start", "hmc-plain": "HMC, `HMCSampler.warmup` alone", "stretch": "stretch move"}
        out.append(("warm-up steps from prior draws until split-R̂ < 1.01 (R̂ over as many steps as the warm-up)",
                    "; ".join("%s: %s" % (names[r["sampler"]], r["steps"] if r["steps"] else "not reached (last R̂ %.3f after %d)"
                                          % (r.get("last_rhat", float("nan")), r.get("last_steps", 0))) for r in rh)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--history", default="", help="profiles/HISTORY.md: append this run's entry (or rows to it)")
    ap.add_argument("--launches", type=int, default=0)
    ap.add_argument("--summarise-trace", default="")
    ap.add_argument("--steps", type=int, default=10, help="steps per timed run of the step cost")
    ap.add_argument("--hmc-steps", type=int, default=100)
    ap.add_argument("--hmc-warmup", type=int, default=60)
    ap.add_argument("--ess-chains", type=int, default=1024)
    ap.add_argument("--stretch-burn", type=int, default=500)
    ap.add_argument("--stretch-steps", type=int, default=1000)
    ap.add_argument("--rhat-budget", type=int, default=180, help="seconds per sampler for the R-hat section")
    ap.add_argument("--skip", default="", help="comma list of sections to skip (cost, ess, rhat, rhat-stretch)")
    a = ap.parse_args()
    if a.summarise_trace:
        text = summarise_trace(a.summarise_trace)
        Report(a.out, append=True).line(text)
        return history(a.history, [("launches per step, kernel trace of adaptive steps at C = 1024 (a run of its own)", text)])
    import torch
    from gpbayestools_hic_amd.workload import build_multi_chain
    chain, emus, info = build_multi_chain([(1000, 60, 10, "RBF")] * 9, 20)
    xstar = info["xstar"]
    if a.launches:
        from gpbayestools_hic_amd.hmc import HMCSampler
        s = HMCSampler(chain, 1024, seed=1, nleapfrog=L)
        s.set_state(_near(chain, xstar, 1024, 0))
        s._advance(a.launches, True)
        torch.cuda.synchronize()
        return
    skip = set(a.skip.split(",")) if a.skip else set()
    rep = Report(a.out)
    rep.line("HMC on the nine-emulator chain (9 x N = 1000, 540 observables, 20 parameters), %s, L = %d"
             % (torch.cuda.get_device_name(0), L))
    if "cost" not in skip:
        for C in (1024, 4096):
            step_cost(rep, chain, xstar, C, a.steps)
    if "ess" not in skip:
        h = [ess_hmc(rep, chain, xstar, a.ess_chains, seed, a.hmc_warmup, a.hmc_steps) for seed in (1, 2, 3)]
        st = [ess_stretch(rep, chain, xstar, 4096, seed, a.stretch_burn, a.stretch_steps) for seed in (1, 2, 3)]
        rep.line("worst-parameter ESS/s over three seeds: HMC (C = %d) %.0f .. %.0f (median %.0f), stretch move (4096 walkers) "
                 "%.0f .. %.0f (median %.0f): ratio of the medians %.2f"
                 % (a.ess_chains, min(h), max(h), np.median(h), min(st), max(st), np.median(st), np.median(h) / np.median(st)),
                 section="ess_summary", hmc=h, stretch=st)
    if "rhat" not in skip:
        warmup_to_rhat(rep, chain, "hmc", 1024, (32, 64, 128, 256), a.rhat_budget)
        warmup_to_rhat(rep, chain, "hmc-plain", 1024, (64, 256), a.rhat_budget)       # without the re-seeding, for the record
        if "rhat-stretch" not in skip:
            warmup_to_rhat(rep, chain, "stretch", 4096, (125, 250, 500, 1000, 2000, 4000), a.rhat_budget)
    history(a.history, history_rows(a, rep.rows))
    print(json.dumps(rep.rows))


if __name__ == "__main__":
    main()
