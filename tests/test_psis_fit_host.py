"""CPU tier: csrc/psis_fit.h on the host — tests/host/psis_fit_check.cpp includes that header alone, is built with the address and
undefined-behaviour sanitizers and -ffp-contract=off and run as a child process on the sorted tails of the input sets of
tests/psis_reference.py; the fit and the quantile function are compared with the numpy model."""
import os
import subprocess

import numpy as np

import psis_reference as R
from conftest import REPO
from test_curve_fn_host import _compiler

KHAT_BAR = 1e-12          # the GPU tier's bar for khat
VALUE_BAR = 1e-11         # and for a smoothed log weight


def run_host_program(tmp_path, lines):
    exe = str(tmp_path / "psis_fit_check")
    src = os.path.join(REPO, "tests", "host", "psis_fit_check.cpp")
    build = subprocess.run([_compiler(), "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-ffp-contract=off", "-g", src, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert build.returncode == 0, build.stdout.decode()
    cases = tmp_path / "cases.txt"
    cases.write_text("\n".join(lines) + "\n")
    run = subprocess.run([exe, str(cases)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert run.returncode == 0, run.stdout.decode()
    out = run.stdout.decode().splitlines()
    assert out[-1] == "psis_fit_check: ok %d" % len(lines), out[-1]
    return [ln.split() for ln in out[:-1]]


def fit_line(t):
    return "fit %d %s" % (len(t), " ".join(float(v).hex() for v in t))


def sorted_tail(lr):
    d = {}
    R.psis_row(lr, details=d)
    x = d["x"]
    return np.exp(x[d["tail"]]) - np.exp(d["cutoff"])


def check_fit(tok, t):
    """the program's line for the tail t against the model: worst deviations (khat, smoothed values)"""
    n = len(t)
    det = {}
    khat, sigma = R.gpd_fit(t, details=det)
    got = [float.fromhex(v) for v in tok[1:7]]
    assert tok[0] == "fit" and int(tok[7]) == det["m_est"]
    p = (np.array([0, n // 2, n - 1]) + 0.5) / n
    want = np.log(R.gpd_quantile(p, khat, sigma))
    kept = det["w"][det["w"] >= 10 * np.finfo(float).eps]
    assert abs(got[5] - kept.min()) <= 1e-9 * kept.min()
    assert abs(got[1] - sigma) <= 1e-12 * abs(sigma)
    return abs(got[0] - khat), float(np.abs(np.array(got[2:5]) - want).max())


def test_fit_and_quantiles_on_the_shared_sets(tmp_path):
    """every input set of the GPU tier with a tail of five or more: khat within 1e-12 of the model and the smoothed values at ranks
    0, n / 2 and n - 1 within 1e-11 (measured on the host: khat 3.1e-15, values 1.4e-14)"""
    tails = {name: sorted_tail(lr) for name, lr in R.named_sets().items() if name not in R.SHORT_TAIL_SETS}
    toks = run_host_program(tmp_path, [fit_line(t) for t in tails.values()])
    dk = dv = 0.0
    for tok, (name, t) in zip(toks, tails.items()):
        a, b = check_fit(tok, t)
        dk, dv = max(dk, a), max(dv, b)
    print("psis_fit host: khat within %.1e, smoothed values within %.1e over %d tails" % (dk, dv, len(tails)))
    assert dk <= KHAT_BAR and dv <= VALUE_BAR


def test_small_and_denormal_tails(tmp_path):
    """n = 5, the shortest tail that is fitted, and a tail whose smallest excess is a denormal"""
    r = np.random.default_rng(8)
    five = np.sort(r.pareto(2.0, 5))
    den = np.sort(r.pareto(3.0, 40))
    den[0] = 5e-324
    toks = run_host_program(tmp_path, [fit_line(five), fit_line(den)])
    for tok, t in zip(toks, (five, den)):
        a, b = check_fit(tok, t)
        assert a <= KHAT_BAR and b <= VALUE_BAR
        assert np.isfinite(float.fromhex(tok[1]))


def test_quantile_branches_and_tail_rule(tmp_path):
    """khat == 0 takes the exponential's quantile, -sigma log1p(-p), the limit of the other branch; the tail length rule"""
    ps = [0.5 / 425, 0.3, 0.5, 1 - 0.5 / 425]
    sizes = [1, 4, 5, 20, 25, 26, 225, 226, 4096, 4097, 20000, 1 << 24]
    lines = ["q %s %s %s" % (float(p).hex(), float(k).hex(), float(2.5).hex()) for p in ps for k in (0.0, 1e-9, -0.2, 0.7)]
    toks = run_host_program(tmp_path, lines + ["m %d" % s for s in sizes])
    i = 0
    for p in ps:
        for k in (0.0, 1e-9, -0.2, 0.7):
            got = float.fromhex(toks[i][1])
            want = R.gpd_quantile(p, k, 2.5)
            assert abs(got - want) <= 4e-16 * abs(want), (p, k, got, want)
            if k == 0.0:
                assert abs(got + 2.5 * np.log1p(-p)) <= 4e-16 * abs(got)
            if k == 1e-9:
                assert abs(got - R.gpd_quantile(p, 0.0, 2.5)) <= 1e-7 * abs(got)
            i += 1
    assert [int(t[1]) for t in toks[i:]] == [R.tail_max(s) for s in sizes]
