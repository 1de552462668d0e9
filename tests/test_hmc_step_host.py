"""CPU tier: csrc/hmc_step.h on the host — tests/host/hmc_step_check.cpp includes that header alone, is built with the address and
undefined-behaviour sanitizers and -ffp-contract=off and run as a child process (nothing is preloaded); every line it prints is
recomputed with tests/hmc_reference.py.  Kick, drift with the wall rule and kinetic energy call no transcendental function: bit
for bit.  The dual-averaging update, the accept probability and the step size call exp, sqrt and pow: 1e-15."""
import os
import subprocess

import numpy as np

import hmc_reference as R
from conftest import REPO
from test_curve_fn_host import _compiler

ESCAPED = 16


def run_host_program(tmp_path, sanitize=True):
    """the program's lines as lists of tokens, keyed by their first word"""
    exe = str(tmp_path / "hmc_step_check")
    src = os.path.join(REPO, "tests", "host", "hmc_step_check.cpp")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    build = subprocess.run([_compiler(), "-std=c++17", "-O1"] + san + ["-ffp-contract=off", "-g", src, "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert build.returncode == 0, build.stdout.decode()
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert run.returncode == 0, run.stdout.decode()
    lines = run.stdout.decode().splitlines()
    assert lines[-1].startswith("hmc_step_check: ok") and int(lines[-1].split()[2]) == len(lines) - 1
    out = {}
    for ln in lines[:-1]:
        tok = ln.split()
        out.setdefault(tok[0], []).append(tok[1:])
    return out


def _f(tok):
    return np.array([float.fromhex(t) for t in tok])


def _same_bits(a, b):
    a, b = np.atleast_1d(np.asarray(a, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64))
    return bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


def test_kick_drift_and_kinetic_bit_for_bit(tmp_path):
    out = run_host_program(tmp_path)
    seen = dict(none=0, low=0, high=0, two=0, eight=0, escaped=0, on_wall=0, nan=0)
    for tok in out["drift"]:
        x, p, eps, minv, lo, hi = _f(tok[:6])
        gx, gp, gr = float.fromhex(tok[7]), float.fromhex(tok[8]), int(tok[9])
        rx, rp, rn, resc = R.drift(np.array([x]), np.array([p]), eps, minv, lo, hi)
        assert _same_bits(gx, rx) and _same_bits(gp, rp), tok
        assert gr == int(rn[0]) + (ESCAPED if resc[0] else 0), tok
        n = gr & ~ESCAPED
        inside0 = lo <= x <= hi
        seen["none"] += n == 0 and gr == 0 and inside0
        seen["low"] += n == 1 and inside0 and p < 0
        seen["high"] += n == 1 and inside0 and p > 0
        seen["two"] += n == 2
        seen["eight"] += gr == 8
        seen["escaped"] += bool(gr & ESCAPED)
        seen["on_wall"] += gx == lo or gx == hi
        seen["nan"] += bool(np.isnan(gx))
        if not (gr & ESCAPED) and not np.isnan(gx):
            assert lo <= gx <= hi, tok
        assert n <= R.MAX_REFLECT
    assert all(v >= 1 for v in seen.values()), seen
    assert seen["on_wall"] >= 3 and seen["nan"] >= 2 and seen["two"] >= 5
    for tok in out["kick"]:
        p, h, g = _f(tok[:3])
        assert _same_bits(float.fromhex(tok[4]), R.kick(p, h, g)), tok
    assert len(out["kick"]) >= 100
    dims = []
    for tok in out["kinetic"]:
        d = int(tok[0])
        v = _f(tok[1:1 + 2 * d])
        assert _same_bits(float.fromhex(tok[2 + 2 * d]), R.kinetic(v[:d], v[d:])), tok
        dims.append(d)
    assert {1, 2, 3, 20, 71, 127, 256} <= set(dims)
    for tok in out["afixed"]:
        a = float.fromhex(tok[0])
        assert int(tok[2]) == int(np.uint64(a * R.A_SCALE))
    tok = out["amean"][0]
    assert _same_bits(float.fromhex(tok[3]), (float(int(tok[0])) / R.A_SCALE) / float(int(tok[1])))


def dual_average_errors(out):
    """|host program - restatement| of every dual-averaging line's five results, relative to max(|value|, 1)"""
    errs = []
    for tok in out["dual"]:
        v = _f(tok[:7])
        got = _f(tok[8:13])
        ref = R.dual_average(v[:5], v[5], v[6])
        errs.append(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1.0)))
    return np.array(errs)


def test_dual_averaging_accept_probability_and_step_size(tmp_path):
    out = run_host_program(tmp_path)
    errs = dual_average_errors(out)
    assert len(errs) == 80 and np.max(errs) <= 1e-15, np.max(errs)
    # the 60 updates in a row carry their own results forward: the count runs 1 .. 60 and mu never changes
    last = _f(out["dual"][59][8:13])
    assert last[4] == 60.0 and last[3] == float.fromhex(out["dual"][0][3])
    for tok in out["accept"]:
        dH, a = float.fromhex(tok[0]), float.fromhex(tok[2])
        ref = float(R.accept_prob(np.array(dH)))
        assert abs(a - ref) <= 1e-15 and 0.0 <= a <= 1.0, tok
    assert float.fromhex(out["accept"][7][2]) == 0.0                     # NaN -> 0
    for tok in out["eps"]:
        le, jit, u = _f(tok[:3])
        ref = R.step_size(le, jit, u)
        assert abs(float.fromhex(tok[4]) - ref) <= 1e-15 * ref, tok
