"""CPU tier: the curve functions gpb_chain_curves evaluates (csrc/curve_fn.h) on the host — tests/host/curve_fn_check.cpp includes
that header alone, is built with the address and undefined-behaviour sanitizers and -ffp-contract=off and run as a child process;
every value it prints is compared with the numpy model of tests/curves_reference.py."""
import os
import shutil
import subprocess

import numpy as np

import curves_reference as R
from conftest import REPO


def _compiler():
    for cxx in (os.environ.get("CXX"), "g++", "/opt/rocm/llvm/bin/clang++", "clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    raise AssertionError("no host C++ compiler (g++ or ROCm's clang++) to build tests/host/curve_fn_check.cpp")


def test_every_branch_boundary_rounds_as_numpy_does(tmp_path):
    """All four functions at 0, 0.2, 0.4, 2, 4 and g == T0 with both one-ulp neighbours, and at negative g.  eta/s, y_loss and
    the closure distance: bit for bit the numpy model.  zeta/s: within 2^-51 relative — the two libm exps are each within an
    ulp of the truth, everything around them is the same rounded operation."""
    exe = str(tmp_path / "curve_fn_check")
    src = os.path.join(REPO, "tests", "host", "curve_fn_check.cpp")
    build = subprocess.run([_compiler(), "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-ffp-contract=off", "-g", src, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert build.returncode == 0, build.stdout.decode()
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert run.returncode == 0, run.stdout.decode()
    lines = run.stdout.decode().splitlines()
    assert lines[-1].startswith("curve_fn_check: ok")
    seen = {0: 0, 1: 0, 2: 0, 3: 0}
    worst = 0.0
    for ln in lines[:-1]:
        tok = ln.split()
        fn = int(tok[1])
        v = float.fromhex(tok[-1])
        if fn == 3:
            d = int(tok[3])
            theta = np.array([float.fromhex(t) for t in tok[5:5 + d]])
            aux = np.array([float.fromhex(t) for t in tok[6 + d:6 + 3 * d]])
            want = R.curve_value(3, theta[None, :], 0.0, aux)[0]
            assert v == want, ln
        else:
            g = float.fromhex(tok[3])
            p = np.array([float.fromhex(t) for t in tok[5:9]])
            want = R.curve_value(fn, p[None, :R.NPAR[fn]], g)[0]
            if fn == 0:
                err = abs(v - want) / abs(want) if want != 0.0 else abs(v)
                worst = max(worst, err)
                assert err <= 2.0 ** -51, (ln, want.hex())
            else:
                assert v == want and np.signbit(v) == np.signbit(want), (ln, want.hex())
        seen[fn] += 1
    assert all(n >= 16 for n in seen.values()), seen
    assert int(lines[-1].split()[-1]) == sum(seen.values())
