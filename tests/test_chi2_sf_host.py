"""CPU tier: the chi-square survival function of csrc/chi2_sf.h on the host — tests/host/chi2_sf_check.cpp includes that header
alone, is built with the address and undefined-behaviour sanitizers and -ffp-contract=off and run as a child process; every value
it prints is compared with mpmath at 50 digits (tests/gof_reference.py)."""
import os
import subprocess

import numpy as np
import scipy.special

import gof_reference as R
from conftest import REPO
from test_curve_fn_host import _compiler


def run_host_program(tmp_path, sanitize=True):
    """[(ndf, x, Q, iterations)] of the grid and the special values, and the last line's (max iterations, bound).  sanitize=False:
    the plain build (the GPU tier compares the device's values with the host's and runs nothing under a sanitizer)"""
    exe = str(tmp_path / "chi2_sf_check")
    src = os.path.join(REPO, "tests", "host", "chi2_sf_check.cpp")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    build = subprocess.run([_compiler(), "-std=c++17", "-O1"] + san + ["-ffp-contract=off", "-g", src, "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert build.returncode == 0, build.stdout.decode()
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert run.returncode == 0, run.stdout.decode()
    lines = run.stdout.decode().splitlines()
    assert lines[-1].startswith("chi2_sf_check: ok")
    vals = []
    for ln in lines[:-1]:
        tok = ln.split()
        vals.append((float.fromhex(tok[1]), float.fromhex(tok[3]), float.fromhex(tok[5]), int(tok[7])))
    last = lines[-1].split()
    assert int(last[2]) == len(vals)
    return vals, int(last[4]), int(last[6])


def grid_errors(vals):
    """per grid value with a true Q >= 1e-290: (ndf, x, error of the value, scipy's error); the others must lie in [0, 1e-289]"""
    out = []
    for ndf, x, q, _ in vals:
        e, true = R.sf_relerr(q, x, ndf)
        if true >= 1e-290:
            es, _ = R.sf_relerr(float(scipy.special.gammaincc(ndf / 2.0, x / 2.0)), x, ndf)
            out.append((ndf, x, e, es))
        else:
            assert 0.0 <= q <= 1e-289, (ndf, x, q)
    return out


def test_chi2_sf_on_the_grid_against_mpmath(tmp_path):
    """ndf in {1, 2, 3, 16, 55, 64, 540, 2048} times x / ndf in {0, 1e-3, 0.3, 0.9, 1, 1.1, 2, 5, 40} and the switch between the
    series and the continued fraction, x = ndf + 2, with both one-ulp neighbours.  Bar: relative error <= max(8 x scipy
    gammaincc's own worst error on the same grid, 64 2^-53) wherever the true Q >= 1e-290; below that 0 <= Q <= 1e-289.
    Measured: worst 7.9e-13 (ndf = 2048, x just above the switch) against scipy's worst 4.5e-13 (ndf = 2048, x = 2 ndf): the bar
    is 3.6e-12.  Iterations: 272 at most, bound 600."""
    vals, worst_iter, bound = run_host_program(tmp_path)
    grid = vals[:-4]
    assert [(v[0], v[1]) for v in grid] == R.sf_grid()
    errs = grid_errors(grid)
    assert len(errs) >= 80
    err_scipy = max(e[3] for e in errs)
    bar = R.sf_bar(err_scipy)
    w = max(errs, key=lambda e: e[2])
    print("chi2_sf host: worst relative error %.3e at ndf=%g x/ndf=%.6g; scipy's worst %.3e; bar %.3e; iterations %d of %d"
          % (w[2], w[0], w[1] / w[0], err_scipy, bar, worst_iter, bound))
    for ndf, x, e, _ in errs:
        assert e <= bar, (ndf, x, e, bar)
    assert max(v[3] for v in vals) == worst_iter < bound
    assert all(q == 1.0 for _, x, q, _ in grid if x == 0.0)
    # the special values: NaN -> NaN, x <= 0 -> 1, +inf -> 0
    sp = vals[-4:]
    assert np.isnan(sp[0][2]) and sp[1][2] == 1.0 and sp[2][2] == 1.0 and sp[3][2] == 0.0
