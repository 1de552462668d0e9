"""CPU tier: the inverse normal distribution function of csrc/ndtri.h on the host — tests/host/ndtri_check.cpp includes that header
alone, is built with the address and undefined-behaviour sanitizers and -ffp-contract=off and run as a child process; every value
it prints is compared with scipy.special.ndtri."""
import os
import subprocess

import numpy as np
import scipy.special

from conftest import REPO
from test_curve_fn_host import _compiler


def run_host_program(tmp_path, sanitize=True):
    """(p, z) of the grid and of the six special values.  sanitize=False: the plain build (the GPU tier runs nothing under a
    sanitizer)"""
    exe = str(tmp_path / "ndtri_check")
    src = os.path.join(REPO, "tests", "host", "ndtri_check.cpp")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    build = subprocess.run([_compiler(), "-std=c++17", "-O1"] + san + ["-ffp-contract=off", "-g", src, "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert build.returncode == 0, build.stdout.decode()
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert run.returncode == 0, run.stdout.decode()
    lines = run.stdout.decode().splitlines()
    assert lines[-1].startswith("ndtri_check: ok")
    vals = np.array([[float.fromhex(ln.split()[1]), float.fromhex(ln.split()[3])] for ln in lines[:-1]])
    assert int(lines[-1].split()[2]) == len(vals)
    return vals[:-6], vals[-6:]


def test_ndtri_on_the_grid_against_scipy(tmp_path):
    """p = 1e-10 ... 1 - 1e-10: both tails log-spaced (16 per decade), k / 4096 in the middle, the three switches of AS 241 with
    their one-ulp neighbours, and the rank transform's own arguments (r - 3/8) / (n + 1/4) for n = 2048 at both ends, half ranks
    included.  Measured: the largest relative deviation from scipy.special.ndtri is 7.8e-16 (p = 0.12695, z = -1.141; against
    mpmath at 40 digits this header is within 5.9e-16 and scipy within 4.3e-16 on every seventh grid value).  The bar is 8 x the
    measured value, 6.3e-15: below the 1e-13 that double accuracy asks for.  p = 1/2 gives exactly 0."""
    measured = 7.8e-16
    bar = 8.0 * measured
    assert bar < 1e-13
    grid, special = run_host_program(tmp_path)
    p, z = grid[:, 0], grid[:, 1]
    assert len(p) > 4500 and 1e-10 in p and 1.0 - 1e-10 in p and p.min() == np.nextafter(np.exp(-25.0), 0.0)
    n = 2048
    for r in (1.0, 1.5, float(n) - 0.5, float(n)):
        assert (r - 0.375) / (n + 0.25) in p
    ref = scipy.special.ndtri(p)
    mid = p == 0.5
    assert np.all(z[mid] == 0.0) and mid.sum() == 1
    rel = np.abs(z[~mid] - ref[~mid]) / np.abs(ref[~mid])
    i = int(np.argmax(rel))
    print("ndtri host: largest relative deviation from scipy %.3e at p = %.17g (z = %.6g); bar %.3e" % (rel[i], p[~mid][i], z[~mid][i], bar))
    assert rel[i] <= bar
    assert np.all(np.diff(z[np.argsort(p, kind="stable")]) >= 0.0)                  # monotone on the grid
    # the special values: 1/2 -> 0, p <= 0 -> -inf, p >= 1 -> +inf, NaN -> NaN
    assert special[0, 1] == 0.0 and special[1, 1] == -np.inf and special[2, 1] == np.inf
    assert special[3, 1] == -np.inf and special[4, 1] == np.inf and np.isnan(special[5, 1])
