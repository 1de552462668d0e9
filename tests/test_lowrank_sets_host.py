"""CPU tier: the factorisation of the low-rank block likelihood and the data terms of many data vectors against it
(csrc/lowrank_setup.h) on the host — tests/host/lowrank_sets_check.cpp includes that header alone, is built with the address
and undefined-behaviour sanitizers and run as a child process."""
import os
import subprocess

from conftest import REPO
from test_ws_carve_host import _compiler


def test_data_terms_of_many_sets_against_one_factorisation(tmp_path):
    """Shapes (M, P) = (7, 3), (12, 12), (40, 16), (5, 1), K = 6 data vectors (one shifted far from the others), 20 random
    (m, g) each: the closed form from (R, v0_k, c_perp_k, logdet0) against a dense long-double Cholesky of C0 + A^T diag(g) A
    with dY_k, 1e-13 relative; the terms of set k equal, bit for bit, those of a set-up of its own with yexp = data[k]; an
    indefinite C0 and a repeated row of A are reported as "does not apply".  All asserted by the program itself, under
    -fsanitize=address,undefined."""
    exe = str(tmp_path / "lowrank_sets_check")
    src = os.path.join(REPO, "tests", "host", "lowrank_sets_check.cpp")
    build = subprocess.run([_compiler(), "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g",
                            src, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert build.returncode == 0, build.stdout.decode()
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert run.returncode == 0, run.stdout.decode()
    assert b"lowrank_sets_check: ok" in run.stdout
