"""CPU tier: the joint factorisation of a coupled chain likelihood (csrc/coupled_setup.h) on the host —
tests/host/coupled_setup_check.cpp includes that header alone, is built with the address and undefined-behaviour sanitizers and
run as a child process."""
import os
import subprocess

from conftest import REPO
from test_ws_carve_host import _compiler


def test_closed_form_equals_the_dense_cholesky_and_refusals(tmp_path):
    """For random block structures — Ms = (7, 5, 9) with Ps = (3, 2, 4), a single emulator, P_e = M_e, and more — with and
    without truncation blocks, 20 random (m, g) each: the closed form from the tables (R, v0, c_perp, logdet0) against a dense
    long-double Cholesky of C0 + A^T diag(g) A, 1e-13 relative.  An indefinite C0, a repeated row of A and a chain beyond the
    limits are reported as "does not apply".  All asserted by the program itself, under -fsanitize=address,undefined."""
    exe = str(tmp_path / "coupled_setup_check")
    src = os.path.join(REPO, "tests", "host", "coupled_setup_check.cpp")
    build = subprocess.run([_compiler(), "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g",
                            src, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert build.returncode == 0, build.stdout.decode()
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert run.returncode == 0, run.stdout.decode()
    assert b"coupled_setup_check: ok" in run.stdout
