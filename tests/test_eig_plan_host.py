"""CPU tier: the plan and the workspace layout of gpb_eig_lse (csrc/eig_plan.h, EigWs of csrc/ws_layout.h) on the host —
tests/host/eig_plan_check.cpp includes the three host-only headers alone, is built with the address and undefined-behaviour
sanitizers and run as a child process."""
import os
import subprocess

from conftest import REPO
from test_ws_carve_host import _compiler


def test_eig_plan_and_layout(tmp_path):
    """Over a grid of sizes up to the largest sample count: the padded widths are whole tiles, the ranges of the inner axis
    cover every tile and none is empty; the counting pass and the carving pass agree, every piece is 16-byte aligned and no
    piece overruns or overlaps another; the automatic number of ranges at the sizes the GPU tier and the timing tool use."""
    exe = str(tmp_path / "eig_plan_check")
    src = os.path.join(REPO, "tests", "host", "eig_plan_check.cpp")
    build = subprocess.run([_compiler(), "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g",
                            src, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert build.returncode == 0, build.stdout.decode()
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert run.returncode == 0, run.stdout.decode()
    assert b"eig_plan_check: ok" in run.stdout
