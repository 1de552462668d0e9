"""CPU tier: the plans and the workspace layouts of gpb_stein_thin and gpb_stein_ksd (csrc/stein_plan.h) on the host —
tests/host/stein_plan_check.cpp includes the host-only header alone, is built with the address and undefined-behaviour
sanitizers and run as a child process."""
import os
import subprocess

from conftest import REPO
from test_ws_carve_host import _compiler


def test_stein_plan_and_layout(tmp_path):
    """Over a grid of sizes up to 2^31 - 1 rows: the workgroups of a thinning pass and the column ranges of the full discrepancy
    cover everything once and none is empty, the slabs cover the query rows in whole tiles and stay under the budget; the
    counting pass and the carving pass agree and no piece overruns or overlaps another; the size at which the GPU tier relies
    on three slabs gives exactly those."""
    exe = str(tmp_path / "stein_plan_check")
    src = os.path.join(REPO, "tests", "host", "stein_plan_check.cpp")
    build = subprocess.run([_compiler(), "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g",
                            src, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert build.returncode == 0, build.stdout.decode()
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert run.returncode == 0, run.stdout.decode()
    assert b"stein_plan_check: ok" in run.stdout
