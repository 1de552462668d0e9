"""CPU tier: the plan and the workspace layout of gpb_chain_knn (csrc/knn_plan.h, KnnWs of csrc/ws_layout.h) on the host —
tests/host/knn_plan_check.cpp includes the three host-only headers alone, is built with the address and undefined-behaviour
sanitizers and run as a child process."""
import os
import subprocess

from conftest import REPO
from test_ws_carve_host import _compiler


def test_knn_plan_and_layout(tmp_path):
    """Over a grid of sizes up to 2^31 - 1 rows: the ranges of B cover every row and none is empty, the slabs cover A in whole
    tiles and stay under the budget; the counting pass and the carving pass agree and no piece overruns or overlaps another;
    the sizes at which the GPU tier relies on one, two and three slabs give exactly those."""
    exe = str(tmp_path / "knn_plan_check")
    src = os.path.join(REPO, "tests", "host", "knn_plan_check.cpp")
    build = subprocess.run([_compiler(), "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g",
                            src, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert build.returncode == 0, build.stdout.decode()
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert run.returncode == 0, run.stdout.decode()
    assert b"knn_plan_check: ok" in run.stdout
