"""CPU tier: the workspace layout of gpb_chain_curves (CurvesWs, csrc/ws_layout.h) on the host — tests/host/curves_ws_check.cpp
includes ws_carve.h and ws_layout.h alone, is built with the address and undefined-behaviour sanitizers and run as a child
process."""
import os
import subprocess

from conftest import REPO
from test_ws_carve_host import _compiler


def test_curves_layout_counts_what_it_carves(tmp_path):
    """At a smallest, the default and the largest shape, with and without the select's pieces and the closure distance's aux: the
    counting pass and the carving pass agree; on a malloc of exactly that many bytes every byte of every piece is written with
    the piece's tag and read back (overrun: the sanitizer; overlap: the tags).  The layout takes no number of samples."""
    exe = str(tmp_path / "curves_ws_check")
    src = os.path.join(REPO, "tests", "host", "curves_ws_check.cpp")
    build = subprocess.run([_compiler(), "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g",
                            src, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert build.returncode == 0, build.stdout.decode()
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert run.returncode == 0, run.stdout.decode()
    assert b"curves_ws_check: ok" in run.stdout
