"""CPU tier: the workspace layout of gpb_chain_kmeans (KmeansWs, csrc/ws_layout.h) on the host — tests/host/kmeans_ws_check.cpp
includes ws_carve.h and ws_layout.h alone, is built with the address and undefined-behaviour sanitizers and run as a child
process."""
import os
import subprocess

from conftest import REPO
from test_ws_carve_host import _compiler


def test_kmeans_layout_counts_what_it_carves(tmp_path):
    """At a smallest, an odd and the largest shape, with and without the seeding's pieces: the counting pass and the carving
    pass agree; on a malloc of exactly that many bytes every byte of every piece is written with the piece's tag and read back
    (overrun: the sanitizer; overlap: the tags); the run that a call zeroes holds the state pieces and no other."""
    exe = str(tmp_path / "kmeans_ws_check")
    src = os.path.join(REPO, "tests", "host", "kmeans_ws_check.cpp")
    build = subprocess.run([_compiler(), "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g",
                            src, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert build.returncode == 0, build.stdout.decode()
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert run.returncode == 0, run.stdout.decode()
    assert b"kmeans_ws_check: ok" in run.stdout
