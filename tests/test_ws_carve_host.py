"""CPU tier: the buffer carver (csrc/ws_carve.h) and every workspace layout built on it (csrc/ws_layout.h) on the host —
tests/host/ws_carve_check.cpp includes those two headers alone, is built with the address and undefined-behaviour sanitizers and
run as a child process."""
import os
import shutil
import subprocess

from conftest import REPO


def _compiler():
    for cxx in (os.environ.get("CXX"), "g++", "/opt/rocm/llvm/bin/clang++", "clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    raise AssertionError("no host C++ compiler (g++ or ROCm's clang++) to build tests/host/ws_carve_check.cpp")


def test_layouts_count_what_they_carve_and_keep_their_offsets(tmp_path):
    """The carver: granule rounding, n == 0 gives null, mixed element types on 4- and 8-byte bases.  Every layout at a smallest
    and an odd shape: the counting pass and the carving pass agree on the total; on a malloc of exactly that many bytes every
    byte of every piece is written with the piece's tag and read back (overrun: the sanitizer; overlap: the tags); every offset
    and total equals the hand-written expression it replaced — all asserted by the program itself, under
    -fsanitize=address,undefined."""
    exe = str(tmp_path / "ws_carve_check")
    src = os.path.join(REPO, "tests", "host", "ws_carve_check.cpp")
    build = subprocess.run([_compiler(), "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g",
                            src, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert build.returncode == 0, build.stdout.decode()
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert run.returncode == 0, run.stdout.decode()
    assert b"ws_carve_check: ok" in run.stdout
