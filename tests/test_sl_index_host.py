"""CPU tier: the index arithmetic of the int8 predict kernel's K loop (csrc/sl_index.h) on the host — tests/host/sl_index_check.cpp
includes that header alone, is built with the address and undefined-behaviour sanitizers and run as a child process."""
import os
import shutil
import subprocess

from conftest import REPO


def _compiler():
    for cxx in (os.environ.get("CXX"), "g++", "/opt/rocm/llvm/bin/clang++", "clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    raise AssertionError("no host C++ compiler (g++ or ROCm's clang++) to build tests/host/sl_index_check.cpp")


def test_dma_sources_moved_by_the_stride_stay_inside_the_planes(tmp_path):
    """Np in {64, 128, 192, 256, 320, 1024, 2048} x Wld in {64, 128, 192, 2048} x both depths x both walker-tile widths x front
    padding in {0, 16, 32, 48, 96}, every row block, walker tile, wave, piece and K-step.  Addresses: the source a wave moves by
    the stride from step to step equals the closed form, which equals the plane layout restated; all 64 lanes' 16 bytes lie inside
    the GP's planes as sliced_prepare sizes them; a stage's pieces cover every (plane, k-block, 64 rows) once — all asserted by
    the program itself, under -fsanitize=address,undefined."""
    exe = str(tmp_path / "sl_index_check")
    src = os.path.join(REPO, "tests", "host", "sl_index_check.cpp")
    build = subprocess.run([_compiler(), "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g",
                            src, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert build.returncode == 0, build.stdout.decode()
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert run.returncode == 0, run.stdout.decode()
    assert b"sl_index_check: ok" in run.stdout
