"""CPU tier: the owner of the device buffers (csrc/dev_buf.h) on the host — tests/host/dev_buf_check.cpp plays the buffer cache with
malloc / free, is built with the address and undefined-behaviour sanitizers and run as a child process."""
import os
import shutil
import subprocess

from conftest import REPO


def _compiler():
    for cxx in (os.environ.get("CXX"), "g++", "/opt/rocm/llvm/bin/clang++", "clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    raise AssertionError("no host C++ compiler (g++ or ROCm's clang++) to build tests/host/dev_buf_check.cpp")


def test_dev_buf_owns_and_returns_its_buffer(tmp_path):
    """alloc(n): non-null, cap == n; alloc(0): one element; a failing alloc on a held buffer returns the old buffer and leaves
    p == nullptr, cap == 0; release() twice is harmless; the destructor returns the buffer (live counter 0 at exit); the type is
    not copy-constructible (static_assert) — all asserted by the program itself, under -fsanitize=address,undefined."""
    exe = str(tmp_path / "dev_buf_check")
    src = os.path.join(REPO, "tests", "host", "dev_buf_check.cpp")
    build = subprocess.run([_compiler(), "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                            "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", src, "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert build.returncode == 0, build.stdout.decode()
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert run.returncode == 0, run.stdout.decode()
    assert b"dev_buf_check: ok" in run.stdout
