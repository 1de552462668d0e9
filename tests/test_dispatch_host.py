"""CPU tier: the launch dispatch (csrc/dispatch.h: with_int, with_dpad, with_kind, pick_dpad) on the host —
tests/host/dispatch_check.cpp includes that header alone, is built with the address and undefined-behaviour sanitizers and run as
a child process."""
import os
import shutil
import subprocess

from conftest import REPO


def _compiler():
    for cxx in (os.environ.get("CXX"), "g++", "/opt/rocm/llvm/bin/clang++", "clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    raise AssertionError("no host C++ compiler (g++ or ROCm's clang++) to build tests/host/dispatch_check.cpp")


def test_a_listed_value_runs_once_and_an_unlisted_one_fails(tmp_path):
    """For every listed value (the seven widths, restated in the program; the three kernel ids; the lists the launch sites write
    out) the lambda runs exactly once with that value and its result comes back; for an unlisted value it does not run and
    NO_CASE comes back, which is no GPB_E_* code.  pick_dpad(d), d = 1 ... 64, is the smallest listed width >= d and -1 above
    64, and every width it returns dispatches — all asserted by the program itself, under -fsanitize=address,undefined."""
    exe = str(tmp_path / "dispatch_check")
    src = os.path.join(REPO, "tests", "host", "dispatch_check.cpp")
    build = subprocess.run([_compiler(), "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g",
                            src, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert build.returncode == 0, build.stdout.decode()
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert run.returncode == 0, run.stdout.decode()
    assert b"dispatch_check: ok" in run.stdout
