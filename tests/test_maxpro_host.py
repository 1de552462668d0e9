"""CPU tier: the host-includable pieces of the MaxPro generator on the host — tests/host/maxpro_ws_check.cpp (the workspace
layout MaxproWs of csrc/ws_layout.h) and tests/host/maxpro_index_check.cpp (csrc/maxpro_index.h: the proposal decoding and the
strided row loop) — built with the address and undefined-behaviour sanitizers and run as child processes."""
import os
import subprocess

import pytest

from conftest import REPO
from test_ws_carve_host import _compiler


@pytest.mark.parametrize("name", ["maxpro_ws_check", "maxpro_index_check"])
def test_host_program_holds(tmp_path, name):
    exe = str(tmp_path / name)
    src = os.path.join(REPO, "tests", "host", name + ".cpp")
    build = subprocess.run([_compiler(), "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g",
                            src, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert build.returncode == 0, build.stdout.decode()
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert run.returncode == 0, run.stdout.decode()
    assert (name + ": ok").encode() in run.stdout
