"""The staging table of the host-pointer rollouts (csrc/api_stage.h: offsets, sizes, the row-0 split of the
[T+1] trajectories) on the CPU: host/tests/stage_layout.cpp declares the library's own field sets for every
optional array on, off and alone and replays a call's copies, under AddressSanitizer and UBSan. A plain
executable: nothing is preloaded."""
import os
import shutil
import subprocess

import pytest
from conftest import ROOT

PKG = os.path.join(ROOT, "f110-mpc_amd")
SRC = os.path.join(PKG, "host", "tests", "stage_layout.cpp")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def test_stage_layout_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "stage_layout")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + os.path.join(PKG, "csrc"),
                           "-I" + os.path.join(ROOT, "include"), SRC, "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "Sanitizer" not in p.stderr, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    assert p.stdout.strip().endswith("stage layout ok")
