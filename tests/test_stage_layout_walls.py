"""The staging table of f110qp_rollout_walls (csrc/api_stage.h) on the CPU: host/tests/stage_layout_walls.cpp
declares the walls family's field set with the segments present, absent and alone and replays a call's copies
against an exactly sized buffer, under AddressSanitizer and UBSan. A plain executable: nothing is preloaded."""
import os
import shutil
import subprocess

import pytest
from conftest import ROOT

PKG = os.path.join(ROOT, "f110-mpc_amd")
SRC = os.path.join(PKG, "host", "tests", "stage_layout_walls.cpp")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def test_stage_layout_walls_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "stage_layout_walls")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + os.path.join(PKG, "csrc"),
                           "-I" + os.path.join(ROOT, "include"), SRC, "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "Sanitizer" not in p.stderr, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    assert p.stdout.strip().endswith("stage layout walls ok")
