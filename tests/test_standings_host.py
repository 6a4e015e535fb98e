"""The host half of the standings calls (csrc/standings_host.h: f110qp_path_lengths' sums and the argument rules
of the three calls) on the CPU: host/tests/standings_host.cpp runs them on exactly sized heap arrays under
AddressSanitizer and UBSan. A plain executable: nothing is preloaded."""
import os
import shutil
import subprocess

import pytest
from conftest import ROOT

PKG = os.path.join(ROOT, "f110-mpc_amd")
SRC = os.path.join(PKG, "host", "tests", "standings_host.cpp")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def test_standings_host_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "standings_host")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + os.path.join(PKG, "csrc"),
                           "-I" + os.path.join(ROOT, "include"), SRC, "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "Sanitizer" not in p.stderr, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    assert p.stdout.strip().endswith("standings host ok")
