"""Position-major halo tiles (csrc/halo_pm.h, plan_halo_pm) on the CPU: builds
csrc/halo_pm_check.cpp as a stand-alone program under AddressSanitizer +
UndefinedBehaviorSanitizer and runs it.  The program checks the tap-validity
table against brute-force geometry, walks the kernel's DMA / fragment / epilogue
maps through a small integer conv (B in {1, 16, 17}, both tap orders) and counts
the bank conflicts of every live A-fragment read."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributed_ml_pytorch_amd", "csrc")


@pytest.fixture(scope="module")
def pm_check(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("halo_pm") / "halo_pm_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(CSRC, "halo_pm_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    return r.returncode, r.stdout


def test_halo_pm_maps_check_clean(pm_check):
    rc, out = pm_check
    assert rc == 0, out
    assert "FAIL" not in out and "runtime error" not in out and "AddressSanitizer" not in out, out
    m = re.search(r"halo_pm_check: (\d+) checks, (\d+) failed, A-read conflict degree (\d+)", out)
    assert m, out
    assert int(m.group(1)) > 10000 and int(m.group(2)) == 0
    assert int(m.group(3)) == 1          # every live ds_read_b128 lane group: 16 distinct slots


def test_halo_pm_live_pairs(pm_check):
    """100 of the 144 (pixel, tap) pairs of a 4 x 4 image are in the image; the
    Latin-square fragment map deals them 26 / 25 / 24 / 25 to the wave rows."""
    _, out = pm_check
    m = re.search(r"per wave row: (\d+) (\d+) (\d+) (\d+) of 36", out)
    assert m, out
    live = [int(v) for v in m.groups()]
    assert live == [26, 25, 24, 25] and sum(live) == 100
