"""The wide training step's plan (csrc/hip/wide_plan.hpp over wide_layout.hpp)
on the host, for every tile 17..34 x 17..34, batches 1, 8 and 4096 and both
arithmetics (CPU).

The workspace and dispatch tables pin which kernels the wide step takes and its
workspace size; no GPU test sees a grid size or a dynamic-LDS byte count, and
a wrong one shows up only as a kernel writing past its LDS.
tests/wide_plan_check.cpp includes the two headers with the device qualifiers
defined away, prints every WidePlan (served or not, the six variant flags,
grids, LDS bytes, slab counts, the gW2 band geometry, the workspace regions)
and checks the LDS limits and the op-level geometry builders against the
step's; the print-out is compared with tests/golden/wide_plan_table.txt,
recorded from the formulas plan_step() had inside train_wide.hip before the
layouts were single-sourced.
"""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "wide_plan_check.cpp")
INC = os.path.join(ROOT, "cnn-super-resolution_amd", "csrc", "hip")
GOLDEN = os.path.join(ROOT, "tests", "golden", "wide_plan_table.txt")
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")


@pytest.mark.skipif(CXX is None, reason="needs a host C++ compiler")
def test_wide_plan_table(tmp_path):
    exe = str(tmp_path / "wide_plan_check")
    c = subprocess.run([CXX, "-std=c++17", "-O2", "-Wall", "-Werror", "-I", INC, SRC, "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert c.returncode == 0, c.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    failures = [l for l in r.stdout.splitlines() if l.startswith("FAIL")]
    assert failures == [], failures[:20]
    assert r.returncode == 0, r.stdout[-2000:]
    got = r.stdout.splitlines()
    assert got[-1] == "tiles=648 served=642 failures=0", got[-1]
    with open(GOLDEN) as f:
        want = f.read().splitlines()
    diff = [(i + 1, a, b) for i, (a, b) in enumerate(zip(want, got)) if a != b]
    assert diff == [], diff[:10]
    assert len(got) == len(want)
