"""The fused training step's plan (csrc/hip/fused_plan.hpp over
fused_layout.hpp) on the host (CPU): for the default net every tile 13..41 x
13..41 under both arithmetics and the columns 42..58 at 13 and 14 rows, for the
other three nets the squares 11..41 and the rows and columns through 33, at
batches 1, 300, 700 and 4096.

The workspace table pins the step's total workspace and the dispatch table
(GPU) its kernel names; no GPU test sees a grid size, a slab region or a
dynamic-LDS byte count, and a wrong one shows up only as a kernel writing past
its LDS.  tests/fused_plan_check.cpp includes the two headers with the device
qualifiers defined away, prints every StepPlan (served or not, the variant
flags and names, grids, LDS bytes, d1c_parts, m2_off, the slab regions) and
checks the LDS limits and the implications between the flags; the print-out is
compared with tests/golden/fused_plan_table.txt, recorded from plan_step() as
it stood inside train_fused.hip, moved to the header verbatim (the names
column, which the plan gained afterwards, added to that record).  The plan's
three kernel names are also compared with tests/golden/dispatch_table.json
for every case there that the fused step serves.
"""
import importlib.util
import json
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "fused_plan_check.cpp")
INC = os.path.join(ROOT, "cnn-super-resolution_amd", "csrc", "hip")
GOLDEN = os.path.join(ROOT, "tests", "golden", "fused_plan_table.txt")
DISPATCH = os.path.join(ROOT, "tests", "golden", "dispatch_table.json")
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")

pytestmark = pytest.mark.skipif(CXX is None, reason="needs a host C++ compiler")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fused_plan") / "fused_plan_check")
    c = subprocess.run([CXX, "-std=c++17", "-O2", "-Wall", "-Werror", "-I", INC, "-I", os.path.join(ROOT, "include"),
                        SRC, "-o", out], capture_output=True, text=True, timeout=300)
    assert c.returncode == 0, c.stderr[-4000:]
    return out


def test_fused_plan_table(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    failures = [l for l in r.stdout.splitlines() if l.startswith("FAIL")]
    assert failures == [], failures[:20]
    assert r.returncode == 0, r.stdout[-2000:]
    got = r.stdout.splitlines()
    assert got[-1] == "tiles=2023 served=1934 failures=0", got[-1]
    with open(GOLDEN) as f:
        want = f.read().splitlines()
    diff = [(i + 1, a, b) for i, (a, b) in enumerate(zip(want, got)) if a != b]
    assert diff == [], diff[:10]
    assert len(got) == len(want)


def test_plan_names_are_the_dispatch_table_s(exe):
    """Every fused train_fwd_bwd case of the recorded dispatch table, at its
    batch, under both arithmetics: the first three kernels are the plan's."""
    spec = importlib.util.spec_from_file_location("record_dispatch_table",
                                                  os.path.join(ROOT, "tools", "record_dispatch_table.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    with open(DISPATCH) as f:
        table = json.load(f)
    seen = 0
    for name, size, path in tool.CASES:
        for arith in (0, 1):
            want = table[tool.case_id(name, size, path, arith)]["train_fwd_bwd"]
            n1, n2, f1, f2, f3 = tool.NETS[name]
            if f2 != 1 or path != 0:
                assert want["path"] != "fused"
                continue
            r = subprocess.run([exe, "names"] + [str(v) for v in (n1, n2, f1, f3, arith, size, size, tool.BATCH)],
                               capture_output=True, text=True, timeout=60)
            assert r.returncode == 0, r.stderr
            if want["path"] != "fused":  # (default 40 x 40, the tiny net)
                assert r.stdout.split() == ["-"], (name, size, arith, r.stdout)
                continue
            assert r.stdout.split() == want["kernels"][:3], (name, size, arith, r.stdout)
            assert len(want["kernels"]) == 4 and want["kernels"][3].startswith("slab_reduce")
            seen += 1
    assert seen == 2 * 7  # default 33, 21, 13, 36, 39; default_f3 33; example 33
