"""The pair-slot <-> tap map of d1x6's delta2 GEMM (csrc/hip/d3taps.hpp) on the
host, for every filter size the delta3 mode admits (f3 = 1 .. 5) (CPU).

d1x6 builds its W3 operand image and the per-pair delta3 image offsets from
this one map; the GPU parity tests reach it only at the filter sizes they run.
tests/d3_tap_slots_check.cpp includes d3taps.hpp with the device qualifiers
defined away and checks, over all 16 pair slots: every tap exactly once, every
other element zero-weight, the two elements of a pair in columns c, c + 1 of
one row, and no tap in need of a slot index >= 16.  It prints one line per
failure.
"""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "d3_tap_slots_check.cpp")
INC = os.path.join(ROOT, "cnn-super-resolution_amd", "csrc", "hip")
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")


@pytest.mark.skipif(CXX is None, reason="needs a host C++ compiler")
def test_d3_tap_slot_map(tmp_path):
    exe = str(tmp_path / "d3_tap_slots_check")
    c = subprocess.run([CXX, "-std=c++17", "-O2", "-Wall", "-Werror", "-I", INC, SRC, "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert c.returncode == 0, c.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(r.stdout[-4000:])
    failures = [l for l in r.stdout.splitlines() if l.startswith("FAIL")]
    assert failures == [], failures[:20]
    assert r.returncode == 0, r.stdout[-2000:]
    last = r.stdout.strip().splitlines()[-1]
    # 1 + 4 + 9 + 16 + 25 taps over the five filter sizes
    assert last == "filters=5 taps=55 failures=0", last
