"""The slot <-> pixel maps of the split-bf16 fused step (csrc/hip/runs.hpp:
run_geom, run_div's float-reciprocal division, run_origin, slot_pixel,
slot_coord) on the host, for every output tile up to 49 x 49 (CPU).

l12x6 stores A1 in this order, d1x6 reads X, A1, A2 and delta3 through it and
srcnn_train_activations undoes it; the GPU parity tests reach it only at the
few tile sizes they run.  tests/run_geometry_check.cpp includes runs.hpp with
the device qualifiers defined away and checks every map exhaustively; it
prints one line per failure.
"""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "run_geometry_check.cpp")
INC = os.path.join(ROOT, "cnn-super-resolution_amd", "csrc", "hip")
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")


@pytest.mark.skipif(CXX is None, reason="needs a host C++ compiler")
def test_run_geometry_maps(tmp_path):
    exe = str(tmp_path / "run_geometry_check")
    # no fast-math, no contraction: the float arithmetic of run_div as written
    c = subprocess.run([CXX, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I", INC, SRC,
                        "-o", exe], capture_output=True, text=True, timeout=300)
    assert c.returncode == 0, c.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:])
    failures = [l for l in r.stdout.splitlines() if l.startswith("FAIL")]
    assert failures == [], failures[:20]
    assert r.returncode == 0, r.stdout[-2000:]
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("tiles=2401 ") and last.endswith(" failures=0"), last
