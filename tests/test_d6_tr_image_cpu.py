"""The per-wave delta2 part image of d1x6 (csrc/hip/d6tr.hpp) on the host (CPU).

d1x6's delta3 form writes the split parts of delta1's delta2 operand into a
bf16 image and reads gW2's delta2 operand back with transposed LDS reads; both
address maps come from d6tr.hpp.  tests/d6_tr_image_check.cpp includes it with
the device qualifiers defined away, fills the image through the write map with
tagged values for the four waves, models the transposed read's gather (lane
4 i + p of a 16-lane group addresses row i, columns 4 p .. 4 p + 3; lane c
receives column c of the four rows) and checks every element every lane
receives, the alignment and region of every address, that the waves' regions
are disjoint, and the modelled bank-conflict degree of the writes (dword mod
32 per 16 lanes) and of the reads (dword mod 64 per 32 lanes), which may not
pass 2-way.  It prints one line per failure.
"""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "d6_tr_image_check.cpp")
INC = os.path.join(ROOT, "cnn-super-resolution_amd", "csrc", "hip")
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")


@pytest.mark.skipif(CXX is None, reason="needs a host C++ compiler")
def test_d6_tr_image_maps(tmp_path):
    exe = str(tmp_path / "d6_tr_image_check")
    c = subprocess.run([CXX, "-std=c++17", "-O2", "-Wall", "-Werror", "-I", INC, SRC, "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert c.returncode == 0, c.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(r.stdout[-4000:])
    failures = [l for l in r.stdout.splitlines() if l.startswith("FAIL")]
    assert failures == [], failures[:20]
    assert r.returncode == 0, r.stdout[-2000:]
    last = r.stdout.strip().splitlines()[-1]
    # 4 waves x 2 k-steps x 3 parts x 2 reads x 64 lanes x 4 elements; the
    # reads conflict-free, the writes 2-way (slots s and s + 8 of a 16-lane group)
    assert last == "elements=12288 write_degree=2 read_degree=1 failures=0", last
