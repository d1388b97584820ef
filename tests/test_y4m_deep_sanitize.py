"""The Y4M reader on streams of more than 8 bits per sample under
AddressSanitizer + UndefinedBehaviorSanitizer (CPU).

As tests/test_y4m_sanitize.py: host/test/y4m_fuzz.cpp, the stand-alone
deterministic mutation fuzzer with its own main, is compiled here together
with Y4m.cpp (and the image codecs, for image::check_dims) with g++
-fsanitize=address,undefined -fno-sanitize-recover=all and run directly.  The
seeds are C420p10, C422p12 and C444p16 streams, whose frames are twice the
bytes of their sample counts; mutations of the C token also move a stream
between the one-byte and the two-byte sizes.  Every mutation must read to its
end or raise; a crash or a sanitizer report fails the test."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HOST = os.path.join(ROOT, "cnn-super-resolution_amd", "host")


def _seeds(d):
    rng = np.random.default_rng(6)
    out = []
    for name, head, bits, (w, h, cw, ch) in (
            ("a420p10.y4m", "YUV4MPEG2 W37 H23 F30:1 Ip A1:1 C420p10 XYSCSS=420P10", 10, (37, 23, 19, 12)),
            ("b422p12.y4m", "YUV4MPEG2 W18 H7 F25:1 Ip C422p12 XCOLORRANGE=FULL", 12, (18, 7, 9, 7)),
            ("c444p16.y4m", "YUV4MPEG2 W5 H3 C444p16", 16, (5, 3, 5, 3))):
        p = os.path.join(d, name)
        with open(p, "wb") as fh:
            fh.write(head.encode() + b"\n")
            for k in range(3):
                fh.write(b"FRAME Ip\n" if k == 1 else b"FRAME\n")
                fh.write(rng.integers(0, 1 << bits, w * h + 2 * cw * ch).astype("<u2").tobytes())
        out.append(p)
    return out


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_deep_y4m_reader_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "y4m_fuzz")
    src = [os.path.join(HOST, "test", "y4m_fuzz.cpp")] + [os.path.join(HOST, "src", f)
                                                         for f in ("Y4m.cpp", "Image.cpp", "Jpeg.cpp")]
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(HOST, "src")] + src + ["-o", exe, "-lz"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    seeds = _seeds(str(tmp_path))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, "--iters", "400"] + seeds, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = [l for l in r.stdout.splitlines() if "mutations=" in l]
    assert len(lines) == len(seeds)  # 3 x 400 = 1200 mutations
    # the unmutated seeds are read whole (a reader that took them for 8-bit
    # streams would stop at the second FRAME line), and the mutations exercise
    # both outcomes
    ok = sum(int(l.split("read=")[1].split()[0]) for l in lines)
    rej = sum(int(l.split("rejected=")[1].split()[0]) for l in lines)
    assert ok > 100 and rej > 300, lines
