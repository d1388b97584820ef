"""CPU-side checks of the deep and semi-planar frame formats: the
fp32 round trip of every sample value, the float64 reference
(tests/yuv_deep_ref.py) against itself and against tests/yuv_ref.py at 8 bits,
the exempt shares tests/test_yuv_deep_gpu.py relies on, and Y4M streams of
more than 8 bits through bin/y4m_tool.  No device needed."""
import os
import subprocess

import numpy as np
import pytest

import yuv_deep_ref as D
import yuv_ref as R
from conftest import ROOT

TOOL = os.path.join(ROOT, "cnn-super-resolution_amd", "bin", "y4m_tool")
SHAPES = [(1, 1), (2, 3), (5, 4), (17, 9), (37, 23), (135, 37)]
PLANES_SEED = 3
COMPOSE_SEEDS = {10: 0, 12: 0, 16: 2}


# ---- the arithmetic of the spec in fp32 ----
@pytest.mark.parametrize("yuv_range", [D.FULL, D.LIMITED])
@pytest.mark.parametrize("bits", range(9, 17))
def test_fp32_round_trip_is_exact_for_every_value(bits, yuv_range):
    """Y -> v = (float(Y) - off) / gain -> rint(fma(v, gain, off)) gives Y back
    for every Y in 0 .. 2^bits - 1: the division errs by half an ulp of v,
    which times gain stays far below the 0.5 that would change the rounding.
    The fma is one rounding of the exact v * gain + off, which float64 holds
    exactly (24 + 16 bits)."""
    off, gain = (np.float32(a) for a in D.levels(bits, yuv_range))
    assert float(off) == D.levels(bits, yuv_range)[0] and float(gain) == D.levels(bits, yuv_range)[1]
    y = np.arange(1 << bits, dtype=np.int64)
    v = (y.astype(np.float32) - off) / gain
    assert v.dtype == np.float32
    back = np.rint((v.astype(np.float64) * float(gain) + float(off)).astype(np.float32))
    assert np.array_equal(back.astype(np.int64), y)
    # and the reference's own round trip, through both word layouts
    sq = y.reshape(-1, 1 << (bits // 2))  # (a small matrix: the reference resamples with dense matrices)
    for msb in (0, 1):
        words = D.encode(sq, bits, msb)
        assert np.array_equal(D.decode(words, bits, msb), sq)
        got, _ = D.compose_luma(D.luma_plane(words, 1, 0, bits, msb, yuv_range), bits, msb, yuv_range)
        assert np.array_equal(got, words)
        if msb:
            assert not (words & ((1 << (16 - bits)) - 1)).any()


def test_8_bits_is_the_8_bit_reference():
    rng = np.random.default_rng(0)
    y = rng.integers(0, 256, (9, 17), dtype=np.uint8)
    for r in (D.FULL, D.LIMITED):
        assert D.levels(8, r) == R.RANGES[r]
        assert np.array_equal(D.luma_plane(y, 3, 7, 8, 0, r), R.luma_plane(y, 3, 7, r))
        v = rng.uniform(-0.1, 1.1, (5, 7))
        assert np.array_equal(D.compose_luma(v, 8, 0, r)[0], R.compose_luma(v, r)[0])
    p = rng.integers(0, 256, (2, 12, 19), dtype=np.uint8)
    a, b = D.planes(p, 2, 37, 23, 8, 0), R.planes_u8(p, 2, 37, 23)
    assert a[0].dtype == np.uint8 and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_layouts_and_word_positions():
    rng = np.random.default_rng(1)
    p = rng.integers(0, 1 << 10, (2, 4, 5)).astype(np.uint16)
    il = D.interleave(p)
    assert il.shape == (4, 10) and np.array_equal(il[:, 0::2], p[0]) and np.array_equal(il[:, 1::2], p[1])
    assert np.array_equal(D.deinterleave(il), p)
    # scale 1 is the identity, in both word layouts; msb words keep their low bits zero
    for msb in (0, 1):
        w = D.encode(p, 10, msb)
        out, raw = D.planes(w, 1, 5, 4, 10, msb)
        assert np.array_equal(out, w) and np.array_equal(raw, p)
    out, _ = D.planes(D.encode(p, 10, 1), 3, 15, 12, 10, 1)
    assert not (out & 63).any() and np.array_equal(out >> 6, D.planes(p, 3, 15, 12, 10, 0)[0])
    # lsb words are used as they are: a 10-bit stream holding 11-bit values is not masked
    big = np.full((1, 3, 3), 1500, np.uint16)
    out, raw = D.planes(big, 2, 6, 6, 10, 0)
    assert np.allclose(raw, 1500) and (out == 1023).all()
    with pytest.raises(AssertionError):
        D.shift(8, 1)


# ---- the exempt shares of tests/test_yuv_deep_gpu.py, on the reference alone ----
def test_gpu_test_seeds_keep_their_exemptions_within_the_conditions():
    """Chroma (band 2e-3 * 2^(bits-8)): at most 2.5 % of a case at 10 bits, 10 %
    at 12; the worst cases are the cropped 19 x 12 -> 37 x 23 one (2.06 %) and
    5 x 4 at scale 2 (8.13 %).  Compose (band 1e-4 * 2^(bits-8)): 0.25 %, 0.5 %
    and 7 % at 10, 12 and 16 bits; worst 0.18 %, 0.42 % and 5.3 %."""
    for bits, cond, want in ((10, 0.025, 0.0206), (12, 0.10, 0.0813)):
        band, worst = 2e-3 * 2 ** (bits - 8), 0.0
        cases = [(pw, ph, s, s * pw, s * ph) for pw, ph in SHAPES for s in (2, 3, 4)] + [(19, 12, 2, 37, 23)]
        for pw, ph, s, ow, oh in cases:
            p = np.random.default_rng(PLANES_SEED).integers(0, 1 << bits, (2, ph, pw)).astype(np.uint16)
            _, raw = D.planes(p, s, ow, oh, bits, 0)
            worst = max(worst, float(D.near_boundary(raw, band).mean()))
        print("chroma, %d bits: worst exempt share %.4f" % (bits, worst))
        assert worst <= cond and abs(worst - want) < 1e-4, (bits, worst)
    for bits, cond, want in ((10, 0.0025, 0.0018), (12, 0.005, 0.0042), (16, 0.07, 0.053)):
        band, worst = 1e-4 * 2 ** (bits - 8), 0.0
        for W, H in SHAPES + [(1100, 3)]:
            v = np.random.default_rng(COMPOSE_SEEDS[bits]).uniform(-0.1, 1.1, (H, W)).astype(np.float32)
            for r in (D.FULL, D.LIMITED):
                _, raw = D.compose_luma(v, bits, 0, r)
                worst = max(worst, float(D.near_boundary(raw, band).mean()))
        print("compose, %d bits: worst exempt share %.4f" % (bits, worst))
        assert worst <= cond and abs(worst - want) < 5e-4, (bits, worst)


# ---- Y4M ----
def y4m_bytes(w, h, chroma, frames, tokens="F30:1 Ip A1:1", seed=0):
    cx, cy = {"420": (2, 2), "422": (2, 1), "444": (1, 1)}[chroma[:3]]
    bits = int(chroma[4:])
    cw, ch = D.chroma_size(w, h, cx, cy)
    rng = np.random.default_rng(seed)
    head = "YUV4MPEG2 W%d H%d %s C%s" % (w, h, tokens, chroma)
    data = [rng.integers(0, 1 << bits, w * h + 2 * cw * ch).astype("<u2").tobytes() for _ in range(frames)]
    return (head + "\n").encode() + b"".join(b"FRAME\n" + d for d in data), data


def run_tool(tmp_path, raw):
    src, dst = tmp_path / "in.y4m", tmp_path / "out.y4m"
    src.write_bytes(raw)
    p = subprocess.run([TOOL, str(src), str(dst)], capture_output=True, text=True, timeout=60)
    return p, (dst.read_bytes() if dst.exists() else b"")


@pytest.mark.parametrize("chroma", ["420p10", "422p12", "444p16"])
@pytest.mark.parametrize("w,h", [(37, 23), (1, 1)])
def test_deep_y4m_round_trip(tmp_path, chroma, w, h):
    raw, data = y4m_bytes(w, h, chroma, 3)
    p, out = run_tool(tmp_path, raw)
    assert p.returncode == 0, p.stdout
    cx, cy = {"420": (2, 2), "422": (2, 1), "444": (1, 1)}[chroma[:3]]
    assert p.stdout.split() == [str(w), str(h), str(cx), str(cy), "limited", "3", chroma[4:]]
    assert out == raw  # same tokens (the C token with its depth), same two-byte samples


@pytest.mark.parametrize("chroma", ["420p9", "420p14", "422p10", "444p9", "444p14"])
def test_other_deep_y4m_formats_are_read(tmp_path, chroma):
    raw, data = y4m_bytes(5, 3, chroma, 1)
    p, out = run_tool(tmp_path, raw)
    assert p.returncode == 0 and p.stdout.split()[-1] == chroma[4:] and out == raw, p.stdout


@pytest.mark.parametrize("chroma", ["420p8", "420p11", "420p17", "420p", "420p1x", "411p10", "monop10", "mono16"])
def test_unknown_depths_are_rejected(tmp_path, chroma):
    raw = b"YUV4MPEG2 W4 H4 C" + chroma.encode() + b"\nFRAME\n" + bytes(64)
    p, out = run_tool(tmp_path, raw)
    assert p.returncode == 1 and "[ERROR]" in p.stdout, p.stdout


def test_truncated_deep_frame_is_an_error_after_the_whole_ones(tmp_path):
    raw, data = y4m_bytes(37, 23, "420p10", 3)
    one = len(b"FRAME\n") + len(data[0])
    assert len(data[0]) == 2 * (37 * 23 + 2 * 19 * 12)
    head = len(raw) - 3 * one
    p, out = run_tool(tmp_path, raw[:head + 2 * one + one // 2])
    assert p.returncode == 1 and "truncated" in p.stdout
    assert p.stdout.split()[-2:] == ["2", "10"]
    assert out == raw[:head + 2 * one]
    # a frame of the 8-bit size under a deep header is half a frame
    p, out = run_tool(tmp_path, raw[:head] + b"FRAME\n" + data[0][:len(data[0]) // 2])
    assert p.returncode == 1 and "truncated" in p.stdout and p.stdout.split()[-2:] == ["0", "10"]
