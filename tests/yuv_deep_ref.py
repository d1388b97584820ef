"""Float64 numpy restatement of the frame formats of DESIGN.md 15 (8 to 16 bits
per sample, planar or semi-planar chroma), the yardstick of
tests/test_yuv_deep_cpu.py and tests/test_yuv_deep_gpu.py.  Built on yuv_ref
 and upscale_ref.bicubic.

A sample of more than 8 bits is a 16-bit word x: the value is x (msb 0,
nothing masked) or x >> (16 - bits) (msb 1); a written value q is stored as q
or as q << (16 - bits).  Limited range: (16, 219) * 2^(bits-8); full range:
(0, 2^bits - 1).  Rounding is to nearest, ties to even, then the clamp to
[0, 2^bits - 1].  `raw` values are the unrounded, unclipped ones, in units of
the sample value (not of the word)."""
import numpy as np

import upscale_ref as U
import yuv_ref as R

FULL, LIMITED = R.FULL, R.LIMITED
chroma_size = R.chroma_size


def levels(bits, yuv_range):
    """(offset, gain): luma = (Y - offset) / gain."""
    if yuv_range == FULL:
        return 0.0, float((1 << bits) - 1)
    off, gain = R.RANGES[LIMITED]
    return off * (1 << (bits - 8)), gain * (1 << (bits - 8))


def dtype(bits):
    return np.uint8 if bits == 8 else np.uint16


def shift(bits, msb):
    assert 8 <= bits <= 16 and msb in (0, 1) and not (msb and bits == 8), (bits, msb)
    return 16 - bits if msb else 0


def decode(x, bits, msb):
    """words -> sample values (int64)"""
    return np.asarray(x).astype(np.int64) >> shift(bits, msb)


def encode(q, bits, msb):
    """sample values 0 .. 2^bits - 1 -> words"""
    return (np.asarray(q).astype(np.int64) << shift(bits, msb)).astype(dtype(bits))


def quantise(raw, bits, msb):
    return encode(np.clip(np.rint(raw), 0, (1 << bits) - 1), bits, msb)


def luma_plane(x, s, pad, bits, msb, yuv_range):
    """Y words [h][w] -> the padded plane [(s*h+pad)][(s*w+pad)]: bicubic of the
    normalised luma, edge replicated, margin pad // 2 on the left and top."""
    off, gain = levels(bits, yuv_range)
    up = U.bicubic((decode(x, bits, msb).astype(np.float64) - off) / gain, s)
    H, W = up.shape
    m = pad // 2
    ys = np.clip(np.arange(H + pad) - m, 0, H - 1)
    xs = np.clip(np.arange(W + pad) - m, 0, W - 1)
    return up[np.ix_(ys, xs)]


def planes(p, s, ow, oh, bits, msb):
    """p [..., ph, pw] words -> (words, raw) [..., oh, ow]: the top-left ow x oh
    of the bicubic x s of each plane's values; s*(pw-1) < ow <= s*pw, rows
    likewise."""
    p = np.asarray(p)
    ph, pw = p.shape[-2:]
    assert s * (pw - 1) < ow <= s * pw and s * (ph - 1) < oh <= s * ph, (p.shape, s, ow, oh)
    flat = decode(p, bits, msb).astype(np.float64).reshape((-1, ph, pw))
    raw = np.stack([U.bicubic(a, s)[:oh, :ow] for a in flat]).reshape(p.shape[:-2] + (oh, ow))
    return quantise(raw, bits, msb), raw


def interleave(p):
    """two planes [2][h][w] -> the semi-planar plane [h][2 * w] of (U, V) pairs"""
    p = np.asarray(p)
    return np.ascontiguousarray(np.moveaxis(p, 0, -1)).reshape(p.shape[1], 2 * p.shape[2])


def deinterleave(a):
    """[h][2 * w] -> [2][h][w]"""
    a = np.asarray(a)
    return np.ascontiguousarray(np.moveaxis(a.reshape(a.shape[0], -1, 2), -1, 0))


def compose_luma(v, bits, msb, yuv_range):
    """luma [H][W] -> (Y words, raw)."""
    off, gain = levels(bits, yuv_range)
    raw = np.asarray(v, np.float64) * gain + off
    return quantise(raw, bits, msb), raw


def near_boundary(raw, band):
    """where raw is within `band` of a rounding boundary k + 0.5"""
    return np.abs(raw - np.floor(raw) - 0.5) <= band
