"""Float64 numpy restatement of the downscale of a Y'CbCr frame's planes
(DESIGN.md 18.1), the yardstick of tests/test_frame_down_cpu.py and
tests/test_frame_down_gpu.py.  Built on pairs_ref.taps, with
yuv_deep_ref's sample formats and quality_frame_ref.pack for frames.

A plane [PH][PW] of code values goes to [oh][ow], ow <= ceil(PW / s), oh <=
ceil(PH / s): output j takes the source indices s*j + o of pairs_ref.taps(s),
clamped to the plane, with its weights; rows likewise, horizontal pass first,
nothing rounded in between.  The sample is clip(rint(v), 0, 2^bits - 1), ties
to even.  `raw` values are the unrounded ones, in code values.

cases() lists what both tests run; seed_of() is the seed search both make, so
that the GPU test cannot fail for want of a seed."""
import functools

import numpy as np

import pairs_ref as P
import quality_frame_ref as QF
import yuv_deep_ref as D

ceil_div = QF.ceil_div


def matrix(n, s, out):
    """(out, n) float64 downscale matrix of one axis, out <= ceil(n / s), taps clamped to [0, n-1]."""
    assert 1 <= out <= ceil_div(n, s), (n, s, out)
    o0, w = P.taps(s)
    M = np.zeros((out, n))
    for j in range(out):
        for i, wt in enumerate(w):
            M[j, min(max(s * j + o0 + i, 0), n - 1)] += wt
    return M


def down(a, s, ow, oh):
    """code values a [PH][PW] -> raw [oh][ow], float64"""
    a = np.asarray(a, np.float64)
    return matrix(a.shape[0], s, oh) @ a @ matrix(a.shape[1], s, ow).T


def planes(p, s, ow, oh, bits, msb):
    """p [..., ph, pw] words -> (words, raw) [..., oh, ow]"""
    p = np.asarray(p)
    ph, pw = p.shape[-2:]
    flat = D.decode(p, bits, msb).astype(np.float64).reshape((-1, ph, pw))
    raw = np.stack([down(a, s, ow, oh) for a in flat]).reshape(p.shape[:-2] + (oh, ow))
    return D.quantise(raw, bits, msb), raw


def frame_sizes(W, H, s, cx, cy):
    """(w, h), the source's chroma (CW, CH), the output's (cw, ch)"""
    w, h = W // s, H // s
    return (w, h), (ceil_div(W, cx), ceil_div(H, cy)), (ceil_div(w, cx), ceil_div(h, cy))


def frame(A, s, bits, cx, cy):
    """(Y, U, V) code values of a W x H frame -> the small frame's (Y, U, V)
    (int64) and their raw values"""
    H, W = A[0].shape
    (w, h), _, (cw, ch) = frame_sizes(W, H, s, cx, cy)
    raws = [down(A[0], s, w, h), down(A[1], s, cw, ch), down(A[2], s, cw, ch)]
    return tuple(np.clip(np.rint(r), 0, (1 << bits) - 1).astype(np.int64) for r in raws), raws


# ---- the exempt band of a device-against-reference comparison ----
# downscale_rgba's chain scaled to the sample magnitude: at
# most 68 roundings of half an ulp at magnitude < 2^(bits+1)
def band(bits):
    return 1e-3 * 2.0 ** (bits - 8)


CAP = {8: 0.01, 10: 0.025, 12: 0.10}  # the share of a case that may be exempt


def near_half(raw, bits):
    return D.near_boundary(raw, band(bits))


# ---- the cases of both tests ----
# output shapes: one sample, fewer than a tile, and 135 x 37, which spans five
# tiles of 32 columns and three (s <= 2) or five tiles of 16 / 8 rows, the last
# of each ragged; for pairs the tile is 16 wide
SHAPES = [(1, 1), (2, 3), (5, 4), (17, 9), (37, 23), (135, 37)]
SCALES = [2, 3, 4]
BITS = [8, 10, 12, 16]
# the source of an ow x oh output: exactly s times as large; with s - 1
# trailing columns and rows that are tap sources only; and s - 1 columns and
# rows short, so that ow = ceil(PW / s) > PW / s and the last cell is cut
VARIANTS = ["exact", "trailing", "cut"]
SEEDS = range(8)


def source_size(ow, oh, s, variant):
    d = {"exact": 0, "trailing": s - 1, "cut": 1 - s}[variant]
    return s * ow + d, s * oh + d


@functools.lru_cache(maxsize=None)
def values_of(pw, ph, bits, seed):
    """two planes [2][ph][pw] of code values, uniform over the whole code range"""
    a = np.random.default_rng(seed).integers(0, 1 << bits, (2, ph, pw)).astype(D.dtype(bits))
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def reference(ow, oh, s, variant, bits, seed):
    """(source values [2][ph][pw], q [2][oh][ow], raw, near)"""
    pw, ph = source_size(ow, oh, s, variant)
    src = values_of(pw, ph, bits, seed)
    q, raw = planes(src, s, ow, oh, bits, 0)
    near = near_half(raw, bits)
    for a in (q, raw, near):
        a.setflags(write=False)
    return src, q, raw, near


@functools.lru_cache(maxsize=None)
def seed_of(ow, oh, s, variant, bits):
    """the first seed for which the reference alone stays within the cap (16
    bits: no cap, the band approaches half a code value), None if there is none"""
    if bits not in CAP:
        return 0
    for seed in SEEDS:
        if reference(ow, oh, s, variant, bits, seed)[3].mean() <= CAP[bits]:
            return seed
    return None


def cases():
    return [(ow, oh, s, v) for ow, oh in SHAPES for s in SCALES for v in VARIANTS]


# ---- ramps (alignment) ----
def ramp(W, H, ax, ay):
    """Y = ax*x + ay*y + 16"""
    y, x = np.mgrid[0:H, 0:W]
    return ax * x + ay * y + 16


RAMPS = [(88, 60, 2, 1), (60, 88, 1, 2)]  # (W, H, ax, ay): at most 249, a valid 8-bit code
