"""Float64 numpy restatement of the any-size resampling spec,
the yardstick of tests/test_resize_cpu.py and tests/test_resize_gpu.py.  Built
on upscale_ref (keys, luma, composition), yuv_ref (14.1) and
yuv_deep_ref (15: sample formats and ranges).

One axis: the source step per output sample is the fraction rn / rd with
1 <= rd / rn <= 4.  For output index X: n = (2X+1) rn - rd, D = 2 rd,
b = floor(n / D), t = (n - b D) / D in [0, 1); taps b-1 .. b+2 clamped to the
source, weights the Keys cubic at t+1, t, 1-t, 2-t.  Integers are exact
(Python's), the one division is a correctly rounded double, weights and sums
stay in float64 (the library rounds the weights once to fp32).  A ratio is a
pair (rn, rd).  `raw` values are the unrounded, unclipped ones.

The module also holds what the two test files share: the cases and the inputs
drawn for them."""
import functools

import numpy as np

import upscale_ref as U
import yuv_deep_ref as D


def phase(X, rn, rd):
    """(b, [4 weights]) of output index X at ratio rn / rd."""
    n = (2 * int(X) + 1) * int(rn) - int(rd)
    den = 2 * int(rd)
    b = n // den
    t = (n - b * den) / den
    return b, [U.keys(t + 1), U.keys(t), U.keys(1 - t), U.keys(2 - t)]


def matrix(n, N, rn, rd):
    """(N, n) float64 resampling matrix of one axis, taps clamped to [0, n-1]."""
    assert rn > 0 and rn <= rd <= 4 * rn, (rn, rd)
    M = np.zeros((N, n))
    for X in range(N):
        b, w = phase(X, rn, rd)
        for i in range(4):
            M[X, min(max(b - 1 + i, 0), n - 1)] += w[i]
    return M


def resize(a, W, H, rx, ry):
    """a [h][w] -> [H][W] at the ratios rx, ry; separable, float64."""
    a = np.asarray(a, np.float64)
    return matrix(a.shape[0], H, *ry) @ a @ matrix(a.shape[1], W, *rx).T


def pad_plane(up, pad):
    """edge replication of [H][W] into [(H+pad)][(W+pad)], margin pad // 2 on the left and top"""
    H, W = up.shape
    m = pad // 2
    return up[np.ix_(np.clip(np.arange(H + pad) - m, 0, H - 1), np.clip(np.arange(W + pad) - m, 0, W - 1))]


def luma_plane(rgba, W, H, pad):
    """rgba [h][w][4] u8 -> the padded plane [(H+pad)][(W+pad)] of the resized luma."""
    h, w = np.asarray(rgba).shape[:2]
    return pad_plane(resize(U.source_luma(rgba), W, H, (w, W), (h, H)), pad)


def yuv_luma_plane(x, W, H, pad, bits, msb, yuv_range):
    """Y words [h][w] -> the padded plane of the resized normalised luma."""
    off, gain = D.levels(bits, yuv_range)
    v = (D.decode(x, bits, msb).astype(np.float64) - off) / gain
    h, w = v.shape
    return pad_plane(resize(v, W, H, (w, W), (h, H)), pad)


def compose(rgba, new_luma, W, H):
    """(rgb [H][W][3] u8, the unclipped, untruncated float64 channel values):
    resized r, g, b + new_luma * 255 through swap_luma's constants."""
    c = np.asarray(rgba, np.float64)
    h, w = c.shape[:2]
    r, g, b = (resize(c[..., i], W, H, (w, W), (h, H)) for i in range(3))
    Y = np.asarray(new_luma, np.float64) * 255.0
    cb = U.CB[0] * r + U.CB[1] * g + U.CB[2] * b
    cr = U.CR[0] * r + U.CR[1] * g + U.CR[2] * b
    raw = np.stack([Y + U.R_CR * cr, Y + U.G_CB * cb + U.G_CR * cr, Y + U.B_CB * cb], axis=-1)
    return np.trunc(np.clip(raw, 0.0, 255.0)).astype(np.uint8), raw


def planes(p, ow, oh, rx, ry, bits=8, msb=0):
    """p [..., ph, pw] words -> (words, raw) [..., oh, ow] at the ratios rx, ry;
    ow <= ceil(pw * rd / rn), rows likewise."""
    p = np.asarray(p)
    ph, pw = p.shape[-2:]
    assert ow <= -(-pw * rx[1] // rx[0]) and oh <= -(-ph * ry[1] // ry[0]), (p.shape, ow, oh, rx, ry)
    flat = D.decode(p, bits, msb).astype(np.float64).reshape((-1, ph, pw))
    raw = np.stack([resize(a, ow, oh, rx, ry) for a in flat]).reshape(p.shape[:-2] + (oh, ow))
    return D.quantise(raw, bits, msb), raw


def frame(y, uv, W, H, cx, cy, pad, bits, msb, yuv_range):
    """A frame's Y words [h][w] and chroma words uv [2][ch][cw] -> (the padded
    luma plane, the output chroma words [2][CH][CW], their raw values): the
    chroma at the luma's ratios w / W and h / H."""
    h, w = np.asarray(y).shape
    CW, CH = D.chroma_size(W, H, cx, cy)
    assert np.asarray(uv).shape[1:] == D.chroma_size(w, h, cx, cy)[::-1]
    q, raw = planes(uv, CW, CH, (w, W), (h, H), bits, msb)
    return yuv_luma_plane(y, W, H, pad, bits, msb, yuv_range), q, raw


# ---- what tests/test_resize_cpu.py and tests/test_resize_gpu.py share ----
# (w, h) -> (W, H).  A workgroup of resize.hip owns a tile of 64 x 16 outputs
# (of the padded plane for the luma): every tap clamps, below the 4-tap support
# with a ratio per axis, a small source, ratios 2.35 and 1.44, more than one
# tile, 720p's exact 3/2, the x4 limit, three or more tiles each way with a
# ragged last one, an integer ratio.
CASES = [((1, 1), (1, 1)), ((1, 1), (3, 4)), ((2, 3), (3, 7)), ((5, 4), (7, 9)), ((17, 9), (40, 13)),
         ((37, 23), (53, 52)), ((48, 32), (72, 48)), ((33, 10), (132, 40)), ((135, 37), (203, 56)),
         ((135, 37), (270, 74))]
CASE_IDS = ["%dx%d-%dx%d" % (c[0] + c[1]) for c in CASES]
# a chroma case: the planes, their output size and the two ratios.  The ten
# cases as planes of their own, and the 19 x 12 -> 28 x 18 chroma of the odd
# 4:2:0 frame 37 x 23 -> 55 x 35, at the luma's ratios.
PLANE_CASES = [(c[0], c[1], (c[0][0], c[1][0]), (c[0][1], c[1][1])) for c in CASES] + \
              [((19, 12), (28, 18), (37, 55), (23, 35))]
PLANE_IDS = CASE_IDS + ["19x12-28x18-of-37x23-55x35"]
RGBA_SEED, LUMA_SEED = 0, 3
PLANE_SEEDS = {8: 1, 10: 2, 16: 2}
# (band around a rounding boundary, cap on the exempt share of a case)
COMPOSE_BAND, COMPOSE_CAP = 2e-3, 0.01
PLANE_BANDS = {8: (2e-3, 0.01), 10: (8e-3, 0.025)}


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def rgba_of(w, h):
    return _frozen(np.random.default_rng(RGBA_SEED).integers(0, 256, (h, w, 4), dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def new_luma_of(W, H):
    return _frozen(np.random.default_rng(LUMA_SEED).uniform(-0.1, 1.1, (H, W)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def y_of(w, h, bits):
    """sample values, not words"""
    return _frozen(np.random.default_rng(0).integers(0, 1 << bits, (h, w)).astype(D.dtype(bits)))


@functools.lru_cache(maxsize=None)
def planes_of(pw, ph, bits):
    """sample values of two planes (the int64 draw, cast)"""
    return _frozen(np.random.default_rng(PLANE_SEEDS[bits]).integers(0, 1 << bits, (2, ph, pw)).astype(D.dtype(bits)))


@functools.lru_cache(maxsize=None)
def ref_compose(w, h, W, H):
    q, raw = compose(rgba_of(w, h), new_luma_of(W, H), W, H)
    return _frozen(q), _frozen(raw)


@functools.lru_cache(maxsize=None)
def ref_planes(pw, ph, ow, oh, rx, ry, bits):
    """(values, raw) of the reference, shared by the word layouts"""
    q, raw = planes(planes_of(pw, ph, bits), ow, oh, rx, ry, bits, 0)
    return _frozen(q), _frozen(raw)


def near_integer(raw, band):
    return np.abs(raw - np.rint(raw)) <= band
