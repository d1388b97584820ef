"""Float64 numpy restatement of the downscale / tile-grid spec,
the yardstick of tests/test_pairs_cpu.py and tests/test_pairs_gpu.py.

Downscale by integer s: output index j has its centre at source coordinate
c = s*j + (s-1)/2; taps are the source indices s*j + o for every integer o with
|o - (s-1)/2| / s < 2, clamped to the source; the weight is the Keys cubic
(a = -0.5, upscale_ref.keys) at (o - (s-1)/2) / s, divided by the sum over o.
Rows likewise, horizontal pass first; byte = floor(clip(v, 0, 255) + 0.5).
Weights and sums stay in float64 here (the library rounds the weights once to
fp32)."""
import numpy as np

import upscale_ref as U


def taps(s):
    """(first offset o, [weights]) of scale s: 3 / 8 / 11 / 16 taps at s = 1 .. 4."""
    c = (s - 1) / 2.0
    os_ = [o for o in range(-3 * s, 4 * s + 1) if abs(o - c) / s < 2]
    k = [U.keys((o - c) / s) for o in os_]
    assert os_ == list(range(os_[0], os_[0] + len(os_)))
    total = sum(k)
    return os_[0], [v / total for v in k]


def matrix(n, s):
    """(n // s, n) float64 downscale matrix of one axis, taps clamped to [0, n-1]."""
    o0, w = taps(s)
    M = np.zeros((n // s, n))
    for j in range(n // s):
        for i, wt in enumerate(w):
            M[j, min(max(s * j + o0 + i, 0), n - 1)] += wt
    return M


def down(a, s):
    """a [H][W] -> [H // s][W // s], separable, float64, not rounded."""
    a = np.asarray(a, np.float64)
    return matrix(a.shape[0], s) @ a @ matrix(a.shape[1], s).T


def quantise(v):
    """round to nearest, halves up, of the value clipped to [0, 255]"""
    return np.floor(np.clip(v, 0.0, 255.0) + 0.5).astype(np.uint8)


def down_rgba(rgba, s):
    """(small [H//s][W//s][4] u8 with alpha 255, the unrounded float64 r, g, b
    [H//s][W//s][3]) of rgba [H][W][4] u8."""
    c = np.asarray(rgba, np.float64)
    raw = np.stack([down(c[..., i], s) for i in range(3)], axis=-1)
    small = np.full(raw.shape[:2] + (4,), 255, np.uint8)
    small[..., :3] = quantise(raw)
    return small, raw


def tile_grid(W, H, s, tile, stride):
    """(nx, ny) of srcnn_make_pairs' grid on a W x H image, (0, 0) if none fits."""
    if not (1 <= s <= 4) or W < s or H < s or tile <= 0 or stride <= 0:
        return 0, 0
    Wc, Hc = W // s * s, H // s * s
    if tile > Wc or tile > Hc:
        return 0, 0
    return (Wc - tile) // stride + 1, (Hc - tile) // stride + 1


def windows(plane, x0, y0, stride, nx, ny, tw, th):
    """[nx*ny][th][tw]: tile iy*nx + ix is the window at (x0 + ix*stride, y0 + iy*stride)."""
    plane = np.asarray(plane)
    return np.stack([plane[y0 + iy * stride:y0 + iy * stride + th, x0 + ix * stride:x0 + ix * stride + tw]
                     for iy in range(ny) for ix in range(nx)])
