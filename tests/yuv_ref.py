"""Float64 numpy restatement of the Y'CbCr upscale spec, the
yardstick of tests/test_yuv_cpu.py and tests/test_yuv_gpu.py.  The resampling
is upscale_ref.bicubic.

Range: full maps a Y byte to Y / 255 and back by rint(v * 255); limited maps it
to (Y - 16) / 219 and back by rint(v * 219 + 16).  Rounding is to nearest, ties
to even (numpy's rint), then the clamp to [0, 255].  `raw` values are the
unrounded, unclipped ones."""
import numpy as np

import upscale_ref as U

FULL, LIMITED = "full", "limited"
# (offset, gain) of a range: luma = (Y - offset) / gain
RANGES = {FULL: (0.0, 255.0), LIMITED: (16.0, 219.0)}


def chroma_size(w, h, cx, cy):
    """(cw, ch) of a w x h frame subsampled by cx x cy."""
    return -(-w // cx), -(-h // cy)


def luma_plane(y, s, pad, yuv_range):
    """Y [h][w] u8 -> the padded plane [(s*h+pad)][(s*w+pad)]: bicubic of the
    normalised luma, edge replicated, margin pad // 2 on the left and top."""
    off, gain = RANGES[yuv_range]
    up = U.bicubic((np.asarray(y, np.float64) - off) / gain, s)
    H, W = up.shape
    m = pad // 2
    ys = np.clip(np.arange(H + pad) - m, 0, H - 1)
    xs = np.clip(np.arange(W + pad) - m, 0, W - 1)
    return up[np.ix_(ys, xs)]


def planes_u8(p, s, ow, oh):
    """p [..., ph, pw] u8 -> (u8, raw) [..., oh, ow]: the top-left ow x oh of the
    bicubic x s of each plane; s*(pw-1) < ow <= s*pw, rows likewise."""
    p = np.asarray(p)
    ph, pw = p.shape[-2:]
    assert s * (pw - 1) < ow <= s * pw and s * (ph - 1) < oh <= s * ph, (p.shape, s, ow, oh)
    flat = p.reshape((-1, ph, pw))
    raw = np.stack([U.bicubic(a, s)[:oh, :ow] for a in flat]).reshape(p.shape[:-2] + (oh, ow))
    return np.clip(np.rint(raw), 0, 255).astype(np.uint8), raw


def compose_luma(v, yuv_range):
    """luma [H][W] -> (Y u8, raw)."""
    off, gain = RANGES[yuv_range]
    raw = np.asarray(v, np.float64) * gain + off
    return np.clip(np.rint(raw), 0, 255).astype(np.uint8), raw
