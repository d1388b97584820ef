"""Float64 numpy restatement of the upscale resampling spec,
the yardstick of tests/test_upscale_cpu.py and tests/test_upscale_gpu.py.

For a hi-res index X' of scale s: j = X' // s, k = X' % s, d = (k+0.5)/s - 0.5,
b = floor(d), t = d - b; taps j+b-1 .. j+b+2 clamped to the source, weights the
Keys cubic (a = -0.5) at distances t+1, t, 1-t, 2-t.  Rows likewise.  Weights
and sums stay in float64 here (the library rounds the weights once to fp32)."""
import numpy as np

# the fp32 constants of extract_luma_kernel / swap_luma_kernel, as doubles
_F = lambda v: float(np.float32(v))
LUMA = (_F(0.299), _F(0.587), _F(0.114))
CB = (_F(-0.1687), _F(-0.3312), _F(0.5))
CR = (_F(0.5), _F(-0.4186), _F(-0.0813))
R_CR, G_CB, G_CR, B_CB = _F(1.4), _F(-0.343), _F(-0.711), _F(1.765)


def keys(x):
    x = abs(x)
    if x <= 1:
        return (1.5 * x - 2.5) * x * x + 1
    if x < 2:
        return ((-0.5 * x + 2.5) * x - 4) * x + 2
    return 0.0


def phase(s, k):
    """(b, [4 weights]) of phase k at scale s."""
    d = (k + 0.5) / s - 0.5
    b = int(np.floor(d))
    t = d - b
    return b, [keys(t + 1), keys(t), keys(1 - t), keys(2 - t)]


def matrix(n, s):
    """(s*n, n) float64 resampling matrix of one axis, taps clamped to [0, n-1]."""
    M = np.zeros((s * n, n))
    for X in range(s * n):
        j, k = divmod(X, s)
        b, w = phase(s, k)
        for i in range(4):
            M[X, min(max(j + b - 1 + i, 0), n - 1)] += w[i]
    return M


def bicubic(a, s):
    """a [h][w] -> [s*h][s*w], separable, float64."""
    a = np.asarray(a, np.float64)
    return matrix(a.shape[0], s) @ a @ matrix(a.shape[1], s).T


def source_luma(rgba):
    """(0.299f r + 0.587f g + 0.114f b) / 255 of rgba [h][w][4] u8, float64."""
    c = np.asarray(rgba, np.float64)
    return (LUMA[0] * c[..., 0] + LUMA[1] * c[..., 1] + LUMA[2] * c[..., 2]) / 255.0


def luma_plane(rgba, s, pad):
    """The padded plane [(s*h+pad)][(s*w+pad)]: bicubic luma, edge replicated,
    margin pad // 2 on the left and top."""
    up = bicubic(source_luma(rgba), s)
    H, W = up.shape
    m = pad // 2
    ys = np.clip(np.arange(H + pad) - m, 0, H - 1)
    xs = np.clip(np.arange(W + pad) - m, 0, W - 1)
    return up[np.ix_(ys, xs)]


def compose(rgba, new_luma, s):
    """(rgb [s*h][s*w][3] u8, the unclipped, untruncated float64 channel
    values): bicubic r, g, b + new_luma * 255 through swap_luma's constants."""
    c = np.asarray(rgba, np.float64)
    r, g, b = (bicubic(c[..., i], s) for i in range(3))
    Y = np.asarray(new_luma, np.float64) * 255.0
    cb = CB[0] * r + CB[1] * g + CB[2] * b
    cr = CR[0] * r + CR[1] * g + CR[2] * b
    raw = np.stack([Y + R_CR * cr, Y + G_CB * cb + G_CR * cr, Y + B_CB * cb], axis=-1)
    return np.trunc(np.clip(raw, 0.0, 255.0)).astype(np.uint8), raw
