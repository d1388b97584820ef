"""The yardstick of srcnn_quality: DESIGN.md 12.1 in numpy.

quality(a, b, shave, dtype) returns (mse, psnr, ssim) of two images, each a
uint8 array [H][W][3] (RGB8) or [H][W][4] (RGBA8) or a float32 array [H][W]
(normalised luma).  dtype = float64 is the reference; dtype = float32 restates
the spec in its operation order (every product and sum rounded to fp32, the
8-bit luma as two rounded products, an add and one fma, the filter's taps in
ascending order, the two means summed in double), so that |float32 - float64|
measures what fp32 arithmetic costs on a given input.  The spec leaves open
whether a filter tap is a rounded product plus an add or one fused
multiply-add: fused=False / True restate either choice.
tests/test_quality_cpu.py derives the GPU test's tolerances from both.

Both use the spec's fp32 constants (the luma weights and the 11-tap window are
fp32 values by definition); only the arithmetic differs.

cases() lists the inputs tests/test_quality_gpu.py runs, so that the CPU test
measures the tolerances on exactly those.
"""
import numpy as np

WIN = 11
PIX_LUMA_F32, PIX_RGB8, PIX_RGBA8 = 1, 3, 4

# the kernel's tile of the SSIM map (quality.hip TX x TY): the shapes below
# are chosen against it
TILE = 32


def gauss_table(sigma=1.5):
    """g[i] = exp(-(i-5)^2 / (2 sigma^2)) / sum, in double, rounded once to fp32."""
    i = np.arange(WIN, dtype=np.float64)
    g = np.exp(-(i - 5.0) ** 2 / (2.0 * sigma * sigma))
    return (g / g.sum()).astype(np.float32)


def _fma32(x, y, z):
    """fp32 fma: the product of two fp32 values is exact in double"""
    return (x.astype(np.float64) * np.float64(y) + z.astype(np.float64)).astype(np.float32)


def luma255(img, dtype=np.float64):
    """Luma on the 0 - 255 scale: Y = 0.299f r + 0.587f g + 0.114f b for 8-bit
    pixels (fp32: extract_luma_kernel's sequence, two rounded products, an add,
    one fma), Y = 255.0f v for a float plane.  Not rounded, not clamped."""
    img = np.asarray(img)
    if img.dtype == np.uint8:
        assert img.ndim == 3 and img.shape[2] in (3, 4), img.shape
        kr, kg, kb = np.float32(0.299), np.float32(0.587), np.float32(0.114)
        if dtype == np.float32:
            r, g, b = (img[..., c].astype(np.float32) for c in range(3))
            return _fma32(b, kb, r * kr + g * kg)
        r, g, b = (img[..., c].astype(np.float64) for c in range(3))
        return np.float64(kr) * r + np.float64(kg) * g + np.float64(kb) * b
    assert img.dtype == np.float32 and img.ndim == 2, (img.dtype, img.shape)
    return (np.float32(255.0) * img).astype(dtype) if dtype == np.float32 else 255.0 * img.astype(np.float64)


def _filter(p, g, dt, fused=False):
    """separable 'valid' filter: horizontal pass first, taps in ascending
    order; fused (fp32 only): each tap as one fma, the choice the spec leaves
    to the compiler"""
    H, W = p.shape
    if fused:
        assert dt == np.float32
        step = lambda acc, gt, x: _fma32(x, gt, acc)
    else:
        step = lambda acc, gt, x: acc + gt * x
    h = np.zeros((H, W - WIN + 1), dt)
    for t in range(WIN):
        h = step(h, g[t], p[:, t:t + W - WIN + 1])
    v = np.zeros((H - WIN + 1, W - WIN + 1), dt)
    for t in range(WIN):
        v = step(v, g[t], h[t:t + H - WIN + 1, :])
    return v


def ssim_map(Ya, Yb, dtype=np.float64, sigma=1.5, fused=False):
    dt = np.dtype(dtype).type
    g = gauss_table(sigma).astype(dt)
    xa, xb = Ya - dt(128.0), Yb - dt(128.0)
    f = lambda p: _filter(p, g, dt, fused)
    ma, mb = f(xa), f(xb)
    saa, sbb, sab = f(xa * xa), f(xb * xb), f(xa * xb)
    va, vb, cab = saa - ma * ma, sbb - mb * mb, sab - ma * mb
    Ma, Mb = ma + dt(128.0), mb + dt(128.0)
    C1 = (dt(0.01) * dt(255.0)) * (dt(0.01) * dt(255.0))
    C2 = (dt(0.03) * dt(255.0)) * (dt(0.03) * dt(255.0))
    num = (dt(2.0) * (Ma * Mb) + C1) * (dt(2.0) * cab + C2)
    den = ((Ma * Ma + Mb * Mb) + C1) * ((va + vb) + C2)
    out = num / den
    assert out.dtype == dt
    return out


def quality(a, b, shave=0, dtype=np.float64, sigma=1.5, fused=False):
    """(mse, psnr, ssim) as Python floats (doubles)."""
    Ya, Yb = luma255(a, dtype), luma255(b, dtype)
    assert Ya.shape == Yb.shape, (Ya.shape, Yb.shape)
    if shave:
        Ya, Yb = Ya[shave:-shave, shave:-shave], Yb[shave:-shave, shave:-shave]
    assert Ya.shape[0] >= WIN and Ya.shape[1] >= WIN, Ya.shape
    d = Ya - Yb
    mse = float((d * d).astype(np.float64).sum() / d.size)
    psnr = float("inf") if mse == 0 else 10.0 * np.log10(65025.0 / mse)
    ssim = float(ssim_map(Ya, Yb, dtype, sigma, fused).astype(np.float64).mean())
    return mse, float(psnr), ssim


# ---- the GPU test's inputs ----
# (Ws, Hs) after the shave, against the kernel's 32 x 32 tile of windows, i.e.
# 42 x 42 pixels with the halo: one window; a few; exactly one tile plus halo;
# one pixel more each way (a second, one-window-wide tile in x and in y); a
# ragged multi-tile case; a wide flat one (four tiles by one)
SHAPES = [(11, 11), (12, 13), (TILE + 10, TILE + 10), (TILE + 11, TILE + 11), (75, 59), (135, 37)]
FORMATS = [(PIX_RGB8, PIX_RGBA8), (PIX_RGBA8, PIX_RGBA8), (PIX_LUMA_F32, PIX_LUMA_F32),
           (PIX_RGB8, PIX_LUMA_F32)]
SHAVE = 3  # every case carries a shaved ring, so that the offset arithmetic is always exercised


def smooth_field(rng, h, w, up=6):
    """bilinear upsampling of a coarse uniform grid, values in [0, 1]"""
    gh, gw = h // up + 2, w // up + 2
    g = rng.random((gh, gw))
    ys, xs = np.linspace(0, gh - 1.001, h), np.linspace(0, gw - 1.001, w)
    y0, x0 = ys.astype(int), xs.astype(int)
    fy, fx = (ys - y0)[:, None], (xs - x0)[None, :]
    return ((g[y0][:, x0] * (1 - fx) + g[y0][:, x0 + 1] * fx) * (1 - fy) +
            (g[y0 + 1][:, x0] * (1 - fx) + g[y0 + 1][:, x0 + 1] * fx) * fy)


def make_image(rng, fmt, h, w, like=None, noise=0.0):
    """An image of format fmt: a smooth field per channel (or `like`, an image
    of any format, reduced or expanded to fmt) plus Gaussian noise of `noise`
    levels (of 255)."""
    if like is None:
        planes = np.stack([smooth_field(rng, h, w) for _ in range(3)], axis=-1) * 255.0
    elif like.dtype == np.uint8:
        planes = like[..., :3].astype(np.float64)
    else:
        planes = np.repeat(like.astype(np.float64)[..., None], 3, axis=-1) * 255.0
    planes = planes + noise * rng.standard_normal(planes.shape)
    if fmt == PIX_LUMA_F32:
        y = 0.299 * planes[..., 0] + 0.587 * planes[..., 1] + 0.114 * planes[..., 2]
        return np.clip(y / 255.0, 0.0, 1.0).astype(np.float32)
    rgb = np.clip(np.rint(planes), 0, 255).astype(np.uint8)
    if fmt == PIX_RGB8:
        return rgb
    return np.concatenate([rgb, rng.integers(0, 256, (h, w, 1), dtype=np.uint8)], axis=-1)  # alpha: noise


def cases():
    """[(name, a, b, shave)]: structured pairs (a smooth field, b = a + noise of
    8 levels) for every shape x format pair, W = Ws + 2 SHAVE."""
    out = []
    for k, (ws, hs) in enumerate(SHAPES):
        for m, (fa, fb) in enumerate(FORMATS):
            rng = np.random.default_rng(1000 + 10 * k + m)
            w, h = ws + 2 * SHAVE, hs + 2 * SHAVE
            a = make_image(rng, fa, h, w)
            b = make_image(rng, fb, h, w, like=a, noise=8.0)
            out.append(("%dx%d_%d_%d" % (ws, hs, fa, fb), a, b, SHAVE))
    return out


def flat_cases():
    """The input centring does not help: a flat grey image at level 250
    against the same plus a one-level checker; the variance terms cancel."""
    out = []
    for ws, hs in ((TILE + 11, TILE + 11), (75, 59)):
        w, h = ws + 2 * SHAVE, hs + 2 * SHAVE
        y, x = np.mgrid[0:h, 0:w]
        a = np.full((h, w, 3), 250, np.uint8)
        b = np.concatenate([(250 + (x + y) % 2)[..., None].repeat(3, axis=-1),
                            np.full((h, w, 1), 255)], axis=-1).astype(np.uint8)
        out.append(("flat250_%dx%d" % (ws, hs), a, b, SHAVE))
    return out


# ---- tolerances of the GPU test (measured by tests/test_quality_cpu.py on the
# inputs above; see its docstring) ----
SSIM_ATOL = 2.0e-6       # |ssim - float64|, structured pairs
SSIM_ATOL_FLAT = 1.7e-4  # the same on flat_cases()
MSE_RTOL = 7.5e-7        # |mse - float64| / float64, every case
