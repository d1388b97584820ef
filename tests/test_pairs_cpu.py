"""Training pairs from full-size images, without a GPU: the float64 yardstick
(tests/pairs_ref.py) against PIL and against the upscale yardstick (the
alignment of down and up), the host-side validation of srcnn_downscale_rgba,
srcnn_gather_tiles and srcnn_make_pairs*, and the `cnn` argument handling of
the downscale mode and of train --from-images."""
import os
import subprocess

import numpy as np
import pytest

import pairs_ref as P
import upscale_ref as U
from conftest import ROOT

CNN = os.path.join(ROOT, "cnn-super-resolution_amd", "bin", "cnn")


@pytest.fixture(scope="module")
def S():
    import srcnn_amd
    return srcnn_amd


def random_rgba(w, h, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)


def ramp_rgba(W, H, ax, ay):
    """r = g = b = ax*x + ay*y + 1, alpha 255"""
    y, x = np.mgrid[0:H, 0:W]
    v = ax * x + ay * y + 1
    assert v.max() <= 255
    return np.stack([v, v, v, np.full_like(v, 255)], axis=-1).astype(np.uint8)


# ---- the yardstick itself ----
def test_reference_scale_1_is_identity():
    assert P.taps(1) == (-1, [0.0, 1.0, 0.0])
    rgba = random_rgba(17, 9)
    small, raw = P.down_rgba(rgba, 1)
    assert np.array_equal(raw, rgba[..., :3].astype(np.float64))
    assert np.array_equal(small[..., :3], rgba[..., :3]) and (small[..., 3] == 255).all()


def test_reference_taps_and_weight_sums():
    """Tap ranges and the per-axis sum of |weights| DESIGN.md 11.1 states:
    19/16, 31/27 and 75/64, i.e. 1.1875 / 1.1482 / 1.1719 to the four decimals
    given there (one unit of the last one allowed)."""
    for s, first, count, exact, l1 in ((2, -3, 8, 19 / 16, 1.1875), (3, -4, 11, 31 / 27, 1.1482),
                                       (4, -6, 16, 75 / 64, 1.1719)):
        o0, w = P.taps(s)
        assert (o0, len(w)) == (first, count)
        assert abs(sum(w) - 1.0) < 1e-15
        assert abs(sum(abs(x) for x in w) - exact) < 1e-14, (s, sum(abs(x) for x in w))
        assert abs(exact - l1) <= 1e-4
        assert w == w[::-1] or np.allclose(w, w[::-1], rtol=0, atol=1e-16)  # symmetric about the centre


@pytest.mark.parametrize("s", [2, 3, 4])
def test_reference_matches_pil_bicubic_reduce(s):
    """PIL's antialiased float ('F') bicubic reduce is the same stretched Keys
    kernel at half-pixel centres; it renormalises the weights at the border
    instead of replicating the edge, so the outermost two pixels are left out."""
    from PIL import Image
    w, h = 37, 23
    luma = U.source_luma(random_rgba(s * w, s * h)).astype(np.float32)
    ref = P.down(luma, s)
    pil = np.asarray(Image.fromarray(luma, mode="F").resize((w, h), Image.BICUBIC), np.float64)
    diff = np.abs(ref - pil)[2:-2, 2:-2]
    print("s=%d interior max |ref - PIL| = %.3e" % (s, diff.max()))
    assert diff.size > 0 and diff.max() <= 1e-6


@pytest.mark.parametrize("W,H,ax,ay", [(96, 64, 2, 1), (64, 96, 1, 2)])
@pytest.mark.parametrize("s", [1, 2, 3, 4])
def test_reference_down_then_up_is_shift_free(s, W, H, ax, ay):
    """Keys reproduces linear ramps and the down kernel is symmetric about its
    centre, so down by s, then the upscale yardstick by s, returns the ramp at
    least 4s pixels from every edge: to float64 rounding (1e-12 on values <= 1)
    at s = 1, 3; at s = 2, 4 every low-resolution value is a half-integer and
    rounds up, which makes it exactly 0.5 / 255 <= 1.961e-3.  Shifting X by one
    pixel along the slope-2 axis, either way, raises it to at least
    (2 - 0.5) / 255 = 5.882e-3 (the 5.9e-3 of DESIGN.md 11.1 to its two digits;
    the other direction and s = 1, 3 give 2 / 255 or more): three times the
    aligned error, so a half-pixel convention slip cannot hide in the bound."""
    rgba = ramp_rgba(W, H, ax, ay)
    small, _ = P.down_rgba(rgba, s)
    X = U.luma_plane(small, s, 0)
    T = U.source_luma(rgba)[:X.shape[0], :X.shape[1]]  # (s = 3 crops 64 to 63)
    e = 4 * s
    d = np.abs(X - T)[e:-e, e:-e].max()
    print("s=%d %dx%d: interior max |X - T| = %.4e" % (s, W, H, d))
    assert d <= (1e-12 if s in (1, 3) else 1.961e-3)
    if s in (2, 4):
        assert d >= 1.96e-3  # (the half-level is really there: the bound is not slack)
    for step in (1, -1):
        shifted = np.roll(X, step, axis=1 if ax == 2 else 0)
        ds = np.abs(shifted - T)[e:-e, e:-e].max()
        print("   shifted by %+d: %.4e" % (step, ds))
        assert ds >= 1.5 / 255 - 1e-9


# ---- ABI validation (host-side, before any launch) ----
BIG = 1 << 30  # a non-null "pointer" that is never touched


@pytest.mark.parametrize("call", [
    lambda S: S.downscale_rgba(BIG, BIG, 8, 8, 0),
    lambda S: S.downscale_rgba(BIG, BIG, 8, 8, 5),
    lambda S: S.downscale_rgba(BIG, BIG, 2, 8, 3),                     # W < s
    lambda S: S.downscale_rgba(BIG, BIG, 8, 3, 4),                     # H < s
    lambda S: S.downscale_rgba(0, BIG, 8, 8, 2),
    lambda S: S.downscale_rgba(BIG, 0, 8, 8, 2),
    lambda S: S.downscale_rgba(BIG, BIG, 50000, 50000, 2),             # pixels beyond the 32-bit index
    lambda S: S.gather_tiles(BIG, 16, 16, 0, 0, 0, 2, 2, 4, 4, 1, BIG),     # stride 0
    lambda S: S.gather_tiles(BIG, 16, 16, 0, 0, 4, 0, 2, 4, 4, 1, BIG),     # nx 0
    lambda S: S.gather_tiles(BIG, 16, 16, 0, 0, 4, 2, 0, 4, 4, 1, BIG),     # ny 0
    lambda S: S.gather_tiles(BIG, 16, 16, 0, 0, 4, 2, 2, 0, 4, 1, BIG),     # tw 0
    lambda S: S.gather_tiles(BIG, 16, 16, 0, 0, 4, 2, 2, 4, 0, 1, BIG),     # th 0
    lambda S: S.gather_tiles(BIG, 16, 16, 1, 0, 4, 4, 2, 4, 4, 1, BIG),     # 1 + 3*4 + 4 > 16 in x
    lambda S: S.gather_tiles(BIG, 16, 16, 0, 5, 4, 2, 3, 4, 4, 1, BIG),     # 5 + 2*4 + 4 > 16 in y
    lambda S: S.gather_tiles(BIG, 16, 16, 0xFFFFFFFF, 0, 4, 2, 2, 4, 4, 1, BIG),  # x0 that would wrap in 32 bits
    lambda S: S.gather_tiles(0, 16, 16, 0, 0, 4, 2, 2, 4, 4, 1, BIG),
    lambda S: S.gather_tiles(BIG, 16, 16, 0, 0, 4, 2, 2, 4, 4, 1, 0),
    lambda S: S.gather_tiles(BIG, 70000, 70000, 0, 0, 4, 2, 2, 4, 4, 1, BIG),  # plane beyond the 32-bit index
    lambda S: S.make_pairs(BIG, 96, 64, 0, 33, 14, BIG, BIG, BIG, 1 << 30),
    lambda S: S.make_pairs(BIG, 96, 64, 5, 33, 14, BIG, BIG, BIG, 1 << 30),
    lambda S: S.make_pairs(BIG, 2, 64, 3, 1, 1, BIG, BIG, BIG, 1 << 30),     # W < s
    lambda S: S.make_pairs(BIG, 96, 64, 2, 0, 14, BIG, BIG, BIG, 1 << 30),   # tile 0
    lambda S: S.make_pairs(BIG, 96, 64, 2, 33, 0, BIG, BIG, BIG, 1 << 30),   # stride 0
    lambda S: S.make_pairs(BIG, 96, 65, 2, 65, 14, BIG, BIG, BIG, 1 << 30),  # tile > Hc = 64: no tile fits
    lambda S: S.make_pairs(0, 96, 64, 2, 33, 14, BIG, BIG, BIG, 1 << 30),
    lambda S: S.make_pairs(BIG, 96, 64, 2, 33, 14, 0, BIG, BIG, 1 << 30),
    lambda S: S.make_pairs(BIG, 96, 64, 2, 33, 14, BIG, 0, BIG, 1 << 30),
    lambda S: S.make_pairs(BIG, 96, 64, 2, 33, 14, BIG, BIG, 0, 1 << 30),
    lambda S: S.make_pairs(BIG, 30000, 30000, 2, 33, 14, BIG, BIG, BIG, 1 << 40),  # beyond the 32-bit index
], ids=["down_s0", "down_s5", "down_w_lt_s", "down_h_lt_s", "down_null_in", "down_null_out", "down_too_large",
        "gather_stride0", "gather_nx0", "gather_ny0", "gather_tw0", "gather_th0", "gather_leaves_x",
        "gather_leaves_y", "gather_x0_wraps", "gather_null_plane", "gather_null_tiles", "gather_too_large",
        "pairs_s0", "pairs_s5", "pairs_w_lt_s", "pairs_tile0", "pairs_stride0", "pairs_no_tile_fits",
        "pairs_null_rgba", "pairs_null_X", "pairs_null_T", "pairs_null_ws", "pairs_too_large"])
def test_pairs_validation_errors_without_gpu(S, call):
    """Nothing is launched: the non-null "pointers" here are never touched."""
    with pytest.raises(S.SrcnnError) as e:
        call(S)
    assert e.value.code == S.ERR_INVALID
    assert S.last_error()


def test_pairs_size_limit_is_named(S):
    for call in (lambda: S.downscale_rgba(BIG, BIG, 50000, 50000, 2),
                 lambda: S.gather_tiles(BIG, 70000, 70000, 0, 0, 4, 2, 2, 4, 4, 1, BIG)):
        with pytest.raises(S.SrcnnError) as e:
            call()
        assert "2^31-1" in str(e.value)


def test_make_pairs_workspace_too_small_without_gpu(S):
    need = S.make_pairs_workspace_bytes(96, 64, 2)
    assert need > 0
    with pytest.raises(S.SrcnnError) as e:
        S.make_pairs(BIG, 96, 64, 2, 33, 14, BIG, BIG, BIG, need - 1)
    assert e.value.code == S.ERR_WORKSPACE


def test_make_pairs_queries(S):
    assert S.make_pairs_count(96, 64, 2, 33, 14) == (15, 5, 3)
    assert S.make_pairs_count(67, 50, 3, 9, 4) == (15 * 10, 15, 10)  # the ragged crop: Wc = 66, Hc = 48
    assert S.make_pairs_count(2, 2, 2, 2, 1) == (1, 1, 1)
    assert S.make_pairs_count(96, 64, 0, 33, 14) == (0, 0, 0)
    assert S.make_pairs_count(96, 64, 5, 33, 14) == (0, 0, 0)
    assert S.make_pairs_count(96, 65, 2, 65, 14) == (0, 0, 0)        # tile > Hc
    assert S.make_pairs_count(96, 64, 2, 33, 0) == (0, 0, 0)
    assert S.make_pairs_count(96, 64, 2, 0, 14) == (0, 0, 0)
    for W, H, s, tile, stride in ((96, 64, 2, 33, 14), (67, 50, 3, 9, 4), (1920, 1080, 2, 33, 14), (20, 20, 2, 33, 14)):
        nx, ny = P.tile_grid(W, H, s, tile, stride)
        assert S.make_pairs_count(W, H, s, tile, stride) == (nx * ny, nx, ny)
    # the low-resolution image and the two planes, each a multiple of 256 bytes
    b = S.make_pairs_workspace_bytes(67, 50, 3)
    assert b % 256 == 0 and b >= 4 * 22 * 16 + 4 * 66 * 48 + 4 * 67 * 50
    assert S.make_pairs_workspace_bytes(2, 2, 2) == 3 * 256
    assert S.make_pairs_workspace_bytes(96, 64, 0) == 0
    assert S.make_pairs_workspace_bytes(96, 64, 5) == 0
    assert S.make_pairs_workspace_bytes(2, 64, 3) == 0
    assert S.make_pairs_workspace_bytes(50000, 50000, 2) == 0


# ---- CLI ----
def cnn(*args):
    return subprocess.run([CNN, *args], capture_output=True, text=True, timeout=120)


def test_cli_pairs_argument_errors():
    p = cnn("downscale", "-i", "y.png", "-o", "z.png", "--scale", "5")
    assert p.returncode == 1 and "--scale must be 1, 2, 3 or 4" in p.stdout and "usage: cnn" in p.stdout
    p = cnn("downscale", "-o", "z.png", "--scale", "2")
    assert p.returncode == 1 and "--in is required" in p.stdout
    p = cnn("downscale", "upscale", "-c", "x.json", "-i", "y.png", "-o", "z.png")
    assert p.returncode == 1 and "different modes" in p.stdout
    p = cnn("downscale", "-i", "y.png", "--scale", "2")  # -c is not needed; an output or `dry` is
    assert p.returncode == 1 and "Either provide out path or do the dry run" in p.stdout
    p = cnn("train", "-c", "x.json", "-i", "dir", "-o", "p.json", "--scale", "2")
    assert p.returncode == 1 and "--scale needs the upscale mode" in p.stdout and "usage: cnn" in p.stdout
    p = cnn("-c", "x.json", "-i", "y.png", "-o", "z.png", "--from-images")
    assert p.returncode == 1 and "--from-images needs the train mode" in p.stdout
    p = cnn("train", "-c", "x.json", "-i", "dir", "-o", "p.json", "--tile", "33")
    assert p.returncode == 1 and "--tile and --stride need train --from-images" in p.stdout
    p = cnn("train", "-c", "x.json", "-i", "dir", "-o", "p.json", "--stride", "14")
    assert p.returncode == 1 and "--tile and --stride need train --from-images" in p.stdout
    for flag in ("--tile", "--stride"):
        for bad in ("0", "-3", "x", "3x"):
            p = cnn("train", "--from-images", "-c", "x.json", "-i", "dir", "-o", "p.json", flag, bad)
            assert p.returncode == 1 and flag + " must be a positive integer" in p.stdout, (flag, bad, p.stdout)
    p = cnn("train", "--from-images", "-i", "dir", "-o", "p.json", "--scale", "2")
    assert p.returncode == 1 and "--config and --in are required" in p.stdout
    p = cnn("-h")
    assert p.returncode == 0
    for word in ("downscale", "--from-images", "--tile", "--stride", "--scale"):
        assert word in p.stdout
