"""The upscale front and back end without a GPU: the float64 yardstick
(tests/upscale_ref.py) against PIL, the host-side validation of the
srcnn_upscale_* entry points, and the `cnn upscale` argument handling."""
import os
import subprocess

import numpy as np
import pytest

import upscale_ref as U
from conftest import ROOT

CNN = os.path.join(ROOT, "cnn-super-resolution_amd", "bin", "cnn")
DEFAULT = (64, 32, 9, 1, 5)


@pytest.fixture(scope="module")
def S():
    import srcnn_amd
    return srcnn_amd


def random_rgba(w, h, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)


# ---- the yardstick itself ----
@pytest.mark.parametrize("s", [2, 3, 4])
def test_reference_matches_pil_bicubic(s):
    """PIL's float ('F') bicubic is the same Keys a = -0.5 kernel at half-pixel
    centres; it renormalises the weights at the border instead of replicating
    the edge, so only pixels at least 2s from every edge are compared."""
    from PIL import Image
    w, h = 37, 23
    luma = U.source_luma(random_rgba(w, h)).astype(np.float32)
    ref = U.bicubic(luma, s)
    pil = np.asarray(Image.fromarray(luma, mode="F").resize((w * s, h * s), Image.BICUBIC), np.float64)
    e = 2 * s
    diff = np.abs(ref - pil)[e:-e, e:-e]
    print("s=%d interior max |ref - PIL| = %.3e" % (s, diff.max()))
    assert diff.size > 0 and diff.max() <= 2e-7


def test_reference_scale_1_is_identity():
    rgba = random_rgba(17, 9)
    luma = U.source_luma(rgba)
    assert np.array_equal(U.bicubic(luma, 1), luma)
    assert U.phase(1, 0) == (0, [0.0, 1.0, 0.0, 0.0])
    plane = U.luma_plane(rgba, 1, 7)  # margin 3 left / top, 4 right / bottom
    assert plane.shape == (9 + 7, 17 + 7)
    assert np.array_equal(plane[3:3 + 9, 3:3 + 17], luma)
    assert np.array_equal(plane[0, :], plane[3, :]) and np.array_equal(plane[:, -1], plane[:, 3 + 16])


def test_reference_weights_sum_to_one():
    for s in (1, 2, 3, 4):
        for k in range(s):
            b, w = U.phase(s, k)
            assert b in (-1, 0) and abs(sum(w) - 1.0) < 1e-15
            assert sum(abs(x) for x in w) ** 2 <= 1.524  # the GPU tests' error bound uses this


# ---- ABI validation (host-side, before any launch) ----
@pytest.mark.parametrize("call", [
    lambda S: S.upscale_luma(64, 64, 8, 8, 0, 12),
    lambda S: S.upscale_luma(64, 64, 8, 8, 5, 12),
    lambda S: S.upscale_luma(64, 64, 0, 8, 2, 12),
    lambda S: S.upscale_luma(0, 0, 8, 8, 2, 12),
    lambda S: S.upscale_compose(64, 64, 64, 8, 8, 0),
    lambda S: S.upscale_compose(64, 64, 64, 8, 8, 5),
    lambda S: S.upscale_compose(64, 64, 64, 8, 0, 2),
    lambda S: S.upscale_compose(0, 0, 0, 8, 8, 2),
    lambda S: S.upscale(S.Net(*DEFAULT), 64, 8, 8, 0, 64, 64, 64, 1 << 30),
    lambda S: S.upscale(S.Net(*DEFAULT), 64, 8, 8, 5, 64, 64, 64, 1 << 30),
    lambda S: S.upscale(S.Net(*DEFAULT), 64, 0, 8, 2, 64, 64, 64, 1 << 30),
    lambda S: S.upscale(S.Net(*DEFAULT), 0, 8, 8, 2, 0, 0, 0, 1 << 30),
    lambda S: S.upscale(S.Net(64, 32, 9, 2, 5), 64, 8, 8, 2, 64, 64, 64, 1 << 30),  # even f2
    lambda S: S.upscale_luma(64, 64, 30000, 30000, 4, 12),  # plane beyond the 32-bit index
], ids=["luma_s0", "luma_s5", "luma_w0", "luma_null", "compose_s0", "compose_s5", "compose_h0",
        "compose_null", "net_s0", "net_s5", "net_w0", "net_null", "net_invalid", "luma_too_large"])
def test_upscale_validation_errors_without_gpu(S, call):
    """Nothing is launched: the non-null "pointers" here are never touched."""
    with pytest.raises(S.SrcnnError) as e:
        call(S)
    assert e.value.code == S.ERR_INVALID
    assert S.last_error()


def test_upscale_size_limit_is_named(S):
    with pytest.raises(S.SrcnnError) as e:
        S.upscale_luma(64, 64, 30000, 30000, 4, 12)
    assert "2^31-1" in str(e.value)


def test_upscale_workspace_too_small_without_gpu(S):
    net = S.Net(*DEFAULT)
    need = S.upscale_workspace_bytes(net, 8, 8, 2)
    with pytest.raises(S.SrcnnError) as e:
        S.upscale(net, 64, 8, 8, 2, 64, 64, 64, need - 1)
    assert e.value.code == S.ERR_WORKSPACE


def test_upscale_workspace_query(S):
    net = S.Net(*DEFAULT)
    # at least the padded plane and the net output
    assert S.upscale_workspace_bytes(net, 8, 8, 2) >= 4 * ((16 + 12) ** 2 + 16 ** 2)
    assert S.upscale_workspace_bytes(net, 8, 8, 2) % 256 == 0
    assert S.upscale_workspace_bytes(net, 1, 1, 1) > 0
    assert S.upscale_workspace_bytes(S.Net(64, 32, 9, 2, 5), 8, 8, 2) == 0  # invalid net
    assert S.upscale_workspace_bytes(net, 8, 8, 0) == 0
    assert S.upscale_workspace_bytes(net, 8, 8, 5) == 0
    assert S.upscale_workspace_bytes(net, 0, 8, 2) == 0


# ---- CLI ----
def cnn(*args):
    return subprocess.run([CNN, *args], capture_output=True, text=True, timeout=120)


def test_cli_upscale_argument_errors():
    p = cnn("upscale", "-c", "x.json", "-i", "y.png", "-o", "z.png", "--scale", "5")
    assert p.returncode == 1 and "--scale must be 1, 2, 3 or 4" in p.stdout and "usage: cnn" in p.stdout
    p = cnn("upscale", "-c", "x.json", "-i", "y.png", "-o", "z.png", "--scale", "0")
    assert p.returncode == 1 and "--scale must be 1, 2, 3 or 4" in p.stdout
    p = cnn("-c", "x.json", "-i", "y.png", "-o", "z.png", "--scale", "2")
    assert p.returncode == 1 and "--scale needs the upscale mode" in p.stdout and "usage: cnn" in p.stdout
    p = cnn("-h")
    assert p.returncode == 0 and "upscale" in p.stdout and "--scale" in p.stdout
