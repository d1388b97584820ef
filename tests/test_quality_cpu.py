"""PSNR / SSIM on the device, without a GPU: the yardstick itself
(tests/quality_ref.py), the tolerances the GPU test uses, the host-side
validation of srcnn_quality / srcnn_evaluate and the `cnn` argument handling of
the quality and evaluate modes.

Where the GPU test's tolerances come from.  The yardstick has
a float64 reference and a float32 restatement in the spec's operation order,
the latter in both forms the spec leaves open (a filter tap as a rounded
product plus an add, or as one fused multiply-add).  On the GPU test's own
inputs (quality_ref.cases() and flat_cases()) the restatements' errors against
float64, measured here (numpy 2.x, this file's test_tolerance_constants
re-measures them on every run), are

    structured pairs   |ssim32 - ssim64|          <= 4.85e-7 (unfused), 4.05e-7 (fused)
    flat 250 + checker |ssim32 - ssim64|          <= 1.00e-7 (unfused), 4.13e-5 (fused)
    every case         |mse32 - mse64| / mse64    <= 1.87e-7

and the GPU bound is 4 x the largest such error (the margin hip_util's K_REF
gives an fp32 loop nest over its own error; it covers a compiler that fuses
some taps and not others, and the different tree of the double sums), rounded
up to two digits:

    SSIM_ATOL      = 2.0e-6   (4 x 4.85e-7 = 1.94e-6)
    SSIM_ATOL_FLAT = 1.7e-4   (4 x 4.13e-5 = 1.65e-4)
    MSE_RTOL       = 7.5e-7   (4 x 1.87e-7 = 7.49e-7)

The flat case has a constant of its own because its error dwarfs the rest:
centring at 128 leaves 122^2 in the squares, the variance terms are
differences of two numbers near 14,884 and whether a tap is fused decides how
their roundings line up (1.0e-7 against 4.1e-5).

What the bounds can still see, on the same inputs in float64: a window of
sigma 1.4 instead of 1.5 moves the mean SSIM of every structured pair by at
least 5.43e-4, a one-pixel shift of b by at least 1.12e-2 (and the mse by a
factor of more than 3).  SSIM_ATOL and MSE_RTOL are asserted to be at most a
tenth of the smallest sigma displacement (and of the mse's movement under the
shift); the flat images do not tell the two windows apart (they move by 2e-8),
so for SSIM_ATOL_FLAT the assertion is the weaker one that it stays below
every structured pair's sigma displacement -- it is only ever applied to the
flat inputs.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import quality_ref as Q
from conftest import ROOT

CNN = os.path.join(ROOT, "cnn-super-resolution_amd", "bin", "cnn")
KERNELS = os.path.join(ROOT, "cnn-super-resolution_amd", "csrc", "hip", "quality.hip")


@pytest.fixture(scope="module")
def S():
    import srcnn_amd
    return srcnn_amd


# ---- the yardstick itself ----
def test_gauss_table_is_the_formula():
    """The kernel's 11 constants (parsed from quality.hip) are the formula,
    computed in double and rounded once to fp32; they sum to 1 within fp32
    rounding and are symmetric."""
    src = open(KERNELS).read()
    body = re.search(r"c_gauss\[kWin\]\s*=\s*\{([^}]*)\}", src).group(1)
    table = np.array([np.float32(v.rstrip("f")) for v in re.findall(r"[0-9.eE+-]+f", body)], np.float32)
    assert table.size == Q.WIN == 11
    i = np.arange(11.0)
    g = np.exp(-(i - 5.0) ** 2 / 4.5)
    g = (g / g.sum()).astype(np.float32)
    assert np.array_equal(table, g)
    assert np.array_equal(table, Q.gauss_table())
    assert np.array_equal(table, table[::-1])
    assert abs(float(table.astype(np.float64).sum()) - 1.0) <= 11 * 2.0 ** -25


@pytest.mark.parametrize("dtype,fused", [(np.float64, False), (np.float32, False), (np.float32, True)])
def test_identical_images_are_exact(dtype, fused):
    rng = np.random.default_rng(3)
    rgb = rng.integers(0, 256, (31, 45, 3), dtype=np.uint8)
    plane = rng.random((31, 45)).astype(np.float32)
    for img in (rgb, plane):
        assert Q.quality(img, img.copy(), 0, dtype, fused=fused) == (0.0, float("inf"), 1.0)
    # RGB8 against RGBA8 of the same colours, shaved
    rgba = np.concatenate([rgb, rng.integers(0, 256, (31, 45, 1), dtype=np.uint8)], axis=-1)
    assert Q.quality(rgb, rgba, 4, dtype, fused=fused) == (0.0, float("inf"), 1.0)


def closed_form(p, q, dtype=np.float64):
    """(mse, ssim) of constant grey images p, q: the variance terms vanish"""
    Ya = float(Q.luma255(np.full((1, 1, 3), p, np.uint8), dtype)[0, 0])
    Yb = float(Q.luma255(np.full((1, 1, 3), q, np.uint8), dtype)[0, 0])
    C1 = (0.01 * 255) ** 2
    return (Ya - Yb) ** 2, (2 * Ya * Yb + C1) / (Ya * Ya + Yb * Yb + C1), Ya, Yb


@pytest.mark.parametrize("p,q", [(0, 255), (10, 20), (250, 251), (128, 128), (255, 254), (77, 200)])
def test_constant_images_give_the_closed_form(p, q):
    """The window's fp32 constants sum to S = 1 - 1.4e-9 per axis, so a
    filtered constant c is S^2 c and the variance terms are S^2 (1 - S^2) times
    products of the centred levels instead of 0: the second factor of the
    formula is off by at most |S^2 - 1| (Ya - Yb)^2 / C2 and the first by less
    than |S^2 - 1|; twice their sum bounds the float64 yardstick.  The float32
    restatements meet the closed form within the flat inputs' constant."""
    a, b = np.full((20, 23, 3), p, np.uint8), np.full((20, 23, 4), q, np.uint8)
    mse_cf, ssim_cf, Ya, Yb = closed_form(p, q)
    mse, psnr, ssim = Q.quality(a, b, 2)
    s = float(Q.gauss_table().astype(np.float64).sum())
    bound = 2 * abs(s * s - 1) * ((Ya - Yb) ** 2 / (0.03 * 255) ** 2 + 1) + 1e-12
    print("p=%d q=%d: ssim %.12f closed %.12f diff %.2e (bound %.2e)" % (p, q, ssim, ssim_cf, ssim - ssim_cf, bound))
    assert abs(ssim - ssim_cf) <= bound
    assert abs(mse - mse_cf) <= 1e-12 * max(mse_cf, 1.0)
    assert psnr == (float("inf") if p == q else 10 * np.log10(65025.0 / mse))
    for fused in (False, True):
        mse32, _, ssim32 = Q.quality(a, b, 2, np.float32, fused=fused)
        mse32_cf = closed_form(p, q, np.float32)[0]
        assert abs(ssim32 - ssim_cf) <= Q.SSIM_ATOL_FLAT + bound
        assert abs(mse32 - mse32_cf) <= 2.0 ** -23 * mse32_cf  # every pixel's square is the same fp32 number


@pytest.fixture(scope="module")
def measured():
    """The yardstick's three forms, the wrong window and the shifted b on the
    GPU test's inputs: {kind: [per-case dict]}"""
    out = {}
    for kind, cs in (("structured", Q.cases()), ("flat", Q.flat_cases())):
        rows = []
        for name, a, b, k in cs:
            m64, _, s64 = Q.quality(a, b, k)
            m32, _, s32 = Q.quality(a, b, k, np.float32)
            m32f, _, s32f = Q.quality(a, b, k, np.float32, fused=True)
            assert m32f == m32  # (the filter's form does not touch the mse)
            _, _, s14 = Q.quality(a, b, k, sigma=1.4)
            msh, _, ssh = Q.quality(a, np.roll(b, 1, axis=1), k)
            rows.append(dict(name=name, e_ssim=max(abs(s32 - s64), abs(s32f - s64)), e_mse=abs(m32 - m64) / m64,
                             d_sigma=abs(s14 - s64), d_shift=abs(ssh - s64), d_shift_mse=abs(msh - m64) / m64))
            print("%-20s e_ssim %.3e e_mse %.3e | sigma 1.4: %.3e shift: %.3e (mse x %.2f)" % (
                name, rows[-1]["e_ssim"], rows[-1]["e_mse"], rows[-1]["d_sigma"], rows[-1]["d_shift"],
                1 + rows[-1]["d_shift_mse"]))
        out[kind] = rows
    return out


def test_tolerance_constants(measured):
    """Each constant is 4 x the float32 restatements' largest error against
    float64 on the GPU test's inputs, rounded up by at most a tenth."""
    e_s = max(r["e_ssim"] for r in measured["structured"])
    e_f = max(r["e_ssim"] for r in measured["flat"])
    e_m = max(r["e_mse"] for r in measured["structured"] + measured["flat"])
    print("largest errors: ssim structured %.4e, flat %.4e; mse %.4e" % (e_s, e_f, e_m))
    for const, err in ((Q.SSIM_ATOL, e_s), (Q.SSIM_ATOL_FLAT, e_f), (Q.MSE_RTOL, e_m)):
        assert 4 * err <= const <= 1.1 * 4 * err, (const, err)
    assert e_f > 20 * e_s  # why the flat case has a constant of its own


def test_bounds_discriminate(measured):
    """A wrong window (sigma 1.4) or a one-pixel shift of b moves every
    structured pair's result by at least ten times the bounds."""
    rows = measured["structured"]
    d_sigma = min(r["d_sigma"] for r in rows)
    d_shift = min(r["d_shift"] for r in rows)
    d_mse = min(r["d_shift_mse"] for r in rows)
    print("smallest movement: sigma %.4e, shift %.4e, mse under the shift %.4e rel" % (d_sigma, d_shift, d_mse))
    assert Q.SSIM_ATOL <= d_sigma / 10 and Q.SSIM_ATOL <= d_shift / 10
    assert Q.MSE_RTOL <= d_sigma / 10 and Q.MSE_RTOL <= d_mse / 10
    assert Q.SSIM_ATOL_FLAT <= d_sigma and Q.SSIM_ATOL_FLAT <= d_shift / 10


# ---- ABI validation (host-side, before any launch) ----
BIG = 1 << 30  # a non-null, 256-byte aligned "pointer" that is never touched
NET = (64, 32, 9, 1, 5)
RGB8, RGBA8, F32 = Q.PIX_RGB8, Q.PIX_RGBA8, Q.PIX_LUMA_F32


def q(S, a=BIG, fa=RGB8, pa=40, b=BIG, fb=RGBA8, pb=48, W=40, H=30, shave=2, res=BIG, ws=BIG, nb=1 << 20):
    S.quality(a, fa, pa, b, fb, pb, W, H, shave, res, ws, nb)


def ev(S, net=NET, rgba=BIG, W=67, H=50, s=3, shave=3, params=BIG, res=BIG, ws=BIG, nb=1 << 40):
    S.evaluate(S.Net(*net), rgba, W, H, s, shave, params, res, ws, nb)


@pytest.mark.parametrize("call", [
    lambda S: q(S, fa=0),
    lambda S: q(S, fb=2),
    lambda S: q(S, fb=5),
    lambda S: q(S, a=0),
    lambda S: q(S, b=0),
    lambda S: q(S, res=0),
    lambda S: q(S, ws=0),
    lambda S: q(S, pa=39),
    lambda S: q(S, pb=39),
    lambda S: q(S, W=40, H=30, shave=10),                  # Hs = 10
    lambda S: q(S, W=30, pa=30, pb=30, H=40, shave=10),    # Ws = 10
    lambda S: q(S, shave=0x80000000),                      # 2 * shave wraps to 0 in 32 bits
    lambda S: q(S, shave=0x80000005),                      # ... to 10
    lambda S: q(S, b=BIG + 2),                             # RGBA8 base
    lambda S: q(S, fa=F32, a=BIG + 1),                     # F32 base
    lambda S: q(S, W=50000, H=50000, pa=50000, pb=50000),  # pixels beyond the 32-bit index
    lambda S: q(S, pb=1 << 27, H=30),                      # pitch x rows beyond it
    lambda S: ev(S, net=(64, 32, 9, 2, 5)),                # invalid net
    lambda S: ev(S, s=0),
    lambda S: ev(S, s=5),
    lambda S: ev(S, W=2, s=3),                             # W < s
    lambda S: ev(S, W=67, H=50, s=3, shave=19),            # Hc = 48: 48 - 38 = 10
    lambda S: ev(S, W=32, H=50, s=3, shave=10),            # Wc = 30: 30 - 20 = 10
    lambda S: ev(S, shave=0x80000000),
    lambda S: ev(S, rgba=0),
    lambda S: ev(S, params=0),
    lambda S: ev(S, res=0),
    lambda S: ev(S, ws=0),
    lambda S: ev(S, rgba=BIG + 2),
    lambda S: ev(S, W=30000, H=30000, s=2),                # beyond the 32-bit index
], ids=["fmt_a_0", "fmt_b_2", "fmt_b_5", "null_a", "null_b", "null_result", "null_ws", "pitch_a", "pitch_b",
        "hs_10", "ws_10", "shave_wraps_0", "shave_wraps_10", "rgba8_misaligned", "f32_misaligned", "too_large",
        "pitch_too_large", "ev_net", "ev_s0", "ev_s5", "ev_w_lt_s", "ev_hs_10", "ev_ws_10", "ev_shave_wraps",
        "ev_null_rgba", "ev_null_params", "ev_null_result", "ev_null_ws", "ev_rgba_misaligned", "ev_too_large"])
def test_quality_validation_errors_without_gpu(S, call):
    """Nothing is launched: the non-null "pointers" here are never touched."""
    with pytest.raises(S.SrcnnError) as e:
        call(S)
    assert e.value.code == S.ERR_INVALID
    assert S.last_error()


def test_rgb8_base_may_have_any_alignment(S):
    """...so a misaligned RGB8 base passes the checks: with a workspace one
    byte short the call gets as far as the workspace check."""
    need = S.quality_workspace_bytes(40, 30, 2)
    for off in (1, 2, 3):
        with pytest.raises(S.SrcnnError) as e:
            q(S, a=BIG + off, nb=need - 1)
        assert e.value.code == S.ERR_WORKSPACE


def test_quality_size_limit_is_named(S):
    for call in (lambda: q(S, W=50000, H=50000, pa=50000, pb=50000), lambda: q(S, pb=1 << 27),
                 lambda: ev(S, W=30000, H=30000, s=2)):
        with pytest.raises(S.SrcnnError) as e:
            call()
        assert "2^31-1" in str(e.value)


def test_workspace_too_small_without_gpu(S):
    need = S.quality_workspace_bytes(40, 30, 2)
    assert need > 0
    with pytest.raises(S.SrcnnError) as e:
        q(S, nb=need - 1)
    assert e.value.code == S.ERR_WORKSPACE
    need = S.evaluate_workspace_bytes(S.Net(*NET), 67, 50, 3)
    assert need > 0
    with pytest.raises(S.SrcnnError) as e:
        ev(S, nb=need - 1)
    assert e.value.code == S.ERR_WORKSPACE


def test_workspace_queries(S):
    """0 on invalid arguments, a multiple of 256 otherwise; two doubles per
    tile of 32 x 32 windows"""
    assert S.quality_workspace_bytes(11, 11, 0) == 256
    assert S.quality_workspace_bytes(17, 17, 3) == 256
    assert S.quality_workspace_bytes(3840, 2160, 0) == 16 * 120 * 68  # ceil(3830 / 32) x ceil(2150 / 32) tiles
    assert S.quality_workspace_bytes(3840, 2160, 2) % 256 == 0
    assert S.quality_workspace_bytes(10, 11, 0) == 0
    assert S.quality_workspace_bytes(11, 10, 0) == 0
    assert S.quality_workspace_bytes(16, 17, 3) == 0
    assert S.quality_workspace_bytes(40, 30, 0x80000000) == 0
    assert S.quality_workspace_bytes(50000, 50000, 0) == 0
    net = S.Net(*NET)
    b = S.evaluate_workspace_bytes(net, 67, 50, 3)
    # the low-resolution image, the rgb buffer, the plane, srcnn_upscale's workspace and srcnn_quality's
    parts = (4 * 22 * 16, 3 * 66 * 48, 4 * 66 * 48, S.upscale_workspace_bytes(net, 22, 16, 3),
             S.quality_workspace_bytes(66, 48, 0))
    assert b == sum((p + 255) // 256 * 256 for p in parts)
    assert S.evaluate_workspace_bytes(net, 67, 50, 0) == 0
    assert S.evaluate_workspace_bytes(net, 67, 50, 5) == 0
    assert S.evaluate_workspace_bytes(net, 2, 50, 3) == 0
    assert S.evaluate_workspace_bytes(net, 23, 50, 2) > 0    # Wc = 22
    assert S.evaluate_workspace_bytes(net, 10, 50, 1) == 0   # Wc = 10 < 11: nothing to measure
    assert S.evaluate_workspace_bytes(net, 32, 10, 3) == 0   # Hc = 9
    assert S.evaluate_workspace_bytes(S.Net(64, 32, 9, 2, 5), 67, 50, 3) == 0
    assert S.evaluate_workspace_bytes(net, 30000, 30000, 2) == 0


def test_format_constants(S):
    assert (S.PIX_LUMA_F32, S.PIX_RGB8, S.PIX_RGBA8) == (1, 3, 4)
    hdr = open(os.path.join(ROOT, "include", "srcnn.h")).read()
    assert re.search(r"SRCNN_PIX_LUMA_F32 = 1, SRCNN_PIX_RGB8 = 3, SRCNN_PIX_RGBA8 = 4", hdr)
    for name in ("srcnn_quality", "srcnn_quality_workspace_bytes", "srcnn_evaluate",
                 "srcnn_evaluate_workspace_bytes"):
        assert name in S.SIGNATURES


# ---- CLI ----
def cnn(*args):
    return subprocess.run([CNN, *args], capture_output=True, text=True, timeout=120)


def test_cli_quality_argument_errors():
    p = cnn("quality", "-i", "a.png")
    assert p.returncode == 1 and "--in and --ref are required" in p.stdout and "usage: cnn" in p.stdout
    p = cnn("quality", "--ref", "b.png")
    assert p.returncode == 1 and "--in and --ref are required" in p.stdout
    p = cnn("quality", "evaluate", "-i", "a.png", "--ref", "b.png")
    assert p.returncode == 1 and "different modes" in p.stdout
    p = cnn("upscale", "-c", "x.json", "-i", "a.png", "-o", "z.png", "--ref", "b.png")
    assert p.returncode == 1 and "--ref needs the quality mode" in p.stdout
    p = cnn("-c", "x.json", "-i", "a.png", "-o", "z.png", "--shave", "2")
    assert p.returncode == 1 and "--shave needs the quality mode or the evaluate mode" in p.stdout
    for bad in ("-1", "x", "3x", ""):
        p = cnn("quality", "-i", "a.png", "--ref", "b.png", "--shave", bad)
        assert p.returncode == 1 and "--shave must be a non-negative integer" in p.stdout, (bad, p.stdout)
    p = cnn("quality", "-i", "a.png", "--ref", "b.png", "--scale", "2")
    assert p.returncode == 1 and "--scale needs the upscale mode" in p.stdout
    # no config, no output and no `dry` needed: the run gets as far as the first file
    p = cnn("quality", "-i", "/nonexistent/a.png", "--ref", "/nonexistent/b.png")
    assert p.returncode == 1 and "[ERROR]" in p.stdout and "Either provide out path" not in p.stdout


def test_cli_evaluate_argument_errors(tmp_path):
    p = cnn("evaluate", "-i", "dir", "--scale", "2")
    assert p.returncode == 1 and "--config and --in are required" in p.stdout
    p = cnn("evaluate", "-c", "x.json", "--scale", "2")
    assert p.returncode == 1 and "--config and --in are required" in p.stdout
    p = cnn("evaluate", "-c", "x.json", "-i", "dir", "--scale", "5")
    assert p.returncode == 1 and "--scale must be 1, 2, 3 or 4" in p.stdout
    p = cnn("evaluate", "train", "-c", "x.json", "-i", "dir")
    assert p.returncode == 1 and "different modes" in p.stdout
    p = cnn("evaluate", "-c", "x.json", "-i", "dir", "--ref", "b.png")
    assert p.returncode == 1 and "--ref needs the quality mode" in p.stdout
    # no output and no `dry` needed: the run gets as far as the config
    p = cnn("evaluate", "-c", str(tmp_path / "missing.json"), "-i", "dir", "--scale", "3")
    assert p.returncode == 1 and "[ERROR]" in p.stdout and "Either provide out path" not in p.stdout
    assert "Evaluate mode, scale: 3, shave: 3" in p.stdout  # --shave defaults to the scale
    p = cnn("evaluate", "-c", str(tmp_path / "missing.json"), "-i", "dir", "--scale", "3", "--shave", "0")
    assert "Evaluate mode, scale: 3, shave: 0" in p.stdout


def test_cli_help_names_the_new_modes():
    p = cnn("-h")
    assert p.returncode == 0
    for word in ("quality", "evaluate", "--ref", "--shave", "PSNR", "SSIM"):
        assert word in p.stdout
