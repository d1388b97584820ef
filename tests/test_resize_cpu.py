"""The any-size resampling spec on the CPU: the float64
reference (tests/resize_ref.py) against the integer-scale references it
generalises, the conditions under which tests/test_resize_gpu.py exempts
values from exact comparison, the C ABI's validation without a device, the
`cnn upscale --size` argument errors and y4m::Header::resized."""
import os
import subprocess

import numpy as np
import pytest

import resize_ref as R
import upscale_ref as U
import yuv_ref as Y8
from conftest import ROOT

BIN = os.path.join(ROOT, "cnn-super-resolution_amd", "bin")
CNN = os.path.join(BIN, "cnn")
TOOL = os.path.join(BIN, "y4m_resize_tool")
DEFAULT = (64, 32, 9, 1, 5)


@pytest.fixture(scope="module")
def S():
    import srcnn_amd
    return srcnn_amd


# ---- the reference ----
@pytest.mark.parametrize("s", [1, 2, 3, 4])
def test_integer_ratios_are_the_scale_reference(s):
    """At (rn, rd) = (1, s) the map is DESIGN.md 10.1's: the float64 results
    agree to 1e-12 and the fp32-rounded weights of every phase are phase(s,
    k)'s exactly (so c_up's: the doubles differ by 4e-16 at s = 3, k = 2)."""
    a = np.random.default_rng(4).uniform(0, 1, (9, 17))
    assert np.abs(R.resize(a, 17 * s, 9 * s, (1, s), (1, s)) - U.bicubic(a, s)).max() <= 1e-12
    # the same ratio, not reduced
    assert np.abs(R.resize(a, 17 * s, 9 * s, (17, 17 * s), (9, 9 * s)) - U.bicubic(a, s)).max() <= 1e-12
    for X in range(3 * s):
        j, k = divmod(X, s)
        b, w = R.phase(X, 1, s)
        b0, w0 = U.phase(s, k)
        assert b == j + b0
        assert np.array_equal(np.float32(w), np.float32(w0)), (s, k, w, w0)
        b, w = R.phase(X, 7, 7 * s)
        assert b == j + b0 and np.array_equal(np.float32(w), np.float32(w0))


def test_weights_sum_to_one_and_their_moduli_peak_at_one_and_a_quarter():
    """sum |w| <= 1.25 (at t = 0.5): (sum |w|)^2 <= 1.5625 is what the GPU
    tests' error bounds use.  The four doubles sum to 1 within 5e-15: each is
    three roundings of 2^-53 on Horner terms of at most 4."""
    worst = 0.0
    for rn, rd in [(1, 1), (2, 3), (3, 4), (37, 55), (23, 35), (17, 40), (9, 13), (1, 4), (135, 203), (854, 1920)]:
        for X in range(2 * rd):
            b, w = R.phase(X, rn, rd)
            assert abs(sum(w) - 1.0) <= 5e-15
            worst = max(worst, sum(abs(x) for x in w))
    assert abs(worst - 1.25) <= 1e-15


def test_ratio_one_is_the_identity():
    a = np.random.default_rng(5).integers(0, 256, (7, 11)).astype(np.float64)
    assert np.array_equal(R.resize(a, 11, 7, (11, 11), (7, 7)), a)
    for X in range(5):
        assert R.phase(X, 3, 3) == (X, [0.0, 1.0, 0.0, 0.0])


def test_planes_at_one_half_are_the_8_bit_crop_rule():
    """19 x 12 -> 37 x 23 at ratios 1/2: yuv_ref.planes_u8(..., 2, 37, 23),
    DESIGN.md 14.1's crop of the odd 4:2:0 frame."""
    p = R.planes_of(19, 12, 8)
    q, raw = R.planes(p, 37, 23, (1, 2), (1, 2))
    q0, raw0 = Y8.planes_u8(p, 2, 37, 23)
    assert np.array_equal(q, q0) and np.abs(raw - raw0).max() <= 1e-12


def test_the_odd_420_frame_takes_its_chroma_at_the_lumas_ratios():
    """37 x 23 -> 55 x 35 at 4:2:0: chroma 19 x 12 -> 28 x 18 at 37/55 and
    23/35, within the plane call's bound ow <= ceil(pw rd / rn)."""
    y, uv = R.y_of(37, 23, 8), R.planes_of(19, 12, 8)
    plane, q, raw = R.frame(y, uv, 55, 35, 2, 2, 7, 8, 0, "full")
    assert plane.shape == (42, 62) and q.shape == (2, 18, 28)
    assert 28 <= -(-19 * 55 // 37) and 18 <= -(-12 * 35 // 23)
    assert np.array_equal(q, R.planes(uv, 28, 18, (37, 55), (23, 35))[0])


def test_gpu_test_seeds_keep_their_exemptions_within_the_caps():
    """tests/test_resize_gpu.py compares exactly only where the reference's raw
    value is further than a band from where rounding (chroma: k + 0.5) or
    truncation (rgb: an integer) can go the other way, and caps the exempt
    share of a case.  The caps hold on the reference alone, for every case and
    seed that file uses."""
    worst = 0.0
    for (w, h), (W, H) in R.CASES:
        raw = R.ref_compose(w, h, W, H)[1]
        near = R.near_integer(raw, R.COMPOSE_BAND)
        print("compose %dx%d -> %dx%d: %d of %d exempt (%.2f %%)" % (w, h, W, H, near.sum(), near.size, 100 * near.mean()))
        assert near.mean() <= R.COMPOSE_CAP
        worst = max(worst, near.mean())
    print("compose: worst case %.2f %%" % (100 * worst))
    for bits, (band, cap) in R.PLANE_BANDS.items():
        worst = 0.0
        for (pw, ph), (ow, oh), rx, ry in R.PLANE_CASES:
            raw = R.ref_planes(pw, ph, ow, oh, rx, ry, bits)[1]
            near = R.D.near_boundary(raw, band)
            print("planes %d bits %dx%d -> %dx%d: %d of %d exempt (%.2f %%)"
                  % (bits, pw, ph, ow, oh, near.sum(), near.size, 100 * near.mean()))
            assert near.mean() <= cap
            worst = max(worst, near.mean())
        print("planes %d bits: worst case %.2f %%" % (bits, 100 * worst))


# ---- ABI validation (host-side, before any launch) ----
P8 = dict(bits=8, msb=0, layout=0)


def planes_call(S, pw=8, ph=8, ow=12, oh=12, rx=(2, 3), ry=(2, 3), sp=None, dp=None, bits=8, msb=0, layout=0,
                src1=64, dst1=64, src0=64, dst0=64):
    B = (1 if bits == 8 else 2) * (2 if layout == 1 else 1)
    S.resize_planes(src0, src1, pw * B if sp is None else sp, pw, ph, dst0, dst1, ow * B if dp is None else dp, ow, oh,
                    rx[0], rx[1], ry[0], ry[1], bits, msb, layout)


INVALID = {
    "luma_w0": lambda S: S.resize_luma(64, 64, 0, 8, 8, 8, 12),
    "luma_W0": lambda S: S.resize_luma(64, 64, 8, 8, 0, 8, 12),
    "luma_W_below_w": lambda S: S.resize_luma(64, 64, 8, 8, 7, 8, 12),
    "luma_W_above_4w": lambda S: S.resize_luma(64, 64, 8, 8, 33, 8, 12),
    "luma_H_below_h": lambda S: S.resize_luma(64, 64, 8, 8, 8, 7, 12),
    "luma_H_above_4h": lambda S: S.resize_luma(64, 64, 8, 8, 8, 33, 12),
    "luma_null": lambda S: S.resize_luma(0, 0, 8, 8, 12, 12, 12),
    "luma_too_large": lambda S: S.resize_luma(64, 64, 30000, 30000, 100000, 100000, 12),
    "compose_h0": lambda S: S.resize_compose(64, 64, 64, 8, 0, 12, 12),
    "compose_W_below_w": lambda S: S.resize_compose(64, 64, 64, 8, 8, 7, 12),
    "compose_H_above_4h": lambda S: S.resize_compose(64, 64, 64, 8, 8, 12, 33),
    "compose_null": lambda S: S.resize_compose(64, 0, 64, 8, 8, 12, 12),
    "compose_rgb_too_large": lambda S: S.resize_compose(64, 64, 64, 20000, 20000, 30000, 30000),
    "yuv_W_above_4w": lambda S: S.yuv_resize_luma(64, 8, 64, 8, 8, 33, 12, 12, 8, 0, S.YUV_FULL),
    "yuv_H_below_h": lambda S: S.yuv_resize_luma(64, 8, 64, 8, 8, 12, 7, 12, 8, 0, S.YUV_FULL),
    "yuv_h0": lambda S: S.yuv_resize_luma(64, 8, 64, 8, 0, 12, 12, 12, 8, 0, S.YUV_FULL),
    "yuv_pitch": lambda S: S.yuv_resize_luma(64, 7, 64, 8, 8, 12, 12, 12, 8, 0, S.YUV_FULL),
    "yuv_pitch_in_samples": lambda S: S.yuv_resize_luma(64, 8, 64, 8, 8, 12, 12, 12, 10, 0, S.YUV_FULL),
    "yuv_odd_pitch": lambda S: S.yuv_resize_luma(64, 17, 64, 8, 8, 12, 12, 12, 10, 0, S.YUV_FULL),
    "yuv_odd_address": lambda S: S.yuv_resize_luma(65, 16, 64, 8, 8, 12, 12, 12, 10, 0, S.YUV_FULL),
    "yuv_7_bits": lambda S: S.yuv_resize_luma(64, 8, 64, 8, 8, 12, 12, 12, 7, 0, S.YUV_FULL),
    "yuv_17_bits": lambda S: S.yuv_resize_luma(64, 16, 64, 8, 8, 12, 12, 12, 17, 0, S.YUV_FULL),
    "yuv_msb_2": lambda S: S.yuv_resize_luma(64, 16, 64, 8, 8, 12, 12, 12, 10, 2, S.YUV_FULL),
    "yuv_msb_at_8_bits": lambda S: S.yuv_resize_luma(64, 8, 64, 8, 8, 12, 12, 12, 8, 1, S.YUV_FULL),
    "yuv_range": lambda S: S.yuv_resize_luma(64, 8, 64, 8, 8, 12, 12, 12, 8, 0, 2),
    "yuv_null": lambda S: S.yuv_resize_luma(0, 8, 64, 8, 8, 12, 12, 12, 8, 0, S.YUV_FULL),
    "planes_zero_numerator": lambda S: planes_call(S, rx=(0, 3)),
    "planes_ratio_below_1": lambda S: planes_call(S, ow=8, rx=(3, 2)),
    "planes_ratio_above_4": lambda S: planes_call(S, ry=(2, 9)),
    "planes_ow_beyond_its_bound": lambda S: planes_call(S, ow=13),
    "planes_oh_beyond_its_bound": lambda S: planes_call(S, oh=13),
    "planes_pw0": lambda S: planes_call(S, pw=0),
    "planes_oh0": lambda S: planes_call(S, oh=0),
    "planes_src_pitch": lambda S: planes_call(S, sp=7),
    "planes_dst_pitch": lambda S: planes_call(S, dp=11),
    "planes_semi_pitch_of_a_planar_row": lambda S: planes_call(S, layout=1, src1=0, dst1=0, sp=8),
    "planes_odd_pitch": lambda S: planes_call(S, bits=10, sp=17),
    "planes_odd_address": lambda S: planes_call(S, bits=10, dst0=65),
    "planes_bits": lambda S: planes_call(S, bits=18),
    "planes_msb_at_8_bits": lambda S: planes_call(S, msb=1),
    "planes_layout": lambda S: planes_call(S, layout=2),
    "planes_null": lambda S: planes_call(S, src0=0),
    "planes_no_second_plane": lambda S: planes_call(S, dst1=0),
    "planes_second_plane_when_semi": lambda S: planes_call(S, layout=1, src1=0),
    "planes_too_many_samples": lambda S: planes_call(S, pw=65536, ph=32768, ow=65536, oh=32768, rx=(1, 1), ry=(1, 1)),
    "net_W_below_w": lambda S: S.upscale_to(S.Net(*DEFAULT), 64, 8, 8, 7, 12, 64, 64, 64, 1 << 30),
    "net_H_above_4h": lambda S: S.upscale_to(S.Net(*DEFAULT), 64, 8, 8, 12, 33, 64, 64, 64, 1 << 30),
    "net_w0": lambda S: S.upscale_to(S.Net(*DEFAULT), 64, 0, 8, 12, 12, 64, 64, 64, 1 << 30),
    "net_null": lambda S: S.upscale_to(S.Net(*DEFAULT), 0, 8, 8, 12, 12, 0, 0, 0, 1 << 30),
    "net_invalid": lambda S: S.upscale_to(S.Net(64, 32, 9, 2, 5), 64, 8, 8, 12, 12, 64, 64, 64, 1 << 30),
}


@pytest.mark.parametrize("what", sorted(INVALID))
def test_resize_validation_errors_without_gpu(S, what):
    """Nothing is launched: the non-null "pointers" here are never touched."""
    with pytest.raises(S.SrcnnError) as e:
        INVALID[what](S)
    assert e.value.code == S.ERR_INVALID, what
    assert S.last_error()


def frame_call(S, net=None, fmt=None, w=37, h=23, W=55, H=35, ws_bytes=1 << 30, **kw):
    f = S.yuv_format(8, 0, S.YUV_PLANAR, 2, 2, S.YUV_FULL) if fmt is None else fmt
    bits, semi = f.bits, f.layout == S.YUV_SEMIPLANAR
    B = 1 if bits == 8 else 2
    cw, CW = -(-w // max(f.cx, 1)), -(-W // max(f.cx, 1))
    src = dict(y=64, u=64, v=None if semi else 64, pitch_y=w * B, pitch_c=cw * B * (2 if semi else 1))
    dst = dict(y=64, u=64, v=None if semi else 64, pitch_y=W * B, pitch_c=CW * B * (2 if semi else 1))
    src.update(kw.get("src", {}))
    dst.update(kw.get("dst", {}))
    mk = lambda d: S.YuvFrame(d["y"], d["u"], d["v"], d["pitch_y"], d["pitch_c"])
    S.upscale_frame_to(S.Net(*DEFAULT) if net is None else net, f if kw.get("fmt_ok", True) else None, mk(src),
                       mk(dst), w, h, W, H, kw.get("params", 64), kw.get("ws", 64), ws_bytes)


FRAME_INVALID = {
    "W_below_w": dict(W=36), "W_above_4w": dict(W=149), "H_below_h": dict(H=22), "H_above_4h": dict(H=93),
    "zero_width": dict(w=0), "zero_output_height": dict(H=0),
    "source_y_pitch": dict(src=dict(pitch_y=36)), "source_c_pitch": dict(src=dict(pitch_c=18)),
    "output_y_pitch": dict(dst=dict(pitch_y=54)), "output_c_pitch": dict(dst=dict(pitch_c=27)),
    "null_source_y": dict(src=dict(y=None)), "null_output_u": dict(dst=dict(u=None)),
    "no_v_in_a_planar_frame": dict(src=dict(v=None)), "null_params": dict(params=None), "null_ws": dict(ws=None),
    "null_fmt": dict(fmt_ok=False), "invalid_net": dict(net=(64, 32, 9, 2, 5)),
    "subsampling_1x2": dict(fmt=(8, 0, 0, 1, 2, 1)), "subsampling_0x0": dict(fmt=(8, 0, 0, 0, 0, 1)),
    "range": dict(fmt=(8, 0, 0, 2, 2, 2)), "17_bits": dict(fmt=(17, 0, 0, 2, 2, 1)), "msb_2": dict(fmt=(10, 2, 0, 2, 2, 1)),
    "msb_at_8_bits": dict(fmt=(8, 1, 0, 2, 2, 1)), "layout_2": dict(fmt=(8, 0, 2, 2, 2, 1)),
    "v_in_a_semi_planar_frame": dict(fmt=(8, 0, 1, 2, 2, 1), dst=dict(v=64)),
    "odd_address_of_words": dict(fmt=(10, 0, 0, 2, 2, 1), src=dict(u=65)),
    "odd_pitch_of_words": dict(fmt=(10, 0, 0, 2, 2, 1), dst=dict(pitch_y=111)),
    "2^32_plane_elements": dict(w=65536, h=65536, W=65536, H=65536),
}


@pytest.mark.parametrize("what", sorted(FRAME_INVALID))
def test_upscale_frame_to_validation_errors_without_gpu(S, what):
    kw = dict(FRAME_INVALID[what])
    if "fmt" in kw:
        kw["fmt"] = S.yuv_format(*kw["fmt"])
    if "net" in kw:
        kw["net"] = S.Net(*kw["net"])
    with pytest.raises(S.SrcnnError) as e:
        frame_call(S, **kw)
    assert e.value.code == S.ERR_INVALID, what
    assert S.last_error().startswith("upscale_frame_to:") or what == "invalid_net", S.last_error()


def test_resize_limits_are_named(S):
    with pytest.raises(S.SrcnnError) as e:
        S.resize_luma(64, 64, 8, 8, 33, 8, 12)
    assert "1x .. 4x" in str(e.value) and str(e.value).count("resize_luma:") == 1
    with pytest.raises(S.SrcnnError) as e:
        S.resize_luma(64, 64, 30000, 30000, 100000, 100000, 12)
    assert "2^31-1" in str(e.value)
    with pytest.raises(S.SrcnnError) as e:
        planes_call(S, ow=13)
    assert "ceil(8 * 3 / 2) = 12" in str(e.value)


def test_workspaces_without_gpu(S):
    net = S.Net(*DEFAULT)
    for query, call in ((S.upscale_to_workspace_bytes,
                         lambda n: S.upscale_to(net, 64, 8, 8, 12, 20, 64, 64, 64, n)),
                        (S.upscale_frame_to_workspace_bytes,
                         lambda n: frame_call(S, w=8, h=8, W=12, H=20, ws_bytes=n))):
        need = query(net, 8, 8, 12, 20)
        # at least the padded plane and the net output
        assert need >= 4 * ((12 + 12) * (20 + 12) + 12 * 20) and need % 256 == 0
        with pytest.raises(S.SrcnnError) as e:
            call(need - 1)
        assert e.value.code == S.ERR_WORKSPACE
        assert query(net, 1, 1, 1, 1) > 0 and query(net, 1, 1, 4, 4) > 0
        # 0 where the call would be invalid
        assert query(S.Net(64, 32, 9, 2, 5), 8, 8, 12, 20) == 0
        for w, h, W, H in [(0, 8, 12, 20), (8, 8, 0, 20), (8, 8, 7, 20), (8, 8, 33, 20), (8, 8, 12, 7), (8, 8, 12, 33),
                           (30000, 30000, 100000, 100000)]:
            assert query(net, w, h, W, H) == 0, (w, h, W, H)
    # an integer ratio needs what the scale call needs
    assert S.upscale_to_workspace_bytes(net, 8, 8, 16, 16) == S.upscale_workspace_bytes(net, 8, 8, 2)
    assert S.upscale_frame_to_workspace_bytes(net, 8, 8, 16, 16) == S.upscale_yuv_workspace_bytes(net, 8, 8, 2)


# ---- CLI ----
def cnn(*args):
    return subprocess.run([CNN, *args], capture_output=True, text=True, timeout=120)


def test_cli_size_argument_errors(tmp_path):
    base = ("upscale", "-c", "x.json", "-i", "y.png", "-o", "z.png")
    for bad in ("55", "55x", "x35", "0x35", "55x0", "55x35x2", "-55x35", "55X35", "5.5x35"):
        p = cnn(*base, "--size", bad)
        assert p.returncode == 1 and "--size must be WxH" in p.stdout and "usage: cnn" in p.stdout, bad
    p = cnn(*base, "--size", "55x35", "--scale", "2")
    assert p.returncode == 1 and "--size and --scale exclude each other" in p.stdout and "usage: cnn" in p.stdout
    p = cnn("-c", "x.json", "-i", "y.png", "-o", "z.png", "--size", "55x35")
    assert p.returncode == 1 and "--size needs the upscale mode" in p.stdout
    p = cnn(*base, "--size")
    assert p.returncode == 1 and "missing value for --size" in p.stdout
    # --scale's messages stay as they are
    p = cnn(*base, "--scale", "5")
    assert p.returncode == 1 and "--scale must be 1, 2, 3 or 4" in p.stdout
    p = cnn("-h")
    assert p.returncode == 0 and "--size WxH" in p.stdout
    # a size outside [1x, 4x] of the input's names the limits, for an image and for a Y4M stream
    from PIL import Image
    img = tmp_path / "in.png"
    Image.fromarray(np.zeros((23, 37, 3), np.uint8)).save(img)
    y4m = tmp_path / "in.y4m"
    y4m.write_bytes(b"YUV4MPEG2 W37 H23 F25:1 Ip A1:1 C420jpeg\n")
    for src in (img, y4m):
        for size in ("36x35", "149x35", "55x22", "55x93"):
            p = cnn("upscale", "-c", "x.json", "-i", str(src), "-o", str(tmp_path / "o"), "--size", size)
            assert p.returncode == 1, p.stdout
            assert "--size %s is outside 1x .. 4x of the input's 37x23" % size in p.stdout, p.stdout
            assert "37 .. 148" in p.stdout and "23 .. 92" in p.stdout


# ---- y4m::Header::resized ----
@pytest.mark.parametrize("head,W,H,want", [
    # both ratios equal: A stays
    (b"W1280 H720 F30000:1001 Ip A1:1 C420jpeg XCOLORRANGE=FULL", 1920, 1080,
     b"W1920 H1080 F30000:1001 Ip A1:1 C420jpeg XCOLORRANGE=FULL"),
    (b"W37 H23 F25:1 Ip A4:3 C422", 74, 46, b"W74 H46 F25:1 Ip A4:3 C422"),
    # anamorphic 720 x 480 at 32:27 -> 1920 x 1080: 32/27 * (720 * 1080) / (1920 * 480) = 1
    (b"W720 H480 F30000:1001 Ip A32:27 C420jpeg", 1920, 1080, b"W1920 H1080 F30000:1001 Ip A1:1 C420jpeg"),
    # 37 x 23 -> 55 x 35: 1 * (37 * 35) / (55 * 23) = 1295/1265 = 259/253
    (b"W37 H23 F25:1 Ip A1:1 C420p10 XCOLORRANGE=LIMITED", 55, 35,
     b"W55 H35 F25:1 Ip A259:253 C420p10 XCOLORRANGE=LIMITED"),
    (b"W37 H23 F25:1 Ip A10:11 C444", 55, 35, b"W55 H35 F25:1 Ip A2590:2783 C444"),
    # unknown and absent aspect ratios stay as they are
    (b"W37 H23 F25:1 Ip A0:0 C420jpeg", 55, 35, b"W55 H35 F25:1 Ip A0:0 C420jpeg"),
    (b"W37 H23 F25:1", 55, 35, b"W55 H35 F25:1"),
])
def test_y4m_header_resized(tmp_path, head, W, H, want):
    src = tmp_path / "in.y4m"
    src.write_bytes(b"YUV4MPEG2 " + head + b"\n")
    p = subprocess.run([TOOL, str(src), str(W), str(H)], capture_output=True, timeout=60)
    assert p.returncode == 0, p.stdout
    assert p.stdout == b"YUV4MPEG2 " + want + b"\n"
