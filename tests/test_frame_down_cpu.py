"""The downscale of Y'CbCr frames without a GPU: the float64
reference (tests/frame_down_ref.py) against its own anchors, the seed search
the GPU test relies on, the declarations of include/srcnn.h and their Python
binding, and every argument the four new calls reject before a launch (the
"pointers" are small integers that are never dereferenced, as in
tests/test_upscale_abi_cpu.py)."""
import inspect
import os
import re

import numpy as np
import pytest

import frame_down_ref as F
import pairs_ref as P
import yuv_deep_ref as D
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "srcnn.h")
NEW = ["srcnn_downscale_planes", "srcnn_downscale_frame", "srcnn_make_pairs_frame_workspace_bytes",
       "srcnn_make_pairs_frame", "srcnn_evaluate_frame_workspace_bytes", "srcnn_evaluate_frame"]


@pytest.fixture(scope="module")
def S():
    import srcnn_amd
    return srcnn_amd


# ---- 1: the reference ----
@pytest.mark.parametrize("s", [1, 2, 3, 4])
def test_matrix_rows_sum_to_one(s):
    for n in (1, 2, 5, 17, 64, 65):
        for out in {1, max(1, n // s), F.ceil_div(n, s)}:
            M = F.matrix(n, s, out)
            assert M.shape == (out, n)
            assert np.abs(M.sum(axis=1) - 1.0).max() <= 1e-15


@pytest.mark.parametrize("bits,msb", [(8, 0), (10, 0), (10, 1), (16, 0), (16, 1)])
def test_scale_1_is_the_source(bits, msb):
    src = D.encode(F.values_of(37, 23, bits, 0), bits, msb)
    q, raw = F.planes(src, 1, 37, 23, bits, msb)
    assert np.array_equal(q, src)
    assert np.array_equal(raw, D.decode(src, bits, msb))


def test_partial_output_is_the_top_left_of_the_full_one():
    a = F.values_of(37, 23, 10, 0)[0]
    full = F.down(a, 3, 13, 8)
    assert np.abs(F.down(a, 3, 5, 2) - full[:2, :5]).max() <= 1e-9  # (the order of the sums may differ)


@pytest.mark.parametrize("W,H,ax,ay", F.RAMPS)
@pytest.mark.parametrize("s", [1, 2, 3, 4])
@pytest.mark.parametrize("bits,rng", [(8, D.LIMITED), (10, D.FULL)])
def test_reference_down_then_up_is_shift_free(s, W, H, ax, ay, bits, rng):
    """on the ramps Y = 2x + y + 16 and Y = x + 2y + 16, down by
    s, then yuv_deep_ref.luma_plane by s, returns the ramp at least 4s pixels
    from every edge: to float64 rounding at s = 1, 3; at s = 2, 4 every
    low-resolution value is k + 0.5 with k of one parity (odd at s = 2, even at
    s = 4), so ties-to-even moves all of them the same way and the error is
    exactly half a code value.  A shift of X by one pixel along the steep axis
    gives at least 1.5 code values."""
    Y = D.encode(F.ramp(W, H, ax, ay), bits, 0)
    w, h = W // s, H // s
    small, raw = F.planes(Y, s, w, h, bits, 0)
    gain = D.levels(bits, rng)[1]
    X = D.luma_plane(small, s, 0, bits, 0, rng) * gain
    T = (D.luma_plane(Y, 1, 0, bits, 0, rng) * gain)[:s * h, :s * w]
    e = 4 * s
    d = np.abs(X - T)[e:-e, e:-e].max()
    print("reference down/up x%d on %dx%d, %d bits: interior max |X - T| = %.6f code values" % (s, W, H, bits, d))
    if s in (1, 3):
        assert d <= 1e-9
    else:
        assert abs(d - 0.5) <= 1e-9
        frac = raw[e // s:-(e // s), e // s:-(e // s)] % 1.0
        assert np.abs(frac - 0.5).max() <= 1e-9
    for step in (1, -1):
        ds = np.abs(np.roll(X, step, axis=1 if ax == 2 else 0) - T)[e:-e, e:-e].max()
        assert ds >= 1.5 - 1e-9


def test_crop_rule_inequality():
    """ceil(floor(W/s) / cx) <= ceil(ceil(W/cx) / s) for every W <= 64, s <= 4,
    cx <= 2: the chroma output of srcnn_downscale_frame is within
    srcnn_downscale_planes' bound; and s * that can exceed the source (W = 10,
    s = 3, cx = 2: 2 columns from 5), which is why the bound is a ceiling."""
    beyond = []
    for W in range(1, 65):
        for s in range(1, 5):
            if W < s:
                continue
            for cx in (1, 2):
                out, src = F.ceil_div(W // s, cx), F.ceil_div(W, cx)
                assert 1 <= out <= F.ceil_div(src, s), (W, s, cx)
                if s * out > src:
                    beyond.append((W, s, cx))
    assert (10, 3, 2) in beyond
    assert F.frame_sizes(10, 10, 3, 2, 2) == ((3, 3), (5, 5), (2, 2))


@pytest.mark.parametrize("s", [1, 2, 3, 4])
def test_gray_image_is_downscale_rgba_off_the_ties(s):
    """On a gray image the reference equals pairs_ref.down_rgba's channel
    wherever the unrounded value is not an exact half-integer: the two differ
    in the tie rule alone (to even here, upwards there)."""
    g = np.random.default_rng(4).integers(0, 256, (46, 61)).astype(np.uint8)
    rgba = np.stack([g, g, g, np.full_like(g, 255)], axis=-1)
    small, raw_rgba = P.down_rgba(rgba, s)
    q, raw = F.planes(g, s, 61 // s, 46 // s, 8, 0)
    assert np.abs(raw - raw_rgba[..., 0]).max() <= 1e-9  # (the order of the sums may differ)
    tie = np.abs(raw % 1.0 - 0.5) <= 1e-9
    assert np.array_equal(q[~tie], small[..., 0][~tie])
    # the two tie rules themselves
    assert np.array_equal(D.quantise(np.array([0.5, 1.5, 2.5]), 8, 0), [0, 2, 2])
    assert np.array_equal(P.quantise(np.array([0.5, 1.5, 2.5])), [1, 2, 3])


# ---- 2: the seed search ----
@pytest.mark.parametrize("bits", [8, 10, 12])
def test_every_case_finds_a_seed(bits):
    """Each case of the GPU test takes the first seed in 0..7 for which the
    share of reference values within 1e-3 * 2^(bits-8) of a half-integer stays
    within the cap (1 % / 2.5 % / 10 % at 8 / 10 / 12 bits)."""
    worst = 0
    for ow, oh, s, v in F.cases():
        seed = F.seed_of(ow, oh, s, v, bits)
        assert seed is not None, (ow, oh, s, v, bits)
        worst = max(worst, seed)
    print("%d bits: largest seed taken %d" % (bits, worst))


# ---- 3: declarations and binding ----
def test_header_declares_the_new_calls(S):
    src = open(HEADER).read()
    declared = set(re.findall(r"SRCNN_API\s+[\w\s\*]+?\b(srcnn_\w+)\s*\(", src))
    for name in NEW:
        assert name in declared, name
        assert name in S.exported_symbols(), name
    assert "#define SRCNN_ABI_VERSION 1" in src


def test_binding_signatures(S):
    want = {
        "downscale_planes": ["src0", "src1", "src_pitch", "pw", "ph", "dst0", "dst1", "dst_pitch", "ow", "oh", "scale",
                             "bits", "msb", "layout", "s"],
        "downscale_frame": ["fmt", "src", "dst", "W", "H", "scale", "s"],
        "make_pairs_frame_workspace_bytes": ["fmt", "W", "H", "scale"],
        "make_pairs_frame": ["fmt", "frame", "W", "H", "scale", "tile", "stride", "X", "T", "ws", "ws_bytes", "s"],
        "evaluate_frame_workspace_bytes": ["net", "fmt", "W", "H", "scale"],
        "evaluate_frame": ["net", "fmt", "truth", "W", "H", "scale", "shave", "params", "result", "ws", "ws_bytes", "s"],
    }
    for name, args in want.items():
        assert list(inspect.signature(getattr(S, name)).parameters) == args, name
    # as many C arguments as the header's prototype
    src = open(HEADER).read()
    for name in NEW:
        proto = re.search(r"SRCNN_API\s+[\w\s\*]+?\b%s\s*\(([^;]*)\);" % name, src).group(1)
        assert len(S.SIGNATURES[name][1]) == proto.count(",") + 1, name


# ---- 4: invalid arguments, before any launch ----
A = 1 << 20  # an even, 8-byte aligned "address"
BIG = 1 << 40


def fails(S, call, code, part):
    with pytest.raises(S.SrcnnError) as e:
        call()
    assert e.value.code == code, (code, S.last_error())
    assert part in S.last_error(), (part, S.last_error())


def planes_args(**kw):
    """a valid 10-bit planar two-plane call: 10 x 9 -> 4 x 3 at scale 3"""
    g = dict(src0=A, src1=2 * A, sp=20, pw=10, ph=9, dst0=3 * A, dst1=4 * A, dp=8, ow=4, oh=3, scale=3, bits=10, msb=0,
             layout=0)
    g.update(kw)
    return [g[k] for k in ("src0", "src1", "sp", "pw", "ph", "dst0", "dst1", "dp", "ow", "oh", "scale", "bits", "msb",
                           "layout")]


PLANES_INVALID = {
    "scale_0": (dict(scale=0), "scale 0"), "scale_5": (dict(scale=5), "scale 5"),
    "pw_0": (dict(pw=0), "empty plane"), "ph_0": (dict(ph=0), "empty plane"),
    "ow_0": (dict(ow=0), "empty plane"), "oh_0": (dict(oh=0), "empty plane"),
    "ow_beyond": (dict(ow=5, dp=10), "exceeds ceil"), "oh_beyond": (dict(oh=4), "exceeds ceil"),
    "src1_alone": (dict(dst1=None), "exactly one"), "dst1_alone": (dict(src1=None), "exactly one"),
    "null_src0": (dict(src0=None), "null buffer"), "null_dst0": (dict(dst0=None), "null buffer"),
    "src_pitch_below_row": (dict(sp=18), "pitch 18"), "dst_pitch_below_row": (dict(dp=6), "pitch 6"),
    "pitch_in_samples": (dict(sp=10), "pitch 10"),
    "odd_src_pitch": (dict(sp=21), "odd"), "odd_dst_pitch": (dict(dp=9), "odd"),
    "semi_pitch_of_a_planar_row": (dict(layout=1, src1=None, dst1=None, sp=20, dp=16), "pitch 20"),
    "second_plane_when_semi": (dict(layout=1, sp=40, dp=16, dst1=None), "semi-planar"),
    "bits_7": (dict(bits=7), "7 bits"), "bits_17": (dict(bits=17), "17 bits"), "msb_2": (dict(msb=2), "msb 2"),
    "msb_at_8_bits": (dict(bits=8, msb=1), "msb 1"), "layout_2": (dict(layout=2), "layout 2"),
    "odd_src0": (dict(src0=A + 1), "odd address"), "odd_src1": (dict(src1=A + 1), "odd address"),
    "odd_dst0": (dict(dst0=A + 1), "odd address"), "odd_dst1": (dict(dst1=A + 1), "odd address"),
    "samples": (dict(pw=65536, ph=32768, sp=131072, ow=4, oh=3), "2^31-1"),
}


@pytest.mark.parametrize("what", sorted(PLANES_INVALID))
def test_downscale_planes_rejects(S, what):
    kw, part = PLANES_INVALID[what]
    fails(S, lambda: S.downscale_planes(*planes_args(**kw)), S.ERR_INVALID, part)
    assert S.last_error().startswith("downscale_planes:")


def fmt_of(S, **kw):
    f = dict(bits=10, msb=0, layout=0, cx=2, cy=2, yuv_range=S.YUV_LIMITED)
    f.update(kw)
    return S.yuv_format(**f)


def frame_of(S, w, h, B=2, nch=1, **kw):
    """a frame of w x h luma samples, 4:2:0, tight pitches"""
    f = dict(y=A, u=2 * A, v=3 * A if nch == 1 else None, pitch_y=w * B, pitch_c=-(-w // 2) * nch * B)
    f.update(kw)
    return S.yuv_frame(f["y"], f["u"], f["v"], f["pitch_y"], f["pitch_c"])


# what every frame-level call rejects in its format: (fmt keywords, part of the message)
FORMAT_INVALID = {
    "bits_7": (dict(bits=7), "7 bits"), "bits_17": (dict(bits=17), "17 bits"), "msb_2": (dict(msb=2), "msb 2"),
    "msb_at_8_bits": (dict(bits=8, msb=1), "msb 1"), "layout_2": (dict(layout=2), "layout 2"),
    "subsampling_1x2": (dict(cx=1, cy=2), "subsampling"), "subsampling_0x0": (dict(cx=0, cy=0), "subsampling"),
    "range_2": (dict(yuv_range=2), "range 2"),
}
# ... and in a frame it reads or writes whole (47 x 35 luma samples of two bytes)
FRAME_INVALID = {
    "null_y": (dict(y=None), "null plane"), "null_u": (dict(u=None), "null plane"),
    "null_v_planar": (dict(v=None), "null plane"),
    "odd_y": (dict(y=A + 1), "odd address"), "odd_u": (dict(u=A + 1), "odd address"),
    "odd_v": (dict(v=A + 1), "odd address"),
    "pitch_y_below_row": (dict(pitch_y=92), "pitch 92"), "pitch_c_below_row": (dict(pitch_c=46), "pitch 46"),
    "odd_pitch_y": (dict(pitch_y=95), "odd"), "odd_pitch_c": (dict(pitch_c=49), "odd"),
}


def down_frame_call(S, fmt="default", src=None, dst=None, W=47, H=35, scale=2, null_src=False, null_dst=False):
    f = fmt_of(S) if fmt == "default" else fmt
    s = None if null_src else (frame_of(S, W, H) if src is None else src)
    d = None if null_dst else (frame_of(S, 23, 17, y=4 * A, u=5 * A, v=6 * A) if dst is None else dst)
    return lambda: S.downscale_frame(f, s, d, W, H, scale)


def test_downscale_frame_rejects(S):
    bad = {
        "null_fmt": (dict(fmt=None), "null srcnn_yuv_format"),
        "scale_0": (dict(scale=0), "scale 0"), "scale_5": (dict(scale=5), "scale 5"),
        "smaller_than_the_scale": (dict(W=1, scale=2), "smaller than the scale"),
        "H_0": (dict(H=0), "smaller than the scale"),
        "null_src": (dict(null_src=True), "null buffer"), "null_dst": (dict(null_dst=True), "null buffer"),
        "v_of_semiplanar": (dict(fmt=fmt_of(S, layout=1), src=frame_of(S, 47, 35, nch=2, v=A)), "semi-planar"),
        "output_y_pitch": (dict(dst=frame_of(S, 23, 17, pitch_y=44)), "pitch 44"),
        "output_c_pitch": (dict(dst=frame_of(S, 23, 17, pitch_c=22)), "pitch 22"),
        "null_output_u": (dict(dst=frame_of(S, 23, 17, u=None)), "null plane"),
        "odd_output_v": (dict(dst=frame_of(S, 23, 17, v=A + 1)), "odd address"),
        "samples": (dict(W=65536, H=32768, src=frame_of(S, 65536, 32768)), "2^31-1"),
    }
    for k, (kw, part) in FORMAT_INVALID.items():
        bad["fmt_" + k] = (dict(fmt=fmt_of(S, **kw)), part)
    for k, (kw, part) in FRAME_INVALID.items():
        bad["src_" + k] = (dict(src=frame_of(S, 47, 35, **kw)), part)
    for what, (kw, part) in bad.items():
        fails(S, down_frame_call(S, **kw), S.ERR_INVALID, part)
        assert S.last_error().startswith("downscale_frame:"), what


def pairs_call(S, fmt="default", frame="default", W=47, H=35, scale=2, tile=9, stride=4, X=4 * A, T=5 * A, ws=6 * A,
               ws_bytes=BIG):
    f = fmt_of(S) if fmt == "default" else fmt
    fr = frame_of(S, W, H, u=None, v=None) if frame == "default" else frame
    return lambda: S.make_pairs_frame(f, fr, W, H, scale, tile, stride, X, T, ws, ws_bytes)


def test_make_pairs_frame_rejects(S):
    bad = {
        "null_fmt": (dict(fmt=None), "null srcnn_yuv_format"),
        "scale_0": (dict(scale=0), "scale 0"), "scale_5": (dict(scale=5), "scale 5"),
        "smaller_than_the_scale": (dict(W=2, scale=3), "smaller than the scale"),
        "tile_0": (dict(tile=0), "must be > 0"), "stride_0": (dict(stride=0), "must be > 0"),
        "no_tile_fits": (dict(tile=35), "holds no"),
        "null_frame": (dict(frame=None), "null buffer"), "null_X": (dict(X=None), "null buffer"),
        "null_T": (dict(T=None), "null buffer"), "null_ws": (dict(ws=None), "null buffer"),
        "null_y": (dict(frame=frame_of(S, 47, 35, y=None)), "null plane"),
        "odd_y": (dict(frame=frame_of(S, 47, 35, y=A + 1)), "odd address"),
        "odd_ws": (dict(ws=A + 1), "odd address"),
        "pitch_y_below_row": (dict(frame=frame_of(S, 47, 35, pitch_y=92)), "pitch 92"),
        "odd_pitch_y": (dict(frame=frame_of(S, 47, 35, pitch_y=95)), "odd"),
        "samples": (dict(W=65536, H=32768), "2^31-1"),
    }
    for k, (kw, part) in FORMAT_INVALID.items():
        bad["fmt_" + k] = (dict(fmt=fmt_of(S, **kw)), part)
    for what, (kw, part) in bad.items():
        fails(S, pairs_call(S, **kw), S.ERR_INVALID, part)
        assert S.last_error().startswith("make_pairs_frame:"), what
    # the chroma planes and their pitch are not looked at: this one fails for its workspace alone
    need = S.make_pairs_frame_workspace_bytes(fmt_of(S), 47, 35, 2)
    # small 23 x 17 words | X 46 x 34 floats | T 47 x 35 floats, each a multiple of 256 bytes
    assert need == 1024 + 6400 + 6656
    fails(S, pairs_call(S, frame=frame_of(S, 47, 35, u=None, v=None, pitch_c=1), ws_bytes=need - 1), S.ERR_WORKSPACE,
          "workspace")
    assert S.make_pairs_frame_workspace_bytes(fmt_of(S, bits=8), 47, 35, 2) == 512 + 6400 + 6656
    for q in (lambda: S.make_pairs_frame_workspace_bytes(None, 47, 35, 2),
              lambda: S.make_pairs_frame_workspace_bytes(fmt_of(S), 47, 35, 0),
              lambda: S.make_pairs_frame_workspace_bytes(fmt_of(S), 47, 35, 5),
              lambda: S.make_pairs_frame_workspace_bytes(fmt_of(S), 1, 35, 2),
              lambda: S.make_pairs_frame_workspace_bytes(fmt_of(S, bits=17), 47, 35, 2),
              lambda: S.make_pairs_frame_workspace_bytes(fmt_of(S, cx=3), 47, 35, 2),
              lambda: S.make_pairs_frame_workspace_bytes(fmt_of(S), 65536, 32768, 2)):
        assert q() == 0


NETS = {"default": (64, 32, 9, 1, 5), "example": (32, 16, 9, 1, 5), "even": (64, 32, 9, 2, 5)}


def eval_call(S, net="default", fmt="default", truth="default", W=47, H=35, scale=2, shave=3, params=4 * A,
              result=5 * A, ws=6 * A, ws_bytes=BIG):
    n = None if net is None else S.Net(*NETS[net])
    f = fmt_of(S) if fmt == "default" else fmt
    t = frame_of(S, W, H) if truth == "default" else truth
    return lambda: S.evaluate_frame(n, f, t, W, H, scale, shave, params, result, ws, ws_bytes)


def test_evaluate_frame_rejects(S):
    bad = {
        "null_net": (dict(net=None), "null srcnn_net"), "even_filter": (dict(net="even"), ""),
        "null_fmt": (dict(fmt=None), "null srcnn_yuv_format"),
        "scale_0": (dict(scale=0), "scale 0"), "scale_5": (dict(scale=5), "scale 5"),
        "smaller_than_the_scale": (dict(W=1, scale=2), "smaller than the scale"),
        "no_window": (dict(W=30, H=30, shave=10, truth=frame_of(S, 30, 30)), "11x11"),
        "shave_wraps": (dict(shave=0x80000003), "11x11"),
        "null_truth": (dict(truth=None), "null buffer"), "null_params": (dict(params=None), "null buffer"),
        "null_result": (dict(result=None), "null buffer"), "null_ws": (dict(ws=None), "null buffer"),
        "v_of_semiplanar": (dict(fmt=fmt_of(S, layout=1), truth=frame_of(S, 47, 35, nch=2, v=A)), "semi-planar"),
        "result_misaligned": (dict(result=5 * A + 4), "8-byte"), "ws_misaligned": (dict(ws=6 * A + 4), "8-byte"),
        "samples": (dict(W=65536, H=32768), "2^31-1"),
    }
    for k, (kw, part) in FORMAT_INVALID.items():
        bad["fmt_" + k] = (dict(fmt=fmt_of(S, **kw)), part)
    for k, (kw, part) in FRAME_INVALID.items():
        bad["truth_" + k] = (dict(truth=frame_of(S, 47, 35, **kw)), part)
    for what, (kw, part) in bad.items():
        fails(S, eval_call(S, **kw), S.ERR_INVALID, part)
        if what != "even_filter":  # (the message is srcnn_forward's own)
            assert S.last_error().startswith("evaluate_frame:"), what
    for net in ("default", "example"):
        n = S.Net(*NETS[net])
        need = S.evaluate_frame_workspace_bytes(n, fmt_of(S), 47, 35, 2)
        up, q = S.upscale_yuv_workspace_bytes(n, 23, 17, 2), S.quality_frame_workspace_bytes(46, 34, 2, 2, 0)
        assert up > 0 and q > 0
        al = lambda b: -(-b // 256) * 256
        # small frame 23 x 17 (chroma 12 x 9), output 46 x 34 (chroma 23 x 17), two bytes a sample; luma plane
        frames = al(46 * 17) + 2 * al(24 * 9) + al(92 * 34) + 2 * al(46 * 17)
        assert need == frames + al(46 * 34 * 4) + al(up) + al(q)
        fails(S, eval_call(S, net=net, ws_bytes=need - 1), S.ERR_WORKSPACE, "workspace")
        # semi-planar: one chroma plane of pairs per frame
        semi = S.evaluate_frame_workspace_bytes(n, fmt_of(S, msb=1, layout=1), 47, 35, 2)
        assert semi == need - 2 * al(24 * 9) - 2 * al(46 * 17) + al(48 * 9) + al(92 * 17)
    n = S.Net(*NETS["default"])
    for q in (lambda: S.evaluate_frame_workspace_bytes(None, fmt_of(S), 47, 35, 2),
              lambda: S.evaluate_frame_workspace_bytes(S.Net(*NETS["even"]), fmt_of(S), 47, 35, 2),
              lambda: S.evaluate_frame_workspace_bytes(n, None, 47, 35, 2),
              lambda: S.evaluate_frame_workspace_bytes(n, fmt_of(S), 47, 35, 0),
              lambda: S.evaluate_frame_workspace_bytes(n, fmt_of(S), 47, 35, 5),
              lambda: S.evaluate_frame_workspace_bytes(n, fmt_of(S), 1, 35, 2),
              lambda: S.evaluate_frame_workspace_bytes(n, fmt_of(S), 10, 10, 2),  # no 11 x 11 window
              lambda: S.evaluate_frame_workspace_bytes(n, fmt_of(S, layout=2), 47, 35, 2),
              lambda: S.evaluate_frame_workspace_bytes(n, fmt_of(S), 65536, 32768, 2)):
        assert q() == 0


# ---- 5: the command line's argument errors ----
def test_cli_argument_errors():
    import subprocess
    cnn = os.path.join(ROOT, "cnn-super-resolution_amd", "bin", "cnn")

    def run(*args):
        return subprocess.run([cnn, *args], capture_output=True, text=True, timeout=60)

    for args, msg in [
        (("downscale", "-i", "x.y4m", "--frame-step", "2"), "--frame-step needs train --from-images"),
        (("train", "-c", "c", "-i", "d", "--frame-step", "2"), "--frame-step needs train --from-images"),
        (("train", "--from-images", "-c", "c", "-i", "d", "--frame-step", "0"), "--frame-step must be a positive integer"),
        (("train", "--from-images", "-c", "c", "-i", "d", "--frame-step", "-1"), "--frame-step must be a positive integer"),
        (("train", "--from-images", "-c", "c", "-i", "d", "--frame-step"), "missing value for --frame-step"),
        (("train", "-c", "c", "-i", "d", "--frames", "2"), "--frames needs the upscale, downscale, quality or evaluate mode"),
        (("evaluate", "-c", "c", "-i", "x.y4m", "--frames", "0"), "--frames must be a positive integer"),
        (("downscale", "-i", "x.y4m", "--scale", "5"), "--scale must be 1, 2, 3 or 4"),
        (("downscale", "--frames", "2"), "--in is required"),
        (("evaluate", "-i", "x.y4m", "--frames", "2"), "--config and --in are required"),
    ]:
        p = run(*args)
        assert p.returncode == 1 and msg in p.stdout, (args, p.stdout[:200])
    usage = run("--help").stdout
    for word in ("--frame-step N", "A Y4M video is streamed frame by frame", "A Y4M video is evaluated frame by frame"):
        assert word in usage
