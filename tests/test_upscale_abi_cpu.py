"""What the upscale family of the C ABI answers to invalid input, pinned: every
entry point's (return code, srcnn_last_error()) on single faults, on pairs of
faults (which message wins) and on a workspace one byte short, and what the
workspace queries return over a grid of nets and sizes, against
tests/golden/upscale_abi_errors.json.

The library validates before any launch, so nothing here needs a device: the
non-null "pointers" are small integers that are never dereferenced.  The last
error is sticky (a call that fails without a message leaves the one before),
so every entry starts from the same one, SENTINEL's.

    python tests/test_upscale_abi_cpu.py record     writes the golden file
"""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "upscale_abi_errors.json")

NETS = {"default": (64, 32, 9, 1, 5), "example": (32, 16, 9, 1, 5), "wide": (128, 64, 9, 5, 5),
        "even": (64, 32, 9, 2, 5), "overflow": (64, 32, 0xffffffff, 0xffffffff, 0xffffffff), "null": None}
BIG = 1 << 40  # a workspace size that is never short


def merged(a, b):
    """b over a; the dicts under "src" and "dst" merge too"""
    out = dict(a)
    for k, v in b.items():
        out[k] = merged(out.get(k) or {}, v) if isinstance(v, dict) else v
    return out


# ---- the entry points: name -> arguments from keywords, every default valid ----
def _net(S, k):
    return None if NETS[k] is None else S.Net(*NETS[k])


def _bytes(bits):
    return 1 if bits == 8 else 2


FMT = dict(bits=8, msb=0, layout=0, cx=2, cy=2, range=1)


def _format(S, fmt):
    """(the format's fields, the YuvFormat or None for fmt=None)"""
    f = merged(FMT, fmt or {})
    return f, None if fmt is None else S.yuv_format(f["bits"], f["msb"], f["layout"], f["cx"], f["cy"], f["range"])


def _frames(S, w, h, W, H, f, src, dst, null_src=False, null_dst=False):
    cx, B, semi = f["cx"], _bytes(f["bits"]), f["layout"] == 1
    cw, CW = -(-w // max(cx, 1)), -(-W // max(cx, 1))
    s = dict(y=64, u=64, v=None if semi else 64, pitch_y=w * B, pitch_c=cw * B * (2 if semi else 1))
    d = dict(y=64, u=64, v=None if semi else 64, pitch_y=W * B, pitch_c=CW * B * (2 if semi else 1))
    s.update(src)
    d.update(dst)
    mk = lambda f: S.YuvFrame(f["y"], f["u"], f["v"], f["pitch_y"] & 0xffffffff, f["pitch_c"] & 0xffffffff)
    return None if null_src else mk(s), None if null_dst else mk(d)


def upscale_luma(S, rgba=64, out=64, w=8, h=8, scale=2, pad=12):
    return rgba, out, w, h, scale, pad, None


def upscale_compose(S, rgba=64, luma=64, rgb=64, w=8, h=8, scale=2):
    return rgba, luma, rgb, w, h, scale, None


def yuv_upscale_luma(S, y=64, pitch=None, out=64, w=8, h=8, scale=2, pad=12, range=1):
    return y, w if pitch is None else pitch, out, w, h, scale, pad, range, None


def yuv_upscale_luma16(S, y=64, pitch=None, out=64, w=8, h=8, scale=2, pad=12, bits=10, msb=0, range=1):
    return y, w * _bytes(bits) if pitch is None else pitch, out, w, h, scale, pad, bits, msb, range, None


def yuv_compose_luma(S, luma=64, y=64, pitch=None, W=16, H=16, range=1):
    return luma, y, W if pitch is None else pitch, W, H, range, None


def yuv_compose_luma16(S, luma=64, y=64, pitch=None, W=16, H=16, bits=10, msb=0, range=1):
    return luma, y, W * _bytes(bits) if pitch is None else pitch, W, H, bits, msb, range, None


def upscale_planes_u8(S, src0=64, src1=64, sp=None, pw=8, ph=8, dst0=64, dst1=64, dp=None, ow=16, oh=16, scale=2):
    return src0, src1, pw if sp is None else sp, pw, ph, dst0, dst1, ow if dp is None else dp, ow, oh, scale, None


def _plane_pitches(pw, ow, sp, dp, bits, layout):
    B = _bytes(bits) * (2 if layout == 1 else 1)
    return (pw * B) & 0xffffffff if sp is None else sp, (ow * B) & 0xffffffff if dp is None else dp


def upscale_planes(S, src0=64, src1=64, sp=None, pw=8, ph=8, dst0=64, dst1=64, dp=None, ow=16, oh=16, scale=2,
                   bits=10, msb=0, layout=0):
    sp, dp = _plane_pitches(pw, ow, sp, dp, bits, layout)
    return src0, src1, sp, pw, ph, dst0, dst1, dp, ow, oh, scale, bits, msb, layout, None


def resize_luma(S, rgba=64, out=64, w=8, h=8, W=12, H=12, pad=12):
    return rgba, out, w, h, W, H, pad, None


def resize_compose(S, rgba=64, luma=64, rgb=64, w=8, h=8, W=12, H=12):
    return rgba, luma, rgb, w, h, W, H, None


def yuv_resize_luma(S, y=64, pitch=None, out=64, w=8, h=8, W=12, H=12, pad=12, bits=10, msb=0, range=1):
    return y, w * _bytes(bits) if pitch is None else pitch, out, w, h, W, H, pad, bits, msb, range, None


def resize_planes(S, src0=64, src1=64, sp=None, pw=8, ph=8, dst0=64, dst1=64, dp=None, ow=12, oh=12, rx=(2, 3),
                  ry=(2, 3), bits=10, msb=0, layout=0):
    sp, dp = _plane_pitches(pw, ow, sp, dp, bits, layout)
    return src0, src1, sp, pw, ph, dst0, dst1, dp, ow, oh, rx[0], rx[1], ry[0], ry[1], bits, msb, layout, None


def upscale(S, net="default", rgba=64, w=8, h=8, scale=2, params=64, rgb=64, ws=64, ws_bytes=BIG):
    return _net(S, net), rgba, w, h, scale, params, rgb, ws, ws_bytes, None


def upscale_to(S, net="default", rgba=64, w=8, h=8, W=12, H=20, params=64, rgb=64, ws=64, ws_bytes=BIG):
    return _net(S, net), rgba, w, h, W, H, params, rgb, ws, ws_bytes, None


def upscale_yuv(S, net="default", w=37, h=23, cx=2, cy=2, scale=2, range=1, params=64, ws=64, ws_bytes=BIG, src={},
                dst={}, **nulls):
    s, d = _frames(S, w, h, w * scale, h * scale, merged(FMT, dict(cx=cx)), src, dst, **nulls)
    return _net(S, net), s, d, w, h, cx, cy, scale, range, params, ws, ws_bytes, None


def upscale_frame(S, net="default", fmt={}, w=37, h=23, scale=2, params=64, ws=64, ws_bytes=BIG,
                  src={}, dst={}, **nulls):
    f, fmt = _format(S, fmt)
    s, d = _frames(S, w, h, w * scale, h * scale, f, src, dst, **nulls)
    return _net(S, net), fmt, s, d, w, h, scale, params, ws, ws_bytes, None


def upscale_frame_to(S, net="default", fmt={}, w=37, h=23, W=55, H=35, params=64, ws=64,
                     ws_bytes=BIG, src={}, dst={}, **nulls):
    f, fmt = _format(S, fmt)
    s, d = _frames(S, w, h, W, H, f, src, dst, **nulls)
    return _net(S, net), fmt, s, d, w, h, W, H, params, ws, ws_bytes, None


def evaluate(S, net="default", rgba=64, W=48, H=40, scale=2, shave=4, params=64, result=64, ws=64, ws_bytes=BIG):
    return _net(S, net), rgba, W, H, scale, shave, params, result, ws, ws_bytes, None


# ---- single faults: entry -> {fault: keywords} ----
SCALE = {"scale_0": dict(scale=0), "scale_5": dict(scale=5)}
RGBA = merged(SCALE, {
    "w0": dict(w=0), "h0": dict(h=0), "null_source": dict(rgba=None),
    "plane_floats": dict(w=30000, h=30000), "rgb_bytes": dict(w=15000, h=15000, scale=2),
    "padded_width": dict(w=0x20000000, h=1, scale=4)})
SAMPLES = {"7_bits": dict(bits=7), "17_bits": dict(bits=17), "msb_2": dict(msb=2), "msb_at_8_bits": dict(bits=8, msb=1)}
YUV_LUMA = {"w0": dict(w=0), "h0": dict(h=0), "short_pitch": dict(pitch=7), "range": dict(range=2),
            "null_y": dict(y=None), "null_plane": dict(out=None), "plane_floats": dict(w=30000, h=30000),
            "samples": dict(w=65536, h=32768, pitch=1 << 20)}
DEEP_LUMA = merged(SAMPLES, {"pitch_in_samples": dict(pitch=8), "odd_pitch": dict(pitch=17),
                             "odd_address": dict(y=65)})
COMPOSE = {"W0": dict(W=0), "H0": dict(H=0), "short_pitch": dict(pitch=15), "range": dict(range=-1),
           "null_luma": dict(luma=None), "null_y": dict(y=None), "samples": dict(W=65536, H=32768)}
PLANES = {"pw0": dict(pw=0), "oh0": dict(oh=0), "src_pitch": dict(sp=7), "dst_pitch": dict(dp=11),
          "null_src0": dict(src0=None), "null_dst0": dict(dst0=None), "null_src1": dict(src1=None),
          "null_dst1": dict(dst1=None), "samples": dict(pw=65536, ph=32768, ow=65536, oh=32768)}
DEEP_PLANES = merged(SAMPLES, {
    "layout_2": dict(layout=2), "odd_pitch": dict(sp=17), "pitch_in_samples": dict(dp=16),
    "semi_pitch_of_a_planar_row": dict(layout=1, src1=None, dst1=None, sp=16),
    "odd_src0": dict(src0=65), "odd_src1": dict(src1=65), "odd_dst0": dict(dst0=65), "odd_dst1": dict(dst1=65),
    "second_plane_when_semi": dict(layout=1, src1=None), "no_second_plane": dict(dst1=None)})
CROP = merged(SCALE, {"ow_above": dict(ow=17), "ow_loses_a_tile": dict(ow=14), "oh_above": dict(oh=17),
                      "oh_loses_a_tile": dict(oh=14)})
NET = {"null_net": dict(net="null"), "even_filter": dict(net="even"), "padding_overflows": dict(net="overflow"),
       "null_params": dict(params=None), "null_ws": dict(ws=None)}
IMAGE = merged(NET, {"w0": dict(w=0), "h0": dict(h=0), "null_rgba": dict(rgba=None), "null_rgb": dict(rgb=None)})
FRAME = merged(NET, {
    "w0": dict(w=0), "h0": dict(h=0), "null_src": dict(null_src=True), "null_dst": dict(null_dst=True),
    "null_source_y": dict(src=dict(y=None)), "null_source_u": dict(src=dict(u=None)),
    "null_output_y": dict(dst=dict(y=None)), "null_output_u": dict(dst=dict(u=None)),
    "no_source_v": dict(src=dict(v=None)), "no_output_v": dict(dst=dict(v=None)),
    "source_y_pitch": dict(src=dict(pitch_y=36)), "source_c_pitch": dict(src=dict(pitch_c=18)),
    "samples": dict(w=65536, h=65536)})
WORDS, SEMI = dict(bits=10), dict(layout=1)
FORMAT = {"null_fmt": dict(fmt=None), "subsampling_1x2": dict(fmt=dict(cx=1, cy=2)),
          "subsampling_0x0": dict(fmt=dict(cx=0, cy=0)), "range": dict(fmt=dict(range=2)),
          "7_bits": dict(fmt=dict(bits=7)), "17_bits": dict(fmt=dict(bits=17)), "msb_2": dict(fmt=dict(bits=10, msb=2)),
          "msb_at_8_bits": dict(fmt=dict(msb=1)), "layout_2": dict(fmt=dict(layout=2)),
          "v_in_a_semi_planar_source": dict(fmt=SEMI, src=dict(v=64)),
          "v_in_a_semi_planar_output": dict(fmt=dict(bits=10, msb=1, layout=1), dst=dict(v=64)),
          "odd_source_y": dict(fmt=WORDS, src=dict(y=65)), "odd_source_u": dict(fmt=WORDS, src=dict(u=65)),
          "odd_source_v": dict(fmt=WORDS, src=dict(v=65)), "odd_output_y": dict(fmt=dict(bits=16), dst=dict(y=65)),
          "odd_output_u": dict(fmt=dict(bits=10, msb=1, layout=1), dst=dict(u=65)),
          "odd_output_v": dict(fmt=WORDS, dst=dict(v=65)),
          "odd_pitch_of_words": dict(fmt=WORDS, src=dict(pitch_c=39)),
          "pitch_in_samples": dict(fmt=WORDS, src=dict(pitch_y=37)),
          "semi_pitch_of_a_planar_row": dict(fmt=SEMI, src=dict(pitch_c=19))}
TO = {"W0": dict(W=0), "H0": dict(H=0), "W_below_w": dict(W=7), "W_above_4w": dict(W=33), "H_below_h": dict(H=7),
      "H_above_4h": dict(H=33)}
FRAME_TO = {"W0": dict(W=0), "H0": dict(H=0), "W_below_w": dict(W=36), "W_above_4w": dict(W=149),
            "H_below_h": dict(H=22), "H_above_4h": dict(H=93), "output_y_pitch": dict(dst=dict(pitch_y=54)),
            "output_c_pitch": dict(dst=dict(pitch_c=27)), "samples": dict(w=65536, h=65536, W=65536, H=65536),
            "plane_floats": dict(w=30000, h=30000, W=60000, H=60000)}
FRAME_SCALE = merged(SCALE, {"output_y_pitch": dict(dst=dict(pitch_y=73)),
                             "output_c_pitch": dict(dst=dict(pitch_c=36)), "plane_floats": dict(w=30000, h=30000)})

SINGLE = {
    upscale_luma: merged(RGBA, {"null_plane": dict(out=None)}),
    upscale_compose: merged(RGBA, {"null_luma": dict(luma=None), "null_rgb": dict(rgb=None)}),
    yuv_upscale_luma: merged(SCALE, YUV_LUMA),
    yuv_upscale_luma16: merged(merged(SCALE, YUV_LUMA), DEEP_LUMA),
    yuv_compose_luma: COMPOSE,
    yuv_compose_luma16: merged(merged(COMPOSE, DEEP_LUMA), {"short_pitch": dict(pitch=30), "odd_pitch": dict(pitch=33),
                                                            "pitch_in_samples": dict(pitch=16)}),
    upscale_planes_u8: merged(PLANES, CROP),
    upscale_planes: merged(merged(PLANES, CROP), DEEP_PLANES),
    resize_luma: merged(TO, {"w0": dict(w=0), "null_source": dict(rgba=None), "null_plane": dict(out=None),
                             "plane_floats": dict(w=30000, h=30000, W=100000, H=100000),
                             "rgb_bytes": dict(w=20000, h=20000, W=30000, H=30000)}),
    resize_compose: merged(TO, {"h0": dict(h=0), "null_luma": dict(luma=None), "null_rgb": dict(rgb=None),
                                "rgb_bytes": dict(w=20000, h=20000, W=30000, H=30000)}),
    yuv_resize_luma: merged(merged(merged(TO, YUV_LUMA), DEEP_LUMA), {
        "plane_floats": dict(w=30000, h=30000, W=60000, H=60000),
        "samples": dict(w=65536, h=32768, W=65536, H=32768, pitch=1 << 20)}),
    resize_planes: merged(merged(PLANES, DEEP_PLANES), {
        "zero_numerator": dict(rx=(0, 3)), "ratio_below_1": dict(ow=8, rx=(3, 2)), "ratio_above_4": dict(ry=(2, 9)),
        "ow_beyond_its_bound": dict(ow=13), "oh_beyond_its_bound": dict(oh=13),
        "map_overflows": dict(pw=1 << 30, ph=1, ow=1 << 30, oh=1, rx=(0xffffffff, 0xffffffff), ry=(1, 1), bits=8),
        "samples": dict(pw=65536, ph=32768, ow=65536, oh=32768, rx=(1, 1), ry=(1, 1))}),
    upscale: merged(merged(IMAGE, SCALE), {"plane_floats": dict(w=30000, h=30000),
                                           "rgb_bytes": dict(w=15000, h=15000, scale=2)}),
    upscale_to: merged(merged(IMAGE, TO), {"plane_floats": dict(w=30000, h=30000, W=100000, H=100000),
                                           "rgb_bytes": dict(w=20000, h=20000, W=27000, H=27000)}),
    upscale_yuv: merged(merged(FRAME, FRAME_SCALE), {
        "subsampling_1x2": dict(cx=1, cy=2), "subsampling_0x0": dict(cx=0, cy=0), "range": dict(range=2)}),
    upscale_frame: merged(merged(FRAME, FRAME_SCALE), FORMAT),
    upscale_frame_to: merged(merged(FRAME, FRAME_TO), FORMAT),
    evaluate: merged(merged(NET, SCALE), {
        "smaller_than_the_scale": dict(W=1, H=1), "pixels": dict(W=65536, H=32768),
        "no_window": dict(W=30, H=30, shave=10), "null_rgba": dict(rgba=None), "null_result": dict(result=None),
        "rgba_alignment": dict(rgba=66), "result_alignment": dict(result=68), "ws_alignment": dict(ws=68)}),
}

# ---- double faults: one from each pair of adjacent checks, in the order the
# call makes them (and a few further apart) ----
IMAGE_PAIRS = [("null_net", "w0"), ("null_net", "null_params"), ("padding_overflows", "w0"), ("w0", "null_rgba"),
               ("plane_floats", "null_rgb"), ("rgb_bytes", "null_ws"), ("null_params", "even_filter"),
               ("null_rgba", "even_filter"), ("w0", "even_filter"), ("h0", "null_ws")]
FRAME_PAIRS = [("null_net", "w0"), ("padding_overflows", "w0"), ("w0", "null_params"), ("samples", "null_ws"),
               ("plane_floats", "null_src"), ("null_params", "null_source_y"), ("null_dst", "null_source_u"),
               ("null_output_u", "no_source_v"), ("no_output_v", "source_y_pitch"),
               ("source_y_pitch", "output_y_pitch"), ("output_y_pitch", "source_c_pitch"),
               ("source_c_pitch", "output_c_pitch"), ("output_c_pitch", "even_filter"), ("null_ws", "even_filter")]
FORMAT_PAIRS = [("null_fmt", "null_net"), ("null_net", "subsampling_1x2"), ("padding_overflows", "subsampling_0x0"),
                ("subsampling_1x2", "w0"), ("w0", "range"), ("samples", "range"), ("range", "17_bits"),
                ("range", "msb_at_8_bits"), ("msb_2", "null_params"), ("7_bits", "null_src"),
                ("layout_2", "null_ws"), ("layout_2", "null_source_y"), ("null_output_y", "odd_source_u"),
                ("odd_output_v", "source_y_pitch"), ("odd_pitch_of_words", "even_filter"),
                ("pitch_in_samples", "output_c_pitch")]
DOUBLE = {
    upscale: IMAGE_PAIRS + [("null_net", "scale_5"), ("padding_overflows", "scale_0"), ("scale_5", "w0"),
                            ("scale_0", "plane_floats"), ("scale_5", "null_rgba"), ("scale_0", "even_filter")],
    upscale_to: IMAGE_PAIRS + [("null_net", "W0"), ("padding_overflows", "W_below_w"), ("w0", "W_above_4w"),
                               ("H0", "H_below_h"), ("H_above_4h", "null_rgba"), ("W_below_w", "even_filter")],
    upscale_yuv: FRAME_PAIRS + [("null_net", "subsampling_1x2"), ("padding_overflows", "subsampling_0x0"),
                                ("subsampling_1x2", "scale_5"), ("scale_0", "w0"), ("scale_5", "range"),
                                ("w0", "range"), ("plane_floats", "range"), ("range", "null_params"),
                                ("range", "null_source_y")],
    upscale_frame: FRAME_PAIRS + FORMAT_PAIRS + [("subsampling_1x2", "scale_5"), ("scale_0", "w0"),
                                                 ("scale_5", "range"), ("scale_0", "layout_2")],
    upscale_frame_to: FRAME_PAIRS + FORMAT_PAIRS + [("subsampling_1x2", "W0"), ("W0", "W_below_w"),
                                                    ("H_above_4h", "range"), ("W_below_w", "layout_2"),
                                                    ("plane_floats", "17_bits")],
    evaluate: [("null_net", "scale_5"), ("scale_0", "smaller_than_the_scale"), ("smaller_than_the_scale", "pixels"),
               ("scale_5", "even_filter"), ("even_filter", "no_window"), ("padding_overflows", "no_window"),
               ("no_window", "null_rgba"), ("null_result", "rgba_alignment"), ("null_params", "ws_alignment"),
               ("result_alignment", "even_filter")],
    # the op level: what two entry points share a check for, against its neighbours
    yuv_upscale_luma16: [("17_bits", "scale_5"), ("scale_0", "w0"), ("short_pitch", "plane_floats"),
                         ("w0", "range"), ("range", "null_y"), ("null_plane", "odd_address")],
    yuv_resize_luma: [("17_bits", "W0"), ("w0", "W_below_w"), ("plane_floats", "short_pitch"), ("W_above_4w", "range"),
                      ("odd_pitch", "range"), ("range", "null_y"), ("null_plane", "odd_address")],
    upscale_planes: [("7_bits", "layout_2"), ("layout_2", "scale_5"), ("scale_0", "pw0"), ("src_pitch", "dst_pitch"),
                     ("dst_pitch", "ow_above"), ("oh_loses_a_tile", "null_src0"), ("null_dst0", "no_second_plane"),
                     ("null_src1", "odd_dst0"), ("second_plane_when_semi", "odd_src0")],
    resize_planes: [("7_bits", "layout_2"), ("layout_2", "pw0"), ("src_pitch", "dst_pitch"),
                    ("dst_pitch", "zero_numerator"), ("ratio_below_1", "ratio_above_4"),
                    ("oh_beyond_its_bound", "null_src0"), ("null_dst0", "no_second_plane"), ("null_src1", "odd_dst0"),
                    ("second_plane_when_semi", "odd_src0")],
}

# ---- workspace queries and the calls they size ----
SIZES = [(1, 1), (8, 8), (37, 23), (30000, 30000)]
GRID_NETS = ["default", "example", "wide", "even"]
SCALE_QUERIES = {"upscale": upscale, "upscale_yuv": upscale_yuv, "evaluate": evaluate}
TO_QUERIES = {"upscale_to": upscale_to, "upscale_frame_to": upscale_frame_to}
INVALID_TO = [(0, 8, 12, 20), (8, 8, 0, 20), (8, 8, 7, 20), (8, 8, 33, 20), (8, 8, 12, 7), (8, 8, 12, 33),
              (30000, 30000, 100000, 100000)]


def outputs(w, h):
    return [(w, h), (2 * w, 2 * h), (4 * w, 4 * h), (-(-3 * w // 2), -(-7 * h // 5))]


def entries(S):
    """name -> thunk returning what the library answered"""
    L = S.lib()
    fn = lambda f: getattr(L, "srcnn_" + f.__name__)
    out = {}
    for f, cases in SINGLE.items():
        for what, kw in cases.items():
            out["%s/%s" % (f.__name__, what)] = (lambda f=f, kw=kw: fn(f)(*f(S, **kw)))
    for f, pairs in DOUBLE.items():
        for a, b in pairs:
            kw = merged(SINGLE[f][a], SINGLE[f][b])
            out["%s/%s+%s" % (f.__name__, a, b)] = (lambda f=f, kw=kw: fn(f)(*f(S, **kw)))
    query = lambda name: getattr(L, "srcnn_%s_workspace_bytes" % name)
    for net in GRID_NETS + ["overflow", "null"]:
        sizes = SIZES if net in GRID_NETS else SIZES[1:2]
        for name in SCALE_QUERIES:
            for w, h in sizes + [(0, 8), (8, 0)]:
                for s in (1, 2, 3, 4) if w and h else (2,):
                    out["%s_workspace_bytes/%s/%ux%u/x%u" % (name, net, w, h, s)] = (
                        lambda name=name, net=net, w=w, h=h, s=s: query(name)(_net(S, net), w, h, s))
            for s in (0, 5):
                out["%s_workspace_bytes/%s/8x8/x%u" % (name, net, s)] = (
                    lambda name=name, net=net, s=s: query(name)(_net(S, net), 8, 8, s))
        for name in TO_QUERIES:
            shapes = [(w, h, W, H) for w, h in sizes for W, H in outputs(w, h)] + INVALID_TO
            for w, h, W, H in shapes:
                out["%s_workspace_bytes/%s/%ux%u/%ux%u" % (name, net, w, h, W, H)] = (
                    lambda name=name, net=net, w=w, h=h, W=W, H=H: query(name)(_net(S, net), w, h, W, H))
    # a workspace one byte short of the query's, and none at all
    for net in ("default", "wide"):
        n = _net(S, net)
        for name, f in list(SCALE_QUERIES.items()) + [("upscale_yuv", upscale_frame)]:
            kw = dict(W=48, H=40) if f is evaluate else dict(w=37, h=23)
            need = query(name)(n, kw.get("W", 37), kw.get("H", 23), 2)
            for short in (need - 1, 0):
                out["%s/%s/workspace_%s" % (f.__name__, net, "one_byte_short" if short else "of_0_bytes")] = (
                    lambda f=f, kw=kw, net=net, short=short: fn(f)(*f(S, net=net, scale=2, ws_bytes=short, **kw)))
        for name, f in TO_QUERIES.items():
            need = query(name)(n, 37, 23, 55, 35)
            out["%s/%s/workspace_one_byte_short" % (name, net)] = (
                lambda f=f, net=net, need=need: fn(f)(*f(S, net=net, w=37, h=23, W=55, H=35, ws_bytes=need - 1)))
    return out


SENTINEL = "srcnn_fill_f32: null pointer"


def answers(S):
    L = S.lib()
    got = {}
    for name, thunk in entries(S).items():
        assert L.srcnn_fill_f32(None, 0.0, 1, None) == S.ERR_INVALID and S.last_error() == SENTINEL
        got[name] = [thunk(), S.last_error()]
    return got


@pytest.fixture(scope="module")
def S():
    import srcnn_amd
    return srcnn_amd


@pytest.fixture(scope="module")
def got(S):
    return answers(S)


def test_the_golden_file_covers_the_table(got):
    with open(GOLDEN) as f:
        want = json.load(f)
    assert sorted(want) == sorted(got)


def test_every_call_of_the_table_fails_before_a_launch(S, got):
    """ERR_INVALID or ERR_WORKSPACE: a call that got past its checks would
    launch.  A query answers a whole number of 256-byte units."""
    for name, (rc, msg) in got.items():
        if "_workspace_bytes/" in name:
            assert rc % 256 == 0, name
        else:
            assert rc in (S.ERR_INVALID, S.ERR_WORKSPACE), (name, rc, msg)


def test_answers_are_the_recorded_ones(got):
    with open(GOLDEN) as f:
        want = json.load(f)
    wrong = {k: (got[k], want[k]) for k in want if got.get(k) != want[k]}
    for k, (g, w) in sorted(wrong.items()):
        print("%s:\n  got  %r\n  want %r" % (k, g, w))
    assert not wrong, "%d of %d entries differ" % (len(wrong), len(want))


if __name__ == "__main__":
    if sys.argv[1:] != ["record"]:
        sys.exit(__doc__)
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "cnn-super-resolution_amd"))
    import srcnn_amd
    table = answers(srcnn_amd)
    with open(GOLDEN, "w") as f:
        json.dump(table, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d entries -> %s" % (len(table), GOLDEN))
