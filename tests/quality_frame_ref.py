"""The yardstick of srcnn_quality_frame: DESIGN.md 17.1 in numpy.

A frame is three arrays of integer code values, Y [h][w] and U, V
[ceil(h/cy)][ceil(w/cx)], of `bits` bits.  quality_frame(A, B, bits, cx, cy,
shave, dtype) returns the integer sums of squared differences and the eight
doubles {mse_y, psnr_y, ssim_y, mse_u, psnr_u, mse_v, psnr_v, psnr_all}.  The
mse values come from integer sums and are exact whatever dtype is; the SSIM is
quality_ref.ssim_map on x / k, k = 2^(bits-8).  dtype = float64 is the
reference; float32, with a filter tap as a rounded product plus an add
(fused=False) or as one fma (fused=True), restates the spec in fp32, so that
|float32 - float64| measures what fp32 arithmetic costs on a given input.
tests/test_quality_frame_cpu.py derives the GPU test's bounds from both.

pack() lays a frame's values out as the C ABI takes them: planar or
semi-planar, one byte or a little-endian 16-bit word per sample with the code
in the low (msb 0) or high (msb 1) bits, rows at a pitch of its own with
garbage in between; unpack() reads them back.

cases() and flat_cases() list the inputs tests/test_quality_frame_gpu.py runs,
so that the CPU test measures the bounds on exactly those.
"""
import math

import numpy as np

import quality_ref as Q

YUV_PLANAR, YUV_SEMIPLANAR = 0, 1
SUBSAMPLINGS = {"420": (2, 2), "422": (2, 1), "444": (1, 1)}
BITS = [8, 10, 12, 16]
SHAVE = Q.SHAVE  # every case carries a shaved ring of 3 luma pixels


def ceil_div(a, b):
    return -(-a // b)


def chroma_shape(w, h, cx, cy):
    return ceil_div(h, cy), ceil_div(w, cx)


def windows(A, cx, cy, shave):
    """The shaved windows of a frame's three planes: `shave` luma pixels per
    side, ceil(shave/cx) columns and ceil(shave/cy) rows of chroma."""
    Y, U, V = A
    sx, sy = ceil_div(shave, cx), ceil_div(shave, cy)
    h, w = Y.shape
    ch, cw = U.shape
    cut = lambda p, r, c, ph, pw: p[r:ph - r, c:pw - c]
    return cut(Y, shave, shave, h, w), cut(U, sy, sx, ch, cw), cut(V, sy, sx, ch, cw)


def sq_sums(A, B, cx, cy, shave):
    """[(S, N)] of the three planes: the sum of the integer (xa - xb)^2 over
    the shaved window, as a Python integer, and the window's sample count."""
    out = []
    for pa, pb in zip(windows(A, cx, cy, shave), windows(B, cx, cy, shave)):
        d = pa.astype(np.int64) - pb.astype(np.int64)
        out.append((int((d * d).sum(dtype=np.uint64)), d.size))
    return out


def psnr(peak, mse):
    return float("inf") if mse == 0 else 10.0 * math.log10(peak * peak / mse)


def luma8(Y, bits, dtype=np.float64, reading="k"):
    """The SSIM's input on the 0 - 256 scale: x / k (exact in fp32).  The wrong
    readings the CPU test tells apart: "2k", a shift off by one; "peak",
    x * 255 / (2^bits - 1)."""
    k = 2 ** (bits - 8)
    dt = np.dtype(dtype).type
    x = Y.astype(dtype)
    if reading == "k":
        return x * dt(1.0 / k)
    if reading == "2k":
        return x * dt(0.5 / k)
    assert reading == "peak"
    return (x * dt(255.0)) / dt(2 ** bits - 1)


def ssim(Ya, Yb, bits, shave=0, dtype=np.float64, sigma=1.5, fused=False, reading="k"):
    if shave:
        Ya, Yb = Ya[shave:-shave, shave:-shave], Yb[shave:-shave, shave:-shave]
    m = Q.ssim_map(luma8(Ya, bits, dtype, reading), luma8(Yb, bits, dtype, reading), dtype, sigma, fused)
    return float(m.astype(np.float64).mean())


def quality_frame(A, B, bits, cx, cy, shave=0, dtype=np.float64, sigma=1.5, fused=False, reading="k"):
    """(sums, result): sums = [(S_y, N_y), (S_u, N_u), (S_v, N_v)], result =
    the eight doubles as Python floats."""
    sums = sq_sums(A, B, cx, cy, shave)
    peak = float(2 ** bits - 1)
    mse = [float(S) / float(N) for S, N in sums]
    (Sy, Ny), (Su, Nu), (Sv, Nv) = sums
    mse_all = ((float(Sy) + float(Su)) + float(Sv)) / float(Ny + Nu + Nv)
    s = ssim(A[0], B[0], bits, shave, dtype, sigma, fused, reading)
    return sums, [mse[0], psnr(peak, mse[0]), s, mse[1], psnr(peak, mse[1]), mse[2], psnr(peak, mse[2]),
                  psnr(peak, mse_all)]


def mse_all_of(sums):
    (Sy, Ny), (Su, Nu), (Sv, Nv) = sums
    return ((float(Sy) + float(Su)) + float(Sv)) / float(Ny + Nu + Nv)


# ---- packing ----
class Packed:
    """A frame as bytes: y, u, v uint8 arrays (v None when semi-planar: u then
    holds the (U, V) pairs), the pitches in bytes, and the format fields."""

    def __init__(self, y, u, v, pitch_y, pitch_c, bits, msb, layout, w, h, cx, cy):
        self.y, self.u, self.v = y, u, v
        self.pitch_y, self.pitch_c = pitch_y, pitch_c
        self.bits, self.msb, self.layout = bits, msb, layout
        self.w, self.h, self.cx, self.cy = w, h, cx, cy


def _plane_bytes(values, bits, msb, pitch, rng):
    """values [rows][n] of codes -> rows of `pitch` bytes, random bytes past each row's samples"""
    rows, n = values.shape
    if bits == 8:
        assert not msb
        body = values.astype(np.uint8)
    else:
        body = (values.astype(np.uint16) << ((16 - bits) if msb else 0)).astype("<u2").view(np.uint8)
    body = body.reshape(rows, -1)
    assert pitch >= body.shape[1]
    out = rng.integers(0, 256, (rows, pitch), dtype=np.uint8) if rng is not None else np.zeros((rows, pitch), np.uint8)
    out[:, :body.shape[1]] = body
    return out.ravel()


def pack(A, bits, msb=0, layout=YUV_PLANAR, cx=2, cy=2, extra_y=0, extra_c=0, rng=None):
    """extra_y / extra_c: samples (of the luma's size) added to the row bytes
    of the pitches; two-byte samples keep even pitches"""
    Y, U, V = A
    B = 1 if bits == 8 else 2
    h, w = Y.shape
    assert U.shape == V.shape == chroma_shape(w, h, cx, cy), (U.shape, V.shape, w, h, cx, cy)
    pitch_y = (w + extra_y) * B
    y = _plane_bytes(Y, bits, msb, pitch_y, rng)
    if layout == YUV_SEMIPLANAR:
        UV = np.stack([U, V], axis=-1).reshape(U.shape[0], -1)
        pitch_c = (UV.shape[1] + extra_c) * B
        return Packed(y, _plane_bytes(UV, bits, msb, pitch_c, rng), None, pitch_y, pitch_c, bits, msb, layout, w, h,
                      cx, cy)
    pitch_c = (U.shape[1] + extra_c) * B
    return Packed(y, _plane_bytes(U, bits, msb, pitch_c, rng), _plane_bytes(V, bits, msb, pitch_c, rng), pitch_y,
                  pitch_c, bits, msb, layout, w, h, cx, cy)


def _plane_values(buf, rows, n, bits, msb, pitch):
    body = buf.reshape(rows, pitch)
    if bits == 8:
        return body[:, :n].astype(np.int64)
    words = np.ascontiguousarray(body[:, :2 * n]).view("<u2").astype(np.int64)
    return words >> ((16 - bits) if msb else 0)


def unpack(p):
    """Packed -> (Y, U, V) code values (int64)"""
    ch, cw = chroma_shape(p.w, p.h, p.cx, p.cy)
    Y = _plane_values(p.y, p.h, p.w, p.bits, p.msb, p.pitch_y)
    if p.layout == YUV_SEMIPLANAR:
        UV = _plane_values(p.u, ch, 2 * cw, p.bits, p.msb, p.pitch_c).reshape(ch, cw, 2)
        return Y, UV[..., 0].copy(), UV[..., 1].copy()
    return (Y, _plane_values(p.u, ch, cw, p.bits, p.msb, p.pitch_c),
            _plane_values(p.v, ch, cw, p.bits, p.msb, p.pitch_c))


# ---- the GPU test's inputs ----
def make_frame(rng, w, h, cx, cy, bits, like=None, noise=0.0):
    """Three planes of codes: a smooth field x peak, rounded (or `like` plus
    Gaussian noise of `noise` code values), clipped to 0 .. peak"""
    peak = 2 ** bits - 1
    ch, cw = chroma_shape(w, h, cx, cy)
    out = []
    for i, (ph, pw) in enumerate(((h, w), (ch, cw), (ch, cw))):
        f = Q.smooth_field(rng, ph, pw) * peak if like is None else like[i].astype(np.float64)
        f = f + noise * rng.standard_normal(f.shape)
        out.append(np.clip(np.rint(f), 0, peak).astype(np.int64))
    return tuple(out)


def cases():
    """[(name, A, B, bits, cx, cy, shave)]: structured pairs (a smooth field,
    b = a + noise of 8 k code values) for every luma window of
    quality_ref.SHAPES (w = Ws + 2 SHAVE: 17, 49, 81 and 141 wide and 17, 19,
    49, 65 and 43 high are odd, so 4:2:0 and 4:2:2 meet ragged chroma) x bits x
    subsampling."""
    out = []
    for i, (ws, hs) in enumerate(Q.SHAPES):
        for j, bits in enumerate(BITS):
            for m, (sub, (cx, cy)) in enumerate(SUBSAMPLINGS.items()):
                rng = np.random.default_rng(17000 + 100 * i + 10 * j + m)
                w, h = ws + 2 * SHAVE, hs + 2 * SHAVE
                A = make_frame(rng, w, h, cx, cy, bits)
                B = make_frame(rng, w, h, cx, cy, bits, like=A, noise=8.0 * 2 ** (bits - 8))
                out.append(("%dx%d_%db_%s" % (ws, hs, bits, sub), A, B, bits, cx, cy, SHAVE))
    return out


def flat_cases():
    """A flat frame at code 250 k against the same plus a checker of k levels
    (quality_ref.flat_cases at every depth): the variance terms cancel."""
    out = []
    for (ws, hs), (sub, (cx, cy)) in zip(((Q.TILE + 11, Q.TILE + 11), (75, 59)), (("420", (2, 2)), ("444", (1, 1)))):
        for bits in BITS:
            k = 2 ** (bits - 8)
            w, h = ws + 2 * SHAVE, hs + 2 * SHAVE
            ch, cw = chroma_shape(w, h, cx, cy)
            A, B = [], []
            for ph, pw in ((h, w), (ch, cw), (ch, cw)):
                y, x = np.mgrid[0:ph, 0:pw]
                A.append(np.full((ph, pw), 250 * k, np.int64))
                B.append(250 * k + k * ((x + y) % 2))
            out.append(("flat250_%dx%d_%db_%s" % (ws, hs, bits, sub), tuple(A), tuple(B), bits, cx, cy, SHAVE))
    return out


def layouts_of(index, bits):
    """((msb_a, layout_a), (msb_b, layout_b)) of case `index`: the four
    (msb, layout) combinations in turn for a, another one for b (msb 0 only at
    8 bits)"""
    combos = [(0, YUV_PLANAR), (1, YUV_SEMIPLANAR), (0, YUV_SEMIPLANAR), (1, YUV_PLANAR)]
    pick = lambda i: (combos[i % 4][0] if bits > 8 else 0, combos[i % 4][1])
    return pick(index), pick(index + 1 + index // 4 % 3)


# ---- bounds of the GPU test (measured by tests/test_quality_frame_cpu.py on
# the inputs above: 4 x the largest error of the two float32 restatements
# against float64, rounded up to two digits; see its docstring) ----
SSIM_ATOL = 4.0e-6       # |ssim_y - float64|, cases(): 4 x 9.83e-7
SSIM_ATOL_FLAT = 1.7e-4  # the same on flat_cases(): 4 x 4.13e-5


# ---- invalid arguments (both tests: the checks run on the host before any launch) ----
def base_args(S, y=1 << 20, u=2 << 20, v=3 << 20, result=4 << 20, ws=5 << 20):
    """A valid call on a 23 x 23 10-bit planar 4:2:0 pair (tight pitches), as a
    dict the INVALID mutations change; the addresses are the caller's."""
    fmt = lambda: dict(bits=10, msb=0, layout=YUV_PLANAR, cx=2, cy=2, yuv_range=S.YUV_LIMITED)
    frame = lambda off: dict(y=y + off, u=u + off, v=v + off, pitch_y=46, pitch_c=24)
    return dict(fa=fmt(), a=frame(0), fb=fmt(), b=frame(1 << 16), w=23, h=23, shave=3, result=result, ws=ws,
                ws_bytes=S.quality_frame_workspace_bytes(23, 23, 2, 2, 3))


def call(S, args):
    g = args
    fmt = lambda f: None if f is None else S.yuv_format(**f)
    frame = lambda f: None if f is None else S.yuv_frame(f["y"], f["u"], f["v"], f["pitch_y"], f["pitch_c"])
    S.quality_frame(fmt(g["fa"]), frame(g["a"]), fmt(g["fb"]), frame(g["b"]), g["w"], g["h"], g["shave"],
                    g["result"], g["ws"], g["ws_bytes"])


def _both(key, **kw):
    def f(g):
        g[key[0]].update(kw)
        g[key[1]].update(kw)
    return f


def _one(key, **kw):
    return lambda g: g[key].update(kw)


def _semi(g):
    """both frames semi-planar (valid: v None, the pitch of the pairs)"""
    for f, fr in (("fa", "a"), ("fb", "b")):
        g[f]["layout"] = YUV_SEMIPLANAR
        g[fr].update(v=None, pitch_c=48)


def _then(*fs):
    def f(g):
        for x in fs:
            x(g)
    return f


# id -> mutation of base_args(); each must give SRCNN_ERR_INVALID.  (An empty
# chroma window cannot be reached with a valid subsampling: Ws >= 11 leaves at
# least 5 chroma columns.)
INVALID = {
    "null_fmt_a": lambda g: g.update(fa=None),
    "null_fmt_b": lambda g: g.update(fb=None),
    "null_frame_a": lambda g: g.update(a=None),
    "null_frame_b": lambda g: g.update(b=None),
    "null_result": lambda g: g.update(result=None),
    "null_ws": lambda g: g.update(ws=None),
    "bits_7": _both(("fa", "fb"), bits=7),
    "bits_17": _both(("fa", "fb"), bits=17),
    "msb_2": _one("fb", msb=2),
    "msb_at_8_bits": _then(_both(("fa", "fb"), bits=8), _one("fa", msb=1)),
    "layout_2": _one("fa", layout=2),
    "subsampling_3x1": _both(("fa", "fb"), cx=3, cy=1),
    "subsampling_1x2": _both(("fa", "fb"), cx=1, cy=2),
    "range_2": _both(("fa", "fb"), yuv_range=2),
    "null_y": _one("a", y=None),
    "null_u": _one("b", u=None),
    "null_v_planar": _one("b", v=None),
    "v_of_semiplanar": _then(_semi, lambda g: g["a"].update(v=g["a"]["u"] + 4096)),
    "odd_address_y": lambda g: g["a"].update(y=g["a"]["y"] + 1),
    "odd_address_v": lambda g: g["b"].update(v=g["b"]["v"] + 1),
    "odd_pitch_y": _one("a", pitch_y=47),
    "odd_pitch_c": _one("b", pitch_c=25),
    "pitch_y_below_row": _one("b", pitch_y=44),
    "pitch_c_below_row": _one("a", pitch_c=22),
    "pitch_c_below_pairs": _then(_semi, _one("b", pitch_c=46)),
    "bits_differ": _one("fb", bits=12),
    "cx_differs": _one("fb", cx=1, cy=1),
    "cy_differs": _one("fb", cy=1),
    "range_differs": _one("fb", yuv_range=1),
    "Ws_10": lambda g: g.update(w=16),
    "Hs_10": lambda g: g.update(h=16),
    "shave_wraps": lambda g: g.update(shave=0x80000003),
    "result_misaligned": lambda g: g.update(result=g["result"] + 4),
    "ws_misaligned": lambda g: g.update(ws=g["ws"] + 4),
    "plane_over_2^31": _then(lambda g: g.update(w=46341, h=46341, shave=0),
                             _both(("a", "b"), pitch_y=92682, pitch_c=46342)),
}
