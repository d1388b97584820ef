"""Frames of 8 to 16 bits per sample, planar and semi-planar, on the GPU
(csrc/hip/yuv.hip): srcnn_yuv_upscale_luma16,
srcnn_upscale_planes, srcnn_yuv_compose_luma16 and the network-level
srcnn_upscale_frame against the float64 restatement of the spec
(tests/yuv_deep_ref.py), against their own composition and the 8-bit calls,
under the memory contract of include/srcnn.h, and through `cnn upscale` on a
C420p10 Y4M file.

Every plane is used once with a tight pitch and once with pitch = (width + 3)
samples, which alternates the rows' 4-byte alignment; the gap bytes hold 0x5A
before the call and must hold it afterwards."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import hip_util
import yuv_deep_ref as D
from conftest import ROOT
from hip_util import H, guarded, guards_intact, make_params
from step_util import S, _settings  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CNN = os.path.join(ROOT, "cnn-super-resolution_amd", "bin", "cnn")
NET = (64, 32, 9, 1, 5)
# the tile-spanning shapes of tests/test_yuv_gpu.py (struct Tile, bicubic.hpp)
SHAPES = [(1, 1), (2, 3), (5, 4), (17, 9), (37, 23), (135, 37)]
# a wavefront of yuv_compose_luma takes 512 two-byte pixels per pass: 1100 x 3
# makes it go round three times
COMPOSE_SHAPES = SHAPES + [(1100, 3)]
SCALES = [1, 2, 3, 4]
PADS = [0, 7, 12]
RANGES = [D.FULL, D.LIMITED]
GAP = 0x5A
# (bits, msb): value in the low bits, in the high bits, and the whole word
LUMA_FORMATS = [(10, 0), (10, 1), (16, 0)]
CHROMA_FORMATS = [(10, 0), (10, 1), (12, 0), (16, 1)]
COMPOSE_FORMATS = [(10, 0), (10, 1), (12, 1), (16, 0)]
PLANES_SEED = 3
# exempt share of a case (tests/test_yuv_deep_cpu.py repeats the counts on the
# reference alone): chroma band 2e-3 * 2^(bits-8), compose band 1e-4 * 2^(bits-8)
PLANES_EXEMPT = {10: 0.025, 12: 0.10}
COMPOSE_EXEMPT = {10: 0.0025, 12: 0.005, 16: 0.07}
COMPOSE_SEEDS = {10: 0, 12: 0, 16: 2}


def rng_code(S, r):
    return S.YUV_FULL if r == D.FULL else S.YUV_LIMITED


def nbytes_of(bits):
    return 1 if bits == 8 else 2


def pitches(n, bits):
    """the two pitches in bytes of a row of n samples"""
    return (n * nbytes_of(bits), (n + 3) * nbytes_of(bits))


def pitched_np(a, pitch):
    """a [h][n] samples -> bytes [h][pitch], gaps GAP"""
    a = np.ascontiguousarray(a)
    b = np.full((a.shape[0], pitch), GAP, np.uint8)
    b[:, :a.shape[1] * a.itemsize] = a.view(np.uint8).reshape(a.shape[0], -1)
    return b


def to_pitched(a, pitch):
    return torch.from_numpy(pitched_np(a, pitch).ravel()).cuda()


def blank_pitched(h, pitch, fill=GAP):
    return torch.full((h * pitch,), fill, dtype=torch.uint8, device="cuda")


def unpitch(b, n, h, pitch, bits, what=""):
    """bytes [h * pitch] -> samples [h][n]; the gap bytes must still be GAP."""
    b = b.reshape(h, pitch)
    nb = n * nbytes_of(bits)
    assert (b[:, nb:] == GAP).all(), "%s: a pitch gap byte was written" % what
    return np.ascontiguousarray(b[:, :nb]).view(D.dtype(bits)).reshape(h, n).copy()


def from_pitched(t, n, h, pitch, bits, what=""):
    return unpitch(H(t), n, h, pitch, bits, what)


@functools.lru_cache(maxsize=None)
def y_of(w, h, bits):
    """sample values, not words"""
    a = np.random.default_rng(0).integers(0, 1 << bits, (h, w)).astype(D.dtype(bits))
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def planes_of(pw, ph, bits):
    a = np.random.default_rng(PLANES_SEED).integers(0, 1 << bits, (2, ph, pw)).astype(D.dtype(bits))
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def luma_of(W, Hh, seed):
    a = np.random.default_rng(seed).uniform(-0.1, 1.1, (Hh, W)).astype(np.float32)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def ref_plane(w, h, s, r, bits):
    """the reference's upscaled luma (no margin), shared by the pads and the word layouts"""
    a = D.luma_plane(y_of(w, h, bits), s, 0, bits, 0, r)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def ref_planes(pw, ph, s, ow, oh, bits):
    """(values, raw) of the reference, shared by the word layouts"""
    q, raw = D.planes(planes_of(pw, ph, bits), s, ow, oh, bits, 0)
    q.setflags(write=False)
    raw.setflags(write=False)
    return q, raw


def pad_plane(up, pad):
    Hh, W = up.shape
    m = pad // 2
    return up[np.ix_(np.clip(np.arange(Hh + pad) - m, 0, Hh - 1), np.clip(np.arange(W + pad) - m, 0, W - 1))]


def gpu_luma_plane(S, w, h, s, pad, r, bits, msb, pitch):
    src = to_pitched(D.encode(y_of(w, h, bits), bits, msb), pitch)
    out = torch.full(((s * h + pad) * (s * w + pad),), float("nan"), dtype=torch.float32, device="cuda")
    S.yuv_upscale_luma16(src, pitch, out, w, h, s, pad, bits, msb, rng_code(S, r))
    from_pitched(src, w, h, pitch, bits, "yuv_upscale_luma16 source")
    return H(out).reshape(s * h + pad, s * w + pad)


def gpu_planes(S, p, s, ow, oh, bits, msb, layout, tight):
    """p [2][ph][pw] words through srcnn_upscale_planes in `layout` -> [2][oh][ow] words"""
    ph, pw = p.shape[1:]
    k = 0 if tight else 1
    if layout == S.YUV_SEMIPLANAR:
        sp, dp = pitches(2 * pw, bits)[k], pitches(2 * ow, bits)[k]
        s0, d0 = to_pitched(D.interleave(p), sp), blank_pitched(oh, dp)
        S.upscale_planes(s0, None, sp, pw, ph, d0, None, dp, ow, oh, s, bits, msb, layout)
        return D.deinterleave(from_pitched(d0, 2 * ow, oh, dp, bits, "semi-planar dst"))
    sp, dp = pitches(pw, bits)[k], pitches(ow, bits)[k]
    s0, s1 = to_pitched(p[0], sp), to_pitched(p[1], sp)
    d0, d1 = blank_pitched(oh, dp), blank_pitched(oh, dp)
    S.upscale_planes(s0, s1, sp, pw, ph, d0, d1, dp, ow, oh, s, bits, msb, layout)
    return np.stack([from_pitched(d0, ow, oh, dp, bits, "planes dst0"), from_pitched(d1, ow, oh, dp, bits, "planes dst1")])


def gpu_compose(S, v, r, bits, msb, pitch):
    Hh, W = v.shape
    dst = blank_pitched(Hh, pitch)
    S.yuv_compose_luma16(torch.from_numpy(v.copy()).cuda(), dst, pitch, W, Hh, bits, msb, rng_code(S, r))
    return from_pitched(dst, W, Hh, pitch, bits, "yuv_compose_luma16")


# ---- 1: luma against the float64 reference ----
@pytest.mark.parametrize("bits,msb", LUMA_FORMATS)
@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("w,h", SHAPES)
def test_luma_vs_reference(S, w, h, s, bits, msb):
    """Full range: |error| <= 4e-6, limited range 4.5e-6: DESIGN.md 14's derived
    bounds (tests/test_yuv_gpu.py).  The samples are normalised before the
    resampling, so the values the fp32 chain works on are those of the 8-bit
    case (at most 1, or (2^bits - 1 - 16 k) / (219 k) < 1.092 with k =
    2^(bits-8)), whatever the depth."""
    for r in RANGES:
        bound = 4e-6 if r == D.FULL else 4.5e-6
        for pad in PADS:
            ref = pad_plane(ref_plane(w, h, s, r, bits), pad)
            for pitch in pitches(w, bits):
                got = gpu_luma_plane(S, w, h, s, pad, r, bits, msb, pitch)
                assert np.isfinite(got).all(), "plane pixels left unwritten"
                err = float(np.abs(got.astype(np.float64) - ref).max())
                print("yuv_upscale_luma16 %dx%d x%d pad %d %s %d bits msb %d pitch %d: max |err| %.3e"
                      % (w, h, s, pad, r, bits, msb, pitch, err))
                assert err <= bound, (r, pad, pitch, err)


# ---- 2: scale 1, full range: Y / (2^bits - 1) and replicate padding, bit for bit ----
@pytest.mark.parametrize("bits,msb", LUMA_FORMATS)
@pytest.mark.parametrize("w,h", SHAPES)
def test_luma_scale_1_anchor(S, w, h, bits, msb):
    ex = y_of(w, h, bits).astype(np.float32) / np.float32((1 << bits) - 1)
    for pad in PADS:
        m = pad // 2
        for pitch in pitches(w, bits):
            got = gpu_luma_plane(S, w, h, 1, pad, D.FULL, bits, msb, pitch)
            assert hip_util.same_bits(got[m:m + h, m:m + w], ex), "interior differs from float(Y) / (2^bits - 1)"
            assert hip_util.same_bits(got, pad_plane(ex, pad)), "a margin pixel differs from the pixel it replicates"


# ---- 3: chroma against the float64 reference, planar and interleaved ----
def check_planes(S, pw, ph, s, ow, oh, bits, msb):
    q, raw = ref_planes(pw, ph, s, ow, oh, bits)
    ref = D.encode(q, bits, msb)
    near = D.near_boundary(raw, 2e-3 * 2 ** (bits - 8))
    if bits in PLANES_EXEMPT:
        assert near.mean() <= PLANES_EXEMPT[bits], "too much of the case exempt: %d of %d" % (near.sum(), near.size)
    src = D.encode(planes_of(pw, ph, bits), bits, msb)
    for tight in (True, False):
        got = gpu_planes(S, src, s, ow, oh, bits, msb, S.YUV_PLANAR, tight)
        if msb:
            assert not (got & ((1 << (16 - bits)) - 1)).any(), "low bits of an msb word set"
        d = np.abs(D.decode(got, bits, msb) - q.astype(np.int64))
        print("upscale_planes %dx%d x%d -> %dx%d %d bits msb %d tight %d: %d of %d exempt, %d differ by 1, max diff %d"
              % (pw, ph, s, ow, oh, bits, msb, tight, near.sum(), near.size, (d == 1).sum(), d.max()))
        assert d.max() <= 1
        if bits < 16:  # at 16 bits the band exceeds 0.5: nothing can be shown exact
            assert np.array_equal(got[~near], ref[~near])
        semi = gpu_planes(S, src, s, ow, oh, bits, msb, S.YUV_SEMIPLANAR, tight)
        assert np.array_equal(semi, got), "the interleaved result differs from the planar one"


@pytest.mark.parametrize("bits,msb", CHROMA_FORMATS)
@pytest.mark.parametrize("s", [2, 3, 4])
@pytest.mark.parametrize("pw,ph", SHAPES)
def test_planes_vs_reference(S, pw, ph, s, bits, msb):
    """Within 1 everywhere; exactly equal wherever the reference's unrounded
    value is further than 2e-3 * 2^(bits-8) from a rounding boundary (k + 0.5):
    the fp32 chain's error, below 1e-3 on 8-bit values, grows with the values.
    At most 2.5 % (10 bits) / 10 % (12 bits) of a case may be exempt; at 16 bits
    the band exceeds 0.5 and only "within 1" is checked."""
    check_planes(S, pw, ph, s, s * pw, s * ph, bits, msb)


@pytest.mark.parametrize("bits,msb", CHROMA_FORMATS)
def test_planes_cropped_420(S, bits, msb):
    """37 x 23 luma at scale 2, 4:2:0: chroma 19 x 12 -> the top-left 37 x 23
    of its 38 x 24; in the interleaved plane the crop counts pairs."""
    check_planes(S, 19, 12, 2, 37, 23, bits, msb)


@pytest.mark.parametrize("bits,msb", CHROMA_FORMATS)
@pytest.mark.parametrize("pw,ph", SHAPES)
def test_planes_scale_1_is_the_source(S, pw, ph, bits, msb):
    src = D.encode(planes_of(pw, ph, bits), bits, msb)
    for tight in (True, False):
        for layout in (S.YUV_PLANAR, S.YUV_SEMIPLANAR):
            assert np.array_equal(gpu_planes(S, src, 1, pw, ph, bits, msb, layout, tight), src)


@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("pw,ph", SHAPES + [(19, 12)])
def test_8_bit_planes_are_upscale_planes_u8(S, pw, ph, s):
    """srcnn_upscale_planes at 8 bits, planar: srcnn_upscale_planes_u8 byte for
    byte; NV12: the same bytes, interleaved."""
    p = planes_of(pw, ph, 8)
    ow, oh = (37, 23) if (pw, ph, s) == (19, 12, 2) else (s * pw, s * ph)
    for tight in (True, False):
        sp, dp = pitches(pw, 8)[not tight], pitches(ow, 8)[not tight]
        s0, s1 = to_pitched(p[0], sp), to_pitched(p[1], sp)
        d0, d1 = blank_pitched(oh, dp), blank_pitched(oh, dp)
        S.upscale_planes_u8(s0, s1, sp, pw, ph, d0, d1, dp, ow, oh, s)
        want = np.stack([from_pitched(d0, ow, oh, dp, 8), from_pitched(d1, ow, oh, dp, 8)])
        assert np.array_equal(gpu_planes(S, p, s, ow, oh, 8, 0, S.YUV_PLANAR, tight), want)
        assert np.array_equal(gpu_planes(S, p, s, ow, oh, 8, 0, S.YUV_SEMIPLANAR, tight), want)


# ---- 4: compose against the float64 reference ----
@pytest.mark.parametrize("bits,msb", COMPOSE_FORMATS)
@pytest.mark.parametrize("W,Hh", COMPOSE_SHAPES)
def test_compose_vs_reference(S, W, Hh, bits, msb):
    """Within 1 everywhere, exact wherever the raw value is further than 1e-4 *
    2^(bits-8) from a rounding boundary (one fma rounding on values <= 1.1 *
    2^bits is 1.7e-5 * 2^(bits-8)).  At most 0.25 % / 0.5 % / 7 % of a case may
    be exempt at 10 / 12 / 16 bits.  The low bits of msb words are zero."""
    v = luma_of(W, Hh, COMPOSE_SEEDS[bits])
    for r in RANGES:
        ref, raw = D.compose_luma(v, bits, msb, r)
        near = D.near_boundary(raw, 1e-4 * 2 ** (bits - 8))
        assert near.mean() <= COMPOSE_EXEMPT[bits], (r, near.mean())
        for pitch in pitches(W, bits):
            got = gpu_compose(S, v, r, bits, msb, pitch)
            d = np.abs(D.decode(got, bits, msb) - D.decode(ref, bits, msb))
            print("yuv_compose_luma16 %dx%d %s %d bits msb %d pitch %d: %d exempt, max diff %d"
                  % (W, Hh, r, bits, msb, pitch, near.sum(), d.max()))
            assert d.max() <= 1
            assert np.array_equal(got[~near], ref[~near])
            if msb:
                assert not (got & ((1 << (16 - bits)) - 1)).any(), "low bits of an msb word set"


@pytest.mark.parametrize("W,Hh", COMPOSE_SHAPES)
def test_8_bit_16_calls_are_the_8_bit_calls(S, W, Hh):
    """bits = 8 through the ...16 calls: yuv_upscale_luma and yuv_compose_luma
    bit for bit."""
    v = luma_of(W, Hh, 0)
    y = y_of(W, Hh, 8)
    for r in RANGES:
        for pitch in pitches(W, 8):
            dst = blank_pitched(Hh, pitch)
            S.yuv_compose_luma(torch.from_numpy(v.copy()).cuda(), dst, pitch, W, Hh, rng_code(S, r))
            assert np.array_equal(gpu_compose(S, v, r, 8, 0, pitch), from_pitched(dst, W, Hh, pitch, 8))
            src = to_pitched(y, pitch)
            out = torch.full(((2 * Hh + 7) * (2 * W + 7),), float("nan"), dtype=torch.float32, device="cuda")
            S.yuv_upscale_luma(src, pitch, out, W, Hh, 2, 7, rng_code(S, r))
            assert hip_util.same_bits(gpu_luma_plane(S, W, Hh, 2, 7, r, 8, 0, pitch).ravel(), H(out))


# ---- 5: srcnn_upscale_frame is its op-level calls ----
FRAME_FORMATS = {"p10": (10, 0, 0), "P010": (10, 1, 1), "NV12": (8, 0, 1)}  # bits, msb, layout


def frame_arrays(w, h, cx, cy, bits, msb, layout):
    """[y, u, v] word arrays of a source frame (v None when semi-planar)"""
    cw, ch = D.chroma_size(w, h, cx, cy)
    y, uv = D.encode(y_of(w, h, bits), bits, msb), D.encode(planes_of(cw, ch, bits), bits, msb)
    return [y, D.interleave(uv), None] if layout else [y, uv[0], uv[1]]


def frame_dims(W, Hh, cx, cy, layout):
    """(samples per row, rows) of the planes of a W x Hh frame"""
    CW, CH = D.chroma_size(W, Hh, cx, cy)
    return [(W, Hh), (2 * CW, CH), None] if layout else [(W, Hh), (CW, CH), (CW, CH)]


def frame_pitches(dims, bits, tight):
    k = 0 if tight else 1
    return pitches(dims[0][0], bits)[k], pitches(dims[1][0], bits)[k]


def device_frame(S, arrays, py, pc):
    t = [None if a is None else to_pitched(a, p) for a, p in zip(arrays, (py, pc, pc))]
    return S.yuv_frame(t[0], t[1], t[2], py, pc), t


def blank_frame(S, dims, py, pc, fill=GAP):
    t = [None if d is None else blank_pitched(d[1], p, fill) for d, p in zip(dims, (py, pc, pc))]
    return S.yuv_frame(t[0], t[1], t[2], py, pc), t


def frame_planes_of(tensors, dims, py, pc, bits, what):
    return [None if d is None else from_pitched(t, d[0], d[1], p, bits, what)
            for t, d, p in zip(tensors, dims, (py, pc, pc))]


@pytest.mark.parametrize("fmt", sorted(FRAME_FORMATS))
@pytest.mark.parametrize("arith", [0, 1])
@pytest.mark.parametrize("cx,cy,s", [(2, 2, 2), (2, 1, 3), (1, 1, 1)])
def test_upscale_frame_is_its_calls(S, cx, cy, s, arith, fmt):
    bits, msb, layout = FRAME_FORMATS[fmt]
    net = S.Net(*NET)
    w, h = 37, 23
    W, Hh, pad = s * w, s * h, NET[2] + NET[3] + NET[4] - 3
    PW, PH = W + pad, Hh + pad
    cw, ch = D.chroma_size(w, h, cx, cy)
    CW, CH = D.chroma_size(W, Hh, cx, cy)
    S.set_arith(arith)
    params = torch.from_numpy(make_params(np.random.default_rng(11), NET, sd=0.05)).cuda()
    rc = S.YUV_LIMITED
    f = S.yuv_format(bits, msb, layout, cx, cy, rc)
    arrays = frame_arrays(w, h, cx, cy, bits, msb, layout)
    sdims, ddims = frame_dims(w, h, cx, cy, layout), frame_dims(W, Hh, cx, cy, layout)

    # what srcnn_upscale's forward runs on a plane of the same size
    rgba = torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda")
    nb_rgba = S.upscale_workspace_bytes(net, w, h, s)
    S.upscale(net, rgba, w, h, s, params, torch.empty(W * Hh * 3, dtype=torch.uint8, device="cuda"),
              torch.empty(nb_rgba, dtype=torch.uint8, device="cuda"), nb_rgba)
    family, kernels = S.last_path(), S.last_kernels()
    assert family == "fused", family

    for tight in (True, False):
        py, pc = frame_pitches(sdims, bits, tight)
        PY, PC = frame_pitches(ddims, bits, tight)
        src, keep_src = device_frame(S, arrays, py, pc)
        # the calls, on buffers of the test
        plane = torch.empty(PW * PH, dtype=torch.float32, device="cuda")
        out = torch.empty(W * Hh, dtype=torch.float32, device="cuda")
        rb = S.reduce_workspace_bytes(PW * PH)
        red = torch.empty(rb, dtype=torch.uint8, device="cuda")
        fb = S.forward_workspace_bytes(net, PW, PH, 1)
        fws = torch.empty(fb, dtype=torch.uint8, device="cuda")
        ops, keep_ops = blank_frame(S, ddims, PY, PC)
        S.yuv_upscale_luma16(src.y, py, plane, w, h, s, pad, bits, msb, rc)
        S.sub_mean(plane, PW * PH, None, red, rb)
        S.forward(net, plane, PW, PH, 1, params, out, fws, fb)
        assert (S.last_path(), S.last_kernels()) == (family, kernels)
        S.yuv_compose_luma16(out, ops.y, PY, W, Hh, bits, msb, rc)
        S.upscale_planes(src.u, src.v, pc, cw, ch, ops.u, ops.v, PC, CW, CH, s, bits, msb, layout)
        # the one call
        nbytes = S.upscale_yuv_workspace_bytes(net, w, h, s)
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        dst, keep_dst = blank_frame(S, ddims, PY, PC)
        S.upscale_frame(net, f, src, dst, w, h, s, params, ws, nbytes)
        assert (S.last_path(), S.last_kernels()) == (family, kernels)
        got = frame_planes_of(keep_dst, ddims, PY, PC, bits, "upscale_frame")
        want = frame_planes_of(keep_ops, ddims, PY, PC, bits, "ops")
        for a, b in zip(got, want):
            assert (a is None and b is None) or np.array_equal(a, b)
        assert len(np.unique(got[0])) > 8, "degenerate result"
        with pytest.raises(S.SrcnnError) as e:
            S.upscale_frame(net, f, src, dst, w, h, s, params, ws, nbytes - 1)
        assert e.value.code == S.ERR_WORKSPACE


@pytest.mark.parametrize("arith", [0, 1])
@pytest.mark.parametrize("cx,cy,s", [(2, 2, 2), (2, 1, 3), (1, 1, 1)])
def test_upscale_frame_8_bit_planar_is_upscale_yuv(S, cx, cy, s, arith):
    net = S.Net(*NET)
    w, h = 37, 23
    W, Hh = s * w, s * h
    S.set_arith(arith)
    params = torch.from_numpy(make_params(np.random.default_rng(11), NET, sd=0.05)).cuda()
    arrays = frame_arrays(w, h, cx, cy, 8, 0, 0)
    sdims, ddims = frame_dims(w, h, cx, cy, 0), frame_dims(W, Hh, cx, cy, 0)
    nbytes = S.upscale_yuv_workspace_bytes(net, w, h, s)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    for r in (S.YUV_LIMITED, S.YUV_FULL):
        for tight in (True, False):
            py, pc = frame_pitches(sdims, 8, tight)
            PY, PC = frame_pitches(ddims, 8, tight)
            src, keep_src = device_frame(S, arrays, py, pc)
            a, keep_a = blank_frame(S, ddims, PY, PC)
            b, keep_b = blank_frame(S, ddims, PY, PC)
            S.upscale_yuv(net, src, a, w, h, cx, cy, s, r, params, ws, nbytes)
            S.upscale_frame(net, S.yuv_format(8, 0, S.YUV_PLANAR, cx, cy, r), src, b, w, h, s, params, ws, nbytes)
            for x, y in zip(keep_a, keep_b):
                assert np.array_equal(H(x), H(y))


# ---- 6: the memory contract ----
def guarded_bytes(a, fill):
    """a: u8 array -> (guarded float32 view over its bytes, padded to whole
    floats with GAP; the number of bytes)."""
    b = np.asarray(a, np.uint8).ravel()
    n = b.size
    b = np.concatenate([b, np.full((-n) % 4, GAP, np.uint8)])
    return guarded(b.view(np.float32), fill), n


@pytest.mark.parametrize("fmt", ["P010", "p10"])
@pytest.mark.parametrize("w,h,s,cx,cy", [(1, 1, 1, 2, 2), (37, 23, 3, 2, 2)])
def test_upscale_frame_memory(S, w, h, s, cx, cy, fmt):
    """srcnn_upscale_frame on an exact-size workspace holding zeros, NaN and
    +1e30, guard bands of the same around every plane, params and ws, pitch =
    (width + 3) samples everywhere.  The output must not depend on the fill,
    the gaps and the spare bytes must keep GAP, and two more runs into planes
    of 0x00 and of 0xFF bytes must give the same samples (every one is
    written)."""
    bits, msb, layout = FRAME_FORMATS[fmt]
    net = S.Net(*NET)
    W, Hh = s * w, s * h
    arrays = frame_arrays(w, h, cx, cy, bits, msb, layout)
    sdims, ddims = frame_dims(w, h, cx, cy, layout), frame_dims(W, Hh, cx, cy, layout)
    py, pc = frame_pitches(sdims, bits, False)
    PY, PC = frame_pitches(ddims, bits, False)
    f = S.yuv_format(bits, msb, layout, cx, cy, S.YUV_FULL)
    params = make_params(np.random.default_rng(w * 100 + h), NET, sd=0.05)
    nbytes = S.upscale_yuv_workspace_bytes(net, w, h, s)
    assert nbytes % 4 == 0

    runs = []
    for fill in (0.0,) + hip_util.POISONS:
        srcs = [None if a is None else guarded_bytes(pitched_np(a, p), fill)[0] for a, p in zip(arrays, (py, pc, pc))]
        dsts = [None if d is None else guarded_bytes(np.full(d[1] * p, GAP, np.uint8), fill)
                for d, p in zip(ddims, (PY, PC, PC))]
        pd, ws = guarded(params, fill), guarded(nbytes // 4, fill)
        src = S.yuv_frame(srcs[0], srcs[1], srcs[2], py, pc)
        dst = S.yuv_frame(dsts[0][0], dsts[1][0], dsts[2][0] if dsts[2] else None, PY, PC)
        S.upscale_frame(net, f, src, dst, w, h, s, pd, ws, nbytes)
        assert S.last_path() == "fused"
        got = []
        for tn, d, p in zip(dsts, ddims, (PY, PC, PC)):
            if d is None:
                continue
            allb = H(tn[0].view(torch.uint8))
            assert (allb[tn[1]:] == GAP).all(), "spare bytes behind a plane written"
            got.append(unpitch(allb[:tn[1]], d[0], d[1], p, bits, "upscale_frame"))
        runs.append(got)
        guards_intact(*[t for t in srcs if t is not None], *[tn[0] for tn in dsts if tn], pd, ws)
        assert hip_util.same_bits(H(pd), params)
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert np.array_equal(a, b), "result depends on the workspace's previous contents"
    src, keep = device_frame(S, arrays, py, pc)
    pd = torch.from_numpy(params).cuda()
    for byte in (0x00, 0xFF):
        dst, planes = blank_frame(S, ddims, PY, PC, fill=byte)
        ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        S.upscale_frame(net, f, src, dst, w, h, s, pd, ws, nbytes)
        live = [(t, d, p) for t, d, p in zip(planes, ddims, (PY, PC, PC)) if d is not None]
        for (t, d, p), a in zip(live, runs[0]):
            b = H(t).reshape(d[1], p)[:, :d[0] * nbytes_of(bits)]
            assert np.array_equal(np.ascontiguousarray(b).view(D.dtype(bits)), a), "an output sample was left unwritten"
    with pytest.raises(S.SrcnnError) as e:
        S.upscale_frame(net, f, src, dst, w, h, s, pd, ws, nbytes - 1)
    assert e.value.code == S.ERR_WORKSPACE


# ---- 7: invalid arguments ----
def test_upscale_frame_rejects_invalid_arguments(S):
    """Every invalid argument gives SRCNN_ERR_INVALID with a message before any
    launch: the outputs keep their bytes."""
    net = S.Net(*NET)
    w, h, s, cx, cy = 37, 23, 2, 2, 2
    W, Hh = s * w, s * h
    cw, ch = D.chroma_size(w, h, cx, cy)
    CW, CH = D.chroma_size(W, Hh, cx, cy)
    params = torch.from_numpy(make_params(np.random.default_rng(1), NET, sd=0.05)).cuda()
    nbytes = S.upscale_yuv_workspace_bytes(net, w, h, s)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    alive, untouched = [], []

    def frames(bits, msb, layout, runs=False):
        sd, dd = frame_dims(w, h, cx, cy, layout), frame_dims(W, Hh, cx, cy, layout)
        py, pc = frame_pitches(sd, bits, True)
        PY, PC = frame_pitches(dd, bits, True)
        src, keep = device_frame(S, frame_arrays(w, h, cx, cy, bits, msb, layout), py, pc)
        dst, planes = blank_frame(S, dd, PY, PC)
        alive.extend(keep + planes)
        if not runs:  # only ever passed to invalid calls: must keep its bytes
            untouched.extend(planes)
        return src, dst

    def frame(f, **kw):
        d = dict(y=f.y, u=f.u, v=f.v, pitch_y=f.pitch_y, pitch_c=f.pitch_c)
        d.update(kw)
        return S.YuvFrame(d["y"], d["u"], d["v"], d["pitch_y"], d["pitch_c"])

    def fmt(bits=10, msb=0, layout=0, cx=cx, cy=cy, r=S.YUV_FULL):
        return S.yuv_format(bits, msb, layout, cx, cy, r)

    src, dst = frames(10, 0, 0)        # 10-bit planar
    ssrc, sdst = frames(10, 1, 1, runs=True)      # P010
    bsrc, bdst = frames(8, 0, 0)       # 8-bit planar
    nsrc, ndst = frames(8, 0, 1, runs=True)       # NV12
    good = dict(net=net, fmt=fmt(), src=src, dst=dst, w=w, h=h, scale=s, params=params, ws=ws, ws_bytes=nbytes)
    semi = dict(good, fmt=fmt(10, 1, 1), src=ssrc, dst=sdst)
    bad = {
        # what srcnn_upscale_yuv rejects
        "scale 0": dict(scale=0), "scale 5": dict(scale=5),
        "subsampling 3x1": dict(fmt=fmt(cx=3, cy=1)), "subsampling 1x2": dict(fmt=fmt(cx=1, cy=2)),
        "subsampling 0x0": dict(fmt=fmt(cx=0, cy=0)),
        "zero width": dict(w=0), "zero height": dict(h=0),
        "source y pitch": dict(src=frame(src, pitch_y=2 * w - 2)), "source c pitch": dict(src=frame(src, pitch_c=2 * cw - 2)),
        "output y pitch": dict(dst=frame(dst, pitch_y=2 * W - 2)), "output c pitch": dict(dst=frame(dst, pitch_c=2 * CW - 2)),
        "source y pitch in samples": dict(src=frame(src, pitch_y=w + 1)),
        "semi-planar c pitch of a planar row": dict(semi, src=frame(ssrc, pitch_c=2 * cw)),
        "semi-planar output c pitch": dict(semi, dst=frame(sdst, pitch_c=4 * CW - 2)),
        "NV12 c pitch": dict(good, fmt=fmt(8, 0, 1), src=frame(nsrc, pitch_c=2 * cw - 1), dst=ndst),
        "null source y": dict(src=frame(src, y=None)), "null source u": dict(src=frame(src, u=None)),
        "null output u": dict(dst=frame(dst, u=None)), "null params": dict(params=None), "null ws": dict(ws=None),
        "invalid net": dict(net=S.Net(64, 32, 9, 2, 5)), "range": dict(fmt=fmt(r=2)),
        "2^32 plane elements": dict(w=65536, h=65536, scale=1, src=frame(src, pitch_y=131072, pitch_c=65536),
                                    dst=frame(dst, pitch_y=131072, pitch_c=65536)),
        "2^31 semi-planar chroma samples": dict(semi, fmt=fmt(10, 1, 1, 1, 1), w=32768, h=32768, scale=1,
                                                src=frame(ssrc, pitch_y=65536, pitch_c=131072),
                                                dst=frame(sdst, pitch_y=65536, pitch_c=131072)),
        # the format
        "7 bits": dict(fmt=fmt(bits=7)), "17 bits": dict(fmt=fmt(bits=17)), "0 bits": dict(fmt=fmt(bits=0)),
        "msb 2": dict(fmt=fmt(msb=2)), "msb at 8 bits": dict(fmt=fmt(8, 1), src=bsrc, dst=bdst),
        "layout 2": dict(fmt=fmt(layout=2)),
        "odd source y address": dict(src=frame(src, y=src.y + 1)), "odd source u address": dict(src=frame(src, u=src.u + 1)),
        "odd source v address": dict(src=frame(src, v=src.v + 1)), "odd output y address": dict(dst=frame(dst, y=dst.y + 1)),
        "odd output v address": dict(dst=frame(dst, v=dst.v + 1)),
        "odd semi-planar u address": dict(semi, src=frame(ssrc, u=ssrc.u + 1)),
        "odd source y pitch": dict(src=frame(src, pitch_y=2 * w + 1)), "odd source c pitch": dict(src=frame(src, pitch_c=2 * cw + 1)),
        "odd output y pitch": dict(dst=frame(dst, pitch_y=2 * W + 1)), "odd output c pitch": dict(dst=frame(dst, pitch_c=2 * CW + 1)),
        "v in a semi-planar source": dict(semi, src=frame(ssrc, v=src.v)),
        "v in a semi-planar output": dict(semi, dst=frame(sdst, v=dst.v)),
        "no v in a planar source": dict(src=frame(src, v=None)), "no v in a planar output": dict(dst=frame(dst, v=None)),
        "null fmt": dict(fmt=None),
    }
    for what, kw in bad.items():
        a = dict(good)
        a.update(kw)
        with pytest.raises(S.SrcnnError) as e:
            S.upscale_frame(a["net"], a["fmt"], a["src"], a["dst"], a["w"], a["h"], a["scale"], a["params"], a["ws"],
                            a["ws_bytes"])
        assert e.value.code == S.ERR_INVALID, what
        assert S.last_error(), what
    # the valid ones do run (the cases above fail for the reason they name)
    S.upscale_frame(net, semi["fmt"], ssrc, sdst, w, h, s, params, ws, nbytes)
    S.upscale_frame(net, fmt(8, 0, 1), nsrc, ndst, w, h, s, params, ws, nbytes)
    for t in untouched:  # the outputs of the 10-bit planar and the 8-bit planar frames
        assert (H(t) == GAP).all(), "an invalid call wrote to its output"

    # the op-level calls reject their own
    op_bad = [
        lambda: S.yuv_upscale_luma16(src.y, 2 * w, ws, w, h, 2, 0, 17, 0, S.YUV_FULL),
        lambda: S.yuv_upscale_luma16(src.y, 2 * w, ws, w, h, 2, 0, 8, 1, S.YUV_FULL),
        lambda: S.yuv_upscale_luma16(src.y, 2 * w, ws, w, h, 2, 0, 10, 2, S.YUV_FULL),
        lambda: S.yuv_upscale_luma16(src.y, 2 * w, ws, w, h, 2, 0, 10, 0, 7),
        lambda: S.yuv_upscale_luma16(src.y + 1, 2 * w, ws, w, h, 2, 0, 10, 0, S.YUV_FULL),
        lambda: S.yuv_upscale_luma16(src.y, 2 * w + 1, ws, w, h, 2, 0, 10, 0, S.YUV_FULL),
        lambda: S.yuv_upscale_luma16(src.y, 2 * w - 2, ws, w, h, 2, 0, 10, 0, S.YUV_FULL),
        lambda: S.yuv_compose_luma16(ws, dst.y, 2 * W - 2, W, Hh, 10, 0, S.YUV_FULL),
        lambda: S.yuv_compose_luma16(ws, dst.y + 1, 2 * W, W, Hh, 10, 0, S.YUV_FULL),
        lambda: S.yuv_compose_luma16(ws, dst.y, 2 * W, W, Hh, 7, 0, S.YUV_FULL),
        lambda: S.upscale_planes(src.u, src.v, 2 * cw, cw, ch, dst.u, dst.v, 2 * CW, 2 * cw + 1, CH, 2, 10, 0, 0),  # wider than the x2
        lambda: S.upscale_planes(src.u, src.v, 2 * cw, cw, ch, dst.u, dst.v, 2 * CW, 2 * cw - 2, CH, 2, 10, 0, 0),  # drops a pair
        lambda: S.upscale_planes(src.u, src.v, 2 * cw, cw, ch, dst.u, dst.v, 2 * CW, CW, CH, 2, 10, 0, 2),
        lambda: S.upscale_planes(ssrc.u, src.v, 4 * cw, cw, ch, sdst.u, None, 4 * CW, CW, CH, 2, 10, 1, 1),
        lambda: S.upscale_planes(ssrc.u, None, 4 * cw, cw, ch, sdst.u, dst.v, 4 * CW, CW, CH, 2, 10, 1, 1),
        lambda: S.upscale_planes(src.u, None, 2 * cw, cw, ch, dst.u, dst.v, 2 * CW, CW, CH, 2, 10, 0, 0),
        lambda: S.upscale_planes(ssrc.u, None, 4 * cw - 2, cw, ch, sdst.u, None, 4 * CW, CW, CH, 2, 10, 1, 1),
    ]
    for k, call in enumerate(op_bad):
        with pytest.raises(S.SrcnnError) as e:
            call()
        assert e.value.code == S.ERR_INVALID and S.last_error(), k
    for t in untouched:
        assert (H(t) == GAP).all(), "an invalid call wrote to its output"


# ---- 8: the command line on a 10-bit Y4M stream ----
def test_cli_upscale_deep_y4m(S, tmp_path):
    """5 frames of 38 x 22 C420p10, every frame different, through `cnn upscale
    --scale 2`: every output frame must be srcnn_upscale_frame's of that frame,
    in a stream of the same depth, C token and range."""
    net = S.Net(*NET)
    params = make_params(np.random.default_rng(3), NET, sd=0.05)
    off = S.net_offsets(net) + [params.size]
    layers = {"layer%d" % (i + 1): {"weights": [float(v) for v in params[off[2 * i]:off[2 * i + 1]]],
                                    "bias": [float(v) for v in params[off[2 * i + 1]:off[2 * i + 2]]]}
              for i in range(3)}
    (tmp_path / "params.json").write_text(json.dumps(dict(epochs=0, **layers)))
    conf = {"n1": 64, "n2": 32, "f1": 9, "f2": 1, "f3": 5, "momentum": 0.9, "weight_decay_parameter": 0.001,
            "learning_rates": [0.001, 0.001, 0.0001], "parameters_file": str(tmp_path / "params.json")}
    for i in (1, 2, 3):
        conf["parameters_distribution_%d" % i] = {"mean_w": 0.0, "mean_b": 0.0, "std_deviation_w": 0.01,
                                                  "std_deviation_b": 0.0}
    (tmp_path / "config.json").write_text(json.dumps(conf))
    w, h, s, n = 38, 22, 2, 5
    cw, ch, W, Hh = 19, 11, 76, 44
    CW, CH = 38, 22
    rng = np.random.default_rng(9)
    frames = [rng.integers(0, 1024, w * h + 2 * cw * ch).astype("<u2") for _ in range(n)]
    head = b"YUV4MPEG2 W38 H22 F30000:1001 Ip A1:1 C420p10 XCOLORRANGE=FULL\n"
    one = len(b"FRAME\n") + 2 * frames[0].size
    raw = head + b"".join(b"FRAME\n" + f.tobytes() for f in frames)
    src_path = tmp_path / "in.y4m"
    src_path.write_bytes(raw)

    # what srcnn_upscale_frame makes of each frame
    pd = torch.from_numpy(params).cuda()
    nbytes = S.upscale_yuv_workspace_bytes(net, w, h, s)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    f = S.yuv_format(10, 0, S.YUV_PLANAR, 2, 2, S.YUV_FULL)
    ddims = frame_dims(W, Hh, 2, 2, 0)
    want = []
    for fr in frames:
        arrays = [fr[:w * h].reshape(h, w), fr[w * h:w * h + cw * ch].reshape(ch, cw), fr[w * h + cw * ch:].reshape(ch, cw)]
        src, keep = device_frame(S, arrays, 2 * w, 2 * cw)
        dst, planes = blank_frame(S, ddims, 2 * W, 2 * CW)
        S.upscale_frame(net, f, src, dst, w, h, s, pd, ws, nbytes)
        want.append(np.concatenate([H(t) for t in planes]).tobytes())
    assert len(set(want)) == n
    assert max(int(np.frombuffer(b, "<u2").max()) for b in want) > 255, "the output does not use its depth"

    def run(inp, out, *extra, ok=True):
        p = subprocess.run([CNN, "upscale", "-c", str(tmp_path / "config.json"), "-i", str(inp), "-o", str(out),
                            "--scale", "2", *extra], capture_output=True, text=True, timeout=120)
        assert (p.returncode == 0) == ok, p.stdout + p.stderr
        return p

    def split(path):
        b = path.read_bytes()
        line, body = b.split(b"\n", 1)
        fb = 2 * (W * Hh + 2 * CW * CH)
        assert len(body) % (6 + fb) == 0
        got = []
        for i in range(0, len(body), 6 + fb):
            assert body[i:i + 6] == b"FRAME\n"
            got.append(body[i + 6:i + 6 + fb])
        return line.decode().split(), got

    out = tmp_path / "out.y4m"
    p = run(src_path, out)
    assert "Frames: 5," in p.stdout and "frames per second" in p.stdout
    tokens, got = split(out)
    assert tokens[0] == "YUV4MPEG2" and "W76" in tokens and "H44" in tokens
    for t in ("F30000:1001", "A1:1", "C420p10", "XCOLORRANGE=FULL"):
        assert t in tokens
    assert len(got) == n
    for k in range(n):
        assert got[k] == want[k], "frame %d differs from srcnn_upscale_frame's" % k
    # one slot gives the same file
    out1 = tmp_path / "out1.y4m"
    run(src_path, out1, "--slots", "1")
    assert out1.read_bytes() == out.read_bytes()
    # --frames 2
    out2 = tmp_path / "out2.y4m"
    p = run(src_path, out2, "--frames", "2")
    tokens, got = split(out2)
    assert got == want[:2] and "Frames: 2," in p.stdout
    # cut in the middle of frame 4 (index 3): three frames, exit status non-zero
    cut = tmp_path / "cut.y4m"
    cut.write_bytes(raw[:len(head) + 3 * one + one // 2])
    out3 = tmp_path / "out3.y4m"
    p = run(cut, out3, ok=False)
    assert "truncated" in p.stdout and "Frames: 3," in p.stdout
    tokens, got = split(out3)
    assert got == want[:3]


# ---- 9: preload, then a first deep frame ----
def test_preload_then_first_deep_frame(S):
    """srcnn_preload resolves the deep and semi-planar kernels of yuv.hip with
    the others; a P010 chroma plane right after it runs as usual."""
    net = S.Net(*NET)
    S.preload(net)
    src = D.encode(planes_of(5, 4, 10), 10, 1)
    got = gpu_planes(S, src, 2, 10, 8, 10, 1, S.YUV_SEMIPLANAR, True)
    q, raw = ref_planes(5, 4, 2, 10, 8, 10)
    near = D.near_boundary(raw, 2e-3 * 4)
    assert np.array_equal(got[~near], D.encode(q, 10, 1)[~near])
    assert np.abs(D.decode(got, 10, 1) - q.astype(np.int64)).max() <= 1


# ---- 10: the 8-bit and the general entry points keep their own names ----
def test_each_entry_point_reports_under_its_own_name(S):
    """The 8-bit entry points are the general ones at 8 bits, yet each of the
    eight reports a rejected call under the name the caller used: scale 5 on a
    5 x 3 frame gives SRCNN_ERR_INVALID and a message that starts with that
    name and a colon; a workspace one byte short gives SRCNN_ERR_WORKSPACE from
    the two net-level calls in the same way.  Nothing is launched: every buffer
    keeps its bytes."""
    net = S.Net(*NET)
    w, h, cw, ch = 5, 3, 3, 2
    params = torch.from_numpy(make_params(np.random.default_rng(1), NET, sd=0.05)).cuda()
    nbytes = S.upscale_yuv_workspace_bytes(net, w, h, 2)
    assert nbytes > 0
    # room for a x5 frame of two-byte samples in every plane
    y, u, v, Y, U, V = bufs = [torch.full((2 * 25 * w * h,), GAP, dtype=torch.uint8, device="cuda") for _ in range(6)]
    ws = torch.full((max(nbytes, 4 * 25 * w * h),), GAP, dtype=torch.uint8, device="cuda")
    f8 = S.yuv_format(8, 0, S.YUV_PLANAR, 2, 2, S.YUV_FULL)

    def calls(s, ws_bytes):
        W, Hh, CW, CH = s * w, s * h, (s * w - 1) // 2 + 1, (s * h - 1) // 2 + 1
        src, dst = S.yuv_frame(y, u, v, w, cw), S.yuv_frame(Y, U, V, W, CW)
        op = {
            "yuv_upscale_luma": lambda: S.yuv_upscale_luma(y, w, ws, w, h, s, 0, S.YUV_FULL),
            "yuv_upscale_luma16": lambda: S.yuv_upscale_luma16(y, 2 * w, ws, w, h, s, 0, 10, 0, S.YUV_FULL),
            # (the two that take no scale: a pitch below the row)
            "yuv_compose_luma": lambda: S.yuv_compose_luma(ws, Y, W - 1, W, Hh, S.YUV_FULL),
            "yuv_compose_luma16": lambda: S.yuv_compose_luma16(ws, Y, 2 * W - 2, W, Hh, 10, 0, S.YUV_FULL),
            "upscale_planes_u8": lambda: S.upscale_planes_u8(u, v, cw, cw, ch, U, V, CW, CW, CH, s),
            "upscale_planes": lambda: S.upscale_planes(u, v, 2 * cw, cw, ch, U, V, 2 * CW, CW, CH, s, 10, 0,
                                                       S.YUV_PLANAR),
        }
        net_level = {
            "upscale_yuv": lambda: S.upscale_yuv(net, src, dst, w, h, 2, 2, s, S.YUV_FULL, params, ws, ws_bytes),
            "upscale_frame": lambda: S.upscale_frame(net, f8, src, dst, w, h, s, params, ws, ws_bytes),
        }
        return op, net_level

    def rejected(named, code):
        for name, call in named.items():
            with pytest.raises(S.SrcnnError) as e:
                call()
            assert e.value.code == code, name
            assert S.last_error().startswith(name + ":"), (name, S.last_error())

    op, net_level = calls(5, nbytes)
    rejected(dict(op, **net_level), S.ERR_INVALID)
    rejected(calls(2, nbytes - 1)[1], S.ERR_WORKSPACE)
    for t in bufs + [ws]:
        assert (H(t) == GAP).all(), "a rejected call wrote to a buffer"
