"""The upscale front and back end for any output size on the GPU
(csrc/hip/resize.hip): srcnn_resize_luma, srcnn_resize_compose,
srcnn_yuv_resize_luma, srcnn_resize_planes and the network-level
srcnn_upscale_to and srcnn_upscale_frame_to against the float64 restatement of
the spec (tests/resize_ref.py), against the existing kernels at ratio 1,
against their own composition, under the memory contract of include/srcnn.h,
and through `cnn upscale --size`.

The error bounds, derived: the weights' moduli sum to at most
1.25 per axis, so (sum |w|)^2 <= 1.5625 where DESIGN.md 10.1's tables give
1.524.  20 roundings of 2^-24 on values <= 1 give 1.5625 * 20 * 2^-24 =
1.86e-6; doubled for fma contraction and the fp32-rounded weights 3.7e-6 <=
4e-6 at full range; at limited range the values reach (255 - 16) / 219 = 1.092:
4.07e-6 <= 4.5e-6.  The byte chain works on values <= 255 * 1.5625 and errs by
9.5e-4 < 1e-3, so a byte can differ from the reference's only where the
reference's unrounded value lies within 2e-3 of where truncation (rgb) or
rounding (chroma) changes; at 10 bits the values and the band are 4 times as
large.

Every plane of samples is used once with a tight pitch and once with pitch =
(width + 3) samples; the gap bytes hold 0x5A and must keep it."""
import json
import os
import subprocess

import numpy as np
import pytest

import hip_util
import resize_ref as R
import yuv_deep_ref as D
from conftest import ROOT
from hip_util import H, guarded, guards_intact, make_params, same_bits
from step_util import S, _settings  # noqa: F401
from test_upscale_gpu import SHAPES
from test_yuv_deep_gpu import (GAP, blank_frame, blank_pitched, device_frame, frame_arrays, frame_dims, frame_pitches,
                               frame_planes_of, from_pitched, guarded_bytes, nbytes_of, pitched_np, pitches, rng_code,
                               to_pitched, unpitch)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CNN = os.path.join(ROOT, "cnn-super-resolution_amd", "bin", "cnn")
NETS = {"default": (64, 32, 9, 1, 5), "wide": (128, 64, 9, 5, 5), "example": (32, 16, 9, 1, 5)}
NET = NETS["default"]
PADS = [0, 7, 12]  # 7: the odd margin (3 left / top, 4 right / bottom)
RANGES = [D.FULL, D.LIMITED]
# (bits, msb): RGBA is source None
Y_FORMATS = [(8, 0), (10, 0), (10, 1), (16, 0)]
CHROMA_FORMATS = [(8, 0), (10, 0), (10, 1), (16, 1)]
case = pytest.mark.parametrize("src,dst", R.CASES, ids=R.CASE_IDS)


def gpu_luma_rgba(S, w, h, W, Hh, pad):
    src = torch.from_numpy(R.rgba_of(w, h).copy()).cuda()
    out = torch.full(((Hh + pad) * (W + pad),), float("nan"), dtype=torch.float32, device="cuda")
    S.resize_luma(src, out, w, h, W, Hh, pad)
    return H(out).reshape(Hh + pad, W + pad)


def gpu_luma_y(S, w, h, W, Hh, pad, r, bits, msb, pitch):
    src = to_pitched(D.encode(R.y_of(w, h, bits), bits, msb), pitch)
    out = torch.full(((Hh + pad) * (W + pad),), float("nan"), dtype=torch.float32, device="cuda")
    S.yuv_resize_luma(src, pitch, out, w, h, W, Hh, pad, bits, msb, rng_code(S, r))
    from_pitched(src, w, h, pitch, bits, "yuv_resize_luma source")
    return H(out).reshape(Hh + pad, W + pad)


def gpu_compose(S, w, h, W, Hh, nl):
    src = torch.from_numpy(R.rgba_of(w, h).copy()).cuda()
    out = torch.full((Hh * W * 3,), 0x5A, dtype=torch.uint8, device="cuda")
    S.resize_compose(src, torch.from_numpy(nl.copy()).cuda(), out, w, h, W, Hh)
    return H(out).reshape(Hh, W, 3)


def gpu_planes(S, p, ow, oh, rx, ry, bits, msb, layout, tight):
    """p [2][ph][pw] words through srcnn_resize_planes in `layout` -> [2][oh][ow] words"""
    ph, pw = p.shape[1:]
    k = 0 if tight else 1
    if layout == S.YUV_SEMIPLANAR:
        sp, dp = pitches(2 * pw, bits)[k], pitches(2 * ow, bits)[k]
        s0, d0 = to_pitched(D.interleave(p), sp), blank_pitched(oh, dp)
        S.resize_planes(s0, None, sp, pw, ph, d0, None, dp, ow, oh, rx[0], rx[1], ry[0], ry[1], bits, msb, layout)
        return D.deinterleave(from_pitched(d0, 2 * ow, oh, dp, bits, "semi-planar dst"))
    sp, dp = pitches(pw, bits)[k], pitches(ow, bits)[k]
    s0, s1 = to_pitched(p[0], sp), to_pitched(p[1], sp)
    d0, d1 = blank_pitched(oh, dp), blank_pitched(oh, dp)
    S.resize_planes(s0, s1, sp, pw, ph, d0, d1, dp, ow, oh, rx[0], rx[1], ry[0], ry[1], bits, msb, layout)
    return np.stack([from_pitched(d0, ow, oh, dp, bits, "planes dst0"), from_pitched(d1, ow, oh, dp, bits, "planes dst1")])


# ---- 1: luma against the float64 reference ----
@case
def test_luma_rgba_vs_reference(S, src, dst):
    """|error| <= 4e-6 (module docstring); every plane float is written."""
    (w, h), (W, Hh) = src, dst
    up = R.luma_plane(R.rgba_of(w, h), W, Hh, 0)
    for pad in PADS:
        got = gpu_luma_rgba(S, w, h, W, Hh, pad)
        assert np.isfinite(got).all(), "plane pixels left unwritten"
        err = float(np.abs(got.astype(np.float64) - R.pad_plane(up, pad)).max())
        print("resize_luma %dx%d -> %dx%d pad %d: max |err| %.3e" % (w, h, W, Hh, pad, err))
        assert err <= 4e-6, (pad, err)


@pytest.mark.parametrize("bits,msb", Y_FORMATS)
@case
def test_luma_y_vs_reference(S, src, dst, bits, msb):
    """Full range: |error| <= 4e-6, limited range 4.5e-6 (module docstring).
    The samples are normalised before the resampling, so the values the fp32
    chain works on are those of the 8-bit case whatever the depth."""
    (w, h), (W, Hh) = src, dst
    for r in RANGES:
        bound = 4e-6 if r == D.FULL else 4.5e-6
        up = R.yuv_luma_plane(R.y_of(w, h, bits), W, Hh, 0, bits, 0, r)
        for pad in PADS:
            ref = R.pad_plane(up, pad)
            for pitch in pitches(w, bits):
                got = gpu_luma_y(S, w, h, W, Hh, pad, r, bits, msb, pitch)
                assert np.isfinite(got).all(), "plane pixels left unwritten"
                err = float(np.abs(got.astype(np.float64) - ref).max())
                print("yuv_resize_luma %dx%d -> %dx%d pad %d %s %d bits msb %d pitch %d: max |err| %.3e"
                      % (w, h, W, Hh, pad, r, bits, msb, pitch, err))
                assert err <= bound, (r, pad, pitch, err)


# ---- 2: the ratio-1 anchors, bit for bit ----
@pytest.mark.parametrize("w,h", SHAPES)
def test_ratio_1_luma_is_extract_luma(S, w, h):
    src = torch.from_numpy(R.rgba_of(w, h).copy()).cuda()
    ex = torch.empty(w * h, dtype=torch.float32, device="cuda")
    S.extract_luma(src, ex, w, h, 1)
    ex = H(ex).reshape(h, w)
    for pad in PADS:
        got = gpu_luma_rgba(S, w, h, w, h, pad)
        m = pad // 2
        assert same_bits(got[m:m + h, m:m + w], ex), "interior differs from srcnn_extract_luma"
        assert same_bits(got, R.pad_plane(ex, pad)), "a margin pixel differs from the interior pixel it replicates"


@pytest.mark.parametrize("bits,msb", Y_FORMATS)
@pytest.mark.parametrize("w,h", SHAPES)
def test_ratio_1_luma_is_y_over_full_scale(S, w, h, bits, msb):
    ex = R.y_of(w, h, bits).astype(np.float32) / np.float32((1 << bits) - 1)
    for pad in PADS:
        m = pad // 2
        for pitch in pitches(w, bits):
            got = gpu_luma_y(S, w, h, w, h, pad, D.FULL, bits, msb, pitch)
            assert same_bits(got[m:m + h, m:m + w], ex), "interior differs from float(Y) / (2^bits - 1)"
            assert same_bits(got, R.pad_plane(ex, pad)), "a margin pixel differs from the pixel it replicates"


@pytest.mark.parametrize("w,h", SHAPES)
def test_ratio_1_compose_is_swap_luma(S, w, h):
    nl = R.new_luma_of(w, h)
    got = gpu_compose(S, w, h, w, h, nl)
    src = torch.from_numpy(R.rgba_of(w, h).copy()).cuda()
    out = torch.zeros(w * h * 3, dtype=torch.uint8, device="cuda")
    S.swap_luma(src, torch.from_numpy(nl.copy()).cuda(), out, w, h, w, h)
    assert np.array_equal(got, H(out).reshape(h, w, 3))


@pytest.mark.parametrize("bits,msb", CHROMA_FORMATS)
@pytest.mark.parametrize("pw,ph", SHAPES)
def test_ratio_1_planes_are_the_source(S, pw, ph, bits, msb):
    src = D.encode(R.planes_of(pw, ph, bits), bits, msb)
    for tight in (True, False):
        for layout in (S.YUV_PLANAR, S.YUV_SEMIPLANAR):
            for rx, ry in (((1, 1), (1, 1)), ((pw, pw), (ph, ph))):
                assert np.array_equal(gpu_planes(S, src, pw, ph, rx, ry, bits, msb, layout, tight), src)


# ---- 3: compose against the float64 reference ----
@case
def test_compose_vs_reference(S, src, dst):
    """Within 1 everywhere; exactly equal wherever the reference's unclipped,
    untruncated value is further than 2e-3 from an integer (module docstring).
    At most 1 % of a case's values may be exempt."""
    (w, h), (W, Hh) = src, dst
    got = gpu_compose(S, w, h, W, Hh, R.new_luma_of(W, Hh))
    ref, raw = R.ref_compose(w, h, W, Hh)
    d = np.abs(got.astype(np.int16) - ref.astype(np.int16))
    near = R.near_integer(raw, R.COMPOSE_BAND)
    print("resize_compose %dx%d -> %dx%d: %d of %d exempt, %d differ by 1, max diff %d"
          % (w, h, W, Hh, near.sum(), near.size, (d == 1).sum(), d.max()))
    assert near.mean() <= R.COMPOSE_CAP
    assert d.max() <= 1
    assert np.array_equal(got[~near], ref[~near])


# ---- 4: planes against the float64 reference ----
@pytest.mark.parametrize("bits,msb", CHROMA_FORMATS)
@pytest.mark.parametrize("pc", R.PLANE_CASES, ids=R.PLANE_IDS)
def test_planes_vs_reference(S, pc, bits, msb):
    """Within 1 everywhere; exactly equal wherever the reference's unrounded
    value is further than the band from a rounding boundary k + 0.5: 2e-3 at 8
    bits (at most 1 % of a case exempt), 8e-3 at 10 bits (2.5 %); at 16 bits
    only "within 1".  msb words keep their low bits zero, the semi-planar
    result is the planar one sample for sample, gap bytes keep their fill."""
    (pw, ph), (ow, oh), rx, ry = pc
    q, raw = R.ref_planes(pw, ph, ow, oh, rx, ry, bits)
    ref = D.encode(q, bits, msb)
    src = D.encode(R.planes_of(pw, ph, bits), bits, msb)
    if bits in R.PLANE_BANDS:
        band, cap = R.PLANE_BANDS[bits]
        near = D.near_boundary(raw, band)
        assert near.mean() <= cap, "too much of the case exempt: %d of %d" % (near.sum(), near.size)
    for tight in (True, False):
        got = gpu_planes(S, src, ow, oh, rx, ry, bits, msb, S.YUV_PLANAR, tight)
        if msb:
            assert not (got & ((1 << (16 - bits)) - 1)).any(), "low bits of an msb word set"
        d = np.abs(D.decode(got, bits, msb) - q.astype(np.int64))
        print("resize_planes %dx%d -> %dx%d %d bits msb %d tight %d: %d differ by 1, max diff %d"
              % (pw, ph, ow, oh, bits, msb, tight, (d == 1).sum(), d.max()))
        assert d.max() <= 1
        if bits in R.PLANE_BANDS:
            assert np.array_equal(got[~near], ref[~near])
        semi = gpu_planes(S, src, ow, oh, rx, ry, bits, msb, S.YUV_SEMIPLANAR, tight)
        assert np.array_equal(semi, got), "the interleaved result differs from the planar one"


# ---- 5: srcnn_upscale_to is its four op-level calls ----
@pytest.mark.parametrize("name,arith", [("default", 0), ("default", 1), ("example", 0), ("wide", 0)])
def test_upscale_to_is_its_four_calls(S, name, arith):
    cfg = NETS[name]
    net = S.Net(*cfg)
    (w, h), (W, Hh) = (37, 23), (53, 52)
    pad = cfg[2] + cfg[3] + cfg[4] - 3
    PW, PH = W + pad, Hh + pad
    S.set_arith(arith)
    params = torch.from_numpy(make_params(np.random.default_rng(11), cfg, sd=0.05)).cuda()
    src = torch.from_numpy(R.rgba_of(w, h).copy()).cuda()
    # the four calls, on buffers of the test
    plane = torch.empty(PW * PH, dtype=torch.float32, device="cuda")
    out = torch.empty(W * Hh, dtype=torch.float32, device="cuda")
    rb = S.reduce_workspace_bytes(PW * PH)
    red = torch.empty(rb, dtype=torch.uint8, device="cuda")
    fb = S.forward_workspace_bytes(net, PW, PH, 1)
    fws = torch.empty(fb, dtype=torch.uint8, device="cuda")
    rgb_ops = torch.zeros(W * Hh * 3, dtype=torch.uint8, device="cuda")
    S.resize_luma(src, plane, w, h, W, Hh, pad)
    S.sub_mean(plane, PW * PH, None, red, rb)
    S.forward(net, plane, PW, PH, 1, params, out, fws, fb)
    family, kernels = S.last_path(), S.last_kernels()
    S.resize_compose(src, out, rgb_ops, w, h, W, Hh)
    # the one call
    nbytes = S.upscale_to_workspace_bytes(net, w, h, W, Hh)
    assert nbytes >= 4 * (PW * PH + W * Hh) + rb + fb
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    rgb = torch.full((W * Hh * 3,), 0xFF, dtype=torch.uint8, device="cuda")
    S.upscale_to(net, src, w, h, W, Hh, params, rgb, ws, nbytes)
    assert (S.last_path(), S.last_kernels()) == (family, kernels)
    if name != "wide":
        assert family == "fused", family
    else:
        assert family in ("fast", "generic", "wide"), family
    a, b = H(rgb), H(rgb_ops)
    assert np.array_equal(a, b)
    assert len(np.unique(a)) > 8, "degenerate result"
    with pytest.raises(S.SrcnnError) as e:
        S.upscale_to(net, src, w, h, W, Hh, params, rgb, ws, nbytes - 1)
    assert e.value.code == S.ERR_WORKSPACE


# ---- 6: srcnn_upscale_frame_to is its op-level calls ----
FRAME_FORMATS = {"u8": (8, 0, 0), "NV12": (8, 0, 1), "p10": (10, 0, 0), "P010": (10, 1, 1)}  # bits, msb, layout


@pytest.mark.parametrize("fmt", sorted(FRAME_FORMATS))
@pytest.mark.parametrize("cx,cy", [(2, 2), (2, 1), (1, 1)])
def test_upscale_frame_to_is_its_calls(S, cx, cy, fmt):
    bits, msb, layout = FRAME_FORMATS[fmt]
    net = S.Net(*NET)
    (w, h), (W, Hh) = (37, 23), (55, 35)
    pad = NET[2] + NET[3] + NET[4] - 3
    PW, PH = W + pad, Hh + pad
    cw, ch = D.chroma_size(w, h, cx, cy)
    CW, CH = D.chroma_size(W, Hh, cx, cy)
    params = torch.from_numpy(make_params(np.random.default_rng(11), NET, sd=0.05)).cuda()
    rc = S.YUV_LIMITED
    f = S.yuv_format(bits, msb, layout, cx, cy, rc)
    arrays = frame_arrays(w, h, cx, cy, bits, msb, layout)
    sdims, ddims = frame_dims(w, h, cx, cy, layout), frame_dims(W, Hh, cx, cy, layout)
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
        S.yuv_resize_luma(src.y, py, plane, w, h, W, Hh, pad, bits, msb, rc)
        S.sub_mean(plane, PW * PH, None, red, rb)
        S.forward(net, plane, PW, PH, 1, params, out, fws, fb)
        family, kernels = S.last_path(), S.last_kernels()
        assert family == "fused", family
        S.yuv_compose_luma16(out, ops.y, PY, W, Hh, bits, msb, rc)
        S.resize_planes(src.u, src.v, pc, cw, ch, ops.u, ops.v, PC, CW, CH, w, W, h, Hh, bits, msb, layout)
        # the one call
        nbytes = S.upscale_frame_to_workspace_bytes(net, w, h, W, Hh)
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        dst, keep_dst = blank_frame(S, ddims, PY, PC)
        S.upscale_frame_to(net, f, src, dst, w, h, W, Hh, params, ws, nbytes)
        assert (S.last_path(), S.last_kernels()) == (family, kernels)
        got = frame_planes_of(keep_dst, ddims, PY, PC, bits, "upscale_frame_to")
        want = frame_planes_of(keep_ops, ddims, PY, PC, bits, "ops")
        for a, b in zip(got, want):
            assert (a is None and b is None) or np.array_equal(a, b)
        assert len(np.unique(got[0])) > 8, "degenerate result"
        with pytest.raises(S.SrcnnError) as e:
            S.upscale_frame_to(net, f, src, dst, w, h, W, Hh, params, ws, nbytes - 1)
        assert e.value.code == S.ERR_WORKSPACE


# ---- 7: the memory contract ----
MEMORY_SIZES = [((1, 1), (1, 1)), ((37, 23), (55, 35))]


@pytest.mark.parametrize("src,dst", MEMORY_SIZES)
def test_upscale_to_memory(S, src, dst):
    """srcnn_upscale_to on an exact-size workspace holding zeros, NaN and
    +1e30, guard bands around rgba, params, rgb and ws (test_upscale_memory's
    scheme): the result must not depend on the fill, every one of the 3WH rgb
    bytes must be written and the spare bytes of rgb's last float kept."""
    (w, h), (W, Hh) = src, dst
    net = S.Net(*NET)
    n_rgb = 3 * W * Hh
    n_rgb_f = (n_rgb + 3) // 4
    params = make_params(np.random.default_rng(w * 100 + h), NET, sd=0.05)
    rgba = R.rgba_of(w, h)
    rgba_f = rgba.copy().view(np.float32).ravel()
    nbytes = S.upscale_to_workspace_bytes(net, w, h, W, Hh)
    assert nbytes % 4 == 0
    nan_bytes = np.array([float("nan")], np.float32).view(np.uint8)
    runs = []
    for fill in (0.0,) + hip_util.POISONS:
        sd, pd = guarded(rgba_f, fill), guarded(params, fill)
        rgb = guarded(n_rgb_f, fill, inner=float("nan"))
        ws = guarded(nbytes // 4, fill)
        S.upscale_to(net, sd, w, h, W, Hh, pd, rgb, ws, nbytes)
        assert S.last_path() == "fused"
        allb = H(rgb.view(torch.uint8))
        spare = allb[n_rgb:]
        assert np.array_equal(spare, nan_bytes[4 - spare.size:] if spare.size else spare), "spare bytes of rgb written"
        runs.append(allb[:n_rgb])
        guards_intact(sd, pd, rgb, ws)
        assert np.array_equal(H(sd.view(torch.uint8)), rgba.ravel()) and same_bits(H(pd), params)
    for r in runs[1:]:
        assert np.array_equal(runs[0], r), "result depends on the workspace's previous contents"
    sd = torch.from_numpy(rgba.copy()).cuda()
    pd = torch.from_numpy(params).cuda()
    for byte in (0x00, 0xFF):
        rgb = torch.full((n_rgb,), byte, dtype=torch.uint8, device="cuda")
        ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        S.upscale_to(net, sd, w, h, W, Hh, pd, rgb, ws, nbytes)
        assert np.array_equal(H(rgb), runs[0]), "an rgb byte was left unwritten"


@pytest.mark.parametrize("fmt", ["P010", "p10"])
@pytest.mark.parametrize("src,dst", MEMORY_SIZES)
def test_upscale_frame_to_memory(S, src, dst, fmt):
    """srcnn_upscale_frame_to under test_upscale_frame_memory's scheme: exact
    workspace of zeros, NaN and +1e30, guard bands around every plane, params
    and ws, pitch = (width + 3) samples everywhere."""
    (w, h), (W, Hh) = src, dst
    cx = cy = 2
    bits, msb, layout = FRAME_FORMATS[fmt]
    net = S.Net(*NET)
    arrays = frame_arrays(w, h, cx, cy, bits, msb, layout)
    sdims, ddims = frame_dims(w, h, cx, cy, layout), frame_dims(W, Hh, cx, cy, layout)
    py, pc = frame_pitches(sdims, bits, False)
    PY, PC = frame_pitches(ddims, bits, False)
    f = S.yuv_format(bits, msb, layout, cx, cy, S.YUV_FULL)
    params = make_params(np.random.default_rng(w * 100 + h), NET, sd=0.05)
    nbytes = S.upscale_frame_to_workspace_bytes(net, w, h, W, Hh)
    assert nbytes % 4 == 0
    runs = []
    for fill in (0.0,) + hip_util.POISONS:
        srcs = [None if a is None else guarded_bytes(pitched_np(a, p), fill)[0] for a, p in zip(arrays, (py, pc, pc))]
        dsts = [None if d is None else guarded_bytes(np.full(d[1] * p, GAP, np.uint8), fill)
                for d, p in zip(ddims, (PY, PC, PC))]
        pd, ws = guarded(params, fill), guarded(nbytes // 4, fill)
        sf = S.yuv_frame(srcs[0], srcs[1], srcs[2], py, pc)
        df = S.yuv_frame(dsts[0][0], dsts[1][0], dsts[2][0] if dsts[2] else None, PY, PC)
        S.upscale_frame_to(net, f, sf, df, w, h, W, Hh, pd, ws, nbytes)
        assert S.last_path() == "fused"
        got = []
        for tn, d, p in zip(dsts, ddims, (PY, PC, PC)):
            if d is None:
                continue
            allb = H(tn[0].view(torch.uint8))
            assert (allb[tn[1]:] == GAP).all(), "spare bytes behind a plane written"
            got.append(unpitch(allb[:tn[1]], d[0], d[1], p, bits, "upscale_frame_to"))
        runs.append(got)
        guards_intact(*[t for t in srcs if t is not None], *[tn[0] for tn in dsts if tn], pd, ws)
        assert same_bits(H(pd), params)
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert np.array_equal(a, b), "result depends on the workspace's previous contents"
    sf, keep = device_frame(S, arrays, py, pc)
    pd = torch.from_numpy(params).cuda()
    for byte in (0x00, 0xFF):
        df, planes = blank_frame(S, ddims, PY, PC, fill=byte)
        ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        S.upscale_frame_to(net, f, sf, df, w, h, W, Hh, pd, ws, nbytes)
        live = [(t, d, p) for t, d, p in zip(planes, ddims, (PY, PC, PC)) if d is not None]
        for (t, d, p), a in zip(live, runs[0]):
            b = H(t).reshape(d[1], p)[:, :d[0] * nbytes_of(bits)]
            assert np.array_equal(np.ascontiguousarray(b).view(D.dtype(bits)), a), "an output sample was left unwritten"


# ---- 8: invalid arguments ----
def test_invalid_arguments_write_nothing(S):
    """Every rule of include/srcnn.h gives SRCNN_ERR_INVALID with a message
    before any launch: the outputs keep their bytes."""
    net = S.Net(*NET)
    (w, h), (W, Hh), cx, cy = (37, 23), (55, 35), 2, 2
    cw, ch = D.chroma_size(w, h, cx, cy)
    CW, CH = D.chroma_size(W, Hh, cx, cy)
    params = torch.from_numpy(make_params(np.random.default_rng(1), NET, sd=0.05)).cuda()
    nbytes = S.upscale_frame_to_workspace_bytes(net, w, h, W, Hh)
    assert S.upscale_to_workspace_bytes(net, w, h, W, Hh) == nbytes
    ws = torch.full((nbytes,), GAP, dtype=torch.uint8, device="cuda")
    rgba = torch.from_numpy(R.rgba_of(w, h).copy()).cuda()
    # room for a 4 x 4 times frame of two-byte samples in every output
    outs = [torch.full((2 * 16 * w * h * 3,), GAP, dtype=torch.uint8, device="cuda") for _ in range(4)]
    rgb, Yo, Uo, Vo = outs
    y, u, v = (torch.zeros(2 * w * h, dtype=torch.uint8, device="cuda") for _ in range(3))

    def fmt(bits=10, msb=0, layout=0, cx=cx, cy=cy, r=S.YUV_FULL):
        return S.yuv_format(bits, msb, layout, cx, cy, r)

    def frame_to(f=None, sy=y, su=u, sv=v, dy=Yo, du=Uo, dv=Vo, w=w, h=h, W=W, H=Hh, py=2 * w, pc=2 * cw, PY=2 * W,
                 PC=2 * CW, p=params, wsp=ws, n=nbytes, nt=net, no_fmt=False):
        S.upscale_frame_to(nt, None if no_fmt else (f or fmt()), S.yuv_frame(sy, su, sv, py, pc),
                           S.yuv_frame(dy, du, dv, PY, PC), w, h, W, H, p, wsp, n)

    def planes(pw=cw, ph=ch, ow=CW, oh=CH, rx=(w, W), ry=(h, Hh), sp=None, dp=None, bits=10, msb=0, layout=0, s0=u,
               s1=v, d0=Uo, d1=Vo):
        B = (1 if bits == 8 else 2) * (2 if layout == 1 else 1)
        S.resize_planes(s0, s1, pw * B if sp is None else sp, pw, ph, d0, d1, ow * B if dp is None else dp, ow, oh,
                        rx[0], rx[1], ry[0], ry[1], bits, msb, layout)

    bad = {
        # sizes
        "luma W < w": lambda: S.resize_luma(rgba, ws, w, h, w - 1, Hh, 12),
        "luma W > 4w": lambda: S.resize_luma(rgba, ws, w, h, 4 * w + 1, Hh, 12),
        "luma H < h": lambda: S.resize_luma(rgba, ws, w, h, W, h - 1, 12),
        "luma H > 4h": lambda: S.resize_luma(rgba, ws, w, h, W, 4 * h + 1, 12),
        "luma zero size": lambda: S.resize_luma(rgba, ws, w, 0, W, Hh, 12),
        "luma null": lambda: S.resize_luma(None, ws, w, h, W, Hh, 12),
        "luma 2^31 plane floats": lambda: S.resize_luma(rgba, ws, 30000, 30000, 100000, 100000, 12),
        "compose W < w": lambda: S.resize_compose(rgba, ws, rgb, w, h, w - 1, Hh),
        "compose H > 4h": lambda: S.resize_compose(rgba, ws, rgb, w, h, W, 4 * h + 1),
        "compose zero size": lambda: S.resize_compose(rgba, ws, rgb, w, h, 0, Hh),
        "compose null": lambda: S.resize_compose(rgba, None, rgb, w, h, W, Hh),
        "compose 2^31 rgb bytes": lambda: S.resize_compose(rgba, ws, rgb, 20000, 20000, 30000, 30000),
        "yuv W > 4w": lambda: S.yuv_resize_luma(y, 2 * w, ws, w, h, 4 * w + 1, Hh, 12, 10, 0, S.YUV_FULL),
        "yuv H < h": lambda: S.yuv_resize_luma(y, 2 * w, ws, w, h, W, h - 1, 12, 10, 0, S.YUV_FULL),
        "yuv pitch": lambda: S.yuv_resize_luma(y, 2 * w - 2, ws, w, h, W, Hh, 12, 10, 0, S.YUV_FULL),
        "yuv odd pitch": lambda: S.yuv_resize_luma(y, 2 * w + 1, ws, w, h, W, Hh, 12, 10, 0, S.YUV_FULL),
        "yuv odd address": lambda: S.yuv_resize_luma(y.data_ptr() + 1, 2 * w, ws, w, h, W, Hh, 12, 10, 0, S.YUV_FULL),
        "yuv 17 bits": lambda: S.yuv_resize_luma(y, 2 * w, ws, w, h, W, Hh, 12, 17, 0, S.YUV_FULL),
        "yuv msb 2": lambda: S.yuv_resize_luma(y, 2 * w, ws, w, h, W, Hh, 12, 10, 2, S.YUV_FULL),
        "yuv msb at 8 bits": lambda: S.yuv_resize_luma(y, w, ws, w, h, W, Hh, 12, 8, 1, S.YUV_FULL),
        "yuv range": lambda: S.yuv_resize_luma(y, 2 * w, ws, w, h, W, Hh, 12, 10, 0, 7),
        "yuv null": lambda: S.yuv_resize_luma(y, 2 * w, None, w, h, W, Hh, 12, 10, 0, S.YUV_FULL),
        # the plane call's ratios and bounds
        "planes zero numerator": lambda: planes(rx=(0, W)),
        "planes ratio below 1": lambda: planes(rx=(W, w)),
        "planes ratio above 4": lambda: planes(ry=(h, 4 * h + 1)),
        "planes ow beyond its bound": lambda: planes(ow=-(-cw * W // w) + 1),
        "planes oh beyond its bound": lambda: planes(oh=-(-ch * Hh // h) + 1),
        "planes zero size": lambda: planes(oh=0),
        "planes source pitch": lambda: planes(sp=2 * cw - 2),
        "planes output pitch": lambda: planes(dp=2 * CW - 2),
        "planes odd pitch": lambda: planes(dp=2 * CW + 1),
        "planes semi-planar pitch of a planar row": lambda: planes(layout=1, s1=None, d1=None, dp=2 * CW),
        "planes odd address": lambda: planes(d1=Vo.data_ptr() + 1),
        "planes 7 bits": lambda: planes(bits=7),
        "planes msb at 8 bits": lambda: planes(bits=8, msb=1),
        "planes layout 2": lambda: planes(layout=2),
        "planes null": lambda: planes(d0=None),
        "planes no second plane": lambda: planes(s1=None),
        "planes second plane when semi-planar": lambda: planes(layout=1, s1=None),
        "planes 2^31 samples": lambda: planes(pw=65536, ph=32768, ow=65536, oh=32768, rx=(1, 1), ry=(1, 1)),
        # the net-level calls
        "upscale_to W > 4w": lambda: S.upscale_to(net, rgba, w, h, 4 * w + 1, Hh, params, rgb, ws, nbytes),
        "upscale_to H < h": lambda: S.upscale_to(net, rgba, w, h, W, h - 1, params, rgb, ws, nbytes),
        "upscale_to zero size": lambda: S.upscale_to(net, rgba, 0, h, W, Hh, params, rgb, ws, nbytes),
        "upscale_to null params": lambda: S.upscale_to(net, rgba, w, h, W, Hh, None, rgb, ws, nbytes),
        "upscale_to null ws": lambda: S.upscale_to(net, rgba, w, h, W, Hh, params, rgb, None, nbytes),
        "upscale_to invalid net": lambda: S.upscale_to(S.Net(64, 32, 9, 2, 5), rgba, w, h, W, Hh, params, rgb, ws, nbytes),
        "frame_to W < w": lambda: frame_to(W=w - 1), "frame_to W > 4w": lambda: frame_to(W=4 * w + 1),
        "frame_to H < h": lambda: frame_to(H=h - 1), "frame_to H > 4h": lambda: frame_to(H=4 * h + 1),
        "frame_to zero width": lambda: frame_to(w=0), "frame_to zero output height": lambda: frame_to(H=0),
        "frame_to subsampling 3x1": lambda: frame_to(fmt(cx=3, cy=1)), "frame_to subsampling 1x2": lambda: frame_to(fmt(cx=1, cy=2)),
        "frame_to source y pitch": lambda: frame_to(py=2 * w - 2), "frame_to source c pitch": lambda: frame_to(pc=2 * cw - 2),
        "frame_to output y pitch": lambda: frame_to(PY=2 * W - 2), "frame_to output c pitch": lambda: frame_to(PC=2 * CW - 2),
        "frame_to odd output y pitch": lambda: frame_to(PY=2 * W + 1),
        "frame_to semi-planar c pitch of a planar row": lambda: frame_to(fmt(10, 1, 1), sv=None, dv=None),
        "frame_to null source y": lambda: frame_to(sy=None), "frame_to null output u": lambda: frame_to(du=None),
        "frame_to no v in a planar output": lambda: frame_to(dv=None),
        "frame_to v in a semi-planar source": lambda: frame_to(fmt(10, 1, 1), dv=None, pc=4 * cw, PC=4 * CW),
        "frame_to odd source u address": lambda: frame_to(su=u.data_ptr() + 1),
        "frame_to odd output v address": lambda: frame_to(dv=Vo.data_ptr() + 1),
        "frame_to null params": lambda: frame_to(p=None), "frame_to null ws": lambda: frame_to(wsp=None),
        "frame_to invalid net": lambda: frame_to(nt=S.Net(64, 32, 9, 2, 5)), "frame_to range": lambda: frame_to(fmt(r=2)),
        "frame_to 7 bits": lambda: frame_to(fmt(bits=7)), "frame_to 17 bits": lambda: frame_to(fmt(bits=17)),
        "frame_to msb 2": lambda: frame_to(fmt(msb=2)), "frame_to msb at 8 bits": lambda: frame_to(fmt(8, 1), py=w, pc=cw, PY=W, PC=CW),
        "frame_to layout 2": lambda: frame_to(fmt(layout=2)), "frame_to null fmt": lambda: frame_to(no_fmt=True),
        "frame_to 2^32 plane elements": lambda: frame_to(w=65536, h=65536, W=65536, H=65536, py=131072, pc=65536,
                                                         PY=131072, PC=65536),
    }
    for what, call in bad.items():
        with pytest.raises(S.SrcnnError) as e:
            call()
        assert e.value.code == S.ERR_INVALID, what
        assert S.last_error(), what
    for t in outs + [ws]:
        assert (H(t) == GAP).all(), "an invalid call wrote to an output"
    # the valid ones do run (the cases above fail for the reason they name)
    frame_to()
    frame_to(fmt(10, 1, 1), sv=None, dv=None, pc=4 * cw, PC=4 * CW)
    planes()
    S.upscale_to(net, rgba, w, h, W, Hh, params, rgb, ws, nbytes)
    assert not (H(rgb)[:3 * W * Hh] == GAP).all()


# ---- 9: the command line ----
def write_config(S, tmp_path, params):
    net = S.Net(*NET)
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
    return net


def run_cnn(tmp_path, inp, out, *extra, ok=True):
    p = subprocess.run([CNN, "upscale", "-c", str(tmp_path / "config.json"), "-i", str(inp), "-o", str(out), *extra],
                       capture_output=True, text=True, timeout=120)
    assert (p.returncode == 0) == ok, p.stdout + p.stderr
    return p


def test_cli_size_on_an_image(S, tmp_path):
    """`cnn upscale --size 55x35` on a 37 x 23 PNG: srcnn_upscale_to's bytes."""
    from PIL import Image
    params = make_params(np.random.default_rng(3), NET, sd=0.05)
    net = write_config(S, tmp_path, params)
    (w, h), (W, Hh) = (37, 23), (55, 35)
    rgba = R.rgba_of(w, h).copy()
    rgba[..., 3] = 255
    Image.fromarray(rgba[..., :3]).save(tmp_path / "in.png")
    nbytes = S.upscale_to_workspace_bytes(net, w, h, W, Hh)
    rgb = torch.zeros(3 * W * Hh, dtype=torch.uint8, device="cuda")
    S.upscale_to(net, torch.from_numpy(rgba).cuda(), w, h, W, Hh, torch.from_numpy(params).cuda(), rgb,
                 torch.empty(nbytes, dtype=torch.uint8, device="cuda"), nbytes)
    p = run_cnn(tmp_path, tmp_path / "in.png", tmp_path / "out.png", "--size", "55x35")
    assert "Upscale mode, size: 55x35" in p.stdout
    img = Image.open(tmp_path / "out.png")
    assert img.size == (W, Hh) and img.mode == "RGB"
    assert np.array_equal(np.asarray(img), H(rgb).reshape(Hh, W, 3))
    p = run_cnn(tmp_path, tmp_path / "in.png", tmp_path / "bad.png", "--size", "149x35", ok=False)
    assert "outside 1x .. 4x" in p.stdout and "37 .. 148" in p.stdout


@pytest.mark.parametrize("bits", [8, 10])
def test_cli_size_on_a_y4m_stream(S, tmp_path, bits):
    """5 frames of 37 x 23 4:2:0, every frame different, through `cnn upscale
    --size 55x35`: every output frame is srcnn_upscale_frame_to's of that
    frame; the header carries the new W, H and A; --slots 1 gives the same
    file; --frames 2 stops after two frames."""
    params = make_params(np.random.default_rng(3), NET, sd=0.05)
    net = write_config(S, tmp_path, params)
    (w, h), (W, Hh), n = (37, 23), (55, 35), 5
    (cw, ch), (CW, CH) = D.chroma_size(w, h, 2, 2), D.chroma_size(W, Hh, 2, 2)
    B = nbytes_of(bits)
    rng = np.random.default_rng(9)
    frames = [rng.integers(0, 1 << bits, w * h + 2 * cw * ch).astype(D.dtype(bits)) for _ in range(n)]
    ctok = b"C420jpeg" if bits == 8 else b"C420p10"
    head = b"YUV4MPEG2 W37 H23 F30000:1001 Ip A1:1 " + ctok + b" XCOLORRANGE=FULL\n"
    src_path = tmp_path / "in.y4m"
    src_path.write_bytes(head + b"".join(b"FRAME\n" + f.tobytes() for f in frames))

    pd = torch.from_numpy(params).cuda()
    nbytes = S.upscale_frame_to_workspace_bytes(net, w, h, W, Hh)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    f = S.yuv_format(bits, 0, S.YUV_PLANAR, 2, 2, S.YUV_FULL)
    ddims = frame_dims(W, Hh, 2, 2, 0)
    want = []
    for fr in frames:
        arrays = [fr[:w * h].reshape(h, w), fr[w * h:w * h + cw * ch].reshape(ch, cw), fr[w * h + cw * ch:].reshape(ch, cw)]
        src, keep = device_frame(S, arrays, B * w, B * cw)
        dst, planes = blank_frame(S, ddims, B * W, B * CW)
        S.upscale_frame_to(net, f, src, dst, w, h, W, Hh, pd, ws, nbytes)
        want.append(np.concatenate([H(t) for t in planes]).tobytes())
    assert len(set(want)) == n

    def split(path):
        b = path.read_bytes()
        line, body = b.split(b"\n", 1)
        fb = B * (W * Hh + 2 * CW * CH)
        assert len(body) % (6 + fb) == 0
        got = []
        for i in range(0, len(body), 6 + fb):
            assert body[i:i + 6] == b"FRAME\n"
            got.append(body[i + 6:i + 6 + fb])
        return line.decode().split(), got

    out = tmp_path / "out.y4m"
    p = run_cnn(tmp_path, src_path, out, "--size", "55x35")
    assert "Frames: 5," in p.stdout and "-> 55x35" in p.stdout
    tokens, got = split(out)
    # A: 1:1 * (37 * 35) / (55 * 23) = 259:253
    assert tokens == ["YUV4MPEG2", "W55", "H35", "F30000:1001", "Ip", "A259:253", ctok.decode(), "XCOLORRANGE=FULL"]
    assert len(got) == n
    for k in range(n):
        assert got[k] == want[k], "frame %d differs from srcnn_upscale_frame_to's" % k
    out1 = tmp_path / "out1.y4m"
    run_cnn(tmp_path, src_path, out1, "--size", "55x35", "--slots", "1")
    assert out1.read_bytes() == out.read_bytes()
    out2 = tmp_path / "out2.y4m"
    p = run_cnn(tmp_path, src_path, out2, "--size", "55x35", "--frames", "2")
    tokens, got = split(out2)
    assert got == want[:2] and "Frames: 2," in p.stdout


# ---- 10: preload, then a first call; each entry point's own name ----
def test_preload_then_first_resize(S):
    """srcnn_preload resolves the kernels of resize.hip with the others; a P010
    chroma plane right after it runs as usual."""
    S.preload(S.Net(*NET))
    (pw, ph), (ow, oh), rx, ry = R.PLANE_CASES[3]
    src = D.encode(R.planes_of(pw, ph, 10), 10, 1)
    got = gpu_planes(S, src, ow, oh, rx, ry, 10, 1, S.YUV_SEMIPLANAR, True)
    q, raw = R.ref_planes(pw, ph, ow, oh, rx, ry, 10)
    near = D.near_boundary(raw, R.PLANE_BANDS[10][0])
    assert np.array_equal(got[~near], D.encode(q, 10, 1)[~near])
    assert np.abs(D.decode(got, 10, 1) - q.astype(np.int64)).max() <= 1


def test_each_entry_point_reports_under_its_own_name(S):
    """A rejected call's message starts with the name the caller used and a
    colon; a run under the profiler lists each op-level call under its own
    name.  Nothing is launched by the rejected calls."""
    net = S.Net(*NET)
    w, h, W, Hh = 5, 3, 21, 4  # W > 4w
    params = torch.from_numpy(make_params(np.random.default_rng(1), NET, sd=0.05)).cuda()
    bufs = [torch.full((4096,), GAP, dtype=torch.uint8, device="cuda") for _ in range(7)]
    y, u, v, Yo, Uo, Vo, ws = bufs
    f8 = S.yuv_format(8, 0, S.YUV_PLANAR, 2, 2, S.YUV_FULL)
    src, dst = S.yuv_frame(y, u, v, w, 3), S.yuv_frame(Yo, Uo, Vo, W, 11)
    invalid = {
        "resize_luma": lambda: S.resize_luma(y, ws, w, h, W, Hh, 0),
        "resize_compose": lambda: S.resize_compose(y, ws, Yo, w, h, W, Hh),
        "yuv_resize_luma": lambda: S.yuv_resize_luma(y, w, ws, w, h, W, Hh, 0, 8, 0, S.YUV_FULL),
        "resize_planes": lambda: S.resize_planes(u, v, 3, 3, 2, Uo, Vo, 11, 11, 2, 1, 5, 1, 1, 8, 0, S.YUV_PLANAR),
        "upscale_to": lambda: S.upscale_to(net, y, w, h, W, Hh, params, Yo, ws, 4096),
        "upscale_frame_to": lambda: S.upscale_frame_to(net, f8, src, dst, w, h, W, Hh, params, ws, 4096),
    }
    short = {
        "upscale_to": lambda: S.upscale_to(net, y, w, h, 7, Hh, params, Yo, ws, S.upscale_to_workspace_bytes(net, w, h, 7, Hh) - 1),
        "upscale_frame_to": lambda: S.upscale_frame_to(net, f8, src, S.yuv_frame(Yo, Uo, Vo, 7, 4), w, h, 7, Hh, params, ws,
                                                       S.upscale_frame_to_workspace_bytes(net, w, h, 7, Hh) - 1),
    }
    for named, code in ((invalid, S.ERR_INVALID), (short, S.ERR_WORKSPACE)):
        for name, call in named.items():
            with pytest.raises(S.SrcnnError) as e:
                call()
            assert e.value.code == code, name
            assert S.last_error().startswith(name + ":"), (name, S.last_error())
    for t in bufs:
        assert (H(t) == GAP).all(), "a rejected call wrote to a buffer"
    # the profile names
    plane = torch.empty(7 * Hh, dtype=torch.float32, device="cuda")
    S.profile_enable(True)
    S.profile_reset()
    try:
        S.resize_luma(y, plane, w, h, 7, Hh, 0)
        S.yuv_resize_luma(y, w, plane, w, h, 7, Hh, 0, 8, 0, S.YUV_FULL)
        S.resize_compose(y, plane, Yo, w, h, 7, Hh)
        S.resize_planes(u, v, 3, 3, 2, Uo, Vo, 4, 4, 2, 5, 7, 3, 4, 8, 0, S.YUV_PLANAR)
        torch.cuda.synchronize()
        names = set(S.profile_stats())
    finally:
        S.profile_enable(False)
    assert {"resize_luma", "yuv_resize_luma", "resize_compose", "resize_planes"} <= names, names
