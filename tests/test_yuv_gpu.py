"""The Y'CbCr front and back end on the GPU (csrc/hip/yuv.hip):
srcnn_yuv_upscale_luma, srcnn_upscale_planes_u8, srcnn_yuv_compose_luma and the
network-level srcnn_upscale_yuv against the float64 restatement of the spec
(tests/yuv_ref.py), against their own composition, under the
memory contract of include/srcnn.h, and through `cnn upscale` on a Y4M file.

Every byte plane is used once with a tight pitch and once with pitch = width +
3; the gap bytes hold 0x5A before the call and must hold it afterwards."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import hip_util
import yuv_ref as R
from conftest import ROOT
from hip_util import H, guarded, guards_intact, make_params
from step_util import S, _settings  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CNN = os.path.join(ROOT, "cnn-super-resolution_amd", "bin", "cnn")
NETS = {"default": (64, 32, 9, 1, 5), "wide": (128, 64, 9, 5, 5), "example": (32, 16, 9, 1, 5)}
# The kernels' tiles are upscale.hip's (struct Tile, bicubic.hpp): 32 x 16
# source pixels for the luma, 64 x 8 (scale <= 2) or 32 x 16 for the byte
# planes, so tests/test_upscale_gpu.py's shapes cover them: every tap clamped
# (1 x 1), smaller than the 4-tap support, odd, more than one tile (37 x 23),
# and at least 3 tiles each way with a ragged last one (135 x 37).
SHAPES = [(1, 1), (2, 3), (5, 4), (17, 9), (37, 23), (135, 37)]
# yuv_compose_luma has no tile: a wavefront takes a row, 1024 pixels per pass;
# 1100 x 3 makes it go round twice.
COMPOSE_SHAPES = SHAPES + [(1100, 3)]
SCALES = [1, 2, 3, 4]
PADS = [0, 7, 12]
RANGES = [R.FULL, R.LIMITED]
GAP = 0x5A
# Chroma planes: seed 1 (the issue's; its worst full-size case exempts 0.63 %
# of the values from the exact comparison).  The cropped 19 x 12 -> 37 x 23 case
# with seed 1 exempts 0.29 % (5 of its 1702 values), checked on the CPU
# against the reference alone (tests/test_yuv_cpu.py repeats both counts).
PLANES_SEED = 1


def rng_code(S, r):
    return S.YUV_FULL if r == R.FULL else S.YUV_LIMITED


def pitches(w):
    return (w, w + 3)


def to_pitched(a, pitch):
    """a [h][w] u8 -> device bytes [h * pitch], gaps GAP."""
    h, w = a.shape
    b = np.full((h, pitch), GAP, np.uint8)
    b[:, :w] = a
    return torch.from_numpy(b.ravel()).cuda()


def blank_pitched(w, h, pitch, fill=GAP):
    return torch.full((h * pitch,), fill, dtype=torch.uint8, device="cuda")


def from_pitched(t, w, h, pitch, what=""):
    """device bytes [h * pitch] -> [h][w]; the gap bytes must still be GAP."""
    b = H(t).reshape(h, pitch)
    assert (b[:, w:] == GAP).all(), "%s: a pitch gap byte was written" % what
    return b[:, :w].copy()


@functools.lru_cache(maxsize=None)
def y_of(w, h):
    a = np.random.default_rng(0).integers(0, 256, (h, w), dtype=np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def planes_of(pw, ph):
    a = np.random.default_rng(PLANES_SEED).integers(0, 256, (2, ph, pw), dtype=np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def luma_of(W, Hh):
    a = np.random.default_rng(0).uniform(-0.1, 1.1, (Hh, W)).astype(np.float32)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def ref_plane(w, h, s, r):
    """the reference's upscaled luma (no margin), shared by the pads"""
    a = R.luma_plane(y_of(w, h), s, 0, r)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def ref_planes(pw, ph, s, ow, oh):
    u8, raw = R.planes_u8(planes_of(pw, ph), s, ow, oh)
    u8.setflags(write=False)
    raw.setflags(write=False)
    return u8, raw


def pad_plane(up, pad):
    Hh, W = up.shape
    m = pad // 2
    return up[np.ix_(np.clip(np.arange(Hh + pad) - m, 0, Hh - 1), np.clip(np.arange(W + pad) - m, 0, W - 1))]


def gpu_luma_plane(S, w, h, s, pad, r, pitch):
    src = to_pitched(y_of(w, h), pitch)
    out = torch.full(((s * h + pad) * (s * w + pad),), float("nan"), dtype=torch.float32, device="cuda")
    S.yuv_upscale_luma(src, pitch, out, w, h, s, pad, rng_code(S, r))
    from_pitched(src, w, h, pitch, "yuv_upscale_luma source")
    return H(out).reshape(s * h + pad, s * w + pad)


def gpu_planes(S, pw, ph, s, ow, oh, sp, dp):
    p = planes_of(pw, ph)
    s0, s1 = to_pitched(p[0], sp), to_pitched(p[1], sp)
    d0, d1 = blank_pitched(ow, oh, dp), blank_pitched(ow, oh, dp)
    S.upscale_planes_u8(s0, s1, sp, pw, ph, d0, d1, dp, ow, oh, s)
    return np.stack([from_pitched(d0, ow, oh, dp, "planes dst0"), from_pitched(d1, ow, oh, dp, "planes dst1")])


def gpu_compose(S, v, r, pitch):
    Hh, W = v.shape
    dst = blank_pitched(W, Hh, pitch)
    S.yuv_compose_luma(torch.from_numpy(v.copy()).cuda(), dst, pitch, W, Hh, rng_code(S, r))
    return from_pitched(dst, W, Hh, pitch, "yuv_compose_luma")


# ---- 1: luma against the float64 reference ----
@pytest.mark.parametrize("r", RANGES)
@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("w,h", SHAPES)
def test_luma_vs_reference(S, w, h, s, r):
    """Full range: |error| <= 4e-6, tests/test_upscale_gpu.py's derived bound
    (20 roundings of 2^-24 on values <= 1 with (sum |w|)^2 <= 1.524 give
    1.8e-6; doubled for fma contraction and the fp32-rounded weights).  Limited
    range: values reach (255 - 16) / 219 = 1.092, so 4.5e-6."""
    bound = 4e-6 if r == R.FULL else 4.5e-6
    for pad in PADS:
        ref = pad_plane(ref_plane(w, h, s, r), pad)
        for pitch in pitches(w):
            got = gpu_luma_plane(S, w, h, s, pad, r, pitch)
            assert np.isfinite(got).all(), "plane pixels left unwritten"
            err = float(np.abs(got.astype(np.float64) - ref).max())
            print("yuv_upscale_luma %dx%d x%d pad %d %s pitch %d: max |err| %.3e" % (w, h, s, pad, r, pitch, err))
            assert err <= bound, (pad, pitch, err)


# ---- 2: scale 1, full range: Y / 255 and replicate padding, bit for bit ----
@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("w,h", SHAPES)
def test_luma_scale_1_anchor(S, w, h, pad):
    ex = y_of(w, h).astype(np.float32) / np.float32(255)
    m = pad // 2
    for pitch in pitches(w):
        got = gpu_luma_plane(S, w, h, 1, pad, R.FULL, pitch)
        assert hip_util.same_bits(got[m:m + h, m:m + w], ex), "interior differs from float(Y) / 255"
        assert hip_util.same_bits(got, pad_plane(ex, pad)), "a margin pixel differs from the pixel it replicates"


# ---- 3: the byte planes against the float64 reference ----
def check_planes(S, pw, ph, s, ow, oh):
    ref, raw = ref_planes(pw, ph, s, ow, oh)
    near = np.abs(raw - np.floor(raw) - 0.5) <= 2e-3
    assert near.mean() <= 0.01, "more than 1 %% of the case exempt: %d of %d" % (near.sum(), near.size)
    for sp, dp in zip(pitches(pw), pitches(ow)):
        got = gpu_planes(S, pw, ph, s, ow, oh, sp, dp)
        d = np.abs(got.astype(np.int16) - ref.astype(np.int16))
        print("upscale_planes_u8 %dx%d x%d -> %dx%d pitch %d/%d: %d of %d exempt, %d differ by 1, max diff %d"
              % (pw, ph, s, ow, oh, sp, dp, near.sum(), near.size, (d == 1).sum(), d.max()))
        assert d.max() <= 1
        assert np.array_equal(got[~near], ref[~near])


@pytest.mark.parametrize("s", [2, 3, 4])
@pytest.mark.parametrize("pw,ph", SHAPES)
def test_planes_vs_reference(S, pw, ph, s):
    """Within 1 everywhere; exactly equal wherever the reference's unrounded
    value is further than 2e-3 from a rounding boundary (k + 0.5): the fp32
    chain on values <= 255 * 1.524 errs below 1e-3.  At most 1 % of a case's
    values may be exempt."""
    check_planes(S, pw, ph, s, s * pw, s * ph)


def test_planes_cropped_420(S):
    """37 x 23 luma at scale 2, 4:2:0: chroma 19 x 12 -> the top-left 37 x 23
    of its 38 x 24."""
    check_planes(S, 19, 12, 2, 37, 23)


@pytest.mark.parametrize("pw,ph", SHAPES)
def test_planes_scale_1_is_the_source(S, pw, ph):
    for sp, dp in zip(pitches(pw), pitches(pw)):
        assert np.array_equal(gpu_planes(S, pw, ph, 1, pw, ph, sp, dp), planes_of(pw, ph))


# ---- 4: compose against the float64 reference ----
@pytest.mark.parametrize("r", RANGES)
@pytest.mark.parametrize("W,Hh", COMPOSE_SHAPES)
def test_compose_vs_reference(S, W, Hh, r):
    """Within 1 everywhere, exact wherever the raw value is further than 1e-4
    from a rounding boundary (one product rounding on values <= 280 is
    1.7e-5).  At most 0.1 % of a case's values may be exempt."""
    v = luma_of(W, Hh)
    ref, raw = R.compose_luma(v, r)
    near = np.abs(raw - np.floor(raw) - 0.5) <= 1e-4
    assert near.mean() <= 0.001
    for pitch in pitches(W):
        got = gpu_compose(S, v, r, pitch)
        d = np.abs(got.astype(np.int16) - ref.astype(np.int16))
        print("yuv_compose_luma %dx%d %s pitch %d: %d exempt, max diff %d" % (W, Hh, r, pitch, near.sum(), d.max()))
        assert d.max() <= 1
        assert np.array_equal(got[~near], ref[~near])


# ---- 5: srcnn_upscale_yuv is its op-level calls ----
def frame_planes(w, h, cx, cy):
    cw, ch = R.chroma_size(w, h, cx, cy)
    return y_of(w, h), planes_of(cw, ch)


def device_frame(S, y, uv, py, pc):
    t = [to_pitched(y, py), to_pitched(uv[0], pc), to_pitched(uv[1], pc)]
    return S.yuv_frame(t[0], t[1], t[2], py, pc), t


def blank_frame(S, W, Hh, CW, CH, py, pc, fill=GAP):
    t = [blank_pitched(W, Hh, py, fill), blank_pitched(CW, CH, pc, fill), blank_pitched(CW, CH, pc, fill)]
    return S.yuv_frame(t[0], t[1], t[2], py, pc), t


@pytest.mark.parametrize("name,arith,cx,cy,s", [
    ("default", 0, 2, 2, 2), ("default", 1, 2, 2, 2), ("example", 0, 2, 2, 2), ("wide", 0, 2, 2, 2),
    ("default", 0, 2, 1, 3), ("default", 0, 1, 1, 1)])
def test_upscale_yuv_is_its_calls(S, name, arith, cx, cy, s):
    cfg = NETS[name]
    net = S.Net(*cfg)
    w, h = 37, 23
    W, Hh, pad = s * w, s * h, cfg[2] + cfg[3] + cfg[4] - 3
    PW, PH = W + pad, Hh + pad
    cw, ch = R.chroma_size(w, h, cx, cy)
    CW, CH = R.chroma_size(W, Hh, cx, cy)
    S.set_arith(arith)
    params = torch.from_numpy(make_params(np.random.default_rng(11), cfg, sd=0.05)).cuda()
    y, uv = frame_planes(w, h, cx, cy)
    rc = S.YUV_LIMITED

    # what srcnn_upscale's forward runs on a plane of the same size
    rgba = torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda")
    nb_rgba = S.upscale_workspace_bytes(net, w, h, s)
    S.upscale(net, rgba, w, h, s, params, torch.empty(W * Hh * 3, dtype=torch.uint8, device="cuda"),
              torch.empty(nb_rgba, dtype=torch.uint8, device="cuda"), nb_rgba)
    family, kernels = S.last_path(), S.last_kernels()

    for py, pc, PY, PC in ((w, cw, W, CW), (w + 3, cw + 3, W + 3, CW + 3)):
        src, keep_src = device_frame(S, y, uv, py, pc)
        # the calls, on buffers of the test
        plane = torch.empty(PW * PH, dtype=torch.float32, device="cuda")
        out = torch.empty(W * Hh, dtype=torch.float32, device="cuda")
        rb = S.reduce_workspace_bytes(PW * PH)
        red = torch.empty(rb, dtype=torch.uint8, device="cuda")
        fb = S.forward_workspace_bytes(net, PW, PH, 1)
        fws = torch.empty(fb, dtype=torch.uint8, device="cuda")
        ops, keep_ops = blank_frame(S, W, Hh, CW, CH, PY, PC)
        S.yuv_upscale_luma(src.y, py, plane, w, h, s, pad, rc)
        S.sub_mean(plane, PW * PH, None, red, rb)
        S.forward(net, plane, PW, PH, 1, params, out, fws, fb)
        assert (S.last_path(), S.last_kernels()) == (family, kernels)
        S.yuv_compose_luma(out, ops.y, PY, W, Hh, rc)
        S.upscale_planes_u8(src.u, src.v, pc, cw, ch, ops.u, ops.v, PC, CW, CH, s)
        # the one call
        nbytes = S.upscale_yuv_workspace_bytes(net, w, h, s)
        assert nbytes >= 4 * (PW * PH + W * Hh) + rb + fb
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        dst, keep_dst = blank_frame(S, W, Hh, CW, CH, PY, PC)
        S.upscale_yuv(net, src, dst, w, h, cx, cy, s, rc, params, ws, nbytes)
        assert (S.last_path(), S.last_kernels()) == (family, kernels)
        if name != "wide":
            assert family == "fused", family
        for a, b, (pw_, ph_, p_) in zip(keep_dst, keep_ops, ((W, Hh, PY), (CW, CH, PC), (CW, CH, PC))):
            assert np.array_equal(from_pitched(a, pw_, ph_, p_, "upscale_yuv"), from_pitched(b, pw_, ph_, p_, "ops"))
        assert len(np.unique(H(keep_dst[0]))) > 8, "degenerate result"
        with pytest.raises(S.SrcnnError) as e:
            S.upscale_yuv(net, src, dst, w, h, cx, cy, s, rc, params, ws, nbytes - 1)
        assert e.value.code == S.ERR_WORKSPACE


# ---- 6: the memory contract ----
def guarded_bytes(a, fill):
    """a: u8 array -> (guarded float32 view over its bytes, padded to whole
    floats with GAP; the number of bytes)."""
    b = np.asarray(a, np.uint8).ravel()
    n = b.size
    b = np.concatenate([b, np.full((-n) % 4, GAP, np.uint8)])
    return guarded(b.view(np.float32), fill), n


@pytest.mark.parametrize("w,h,s,cx,cy", [(1, 1, 1, 2, 2), (37, 23, 3, 2, 2)])
def test_upscale_yuv_memory(S, w, h, s, cx, cy):
    """srcnn_upscale_yuv on an exact-size workspace holding zeros, NaN and
    +1e30, guard bands of the same around every plane, params and ws, pitch =
    width + 3 everywhere.  The output bytes must not depend on the fill, the
    gaps and the spare bytes must keep GAP, and two more runs into planes of
    0x00 and of 0xFF bytes must give the same bytes (every byte is written)."""
    cfg = NETS["default"]
    net = S.Net(*cfg)
    W, Hh = s * w, s * h
    cw, ch = R.chroma_size(w, h, cx, cy)
    CW, CH = R.chroma_size(W, Hh, cx, cy)
    py, pc, PY, PC = w + 3, cw + 3, W + 3, CW + 3
    y, uv = frame_planes(w, h, cx, cy)
    params = make_params(np.random.default_rng(w * 100 + h), cfg, sd=0.05)
    nbytes = S.upscale_yuv_workspace_bytes(net, w, h, s)
    assert nbytes % 4 == 0
    dims = ((W, Hh, PY), (CW, CH, PC), (CW, CH, PC))

    def pitched_np(a, pitch):
        b = np.full((a.shape[0], pitch), GAP, np.uint8)
        b[:, :a.shape[1]] = a
        return b

    runs = []
    for fill in (0.0,) + hip_util.POISONS:
        srcs = [guarded_bytes(pitched_np(a, p), fill)[0] for a, p in ((y, py), (uv[0], pc), (uv[1], pc))]
        dsts = [guarded_bytes(np.full(hh * p, GAP, np.uint8), fill) for _, hh, p in dims]
        pd, ws = guarded(params, fill), guarded(nbytes // 4, fill)
        src = S.yuv_frame(srcs[0], srcs[1], srcs[2], py, pc)
        dst = S.yuv_frame(dsts[0][0], dsts[1][0], dsts[2][0], PY, PC)
        S.upscale_yuv(net, src, dst, w, h, cx, cy, s, S.YUV_FULL, pd, ws, nbytes)
        assert S.last_path() == "fused"
        got = []
        for (t, n), (ww, hh, p) in zip(dsts, dims):
            allb = H(t.view(torch.uint8))
            assert (allb[n:] == GAP).all(), "spare bytes behind a plane written"
            b = allb[:n].reshape(hh, p)
            assert (b[:, ww:] == GAP).all(), "a pitch gap byte was written"
            got.append(b[:, :ww].copy())
        runs.append(got)
        guards_intact(*srcs, *[t for t, _ in dsts], pd, ws)
        assert hip_util.same_bits(H(pd), params)
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert np.array_equal(a, b), "result depends on the workspace's previous contents"
    src, keep = device_frame(S, y, uv, py, pc)
    pd = torch.from_numpy(params).cuda()
    for byte in (0x00, 0xFF):
        dst, planes = blank_frame(S, W, Hh, CW, CH, PY, PC, fill=byte)
        ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        S.upscale_yuv(net, src, dst, w, h, cx, cy, s, S.YUV_FULL, pd, ws, nbytes)
        for t, a, (ww, hh, p) in zip(planes, runs[0], dims):
            assert np.array_equal(H(t).reshape(hh, p)[:, :ww], a), "an output byte was left unwritten"
    with pytest.raises(S.SrcnnError) as e:
        S.upscale_yuv(net, src, dst, w, h, cx, cy, s, S.YUV_FULL, pd, ws, nbytes - 1)
    assert e.value.code == S.ERR_WORKSPACE


def test_upscale_yuv_rejects_invalid_arguments(S):
    """Every invalid argument gives SRCNN_ERR_INVALID before any launch: the
    outputs keep their bytes.  The workspace query returns 0 where the sizes
    or the net are invalid."""
    cfg = NETS["default"]
    net = S.Net(*cfg)
    w, h, s, cx, cy = 37, 23, 2, 2, 2
    W, Hh = s * w, s * h
    cw, ch = R.chroma_size(w, h, cx, cy)
    CW, CH = R.chroma_size(W, Hh, cx, cy)
    y, uv = frame_planes(w, h, cx, cy)
    params = torch.from_numpy(make_params(np.random.default_rng(1), cfg, sd=0.05)).cuda()
    nbytes = S.upscale_yuv_workspace_bytes(net, w, h, s)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    src, keep_src = device_frame(S, y, uv, w, cw)
    dst, planes = blank_frame(S, W, Hh, CW, CH, W, CW)
    good = dict(net=net, src=src, dst=dst, w=w, h=h, cx=cx, cy=cy, scale=s, yuv_range=S.YUV_FULL, params=params,
                ws=ws, ws_bytes=nbytes)

    def frame(f, **kw):
        d = dict(y=f.y, u=f.u, v=f.v, pitch_y=f.pitch_y, pitch_c=f.pitch_c)
        d.update(kw)
        return S.YuvFrame(d["y"], d["u"], d["v"], d["pitch_y"], d["pitch_c"])

    bad = {
        "scale 0": dict(scale=0), "scale 5": dict(scale=5),
        "subsampling 3x1": dict(cx=3, cy=1), "subsampling 1x2": dict(cx=1, cy=2), "subsampling 0x0": dict(cx=0, cy=0),
        "zero width": dict(w=0), "zero height": dict(h=0),
        "source y pitch": dict(src=frame(src, pitch_y=w - 1)), "source c pitch": dict(src=frame(src, pitch_c=cw - 1)),
        "output y pitch": dict(dst=frame(dst, pitch_y=W - 1)), "output c pitch": dict(dst=frame(dst, pitch_c=CW - 1)),
        "null source y": dict(src=frame(src, y=None)), "null source v": dict(src=frame(src, v=None)),
        "null output u": dict(dst=frame(dst, u=None)), "null params": dict(params=None), "null ws": dict(ws=None),
        "invalid net": dict(net=S.Net(64, 32, 9, 2, 5)), "range": dict(yuv_range=2),
        "2^32 plane elements": dict(w=65536, h=65536, scale=1,
                                    src=frame(src, pitch_y=65536, pitch_c=32768),
                                    dst=frame(dst, pitch_y=65536, pitch_c=32768)),
    }
    for what, kw in bad.items():
        a = dict(good)
        a.update(kw)
        with pytest.raises(S.SrcnnError) as e:
            S.upscale_yuv(a["net"], a["src"], a["dst"], a["w"], a["h"], a["cx"], a["cy"], a["scale"], a["yuv_range"],
                          a["params"], a["ws"], a["ws_bytes"])
        assert e.value.code == S.ERR_INVALID, what
        assert S.last_error(), what
    for t in planes:
        assert (H(t) == GAP).all(), "an invalid call wrote to its output"
    assert S.upscale_yuv_workspace_bytes(net, w, h, 0) == 0
    assert S.upscale_yuv_workspace_bytes(net, w, h, 5) == 0
    assert S.upscale_yuv_workspace_bytes(net, 0, h, 2) == 0
    assert S.upscale_yuv_workspace_bytes(net, 65536, 65536, 1) == 0
    assert S.upscale_yuv_workspace_bytes(S.Net(64, 32, 9, 2, 5), w, h, 2) == 0
    # the op-level calls reject their own
    with pytest.raises(S.SrcnnError):
        S.upscale_planes_u8(src.u, src.v, cw, cw, ch, dst.u, dst.v, CW, 2 * cw + 1, CH, 2)   # wider than the x2
    with pytest.raises(S.SrcnnError):
        S.upscale_planes_u8(src.u, src.v, cw, cw, ch, dst.u, dst.v, CW, 2 * cw - 2, CH, 2)   # drops a whole sample
    with pytest.raises(S.SrcnnError):
        S.yuv_compose_luma(ws, dst.y, W - 1, W, Hh, S.YUV_FULL)
    with pytest.raises(S.SrcnnError):
        S.yuv_upscale_luma(src.y, w, ws, w, h, 2, 0, 7)


# ---- 7: the command line on a Y4M stream ----
def test_cli_upscale_y4m(S, tmp_path):
    """5 frames of 38 x 22 C420jpeg, every frame different, through `cnn
    upscale --scale 2`: more frames than slots, so a slot-reuse or ordering
    bug shows.  Every output frame must be srcnn_upscale_yuv's of that frame."""
    cfg = NETS["default"]
    net = S.Net(*cfg)
    params = make_params(np.random.default_rng(3), cfg, sd=0.05)
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
    frames = [rng.integers(0, 256, w * h + 2 * cw * ch, dtype=np.uint8) for _ in range(n)]
    head = b"YUV4MPEG2 W38 H22 F30000:1001 Ip A1:1 C420jpeg\n"
    one = len(b"FRAME\n") + frames[0].size
    raw = head + b"".join(b"FRAME\n" + f.tobytes() for f in frames)
    src_path = tmp_path / "in.y4m"
    src_path.write_bytes(raw)

    # what srcnn_upscale_yuv makes of each frame (limited range: no XCOLORRANGE token)
    pd = torch.from_numpy(params).cuda()
    nbytes = S.upscale_yuv_workspace_bytes(net, w, h, s)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    want = []
    for f in frames:
        y, u, v = f[:w * h].reshape(h, w), f[w * h:w * h + cw * ch].reshape(ch, cw), f[w * h + cw * ch:].reshape(ch, cw)
        src, keep = device_frame(S, y, (u, v), w, cw)
        dst, planes = blank_frame(S, W, Hh, CW, CH, W, CW)
        S.upscale_yuv(net, src, dst, w, h, 2, 2, s, S.YUV_LIMITED, pd, ws, nbytes)
        want.append(np.concatenate([H(t) for t in planes]).tobytes())
    assert len(set(want)) == n

    def run(inp, out, *extra, ok=True):
        p = subprocess.run([CNN, "upscale", "-c", str(tmp_path / "config.json"), "-i", str(inp), "-o", str(out),
                            "--scale", "2", *extra], capture_output=True, text=True, timeout=120)
        assert (p.returncode == 0) == ok, p.stdout + p.stderr
        return p

    def split(path):
        b = path.read_bytes()
        line, body = b.split(b"\n", 1)
        fb = W * Hh + 2 * CW * CH
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
    for t in ("F30000:1001", "A1:1", "C420jpeg"):
        assert t in tokens
    assert len(got) == n
    for k in range(n):
        assert got[k] == want[k], "frame %d differs from srcnn_upscale_yuv's" % k
    # one slot gives the same file
    out1 = tmp_path / "out1.y4m"
    run(src_path, out1, "--slots", "1")
    assert out1.read_bytes() == out.read_bytes()
    # dry: every frame is computed, nothing is written
    dry = tmp_path / "dry.y4m"
    p = subprocess.run([CNN, "upscale", "dry", "-c", str(tmp_path / "config.json"), "-i", str(src_path), "-o", str(dry),
                        "--scale", "2"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "Frames: 5," in p.stdout and not dry.exists(), p.stdout
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


def test_preload_then_first_frame(S):
    """srcnn_preload resolves the kernels of yuv.hip with the others; a frame
    right after it runs as usual."""
    net = S.Net(*NETS["default"])
    S.preload(net)
    assert np.array_equal(gpu_planes(S, 5, 4, 2, 10, 8, 5, 10), ref_planes(5, 4, 2, 10, 8)[0])


def test_host_alloc_round_trip(S):
    """srcnn_host_alloc gives host memory the copies accept; 0 bytes give NULL."""
    import ctypes
    n = 4099
    data = np.random.default_rng(4).integers(0, 256, n, dtype=np.uint8)
    a, b = S.host_alloc(n), S.host_alloc(n)
    try:
        assert a and b and a != b
        ctypes.memmove(a, data.ctypes.data, n)
        d = torch.zeros(n, dtype=torch.uint8, device="cuda")
        S.memcpy_h2d(d.data_ptr(), a, n)
        assert np.array_equal(H(d), data)
        S.memcpy_d2h(b, d.data_ptr(), n)
        assert ctypes.string_at(b, n) == data.tobytes()
    finally:
        S.host_free(a)
        S.host_free(b)
    assert S.host_alloc(0) == 0
    S.host_free(0)
