"""The downscale of Y'CbCr frames on the GPU (csrc/hip/yuv_down.hip, DESIGN.md
18): srcnn_downscale_planes against the float64 restatement of the spec
(tests/frame_down_ref.py), its exact anchors, srcnn_downscale_rgba and the
upscale it mirrors; srcnn_downscale_frame, srcnn_make_pairs_frame and
srcnn_evaluate_frame against the calls they are made of, under the memory
contract of include/srcnn.h.

Every plane is used once with a tight pitch at an aligned address and once
with pitch = (width + 3) samples at an address 3 samples into its buffer (an
odd byte skew for one-byte samples); the gap bytes hold 0x5A before the call
and must hold it afterwards."""
import numpy as np
import pytest

import frame_down_ref as F
import hip_util
import quality_frame_ref as QF
import test_yuv_deep_gpu as G
import yuv_deep_ref as D
from hip_util import H, guarded, guards_intact, make_params
from step_util import S, _settings  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GAP = G.GAP
NETS = {"default": (64, 32, 9, 1, 5), "example": (32, 16, 9, 1, 5)}
# (bits, msb): one byte; the value in the low bits, in the high bits; the whole word
FORMATS = [(8, 0), (10, 0), (10, 1), (12, 0), (12, 1), (16, 0)]


# ---- planes on the device ----
def put(a, tight):
    """a [h][n] samples -> (device bytes, address of the first sample, pitch)"""
    B = a.itemsize
    pitch = a.shape[1] * B if tight else (a.shape[1] + 3) * B
    skew = 0 if tight else 3 * B
    t = torch.full((skew + a.shape[0] * pitch,), GAP, dtype=torch.uint8, device="cuda")
    t[skew:] = torch.from_numpy(G.pitched_np(a, pitch).ravel()).cuda()
    return t, t.data_ptr() + skew, pitch


def blank(n, h, bits, tight):
    B = G.nbytes_of(bits)
    pitch = n * B if tight else (n + 3) * B
    skew = 0 if tight else 3 * B
    t = torch.full((skew + h * pitch,), GAP, dtype=torch.uint8, device="cuda")
    return t, t.data_ptr() + skew, pitch


def take(t, n, h, pitch, bits, tight, what):
    b = H(t)
    skew = 0 if tight else 3 * G.nbytes_of(bits)
    assert (b[:skew] == GAP).all(), "%s: a byte in front of the plane was written" % what
    return G.unpitch(b[skew:], n, h, pitch, bits, what)


def gpu_down(S, p, s, ow, oh, bits, msb, mode, tight):
    """p [k][ph][pw] words through srcnn_downscale_planes -> [k][oh][ow] words;
    mode "one": k launches of one plane; "two": one launch of two planes;
    "semi": one launch on the interleaved pairs"""
    ph, pw = p.shape[1:]
    if mode == "semi":
        s0, a0, sp = put(D.interleave(p), tight)
        d0, b0, dp = blank(2 * ow, oh, bits, tight)
        S.downscale_planes(a0, None, sp, pw, ph, b0, None, dp, ow, oh, s, bits, msb, S.YUV_SEMIPLANAR)
        assert np.array_equal(H(s0), H(put(D.interleave(p), tight)[0])), "the source was written"
        return D.deinterleave(take(d0, 2 * ow, oh, dp, bits, tight, "semi-planar dst"))
    srcs = [put(q, tight) for q in p]
    dsts = [blank(ow, oh, bits, tight) for q in p]
    sp, dp = srcs[0][2], dsts[0][2]
    if mode == "two":
        S.downscale_planes(srcs[0][1], srcs[1][1], sp, pw, ph, dsts[0][1], dsts[1][1], dp, ow, oh, s, bits, msb,
                           S.YUV_PLANAR)
    else:
        for a, b in zip(srcs, dsts):
            S.downscale_planes(a[1], None, sp, pw, ph, b[1], None, dp, ow, oh, s, bits, msb, S.YUV_PLANAR)
    return np.stack([take(d[0], ow, oh, dp, bits, tight, "dst%d" % i) for i, d in enumerate(dsts)])


# ---- 1: against the float64 reference ----
@pytest.mark.parametrize("bits,msb", FORMATS)
@pytest.mark.parametrize("s", F.SCALES)
@pytest.mark.parametrize("ow,oh", F.SHAPES)
def test_planes_vs_reference(S, ow, oh, s, bits, msb):
    """Within 1 everywhere; exactly equal wherever the reference's unrounded
    value is further than 1e-3 * 2^(bits-8) from a half-integer (frame_down_ref:
    the band and the cap on the exempt share; the seed is the first that keeps
    the reference alone within the cap, tests/test_frame_down_cpu.py).  At 16
    bits the band approaches half a code value and only "within 1" is checked.
    The three sources of an output shape: exactly s times as large, with s - 1
    trailing columns and rows, and s - 1 short of it (ow = ceil(PW / s) >
    PW / s)."""
    for variant in F.VARIANTS:
        seed = F.seed_of(ow, oh, s, variant, bits)
        assert seed is not None
        vals, q, raw, near = F.reference(ow, oh, s, variant, bits, seed)
        if bits in F.CAP:
            assert near.mean() <= F.CAP[bits]
        src, ref = D.encode(vals, bits, msb), D.encode(q, bits, msb)
        for tight in (True, False):
            got = gpu_down(S, src, s, ow, oh, bits, msb, "two", tight)
            if msb:
                assert not (got & ((1 << (16 - bits)) - 1)).any(), "low bits of an msb word set"
            d = np.abs(D.decode(got, bits, msb) - q.astype(np.int64))
            differ = int((d != 0).sum())
            print("downscale_planes %dx%d /%d %s -> %dx%d %d bits msb %d tight %d seed %d: %d of %d exempt, %d differ, "
                  "max diff %d" % (vals.shape[2], vals.shape[1], s, variant, ow, oh, bits, msb, tight, seed, near.sum(),
                                   near.size, differ, d.max()))
            hip_util.log_record(dict(check="downscale_planes", pw=vals.shape[2], ph=vals.shape[1], s=s, ow=ow, oh=oh,
                                     bits=bits, msb=msb, tight=tight, seed=seed, exempt=int(near.sum()),
                                     samples=int(near.size), differ=differ, max_diff=int(d.max())))
            assert d.max() <= 1
            if bits < 16:
                assert np.array_equal(got[~near], ref[~near])
            # the same samples through the other two forms of the call
            assert np.array_equal(gpu_down(S, src, s, ow, oh, bits, msb, "one", tight), got), \
                "two planes in one launch differ from two one-plane launches"
            assert np.array_equal(gpu_down(S, src, s, ow, oh, bits, msb, "semi", tight), got), \
                "the interleaved result differs from the planar one"


# ---- 2: exact anchors ----
@pytest.mark.parametrize("bits,msb", FORMATS)
@pytest.mark.parametrize("pw,ph", F.SHAPES)
def test_scale_1_is_the_source(S, pw, ph, bits, msb):
    src = D.encode(F.values_of(pw, ph, bits, 0), bits, msb)
    for tight in (True, False):
        for mode in ("one", "two", "semi"):
            assert np.array_equal(gpu_down(S, src, 1, pw, ph, bits, msb, mode, tight), src), mode


@pytest.mark.parametrize("bits", [10, 12])
@pytest.mark.parametrize("s", [2, 3, 4])
def test_msb_is_lsb_on_the_shifted_values(S, s, bits):
    vals = F.values_of(37 * s + 1, 23 * s + 2, bits, 1)
    for mode in ("two", "semi"):
        lo = gpu_down(S, D.encode(vals, bits, 0), s, 37, 23, bits, 0, mode, False)
        hi = gpu_down(S, D.encode(vals, bits, 1), s, 37, 23, bits, 1, mode, False)
        assert np.array_equal(hi, lo << (16 - bits))


@pytest.mark.parametrize("s", [1, 2, 3, 4])
def test_two_calls_are_bit_identical(S, s):
    src = D.encode(F.values_of(135 * s, 37 * s, 10, 2), 10, 1)
    a = gpu_down(S, src, s, 135, 37, 10, 1, "semi", False)
    assert np.array_equal(gpu_down(S, src, s, 135, 37, 10, 1, "semi", False), a)


def test_output_may_be_any_top_left_part(S):
    """ow and oh below their bounds: the top-left of the full output"""
    src = F.values_of(135, 37, 8, 0)
    full = gpu_down(S, src, 2, 68, 19, 8, 0, "two", True)
    for ow, oh in ((1, 1), (33, 17), (67, 19), (68, 1)):
        assert np.array_equal(gpu_down(S, src, 2, ow, oh, 8, 0, "two", False), full[:, :oh, :ow])


# ---- 3: against srcnn_downscale_rgba ----
@pytest.mark.parametrize("s", [2, 3, 4])
def test_8_bit_plane_against_downscale_rgba(S, s):
    """An 8-bit plane against the r channel of srcnn_downscale_rgba on the gray
    image: equal outside the band, within 1 inside it (the two rounding rules:
    ties to even here, floor(v + 0.5) there).  Observed on one MI355X: 14 / 6 /
    9 of 4,995 samples in the band at s = 2 / 3 / 4, none differs."""
    W, Hh = 135 * s + s - 1, 37 * s
    g = F.values_of(W, Hh, 8, 3)[:1]
    rgba = np.stack([g[0], g[0], g[0], np.full_like(g[0], 255)], axis=-1)
    w, h = W // s, Hh // s
    small = torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda")
    S.downscale_rgba(torch.from_numpy(rgba.copy()).cuda(), small, W, Hh, s)
    want = H(small).reshape(h, w, 4)[..., 0]
    got = gpu_down(S, g, s, w, h, 8, 0, "one", False)[0]
    near = F.near_half(F.down(g[0], s, w, h), 8)
    d = np.abs(got.astype(np.int64) - want)
    print("downscale_planes against downscale_rgba %dx%d /%d: %d of %d in the band, %d differ (%d of them outside)"
          % (W, Hh, s, near.sum(), near.size, (d != 0).sum(), (d[~near] != 0).sum()))
    assert d.max() <= 1
    assert np.array_equal(got[~near], want[~near])


# ---- 4: down then up is shift-free, on the device ----
@pytest.mark.parametrize("W,Hh,ax,ay", F.RAMPS)
@pytest.mark.parametrize("s", [1, 2, 3, 4])
@pytest.mark.parametrize("bits,msb,rng", [(8, 0, D.LIMITED), (10, 1, D.FULL)])
def test_down_then_up_is_aligned(S, s, W, Hh, ax, ay, bits, msb, rng):
    """|X - T| at least 4s pixels from every edge, X = srcnn_yuv_upscale_luma16
    of the downscaled ramp, T = the same call at scale 1 on the ramp: the
    references give 0 at s = 1, 3 and half a code value, 0.5 / gain, at s = 2,
    4 (tests/test_frame_down_cpu.py); upscale_luma's own documented bound
    (4e-6 at full range, 4.5e-6 at limited, tests/test_yuv_deep_gpu.py) sits on
    top once for X and once for T.  A one-pixel shift would give at least
    1.5 / gain, three times that."""
    Y = D.encode(F.ramp(W, Hh, ax, ay), bits, msb)
    w, h = W // s, Hh // s
    gain = D.levels(bits, rng)[1]
    up = 4e-6 if rng == D.FULL else 4.5e-6
    bound = (0.5 / gain if s in (2, 4) else 0.0) + 2 * up
    src, a0, sp = put(Y, False)
    small, b0, dp = blank(w, h, bits, True)
    S.downscale_planes(a0, None, sp, W, Hh, b0, None, dp, w, h, s, bits, msb, S.YUV_PLANAR)
    X = torch.full((s * h * s * w,), float("nan"), dtype=torch.float32, device="cuda")
    T = torch.full((Hh * W,), float("nan"), dtype=torch.float32, device="cuda")
    S.yuv_upscale_luma16(b0, dp, X, w, h, s, 0, bits, msb, G.rng_code(S, rng))
    S.yuv_upscale_luma16(a0, sp, T, W, Hh, 1, 0, bits, msb, G.rng_code(S, rng))
    X = H(X).reshape(s * h, s * w).astype(np.float64)
    T = H(T).reshape(Hh, W)[:s * h, :s * w].astype(np.float64)
    e = 4 * s
    d = np.abs(X - T)[e:-e, e:-e]
    print("down/up x%d on %dx%d, %d bits: interior max |X - T| = %.4e (bound %.4e, a shift gives %.4e)"
          % (s, W, Hh, bits, d.max(), bound, 1.5 / gain))
    assert d.size > 0 and d.max() <= bound
    for step in (1, -1):
        ds = np.abs(np.roll(X, step, axis=1 if ax == 2 else 0) - T)[e:-e, e:-e].max()
        assert ds > bound, "a one-pixel shift passes the bound"


# ---- frames ----
def frame_values(w, h, cx, cy, bits, seed):
    return QF.make_frame(np.random.default_rng(seed), w, h, cx, cy, bits)


def put_frame(S, p, fill=None):
    """a quality_frame_ref.Packed on the device -> (YuvFrame, what keeps it alive);
    with `fill` every plane sits between guard bands of it"""
    if fill is None:
        t = [None if a is None else torch.from_numpy(a).cuda() for a in (p.y, p.u, p.v)]
    else:
        t = [None if a is None else G.guarded_bytes(a, fill)[0] for a in (p.y, p.u, p.v)]
    return S.yuv_frame(t[0], t[1], t[2], p.pitch_y, p.pitch_c), t


def blank_packed(w, h, cx, cy, bits, msb, layout, extra):
    """a frame of GAP bytes"""
    z = [np.zeros(s, np.int64) for s in ((h, w), QF.chroma_shape(w, h, cx, cy), QF.chroma_shape(w, h, cx, cy))]
    p = QF.pack(tuple(z), bits, msb, layout, cx, cy, extra, extra)
    for a in (p.y, p.u, p.v):
        if a is not None:
            a[:] = GAP
    return p


def read_frame(p, tensors, what):
    """the device bytes of a frame laid out as p -> (Y, U, V) code values; the
    gaps must hold GAP (whole floats of a guarded plane may end in spare GAP bytes)"""
    B = G.nbytes_of(p.bits)
    ch, cw = QF.chroma_shape(p.w, p.h, p.cx, p.cy)
    rows = [(p.h, p.w * B, p.pitch_y), (ch, cw * B * (2 if p.v is None else 1), p.pitch_c), (ch, cw * B, p.pitch_c)]
    got = []
    for t, a, (r, nb, pitch) in zip(tensors, (p.y, p.u, p.v), rows):
        if a is None:
            got.append(None)
            continue
        b = H(t.view(torch.uint8))
        assert (b[r * pitch:] == GAP).all(), "%s: spare bytes behind a plane written" % what
        b = b[:r * pitch].reshape(r, pitch)
        assert (b[:, nb:] == GAP).all(), "%s: a pitch gap byte was written" % what
        got.append(b.ravel().copy())
    q = QF.Packed(got[0], got[1], got[2], p.pitch_y, p.pitch_c, p.bits, p.msb, p.layout, p.w, p.h, p.cx, p.cy)
    return QF.unpack(q)


# bits, msb, layout
FRAME_FORMATS = {"yuv8": (8, 0, 0), "p10": (10, 0, 0), "P010": (10, 1, 1), "NV12": (8, 0, 1), "p16": (16, 0, 0)}


# ---- 5: srcnn_downscale_frame is its two calls ----
@pytest.mark.parametrize("fmt", sorted(FRAME_FORMATS))
@pytest.mark.parametrize("W,Hh,cx,cy,s", [(75, 53, 2, 2, 2), (75, 53, 2, 2, 3), (10, 10, 2, 2, 3), (75, 53, 2, 1, 4),
                                          (38, 22, 1, 1, 1), (4, 4, 2, 2, 4)])
def test_downscale_frame_is_its_calls(S, W, Hh, cx, cy, s, fmt):
    """Byte-identical to srcnn_downscale_planes of the luma and of the chroma,
    and within 1 of the reference; at 10 x 10, 4:2:0, s = 3 the chroma goes
    from 5 to 2 columns, beyond floor(5 / 3); guard bands of 0, NaN and +1e30
    around every plane, pitch gaps unchanged, every sample written."""
    bits, msb, layout = FRAME_FORMATS[fmt]
    A = frame_values(W, Hh, cx, cy, bits, 100 * W + s)
    (w, h), (CW, CH), (cw, ch) = F.frame_sizes(W, Hh, s, cx, cy)
    f = S.yuv_format(bits, msb, layout, cx, cy, S.YUV_LIMITED)
    src_p = QF.pack(A, bits, msb, layout, cx, cy, 3, 3, np.random.default_rng(1))
    dst_p = blank_packed(w, h, cx, cy, bits, msb, layout, 3)
    src, keep = put_frame(S, src_p)
    ops, ops_t = put_frame(S, dst_p)
    S.downscale_planes(src.y, None, src.pitch_y, W, Hh, ops.y, None, ops.pitch_y, w, h, s, bits, msb, S.YUV_PLANAR)
    S.downscale_planes(src.u, src.v, src.pitch_c, CW, CH, ops.u, ops.v, ops.pitch_c, cw, ch, s, bits, msb, layout)
    want = read_frame(dst_p, ops_t, "ops")
    ref, _ = F.frame(A, s, bits, cx, cy)
    for a, b in zip(want, ref):
        assert np.abs(a - b).max() <= 1
    if s == 1:
        for a, b in zip(want, A):
            assert np.array_equal(a, b)
    for fill in (0.0,) + hip_util.POISONS:
        gsrc, gs = put_frame(S, src_p, fill)
        gdst, gd = put_frame(S, dst_p, fill)
        S.downscale_frame(f, gsrc, gdst, W, Hh, s)
        got = read_frame(dst_p, gd, "downscale_frame")
        for a, b in zip(got, want):
            assert np.array_equal(a, b), "downscale_frame differs from its two calls"
        guards_intact(*[t for t in gs + gd if t is not None])
        for t, a in zip(gs, (src_p.y, src_p.u, src_p.v)):
            assert a is None or np.array_equal(H(t.view(torch.uint8))[:a.size], a), "the source was written"
    # every sample is written: planes of 0x00 and of 0xFF bytes give the same samples
    for byte in (0x00, 0xFF):
        p = blank_packed(w, h, cx, cy, bits, msb, layout, 0)
        for a in (p.y, p.u, p.v):
            if a is not None:
                a[:] = byte
        d, dt = put_frame(S, p)
        S.downscale_frame(f, src, d, W, Hh, s)
        q = QF.Packed(*[None if t is None else H(t) for t in dt], p.pitch_y, p.pitch_c, bits, msb, layout, w, h, cx, cy)
        for a, b in zip(QF.unpack(q), want):
            assert np.array_equal(a, b), "an output sample was left unwritten"


# ---- 6: srcnn_make_pairs_frame is its five calls ----
@pytest.mark.parametrize("bits,msb,rng", [(8, 0, "limited"), (10, 1, "full"), (12, 0, "limited")])
@pytest.mark.parametrize("W,Hh,s,tile,stride", [(96, 64, 2, 33, 14), (67, 50, 3, 9, 4), (2, 2, 2, 2, 1), (40, 30, 1, 9, 4)])
def test_make_pairs_frame_is_its_five_calls(S, W, Hh, s, tile, stride, bits, msb, rng):
    """Bit-identical to downscale_planes -> yuv_upscale_luma16 (pad 0) ->
    yuv_upscale_luma16 of Y at scale 1 -> gather_tiles with and without the
    mean, on an exact-size workspace holding zeros, NaN and +1e30 with guard
    bands around Y, X, T and ws; u and v are null.  At s = 1 nothing is
    degraded: X plus its tiles' means is T."""
    rc = S.YUV_FULL if rng == "full" else S.YUV_LIMITED
    f = S.yuv_format(bits, msb, S.YUV_PLANAR, 2, 2, rc)
    Y = D.encode(frame_values(W, Hh, 2, 2, bits, 7 * W + s)[0], bits, msb)
    w, h = W // s, Hh // s
    Wc, Hc = s * w, s * h
    n, nx, ny = S.make_pairs_count(W, Hh, s, tile, stride)
    assert n == nx * ny > 0
    B = G.nbytes_of(bits)
    ybytes = G.pitched_np(Y, (W + 3) * B).ravel()
    # the five calls
    yd = torch.from_numpy(ybytes).cuda()
    small = torch.empty(h * w * B, dtype=torch.uint8, device="cuda")
    xp = torch.empty(Hc * Wc, dtype=torch.float32, device="cuda")
    tp = torch.empty(Hh * W, dtype=torch.float32, device="cuda")
    X0 = torch.empty(n * tile * tile, dtype=torch.float32, device="cuda")
    T0 = torch.empty(n * tile * tile, dtype=torch.float32, device="cuda")
    S.downscale_planes(yd, None, (W + 3) * B, W, Hh, small, None, w * B, w, h, s, bits, msb, S.YUV_PLANAR)
    S.yuv_upscale_luma16(small, w * B, xp, w, h, s, 0, bits, msb, rc)
    S.yuv_upscale_luma16(yd, (W + 3) * B, tp, W, Hh, 1, 0, bits, msb, rc)
    S.gather_tiles(xp, Wc, Hc, 0, 0, stride, nx, ny, tile, tile, 1, X0)
    S.gather_tiles(tp, W, Hh, 0, 0, stride, nx, ny, tile, tile, 0, T0)
    X0, T0 = H(X0), H(T0)
    assert np.isfinite(X0).all() and np.isfinite(T0).all() and (len(np.unique(T0)) > 1 or W == 2)
    if s == 1:
        X1 = torch.empty(n * tile * tile, dtype=torch.float32, device="cuda")
        S.gather_tiles(xp, Wc, Hc, 0, 0, stride, nx, ny, tile, tile, 0, X1)
        assert hip_util.same_bits(H(X1), T0)
    nbytes = S.make_pairs_frame_workspace_bytes(f, W, Hh, s)
    assert nbytes > 0 and nbytes % 256 == 0
    for fill in (0.0,) + hip_util.POISONS:
        yg = G.guarded_bytes(ybytes, fill)[0]
        X, T = guarded(n * tile * tile, fill), guarded(n * tile * tile, fill)
        ws = guarded(nbytes // 4, fill)
        S.make_pairs_frame(f, S.yuv_frame(yg, None, None, (W + 3) * B, 0), W, Hh, s, tile, stride, X, T, ws, nbytes)
        assert hip_util.same_bits(H(X), X0) and hip_util.same_bits(H(T), T0)
        assert np.array_equal(H(yg.view(torch.uint8))[:ybytes.size], ybytes)
        guards_intact(yg, X, T, ws)
    with pytest.raises(S.SrcnnError) as e:
        S.make_pairs_frame(f, S.yuv_frame(yd, None, None, (W + 3) * B, 0), W, Hh, s, tile, stride, X, T, ws, nbytes - 1)
    assert e.value.code == S.ERR_WORKSPACE


# ---- 7: srcnn_evaluate_frame is its calls ----
def chain(S, net, f, fmt, truth, truth_p, W, Hh, s, shave, params):
    """the listed calls on buffers of the test -> the 16 doubles"""
    bits, msb, layout = fmt
    cx, cy = f.cx, f.cy
    w, h = W // s, Hh // s
    Wc, Hc = s * w, s * h
    small, ks = put_frame(S, blank_packed(w, h, cx, cy, bits, msb, layout, 0))
    out, ko = put_frame(S, blank_packed(Wc, Hc, cx, cy, bits, msb, layout, 3))
    nb_up = S.upscale_yuv_workspace_bytes(net, w, h, s)
    nb_q = S.quality_frame_workspace_bytes(Wc, Hc, cx, cy, shave)
    ws_up = torch.empty(nb_up, dtype=torch.uint8, device="cuda")
    ws_q = torch.empty(nb_q, dtype=torch.uint8, device="cuda")
    res = torch.full((16,), float("nan"), dtype=torch.float64, device="cuda")
    plane = torch.empty(Hc * Wc, dtype=torch.float32, device="cuda")
    S.downscale_frame(f, truth, small, W, Hh, s)
    S.upscale_frame(net, f, small, out, w, h, s, params, ws_up, nb_up)
    S.quality_frame(f, out, f, truth, Wc, Hc, shave, res, ws_q, nb_q)
    S.yuv_upscale_luma16(small.y, small.pitch_y, plane, w, h, s, 0, bits, msb, f.range)
    S.yuv_compose_luma16(plane, out.y, out.pitch_y, Wc, Hc, bits, msb, f.range)
    S.quality_frame(f, out, f, truth, Wc, Hc, shave, res[8:], ws_q, nb_q)
    return H(res)


EVAL_CASES = [  # fmt, W, H, cx, cy, s, net
    ("yuv8", 75, 53, 2, 2, 2, "default"), ("yuv8", 75, 53, 2, 2, 3, "example"), ("p10", 40, 31, 1, 1, 2, "default"),
    ("P010", 75, 53, 2, 2, 2, "example"), ("NV12", 47, 35, 2, 1, 4, "default")]


@pytest.mark.parametrize("fmt,W,Hh,cx,cy,s,net", EVAL_CASES)
def test_evaluate_frame_is_its_calls(S, fmt, W, Hh, cx, cy, s, net):
    """Result for result bit-identical to downscale_frame -> upscale_frame ->
    quality_frame -> yuv_upscale_luma16 (pad 0) -> yuv_compose_luma16 ->
    quality_frame, on an exact-size workspace holding zeros, NaN and +1e30 with
    guard bands around the truth's planes, params, result and ws.  At 75 x 53
    the crop rule bites (chroma 38 -> 19 at s = 2, 38 -> 13 at s = 3) and Wc <
    W or Hc < H: the truth is read at its own pitches."""
    bits, msb, layout = FRAME_FORMATS[fmt]
    cfg = NETS[net]
    n = S.Net(*cfg)
    shave = 3
    f = S.yuv_format(bits, msb, layout, cx, cy, S.YUV_LIMITED)
    A = frame_values(W, Hh, cx, cy, bits, W + s)
    tp = QF.pack(A, bits, msb, layout, cx, cy, 3, 3, np.random.default_rng(2))
    params = make_params(np.random.default_rng(5), cfg, sd=0.05)
    truth, keep = put_frame(S, tp)
    want = chain(S, n, f, FRAME_FORMATS[fmt], truth, tp, W, Hh, s, shave, torch.from_numpy(params).cuda())
    assert np.isfinite(want[[0, 2, 3, 5, 8, 10]]).all() and want[8] > 0, want
    assert np.array_equal(want[3:7], want[11:15]), "the chroma numbers of the two halves differ"
    nbytes = S.evaluate_frame_workspace_bytes(n, f, W, Hh, s)
    assert nbytes > 0 and nbytes % 256 == 0
    print("evaluate_frame %s %dx%d /%d %s: net psnr_y %.3f dB, bicubic %.3f dB, workspace %d B"
          % (fmt, W, Hh, s, net, want[1], want[9], nbytes))
    for fill in (0.0,) + hip_util.POISONS:
        gt, gk = put_frame(S, tp, fill)
        pd, ws, res = guarded(params, fill), guarded(nbytes // 4, fill), guarded(32, fill)
        S.evaluate_frame(n, f, gt, W, Hh, s, shave, pd, res, ws, nbytes)
        got = H(res).view(np.float64)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (fill, got, want)
        guards_intact(*[t for t in gk if t is not None], pd, ws, res)
        assert hip_util.same_bits(H(pd), params)
        for t, a in zip(gk, (tp.y, tp.u, tp.v)):
            assert a is None or np.array_equal(H(t.view(torch.uint8))[:a.size], a), "the truth was written"
    with pytest.raises(S.SrcnnError) as e:
        S.evaluate_frame(n, f, gt, W, Hh, s, shave, pd, res, ws, nbytes - 1)
    assert e.value.code == S.ERR_WORKSPACE


@pytest.mark.parametrize("fmt", ["yuv8", "P010"])
def test_evaluate_frame_scale_1_bicubic_is_the_truth(S, fmt):
    bits, msb, layout = FRAME_FORMATS[fmt]
    n = S.Net(*NETS["default"])
    W, Hh = 38, 22
    f = S.yuv_format(bits, msb, layout, 2, 2, S.YUV_FULL)
    tp = QF.pack(frame_values(W, Hh, 2, 2, bits, 3), bits, msb, layout, 2, 2, 3, 3, np.random.default_rng(2))
    truth, keep = put_frame(S, tp)
    params = torch.from_numpy(make_params(np.random.default_rng(5), NETS["default"], sd=0.05)).cuda()
    nbytes = S.evaluate_frame_workspace_bytes(n, f, W, Hh, 1)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    res = torch.full((16,), float("nan"), dtype=torch.float64, device="cuda")
    S.evaluate_frame(n, f, truth, W, Hh, 1, 0, params, res, ws, nbytes)
    inf = float("inf")
    got = H(res)
    assert got[8:].tolist() == [0.0, inf, 1.0, 0.0, inf, 0.0, inf, inf], got
    assert got[3:7].tolist() == [0.0, inf, 0.0, inf] and got[0] > 0


# ---- 8: preload, then a first plane ----
def test_preload_then_first_plane(S):
    S.preload(S.Net(*NETS["default"]))
    seed = F.seed_of(5, 4, 2, "exact", 10)
    vals, q, raw, near = F.reference(5, 4, 2, "exact", 10, seed)
    got = gpu_down(S, D.encode(vals, 10, 1), 2, 5, 4, 10, 1, "semi", True)
    assert np.array_equal(got[~near], D.encode(q, 10, 1)[~near])


# ---- 9: the command line on tiny Y4M files ----
import json  # noqa: E402
import os  # noqa: E402
import subprocess  # noqa: E402

from conftest import ROOT  # noqa: E402

CNN = os.path.join(ROOT, "cnn-super-resolution_amd", "bin", "cnn")
Y4M = {"yuv8": ("C420jpeg", 8), "p10": ("C420p10", 10)}


def run_cnn(*args, ok=True):
    p = subprocess.run([CNN, *[str(a) for a in args]], capture_output=True, text=True, timeout=120)
    assert (p.returncode == 0) == ok, p.stdout + p.stderr
    return p


def y4m_frames(W, Hh, bits, n, seed):
    """n different 4:2:0 frames of smooth code values, each (Y, U, V)"""
    return [frame_values(W, Hh, 2, 2, bits, seed + k) for k in range(n)]


def write_y4m(path, W, Hh, token, bits, frames):
    dt = np.uint8 if bits == 8 else "<u2"
    head = ("YUV4MPEG2 W%d H%d F30000:1001 Ip A1:1 %s XCOLORRANGE=FULL\n" % (W, Hh, token)).encode()
    path.write_bytes(head + b"".join(b"FRAME\n" + b"".join(p.astype(dt).tobytes() for p in A) for A in frames))


def read_y4m(path, bits):
    """(header tokens, [(Y, U, V)]) of a 4:2:0 stream"""
    b = path.read_bytes()
    line, body = b.split(b"\n", 1)
    tokens = line.decode().split()
    W, Hh = int([t for t in tokens if t[0] == "W"][0][1:]), int([t for t in tokens if t[0] == "H"][0][1:])
    B = G.nbytes_of(bits)
    ch, cw = QF.chroma_shape(W, Hh, 2, 2)
    fb = B * (W * Hh + 2 * cw * ch)
    assert len(body) % (6 + fb) == 0
    frames = []
    for i in range(0, len(body), 6 + fb):
        assert body[i:i + 6] == b"FRAME\n"
        a = np.frombuffer(body[i + 6:i + 6 + fb], np.uint8 if bits == 8 else "<u2").astype(np.int64)
        frames.append((a[:W * Hh].reshape(Hh, W), a[W * Hh:W * Hh + cw * ch].reshape(ch, cw),
                       a[W * Hh + cw * ch:].reshape(ch, cw)))
    return tokens, frames


def write_net(tmp_path, cfg=NETS["default"], seed=3):
    """config.json with a parameters file -> (path, the flat parameters)"""
    import srcnn_amd
    params = make_params(np.random.default_rng(seed), cfg, sd=0.05)
    off = srcnn_amd.net_offsets(srcnn_amd.Net(*cfg)) + [params.size]
    layers = {"layer%d" % (i + 1): {"weights": [float(v) for v in params[off[2 * i]:off[2 * i + 1]]],
                                    "bias": [float(v) for v in params[off[2 * i + 1]:off[2 * i + 2]]]}
              for i in range(3)}
    (tmp_path / "params.json").write_text(json.dumps(dict(epochs=0, **layers)))
    conf = dict(zip(("n1", "n2", "f1", "f2", "f3"), cfg), momentum=0.9, weight_decay_parameter=0.001,
                learning_rates=[0.001, 0.001, 0.0001], parameters_file=str(tmp_path / "params.json"))
    for i in (1, 2, 3):
        conf["parameters_distribution_%d" % i] = {"mean_w": 0.0, "mean_b": 0.0, "std_deviation_w": 0.01,
                                                  "std_deviation_b": 0.0}
    (tmp_path / "config.json").write_text(json.dumps(conf))
    return tmp_path / "config.json", params


def abi_downscale_frame(S, A, W, Hh, s, bits):
    f = S.yuv_format(bits, 0, S.YUV_PLANAR, 2, 2, S.YUV_FULL)
    src, keep = put_frame(S, QF.pack(A, bits, 0, 0, 2, 2))
    dp = blank_packed(W // s, Hh // s, 2, 2, bits, 0, 0, 0)
    dst, dt = put_frame(S, dp)
    S.downscale_frame(f, src, dst, W, Hh, s)
    return read_frame(dp, dt, "downscale_frame")


@pytest.mark.parametrize("fmt,s", [("yuv8", 2), ("p10", 3)])
def test_cli_downscale_y4m(S, tmp_path, fmt, s):
    """`cnn downscale` on 3 frames of 48 x 36: every output frame is
    srcnn_downscale_frame's, the header repeats F, I, A, C and XCOLORRANGE with
    the new W and H; --frames 2 stops after two; the small stream then goes
    through `cnn upscale --ref` against the source end to end."""
    token, bits = Y4M[fmt]
    W, Hh, n = 48, 36, 3
    frames = y4m_frames(W, Hh, bits, n, 40)
    big, small = tmp_path / "big.y4m", tmp_path / "small.y4m"
    write_y4m(big, W, Hh, token, bits, frames)
    p = run_cnn("downscale", "-i", big, "-o", small, "--scale", s)  # (no -c)
    assert "Frames: 3" in p.stdout
    tokens, got = read_y4m(small, bits)
    assert tokens[0] == "YUV4MPEG2" and "W%d" % (W // s) in tokens and "H%d" % (Hh // s) in tokens
    for t in ("F30000:1001", "Ip", "A1:1", token, "XCOLORRANGE=FULL"):
        assert t in tokens, tokens
    assert len(got) == n
    for k in range(n):
        want = abi_downscale_frame(S, frames[k], W, Hh, s, bits)
        for a, b in zip(got[k], want):
            assert np.array_equal(a, b), "frame %d differs from srcnn_downscale_frame's" % k
    two = tmp_path / "two.y4m"
    p = run_cnn("downscale", "-i", big, "-o", two, "--scale", s, "--frames", 2)
    assert "Frames: 2" in p.stdout and two.read_bytes() == small.read_bytes()[:len(two.read_bytes())]
    assert len(read_y4m(two, bits)[1]) == 2
    cfg, _ = write_net(tmp_path)
    p = run_cnn("upscale", "-c", cfg, "-i", small, "--scale", s, "--ref", big, "-o", tmp_path / "back.y4m")
    assert "stream, 3 frames: psnr y" in p.stdout, p.stdout
    assert read_y4m(tmp_path / "back.y4m", bits)[0][1:3] == ["W48", "H36"]
    p = run_cnn("downscale", "-i", big, "--scale", 4, "--frames", 1, "dry")
    assert "Frames: 1" in p.stdout


@pytest.mark.parametrize("fmt,s", [("yuv8", 2), ("p10", 3)])
def test_cli_evaluate_y4m(S, tmp_path, fmt, s):
    """`cnn evaluate` on a Y4M stream of 50 x 38 (odd chroma, Wc < W at s = 3):
    the JSON's numbers are srcnn_evaluate_frame's, frame by frame, and the
    stream summary is `cnn quality`'s."""
    token, bits = Y4M[fmt]
    W, Hh, n, shave = 50, 38, 3, 2
    frames = y4m_frames(W, Hh, bits, n, 60)
    truth, report = tmp_path / "truth.y4m", tmp_path / "report.json"
    write_y4m(truth, W, Hh, token, bits, frames)
    cfg, params = write_net(tmp_path)
    p = run_cnn("evaluate", "-c", cfg, "-i", truth, "--scale", s, "--shave", shave, "-o", report)
    rep = json.loads(report.read_text())
    net = S.Net(*NETS["default"])
    f = S.yuv_format(bits, 0, S.YUV_PLANAR, 2, 2, S.YUV_FULL)
    nbytes = S.evaluate_frame_workspace_bytes(net, f, W, Hh, s)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    pd = torch.from_numpy(params).cuda()
    keys = ["mse_y", "psnr_y", "ssim_y", "mse_u", "psnr_u", "mse_v", "psnr_v", "psnr_all"]
    assert rep["scale"] == s and rep["net"]["shave"] == shave and rep["net"]["bits"] == bits
    assert (rep["net"]["width"], rep["net"]["height"]) == (W // s * s, Hh // s * s)
    assert len(rep["net"]["frames"]) == len(rep["bicubic"]["frames"]) == len(rep["gain_db"]) == n
    mse = {"net": [], "bicubic": []}
    for k in range(n):
        t, keep = put_frame(S, QF.pack(frames[k], bits, 0, 0, 2, 2))
        res = torch.full((16,), float("nan"), dtype=torch.float64, device="cuda")
        S.evaluate_frame(net, f, t, W, Hh, s, shave, pd, res, ws, nbytes)
        want = H(res)
        for half, name in ((0, "net"), (8, "bicubic")):
            row = rep[name]["frames"][k]
            assert row["frame"] == k
            for i, key in enumerate(keys):
                assert row[key] == want[half + i], (k, name, key, row[key], want[half + i])
            mse[name].append(want[half])
        assert rep["gain_db"][k] == want[1] - want[9]
        assert "frame %d gain:" % k in p.stdout
    peak2 = float((1 << bits) - 1) ** 2
    for name in ("net", "bicubic"):
        assert rep[name]["stream"]["count"] == n
        assert np.isclose(rep[name]["stream"]["psnr_y"], 10 * np.log10(peak2 / np.mean(mse[name])), rtol=1e-12)
    assert np.isclose(rep["stream_gain_db"], rep["net"]["stream"]["psnr_y"] - rep["bicubic"]["stream"]["psnr_y"])
    assert "stream net, 3 frames: psnr y" in p.stdout and "stream bicubic, 3 frames: psnr y" in p.stdout
    p = run_cnn("evaluate", "-c", cfg, "-i", truth, "--scale", s, "--frames", 1)
    assert "stream net, 1 frames" in p.stdout


def test_cli_train_from_y4m(S, tmp_path):
    """A directory of one PNG (80 x 60) and one Y4M of four 64 x 64 frames: 8 + 4
    x 9 pairs from 5 images; the pooled and the --device-batches runs write the
    same parameters file byte for byte; --frame-step 2 takes frames 0 and 2."""
    from PIL import Image
    from test_pairs_gpu import smooth_rgb, write_config
    cfg = write_config(tmp_path)
    d = tmp_path / "images"
    d.mkdir()
    Image.fromarray(smooth_rgb(80, 60, 1)).save(d / "a.png")
    write_y4m(d / "v.y4m", 64, 64, "C420jpeg", 8, y4m_frames(64, 64, 8, 4, 80))
    assert S.make_pairs_count(80, 60, 2, 33, 14)[0] == 8 and S.make_pairs_count(64, 64, 2, 33, 14)[0] == 9
    outs = []
    for name, extra in (("pooled.json", ()), ("device.json", ("--device-batches",))):
        out = tmp_path / name
        p = run_cnn("train", "--from-images", "-c", cfg, "-i", d, "-o", out, "--scale", 2, "--tile", 33, "--stride",
                    14, "-e", 2, "--seed", 7, *extra)
        assert "created 44 sample pairs from 5 images" in p.stdout, p.stdout
        assert "DONE" in p.stdout
        outs.append(out.read_bytes())
        assert json.loads(outs[-1])["epochs"] == 2
    assert outs[0] == outs[1], "the pooled and the --device-batches runs differ"
    p = run_cnn("train", "--from-images", "-c", cfg, "-i", d, "-o", tmp_path / "step.json", "--scale", 2, "-e", 1,
                "--seed", 7, "--frame-step", 2)
    assert "created 26 sample pairs from 3 images" in p.stdout, p.stdout
    p = run_cnn("train", "--from-images", "-c", cfg, "-i", d, "-o", tmp_path / "aug.json", "--scale", 2, "-e", 1,
                "--seed", 7, "--augment", "--random-origins", "--frame-step", 3)
    assert "created 26 sample pairs from 3 images" in p.stdout, p.stdout
