"""PSNR and SSIM of Y'CbCr frames on the GPU (csrc/hip/quality.hip, DESIGN.md
17): srcnn_quality_frame against the numpy yardstick
(tests/quality_frame_ref.py) -- the mse values bit for bit, the SSIM within
the bounds tests/test_quality_frame_cpu.py derives -- its exact anchors
(identical frames, the layouts, the shave as a pointer offset, repeatability),
the memory contract of include/srcnn.h, the argument checks, and `cnn quality`
/ `cnn upscale --ref` on Y4M streams.

The luma windows are quality_ref.SHAPES against quality_tiles' 32 x 32 tile
(one window, one tile plus halo, one sample more each way, ragged multi-tile),
each with a shaved ring of 3 and pitches above the row bytes; every case has
its own pair of (msb, layout) combinations for a and b.

Measured on one MI355X against the float64 yardstick: SSIM off by at most
9.83e-7 on the structured pairs (bound 4.0e-6) and 4.13e-5 on the flat ones
(bound 1.7e-4); every mse equal to float(S) / float(N)."""
import functools
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

import hip_util
import quality_frame_ref as F
import quality_ref as Q
from conftest import ROOT
from hip_util import H, guarded, guards_intact, make_params
from step_util import S, _settings  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CNN = os.path.join(ROOT, "cnn-super-resolution_amd", "bin", "cnn")
INF = float("inf")
EXACT_SAME = [0.0, INF, 1.0, 0.0, INF, 0.0, INF, INF]
GUARD = 4096  # bytes in front of and behind every placed plane


class Placed:
    """A Packed frame on the device: each plane inside `GUARD` random bytes on
    either side, in an allocation of its own.  unchanged() compares every
    allocation with what was uploaded: the guard bands and the frame."""

    def __init__(self, S, p, seed):
        rng = np.random.default_rng(seed)
        self.host, self.dev, addr = [], [], []
        for plane in (p.y, p.u, p.v):
            if plane is None:
                addr.append(None)
                continue
            buf = rng.integers(0, 256, 2 * GUARD + plane.size, dtype=np.uint8)
            buf[GUARD:GUARD + plane.size] = plane
            t = torch.from_numpy(buf).cuda()
            assert t.data_ptr() % 256 == 0
            self.host.append(buf)
            self.dev.append(t)
            addr.append(t.data_ptr() + GUARD)
        self.addr = addr
        self.frame = S.yuv_frame(addr[0], addr[1], addr[2], p.pitch_y, p.pitch_c)
        self.fmt = S.yuv_format(p.bits, p.msb, p.layout, p.cx, p.cy, S.YUV_LIMITED)

    def unchanged(self):
        torch.cuda.synchronize()
        return all(np.array_equal(t.cpu().numpy(), h) for t, h in zip(self.dev, self.host))


def run(S, pa, pb, w, h, shave, ws_fill=0x5A, cx=None, cy=None):
    """the 8 doubles of srcnn_quality_frame on two Placed frames, through a workspace of exactly the queried size"""
    cx, cy = cx or pa.fmt.cx, cy or pa.fmt.cy
    nbytes = S.quality_frame_workspace_bytes(w, h, cx, cy, shave)
    assert nbytes > 0 and nbytes % 256 == 0
    ws = torch.full((nbytes,), ws_fill, dtype=torch.uint8, device="cuda")
    res = torch.full((8,), float("nan"), dtype=torch.float64, device="cuda")
    S.quality_frame(pa.fmt, pa.frame, pb.fmt, pb.frame, w, h, shave, res, ws, nbytes)
    return H(res)


def gpu_quality_frame(S, A, B, bits, cx, cy, shave, la=(0, F.YUV_PLANAR), lb=(0, F.YUV_PLANAR), extra=((5, 3), (2, 7)),
                      seeds=(1, 2), ws_fill=0x5A):
    h, w = A[0].shape
    pa = Placed(S, F.pack(A, bits, la[0], la[1], cx, cy, *extra[0], rng=np.random.default_rng(seeds[0])), seeds[0])
    pb = Placed(S, F.pack(B, bits, lb[0], lb[1], cx, cy, *extra[1], rng=np.random.default_rng(seeds[1])), seeds[1])
    r = run(S, pa, pb, w, h, shave, ws_fill)
    assert pa.unchanged() and pb.unchanged()
    return r


def bits_of(r):
    return np.ascontiguousarray(r, np.float64).view(np.int64).tolist()


@functools.lru_cache(maxsize=None)
def all_cases():
    """{name: (A, B, bits, cx, cy, shave, flat, index, (sums, the float64 yardstick's 8 doubles))}, computed once"""
    out = {}
    for flat, cs in ((False, F.cases()), (True, F.flat_cases())):
        for name, A, B, bits, cx, cy, k in cs:
            out[name] = (A, B, bits, cx, cy, k, flat, len(out), F.quality_frame(A, B, bits, cx, cy, k))
    return out


CASE_NAMES = [c[0] for c in F.cases()] + [c[0] for c in F.flat_cases()]


def check_against_sums(r, sums, bits, what=""):
    """mse bit for bit from the integer sums, every psnr on the device's own mse"""
    peak2 = float(2 ** bits - 1) ** 2
    for i, (Sp, Np) in zip((0, 3, 5), sums):
        assert r[i] == float(Sp) / float(Np), (what, i, r[i], Sp, Np)
        want = INF if r[i] == 0 else 10 * math.log10(peak2 / r[i])
        assert r[i + 1] == want or abs(r[i + 1] - want) <= 1e-12 * abs(want), (what, i, r[i + 1], want)
    mse_all = F.mse_all_of(sums)
    want = INF if mse_all == 0 else 10 * math.log10(peak2 / mse_all)
    assert r[7] == want or abs(r[7] - want) <= 1e-12 * abs(want), (what, r[7], want)


# ---- 1: against the reference ----
@pytest.mark.parametrize("name", CASE_NAMES)
def test_quality_frame_vs_reference(S, name):
    A, B, bits, cx, cy, k, flat, idx, (sums, ref) = all_cases()[name]
    la, lb = F.layouts_of(idx, bits)
    r = gpu_quality_frame(S, A, B, bits, cx, cy, k, la, lb)
    tol = F.SSIM_ATOL_FLAT if flat else F.SSIM_ATOL
    e = abs(r[2] - ref[2])
    print("%s a%s b%s: mse y %.9g u %.9g v %.9g psnr all %.6f ssim %.9f (err %.3e, bound %.1e)" % (
        name, la, lb, r[0], r[3], r[5], r[7], r[2], e, tol))
    hip_util.log_record({"what": "quality_frame " + name, "e_ssim": e})
    check_against_sums(r, sums, bits, name)
    assert e <= tol


def test_shave_3_drops_two_chroma_samples_at_420(S):
    """ceil(3 / 2) = 2 columns and rows of chroma per side"""
    A, B, bits, cx, cy, k, _, _, _ = all_cases()["75x59_10b_420"]
    assert (k, cx, cy) == (3, 2, 2)
    r = gpu_quality_frame(S, A, B, bits, cx, cy, k)
    for i, p in ((3, 1), (5, 2)):
        d = A[p][2:-2, 2:-2] - B[p][2:-2, 2:-2]
        assert r[i] == float(int((d * d).sum())) / float(d.size)
        d1 = A[p][1:-1, 1:-1] - B[p][1:-1, 1:-1]
        assert r[i] != float(int((d1 * d1).sum())) / float(d1.size)


# ---- 2: exact anchors ----
@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("w,h", [(11, 11), (Q.TILE + 11, Q.TILE + 11), (75, 59)])
def test_identical_frames_are_exact(S, w, h, bits):
    rng = np.random.default_rng(7)
    for (sub, (cx, cy)), la, lb in zip(F.SUBSAMPLINGS.items(), ((0, 0), (1, 1), (0, 1)), ((0, 1), (0, 0), (1, 1))):
        ch, cw = F.chroma_shape(w, h, cx, cy)
        A = tuple(rng.integers(0, 2 ** bits, s) for s in ((h, w), (ch, cw), (ch, cw)))
        la, lb = ((la[0] if bits > 8 else 0, la[1]), (lb[0] if bits > 8 else 0, lb[1]))
        r = gpu_quality_frame(S, A, A, bits, cx, cy, 0, la, lb)
        assert r.tolist() == EXACT_SAME, (sub, la, lb, r)


@pytest.mark.parametrize("bits", [8, 10, 16])
def test_layout_does_not_change_the_bits(S, bits):
    """planar against planar = P010 style (msb 1, semi-planar) against planar =
    semi-planar against semi-planar, all 8 doubles; at 8 bits NV12 against planar"""
    A, B, _, cx, cy, k, _, _, _ = all_cases()["75x59_%db_420" % bits]
    P, SP = F.YUV_PLANAR, F.YUV_SEMIPLANAR
    first = gpu_quality_frame(S, A, B, bits, cx, cy, k, (0, P), (0, P))
    assert np.isfinite(first).all() and first[0] > 0 and first[3] > 0 and first[5] > 0
    m = 1 if bits > 8 else 0
    others = [((m, SP), (0, P)), ((0, SP), (0, SP)), ((0, P), (m, SP))] + ([((1, P), (1, SP))] if m else [])
    for n, (la, lb) in enumerate(others):
        r = gpu_quality_frame(S, A, B, bits, cx, cy, k, la, lb, extra=((n, 9), (4, n)), ws_fill=(0x00, 0xFF)[n % 2])
        assert bits_of(r) == bits_of(first), (la, lb, r, first)


@pytest.mark.parametrize("name", ["43x43_10b_420", "75x59_8b_422", "135x37_16b_444", "11x11_12b_420"])
def test_luma_shave_is_a_pointer_offset(S, name):
    """The luma results with shave = k are bit-identical to the call on the
    pointer-offset interior with shave = 0, whatever b's outer ring holds, and
    from call to call."""
    A, B, bits, cx, cy, k, _, idx, _ = all_cases()[name]
    la, lb = F.layouts_of(idx, bits)
    h, w = A[0].shape
    first = gpu_quality_frame(S, A, B, bits, cx, cy, k, la, lb)
    assert np.isfinite(first).all() and first[0] > 0
    rng = np.random.default_rng(9)
    Bg = tuple(p.copy() for p in B)
    ring = np.ones((h, w), bool)
    ring[k:-k, k:-k] = False
    Bg[0][ring] = rng.integers(0, 2 ** bits, int(ring.sum()))
    assert not np.array_equal(Bg[0], B[0])
    other = gpu_quality_frame(S, A, Bg, bits, cx, cy, k, la, lb, extra=((9, 0), (0, 4)), ws_fill=0xFF)
    assert bits_of(other) == bits_of(first)
    # the interior through a pointer offset, shave 0; the chroma planes stay where they are
    Bsz = 1 if bits == 8 else 2
    pa = Placed(S, F.pack(A, bits, la[0], la[1], cx, cy, 4, 2, np.random.default_rng(5)), 5)
    pb = Placed(S, F.pack(Bg, bits, lb[0], lb[1], cx, cy, 6, 0, np.random.default_rng(6)), 6)
    again = run(S, pa, pb, w, h, k)
    for p in (pa, pb):
        p.frame.y = p.addr[0] + k * p.frame.pitch_y + k * Bsz
    inner = run(S, pa, pb, w - 2 * k, h - 2 * k, 0)
    assert bits_of(again) == bits_of(first)
    assert bits_of(inner[:3]) == bits_of(first[:3]), (inner, first)


# ---- 3: the memory contract ----
def test_quality_frame_memory(S):
    """Exact-size workspaces holding 0x00, 0xFF and 0x5A, guard bands around
    the result and the workspace (NaN and +1e30) and around every plane
    (random bytes, different for a and b), pitches above the row bytes: all 8
    doubles are the tight-pitch call's, bit for bit, and nothing but the result
    and the workspace changes."""
    w, h, bits, cx, cy, k = 81, 64, 10, 2, 2, 1
    rng = np.random.default_rng(21)
    A = F.make_frame(rng, w, h, cx, cy, bits)
    B = F.make_frame(rng, w, h, cx, cy, bits, like=A, noise=30.0)
    sums, ref = F.quality_frame(A, B, bits, cx, cy, k)
    tight = gpu_quality_frame(S, A, B, bits, cx, cy, k, (1, F.YUV_SEMIPLANAR), (0, F.YUV_PLANAR), extra=((0, 0), (0, 0)))
    check_against_sums(tight, sums, bits)
    nbytes = S.quality_frame_workspace_bytes(w, h, cx, cy, k)
    assert nbytes == 256 * ((16 * (3 * 2 + 1 * 2) + 255) // 256)  # 3 x 2 luma tiles, 1 x 2 chroma tiles per plane
    for n, (byte, fill) in enumerate(zip((0x00, 0xFF, 0x5A), (0.0,) + hip_util.POISONS)):
        pa = Placed(S, F.pack(A, bits, 1, F.YUV_SEMIPLANAR, cx, cy, 7, 5, np.random.default_rng(30 + n)), 40 + n)
        pb = Placed(S, F.pack(B, bits, 0, F.YUV_PLANAR, cx, cy, 3, 11, np.random.default_rng(50 + n)), 60 + n)
        res = guarded(16, fill, inner=float("nan"))
        ws = guarded(nbytes // 4, fill)
        ws.view(torch.uint8).fill_(byte)
        S.quality_frame(pa.fmt, pa.frame, pb.fmt, pb.frame, w, h, k, res, ws, nbytes)
        r = H(res).view(np.float64)
        guards_intact(res, ws)
        assert pa.unchanged() and pb.unchanged()
        assert bits_of(r) == bits_of(tight), (byte, r, tight)
    assert abs(tight[2] - ref[2]) <= F.SSIM_ATOL


# ---- 4: invalid arguments ----
def test_invalid_arguments(S):
    """every mutation of tests/quality_frame_ref.py INVALID on real buffers;
    all are refused before a launch, so nothing is read or written"""
    rng = np.random.default_rng(3)
    A = F.make_frame(rng, 23, 23, 2, 2, 10)
    pa, pb = (Placed(S, F.pack(A, 10, 0, F.YUV_PLANAR, 2, 2), s) for s in (1, 2))
    res = torch.full((16,), 7.0, dtype=torch.float64, device="cuda")
    ws = torch.zeros(4096, dtype=torch.uint8, device="cuda")

    def args():
        g = F.base_args(S, result=res.data_ptr(), ws=ws.data_ptr())
        for key, p in (("a", pa), ("b", pb)):
            g[key].update(y=p.addr[0], u=p.addr[1], v=p.addr[2])
        return g

    F.call(S, args())  # the base is valid
    assert H(res)[:8].tolist() == EXACT_SAME
    res.fill_(7.0)
    for name, mutate in F.INVALID.items():
        g = args()
        mutate(g)
        with pytest.raises(S.SrcnnError) as e:
            F.call(S, g)
        assert e.value.code == S.ERR_INVALID, (name, S.last_error())
    g = args()
    g["ws_bytes"] -= 1
    with pytest.raises(S.SrcnnError) as e:
        F.call(S, g)
    assert e.value.code == S.ERR_WORKSPACE
    assert (H(res) == 7.0).all() and pa.unchanged() and pb.unchanged()


# ---- 5: the command line ----
Y4M_TOKEN = {(8, "420"): "C420jpeg", (10, "420"): "C420p10"}


def write_y4m(path, frames, w, h, bits, sub="420"):
    """frames: [(Y, U, V)] of code values; planar, the code in the low bits"""
    cx, cy = F.SUBSAMPLINGS[sub]
    with open(path, "wb") as fh:
        fh.write(("YUV4MPEG2 W%d H%d F25:1 Ip A1:1 %s\n" % (w, h, Y4M_TOKEN[(bits, sub)])).encode())
        for A in frames:
            p = F.pack(A, bits, 0, F.YUV_PLANAR, cx, cy)
            fh.write(b"FRAME\n" + p.y.tobytes() + p.u.tobytes() + p.v.tobytes())


def read_y4m(path, bits, sub="420"):
    cx, cy = F.SUBSAMPLINGS[sub]
    data = open(path, "rb").read()
    head, _, rest = data.partition(b"\n")
    tok = dict((t[:1].decode(), t[1:].decode()) for t in head.split()[1:])
    w, h = int(tok["W"]), int(tok["H"])
    ch, cw = F.chroma_shape(w, h, cx, cy)
    B = 1 if bits == 8 else 2
    n = (w * h + 2 * cw * ch) * B
    frames = []
    while rest:
        assert rest.startswith(b"FRAME\n")
        body = np.frombuffer(rest[6:6 + n], np.uint8)
        rest = rest[6 + n:]
        p = F.Packed(body[:w * h * B], body[w * h * B:(w * h + cw * ch) * B], body[(w * h + cw * ch) * B:], w * B,
                     cw * B, bits, 0, F.YUV_PLANAR, w, h, cx, cy)
        frames.append(F.unpack(p))
    return w, h, frames


def cnn(*args):
    return subprocess.run([CNN, *args], capture_output=True, text=True, timeout=120)


FRAME_LINE = re.compile(r"^frame (\d+): psnr y (\S+) dB u (\S+) dB v (\S+) dB all (\S+) dB ssim (\S+)$", re.M)
MSE_LINE = re.compile(r"^stream, (\d+) frames: mse y (\S+) u (\S+) v (\S+) all (\S+)$", re.M)
PSNR_LINE = re.compile(r"^stream, (\d+) frames: psnr y (\S+) dB u (\S+) dB v (\S+) dB all (\S+) dB ssim (\S+)$", re.M)
LOW_LINE = re.compile(r"^lowest psnr y: (\S+) dB at frame (\d+)$", re.M)


def stream_frames(rng, n, w, h, bits, sub="420", noise=6.0):
    cx, cy = F.SUBSAMPLINGS[sub]
    a = [F.make_frame(rng, w, h, cx, cy, bits) for _ in range(n)]
    b = [F.make_frame(rng, w, h, cx, cy, bits, like=x, noise=noise * (i + 1) * 2 ** (bits - 8)) for i, x in enumerate(a)]
    return a, b


def close(got, want):
    return got == want or abs(got - want) <= 1e-12 * abs(want)


def check_stream_lines(stdout, rows, w, h, bits, sub, shave):
    """the stream's lines against the stated aggregation of the per-frame doubles `rows`"""
    cx, cy = F.SUBSAMPLINGS[sub]
    ch, cw = F.chroma_shape(w, h, cx, cy)
    sx, sy = F.ceil_div(shave, cx), F.ceil_div(shave, cy)
    ny, nc = (w - 2 * shave) * (h - 2 * shave), (cw - 2 * sx) * (ch - 2 * sy)
    peak2 = float(2 ** bits - 1) ** 2
    ps = lambda m: INF if m == 0 else 10 * math.log10(peak2 / m)
    n = len(rows)
    mse = [sum(r[i] for r in rows) / n for i in (0, 3, 5)]
    mse_all = sum((r[0] * ny + r[3] * nc + r[5] * nc) / (ny + 2 * nc) for r in rows) / n
    m = MSE_LINE.search(stdout)
    assert m and int(m.group(1)) == n, stdout
    for got, want in zip(m.groups()[1:], mse + [mse_all]):
        assert close(float(got), want), (got, want)
    m = PSNR_LINE.search(stdout)
    assert m and int(m.group(1)) == n, stdout
    for got, want in zip(m.groups()[1:], [ps(x) for x in mse] + [ps(mse_all), sum(r[2] for r in rows) / n]):
        assert close(float(got), want), (got, want)
    m = LOW_LINE.search(stdout)
    low = min(range(n), key=lambda i: rows[i][1])
    assert m and float(m.group(1)) == rows[low][1] and int(m.group(2)) == low, stdout
    return mse, mse_all


@pytest.mark.parametrize("bits", [10, 8])
def test_cli_quality_y4m(S, tmp_path, bits):
    w, h, sub, shave = 48, 36, "420", 2
    a, b = stream_frames(np.random.default_rng(bits), 3, w, h, bits)
    fa, fb = str(tmp_path / "a.y4m"), str(tmp_path / "b.y4m")
    write_y4m(fa, a, w, h, bits)
    write_y4m(fb, b, w, h, bits)
    want = [gpu_quality_frame(S, x, y, bits, 2, 2, shave) for x, y in zip(a, b)]
    report = tmp_path / "report.json"
    p = cnn("quality", "-i", fa, "--ref", fb, "--shave", str(shave), "-o", str(report))
    assert p.returncode == 0, p.stdout + p.stderr
    lines = FRAME_LINE.findall(p.stdout)
    assert [int(l[0]) for l in lines] == [0, 1, 2], p.stdout
    for l, r in zip(lines, want):
        assert [float(v) for v in l[1:]] == [r[1], r[4], r[6], r[7], r[2]], (l, r)
    mse, mse_all = check_stream_lines(p.stdout, want, w, h, bits, sub, shave)
    rep = json.loads(report.read_text())
    assert (rep["width"], rep["height"], rep["bits"], rep["shave"]) == (w, h, bits, shave)
    keys = ["mse_y", "psnr_y", "ssim_y", "mse_u", "psnr_u", "mse_v", "psnr_v", "psnr_all"]
    for i, (fr, r) in enumerate(zip(rep["frames"], want)):
        assert fr["frame"] == i and [fr[k] for k in keys] == r.tolist()
    st = rep["stream"]
    assert st["count"] == 3 and close(st["mse_y"], mse[0]) and close(st["mse_all"], mse_all)
    assert close(st["ssim_y"], sum(r[2] for r in want) / 3) and st["min_psnr_y_frame"] == 2
    assert st["min_psnr_y"] == want[2][1]
    # --frames, and no report
    p = cnn("quality", "-i", fa, "--ref", fb, "--shave", str(shave), "--frames", "2")
    assert p.returncode == 0 and len(FRAME_LINE.findall(p.stdout)) == 2 and "stream, 2 frames" in p.stdout
    # a file against itself
    p = cnn("quality", "-i", fa, "--ref", fa)
    assert p.returncode == 0, p.stdout
    assert p.stdout.count("psnr y inf dB u inf dB v inf dB all inf dB ssim 1\n") == 4, p.stdout
    report.unlink()
    p = cnn("quality", "-i", fa, "--ref", fa, "-o", str(report))
    rep = json.loads(report.read_text())
    assert rep["frames"][0]["psnr_y"] is None and rep["frames"][0]["ssim_y"] == 1 and rep["stream"]["psnr_all"] is None


def test_cli_quality_y4m_errors(S, tmp_path):
    w, h = 48, 36
    a, b = stream_frames(np.random.default_rng(1), 3, w, h, 10)
    fa, fb, fc, fd = (str(tmp_path / n) for n in ("a.y4m", "b.y4m", "c.y4m", "d.y4m"))
    write_y4m(fa, a, w, h, 10)
    write_y4m(fb, b[:2], w, h, 10)          # shorter
    write_y4m(fc, [tuple(p[:34 // (1 if i == 0 else 2), :] for i, p in enumerate(x)) for x in b], w, 34, 10)
    a8, _ = stream_frames(np.random.default_rng(2), 1, w, h, 8)
    write_y4m(fd, a8, w, h, 8)              # another depth
    for other in (fc, fd):
        p = cnn("quality", "-i", fa, "--ref", other)
        assert p.returncode == 1 and p.stdout.count("[ERROR]") == 1 and "differ in size, subsampling or bit depth" in p.stdout
        assert not FRAME_LINE.search(p.stdout)
    p = cnn("quality", "-i", fa, "--ref", fb)
    assert p.returncode == 1 and len(FRAME_LINE.findall(p.stdout)) == 2, p.stdout
    assert "[ERROR] '%s' ends after 2 frames" % fb in p.stdout and "stream, 2 frames" in p.stdout
    p = cnn("quality", "-i", fb, "--ref", fa, "--frames", "2")  # --frames reached first: no error
    assert p.returncode == 0 and len(FRAME_LINE.findall(p.stdout)) == 2, p.stdout
    # a truncated frame ends the run with an error after the pairs in front of it
    data = open(fa, "rb").read()
    ft = str(tmp_path / "t.y4m")
    open(ft, "wb").write(data[:-100])
    p = cnn("quality", "-i", ft, "--ref", fa)
    assert p.returncode == 1 and len(FRAME_LINE.findall(p.stdout)) == 2 and "[ERROR] frame 2" in p.stdout, p.stdout
    # the window must hold an 11 x 11 SSIM window
    p = cnn("quality", "-i", fa, "--ref", fa, "--shave", "13")
    assert p.returncode == 1 and "[ERROR]" in p.stdout and "11x11" in p.stdout


def write_config(tmp_path, S):
    cfg = (64, 32, 9, 1, 5)
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
    return str(tmp_path / "config.json")


def test_cli_upscale_ref(S, tmp_path):
    """`cnn upscale --scale 2 --ref truth.y4m` prints, per frame and for the
    stream, exactly what `cnn quality` prints for the written output against
    the truth (shave defaults to the scale), with and without -o."""
    config = write_config(tmp_path, S)
    w, h, bits = 24, 18, 10
    small, _ = stream_frames(np.random.default_rng(4), 3, w, h, bits)
    truth, _ = stream_frames(np.random.default_rng(5), 3, 2 * w, 2 * h, bits)
    fs, ft, fo = (str(tmp_path / n) for n in ("small.y4m", "truth.y4m", "out.y4m"))
    write_y4m(fs, small, w, h, bits)
    write_y4m(ft, truth, 2 * w, 2 * h, bits)
    p = cnn("upscale", "-c", config, "-i", fs, "-o", fo, "--scale", "2", "--ref", ft)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "shave: 2" in p.stdout
    q = cnn("quality", "-i", fo, "--ref", ft, "--shave", "2")
    assert q.returncode == 0, q.stdout
    pick = lambda out: [l for l in out.splitlines() if l.startswith(("frame ", "stream, ", "lowest psnr"))]
    assert len(pick(p.stdout)) == 6 and pick(p.stdout) == pick(q.stdout), (p.stdout, q.stdout)
    # ... which are the binding's doubles on the written frames
    W, Hh, out_frames = read_y4m(fo, bits)
    want = [gpu_quality_frame(S, x, y, bits, 2, 2, 2) for x, y in zip(out_frames, truth)]
    for l, r in zip(FRAME_LINE.findall(p.stdout), want):
        assert [float(v) for v in l[1:]] == [r[1], r[4], r[6], r[7], r[2]]
    # without -o, one slot, another shave
    p1 = cnn("upscale", "-c", config, "-i", fs, "--scale", "2", "--ref", ft, "--slots", "1", "--shave", "0")
    q1 = cnn("quality", "-i", fo, "--ref", ft)
    assert p1.returncode == 0 and "Either provide out path" not in p1.stdout, p1.stdout
    assert len(pick(p1.stdout)) == 6 and pick(p1.stdout) == pick(q1.stdout)
    # a truth of another size: one error, before any frame
    p = cnn("upscale", "-c", config, "-i", fs, "-o", fo, "--scale", "2", "--ref", fs)
    assert p.returncode == 1 and p.stdout.count("[ERROR]") == 1 and "differ in size" in p.stdout
    assert not FRAME_LINE.search(p.stdout)
    # a shorter truth: the common frames, then the error
    write_y4m(ft, truth[:1], 2 * w, 2 * h, bits)
    p = cnn("upscale", "-c", config, "-i", fs, "-o", fo, "--scale", "2", "--ref", ft)
    assert p.returncode == 1 and len(FRAME_LINE.findall(p.stdout)) == 1 and "ends after 1 frames" in p.stdout
    # an image input
    p = cnn("upscale", "-c", config, "-i", config, "-o", fo, "--ref", ft)
    assert p.returncode == 1 and "--ref needs the quality mode, or the upscale mode with a Y4M input" in p.stdout
