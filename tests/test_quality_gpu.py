"""PSNR and SSIM on the GPU (csrc/hip/quality.hip): srcnn_quality against the
float64 yardstick (tests/quality_ref.py) within the tolerances
tests/test_quality_cpu.py derives, its exact anchors (identical images, the
shave as a pointer offset, repeatability), the memory contract of
include/srcnn.h, srcnn_evaluate against its six calls, and the `cnn` modes
built on them.

quality_tiles gives a workgroup a tile of 32 x 32 windows of the SSIM map,
i.e. 42 x 42 pixels with the halo (quality_ref.TILE), so the shapes after the
shave (quality_ref.SHAPES) are: one window (11 x 11); a few (12 x 13); exactly
one tile plus halo (42 x 42); one pixel more each way (43 x 43: four tiles,
three of them one window wide or high); ragged multi-tile (75 x 59: 3 x 2
tiles); wide and flat (135 x 37: 4 x 1).  Every case has pitches greater than
its width and a shaved ring of 3 pixels; the RGB8 bases sit at byte offsets 1,
2 and 3 mod 4.

Measured on one MI355X against the float64 yardstick: SSIM off by at most
4.05e-7 on the structured pairs (bound 2.0e-6) and 4.13e-5 on the flat ones
(bound 1.7e-4), mse by at most 1.87e-7 relative (bound 7.5e-7)."""
import functools
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

import hip_util
import quality_ref as Q
from conftest import ROOT
from hip_util import H, guarded, guards_intact, make_params
from step_util import S, _settings  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CNN = os.path.join(ROOT, "cnn-super-resolution_amd", "bin", "cnn")
NETS = {"default": (64, 32, 9, 1, 5), "wide": (128, 64, 9, 5, 5)}
INF = float("inf")


def fmt_of(img):
    return Q.PIX_LUMA_F32 if img.dtype == np.float32 else Q.PIX_RGB8 if img.shape[2] == 3 else Q.PIX_RGBA8


def place(img, extra=0, offset=0, seed=0):
    """The image on the device with a row pitch of W + extra pixels, starting
    `offset` bytes into its allocation, garbage in between and around (random
    bytes; NaN and +1e30 for a float plane).  Returns (address, format, pitch
    in pixels, the tensor that keeps it alive)."""
    fmt = fmt_of(img)
    h, w = img.shape[:2]
    pitch = w + extra
    rng = np.random.default_rng(seed)
    if fmt == Q.PIX_LUMA_F32:
        assert offset % 4 == 0
        host = np.where(rng.random(offset // 4 + h * pitch + 8) < 0.5, np.float32("nan"), np.float32(1e30))
        host = host.astype(np.float32)
        rows = host[offset // 4:offset // 4 + h * pitch].reshape(h, pitch)
        rows[:, :w] = img
    else:
        bpp = img.shape[2]
        host = rng.integers(0, 256, offset + h * pitch * bpp + 16, dtype=np.uint8)
        rows = host[offset:offset + h * pitch * bpp].reshape(h, pitch, bpp)
        rows[:, :w] = img
    t =torch.from_numpy(host).cuda()
    assert t.data_ptr() % 256 == 0
    return t.data_ptr() + offset, fmt, pitch, t


def gpu_quality(S, a, b, shave, extra=(5, 3), offsets=(0, 0), seeds=(1, 2), ws_fill=0x5A):
    """(mse, psnr, ssim) of srcnn_quality on freshly placed copies of a and b"""
    h, w = a.shape[:2]
    pa, fa, pita, ka = place(a, extra[0], offsets[0], seeds[0])
    pb, fb, pitb, kb = place(b, extra[1], offsets[1], seeds[1])
    return run_quality(S, pa, fa, pita, pb, fb, pitb, w, h, shave, ws_fill)


def run_quality(S, pa, fa, pita, pb, fb, pitb, w, h, shave, ws_fill=0x5A):
    nbytes = S.quality_workspace_bytes(w, h, shave)
    assert nbytes > 0 and nbytes % 256 == 0
    ws = torch.full((nbytes,), ws_fill, dtype=torch.uint8, device="cuda")
    res = torch.full((3,), float("nan"), dtype=torch.float64, device="cuda")
    S.quality(pa, fa, pita, pb, fb, pitb, w, h, shave, res, ws, nbytes)
    return H(res)


def bits(r):
    return np.ascontiguousarray(r, np.float64).view(np.int64).tolist()


@functools.lru_cache(maxsize=None)
def all_cases():
    """{name: (a, b, shave, flat, the float64 yardstick's (mse, psnr, ssim))}, computed once"""
    out = {}
    for flat, cs in ((False, Q.cases()), (True, Q.flat_cases())):
        for name, a, b, k in cs:
            out[name] = (a, b, k, flat, Q.quality(a, b, k))
    return out


CASE_NAMES = [c[0] for c in Q.cases()] + [c[0] for c in Q.flat_cases()]


# ---- 1: against the float64 yardstick ----
@pytest.mark.parametrize("name", CASE_NAMES)
def test_quality_vs_reference(S, name):
    a, b, k, flat, (mse64, psnr64, ssim64) = all_cases()[name]
    idx = CASE_NAMES.index(name)
    # an RGB8 base at 1, 2 or 3 bytes past a 4-byte boundary; the others 4-byte aligned
    offs = tuple(1 + (idx + j) % 3 if fmt_of(img) == Q.PIX_RGB8 else 4 * ((idx + j) % 3)
                 for j, img in enumerate((a, b)))
    mse, psnr, ssim = gpu_quality(S, a, b, k, extra=(5, 3), offsets=offs)
    tol = Q.SSIM_ATOL_FLAT if flat else Q.SSIM_ATOL
    e_ssim, e_mse = abs(ssim - ssim64), abs(mse - mse64) / mse64
    print("%s offsets %s: mse %.9g (rel err %.3e, bound %.1e) ssim %.9f (err %.3e, bound %.1e) psnr %.6f" % (
        name, offs, mse, e_mse, Q.MSE_RTOL, ssim, e_ssim, tol, psnr))
    hip_util.log_record({"what": "quality " + name, "e_ssim": e_ssim, "e_mse": e_mse})
    assert e_ssim <= tol
    assert e_mse <= Q.MSE_RTOL
    assert abs(psnr - 10 * math.log10(65025.0 / mse)) <= 1e-12 * abs(psnr)


# ---- 2: exact anchors ----
@pytest.mark.parametrize("w,h", [(11, 11), (Q.TILE + 11, Q.TILE + 11), (75, 59)])
def test_identical_images_are_exact(S, w, h):
    rng = np.random.default_rng(7)
    rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    rgba = np.concatenate([rgb, rng.integers(0, 256, (h, w, 1), dtype=np.uint8)], axis=-1)
    plane = rng.random((h, w)).astype(np.float32)
    for a, b, offs in ((rgb, rgb, (1, 3)), (rgb, rgba, (2, 0)), (rgba, rgba, (0, 8)), (plane, plane, (0, 4))):
        r = gpu_quality(S, a, b, 0, extra=(7, 2), offsets=offs)
        assert r.tolist() == [0.0, INF, 1.0], (fmt_of(a), fmt_of(b), r)


@pytest.mark.parametrize("p,q", [(10, 20), (250, 251), (0, 255), (77, 200), (255, 254)])
def test_constant_grey_pairs_match_the_closed_form(S, p, q):
    """Y = 0.299f p + 0.587f p + 0.114f p; the device's luma is that sum with
    three roundings, each at most 2^-24 x 255, so d = Ya - Yb is within 1e-4 of
    the exact difference and the mse within 2 x 1e-4 / |p - q| relative.  The
    ssim is (2 Ya Yb + C1) / (Ya^2 + Yb^2 + C1) up to the flat inputs' bound
    plus what the window's sum (1 - 1.4e-9 per axis) leaves of the variance
    terms (tests/test_quality_cpu.py derives that term)."""
    w, h = 75, 59
    a, b = np.full((h, w, 3), p, np.uint8), np.full((h, w, 4), q, np.uint8)
    k = [np.float64(np.float32(c)) for c in (0.299, 0.587, 0.114)]
    Ya, Yb = sum(k) * p, sum(k) * q
    C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    mse_cf, ssim_cf = (Ya - Yb) ** 2, (2 * Ya * Yb + C1) / (Ya * Ya + Yb * Yb + C1)
    s = float(Q.gauss_table().astype(np.float64).sum())
    window_term = 2 * abs(s * s - 1) * ((Ya - Yb) ** 2 / C2 + 1) + 1e-12
    mse, psnr, ssim = gpu_quality(S, a, b, 2, offsets=(3, 0))
    print("p=%d q=%d: mse %.9g closed %.9g (rel %.3e) ssim %.9f closed %.9f (diff %.3e)" % (
        p, q, mse, mse_cf, abs(mse - mse_cf) / mse_cf, ssim, ssim_cf, ssim - ssim_cf))
    assert abs(mse - mse_cf) <= 2 * 1e-4 / abs(p - q) * mse_cf
    assert abs(ssim - ssim_cf) <= Q.SSIM_ATOL_FLAT + window_term


@pytest.mark.parametrize("name", ["43x43_3_4", "75x59_3_1", "135x37_1_1", "11x11_4_4"])
def test_shave_is_a_pointer_offset(S, name):
    """quality(a, b, shave = k) is bit-identical to the call on the
    pointer-offset interior with shave = 0, whatever b's outer ring holds,
    whatever the pitches and the RGB8 alignment, and from call to call: nothing
    outside the window reaches the result and the order of the sums depends on
    (Ws, Hs) alone."""
    a, b, k, _, _ = all_cases()[name]
    h, w = a.shape[:2]
    first = gpu_quality(S, a, b, k)
    assert np.isfinite(first).all() and first[0] > 0
    ring = np.ones((h, w), bool)
    ring[k:-k, k:-k] = False
    rng = np.random.default_rng(9)
    runs = []
    for trial in range(2):
        bg = b.copy()
        if bg.dtype == np.uint8:
            bg[ring] = rng.integers(0, 256, bg[ring].shape, dtype=np.uint8)
        else:
            bg[ring] = (np.float32("nan"), np.float32(-1e30))[trial]
        assert not np.array_equal(bg, b, equal_nan=True)
        # other pitches, other alignments, another workspace fill
        extra, offs = ((9, 0), (0, 4)), ((2, 4), (3, 8))
        offs = tuple(o if fmt_of(img) == Q.PIX_RGB8 else 4 * (o % 3) for o, img in zip(offs[trial], (a, bg)))
        runs.append(gpu_quality(S, a, bg, k, extra=extra[trial], offsets=offs, ws_fill=(0x00, 0xFF)[trial]))
    # the interior through a pointer offset, shave 0
    pa, fa, pita, ka = place(a, 4, 0, 5)
    pb, fb, pitb, kb = place(bg, 6, 0, 6)
    bpp = {Q.PIX_RGB8: 3, Q.PIX_RGBA8: 4, Q.PIX_LUMA_F32: 4}
    inner = run_quality(S, pa + (k * pita + k) * bpp[fa], fa, pita, pb + (k * pitb + k) * bpp[fb], fb, pitb,
                        w - 2 * k, h - 2 * k, 0)
    again = run_quality(S, pa, fa, pita, pb, fb, pitb, w, h, k)
    for r in runs + [inner, again]:
        assert bits(r) == bits(first), (r, first)


def test_format_does_not_change_the_bits(S):
    """The same colours as RGB8 and as RGBA8 give the same luma, so the same result, bit for bit."""
    a, b, k, _, _ = all_cases()["75x59_3_4"]
    a4 = np.concatenate([a, np.full(a.shape[:2] + (1,), 17, np.uint8)], axis=-1)
    b3 = np.ascontiguousarray(b[..., :3])
    first = gpu_quality(S, a, b, k, offsets=(1, 0))
    for x, y, offs in ((a4, b, (0, 0)), (a, b3, (2, 3)), (a4, b3, (4, 1))):
        assert bits(gpu_quality(S, x, y, k, extra=(1, 8), offsets=offs)) == bits(first)


# ---- 3: the memory contract ----
def test_quality_memory(S):
    """srcnn_quality on an exact-size workspace holding zeros, NaN and +1e30,
    guard bands around a (RGB8, exact size), b (RGBA8), the result and the
    workspace.  The u8 images are byte views of guarded float buffers."""
    w, h = 81, 64  # 3 x 2 tiles; 3 * 81 * 64 bytes are whole floats
    rng = np.random.default_rng(21)
    a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    b = np.clip(a.astype(np.int16) + rng.integers(-9, 10, a.shape), 0, 255).astype(np.uint8)
    b = np.concatenate([b, np.full((h, w, 1), 255, np.uint8)], axis=-1)
    a_f, b_f = a.ravel().copy().view(np.float32), b.ravel().copy().view(np.float32)
    ref = Q.quality(a, b, 1)
    nbytes = S.quality_workspace_bytes(w, h, 1)
    assert nbytes == 256 * ((16 * 6 + 255) // 256)
    runs = []
    for fill in (0.0,) + hip_util.POISONS:
        ad, bd = guarded(a_f, fill), guarded(b_f, fill)
        res = guarded(6, fill, inner=float("nan"))
        ws = guarded(nbytes // 4, fill)
        S.quality(ad, Q.PIX_RGB8, w, bd, Q.PIX_RGBA8, w, w, h, 1, res, ws, nbytes)
        r = H(res).view(np.float64)
        assert np.isfinite(r).all()
        runs.append(r)
        guards_intact(ad, bd, res, ws)
        assert np.array_equal(H(ad.view(torch.uint8)), a.ravel()) and np.array_equal(H(bd.view(torch.uint8)), b.ravel())
    for r in runs[1:]:
        assert bits(r) == bits(runs[0]), "result depends on the workspace's previous contents"
    assert abs(runs[0][2] - ref[2]) <= Q.SSIM_ATOL and abs(runs[0][0] - ref[0]) <= Q.MSE_RTOL * ref[0]


# ---- 4: srcnn_evaluate is its six calls ----
def truth_rgba(W, Hh, seed=4):
    """a smooth picture with some noise: something a net can be better or worse at than bicubic"""
    rng = np.random.default_rng(seed)
    return Q.make_image(rng, Q.PIX_RGBA8, Hh, W, noise=3.0)


def six_calls(S, net, src, W, Hh, s, shave, params):
    w, h = W // s, Hh // s
    Wc, Hc = w * s, h * s
    small = torch.empty(w * h * 4, dtype=torch.uint8, device="cuda")
    rgb = torch.empty(Wc * Hc * 3, dtype=torch.uint8, device="cuda")
    plane = torch.empty(Wc * Hc, dtype=torch.float32, device="cuda")
    ub = S.upscale_workspace_bytes(net, w, h, s)
    uws = torch.empty(ub, dtype=torch.uint8, device="cuda")
    qb = S.quality_workspace_bytes(Wc, Hc, shave)
    qws = torch.empty(qb, dtype=torch.uint8, device="cuda")
    res = torch.full((6,), float("nan"), dtype=torch.float64, device="cuda")
    S.downscale_rgba(src, small, W, Hh, s)
    S.upscale(net, small, w, h, s, params, rgb, uws, ub)
    S.quality(rgb, Q.PIX_RGB8, Wc, src, Q.PIX_RGBA8, W, Wc, Hc, shave, res, qws, qb)
    net_rgb = H(rgb)
    S.upscale_luma(small, plane, w, h, s, 0)
    S.upscale_compose(small, plane, rgb, w, h, s)
    S.quality(rgb, Q.PIX_RGB8, Wc, src, Q.PIX_RGBA8, W, Wc, Hc, shave, res[3:], qws, qb)
    return H(res), net_rgb.reshape(Hc, Wc, 3), H(rgb).reshape(Hc, Wc, 3)


@pytest.mark.parametrize("s", [1, 2, 3, 4])
@pytest.mark.parametrize("name", ["default", "wide"])
def test_evaluate_is_its_six_calls(S, name, s):
    """67 x 50 is ragged at s = 2, 3, 4 (Wc = 66 / 66 / 64 != W: the truth's
    pitch differs from the measured width)."""
    cfg = NETS[name]
    net = S.Net(*cfg)
    W, Hh, shave = 67, 50, s
    truth = truth_rgba(W, Hh)
    src = torch.from_numpy(truth.copy()).cuda()
    params = torch.from_numpy(make_params(np.random.default_rng(11), cfg, sd=0.05)).cuda()
    want, net_rgb, bic_rgb = six_calls(S, net, src, W, Hh, s, shave, params)
    family = S.last_path()
    nbytes = S.evaluate_workspace_bytes(net, W, Hh, s)
    assert nbytes > 0 and nbytes % 256 == 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    res = torch.full((6,), float("nan"), dtype=torch.float64, device="cuda")
    S.evaluate(net, src, W, Hh, s, shave, params, res, ws, nbytes)
    assert S.last_path() == family
    got = H(res)
    print("%s x%d: net psnr %.4f ssim %.6f | bicubic psnr %.4f ssim %.6f" % (name, s, got[1], got[2], got[4], got[5]))
    assert np.isfinite(got[[0, 2, 3, 5]]).all() and bits(got) == bits(want)
    # the numbers are the yardstick's on the images the calls produced; these
    # images are not the inputs the constants were measured on, so the bound
    # is re-derived for each: 4 x the float32 restatements' error on it, where
    # that is more than the constant
    Wc, Hc = W // s * s, Hh // s * s
    for r, img in ((got[:3], net_rgb), (got[3:], bic_rgb)):
        t = np.ascontiguousarray(truth[:Hc, :Wc])
        ref = Q.quality(img, t, shave)
        if ref[0] == 0:
            assert r.tolist() == [0.0, INF, 1.0]
            continue
        r32 = [Q.quality(img, t, shave, np.float32, fused=f) for f in (False, True)]
        tol_s = max(Q.SSIM_ATOL, 4 * max(abs(x[2] - ref[2]) for x in r32))
        tol_m = max(Q.MSE_RTOL, 4 * max(abs(x[0] - ref[0]) / ref[0] for x in r32))
        assert abs(r[2] - ref[2]) <= tol_s and abs(r[0] - ref[0]) <= tol_m * ref[0], (r, ref, tol_s, tol_m)
    if s > 1:
        assert got[3] > 0 and got[0] != got[3]
    for bad_ws, bad_bytes, code in ((ws, nbytes - 1, S.ERR_WORKSPACE), (None, nbytes, S.ERR_INVALID)):
        with pytest.raises(S.SrcnnError) as e:
            S.evaluate(net, src, W, Hh, s, shave, params, res, bad_ws, bad_bytes)
        assert e.value.code == code


def test_evaluate_memory(S):
    """srcnn_evaluate on an exact-size workspace holding zeros, NaN and +1e30,
    guard bands around rgba, params, the result and the workspace."""
    cfg = NETS["default"]
    net = S.Net(*cfg)
    W, Hh, s, shave = 67, 50, 3, 3
    truth = truth_rgba(W, Hh)
    truth_f = truth.copy().view(np.float32).ravel()
    params = make_params(np.random.default_rng(5), cfg, sd=0.05)
    nbytes = S.evaluate_workspace_bytes(net, W, Hh, s)
    runs = []
    for fill in (0.0,) + hip_util.POISONS:
        src, pd = guarded(truth_f, fill), guarded(params, fill)
        res = guarded(12, fill, inner=float("nan"))
        ws = guarded(nbytes // 4, fill)
        S.evaluate(net, src, W, Hh, s, shave, pd, res, ws, nbytes)
        assert S.last_path() == "fused"
        r = H(res).view(np.float64)
        assert np.isfinite(r).all()
        runs.append(r)
        guards_intact(src, pd, res, ws)
        assert np.array_equal(H(src.view(torch.uint8)), truth.ravel()) and hip_util.same_bits(H(pd), params)
    for r in runs[1:]:
        assert bits(r) == bits(runs[0]), "result depends on the workspace's previous contents"


# ---- 5: the command line ----
def run_cnn(*args):
    p = subprocess.run([CNN, *args], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    return p


def test_cli_quality(S, tmp_path):
    from PIL import Image
    rng = np.random.default_rng(8)
    a = Q.make_image(rng, Q.PIX_RGB8, 41, 49)
    b = Q.make_image(rng, Q.PIX_RGB8, 41, 49, like=a, noise=6.0)
    Image.fromarray(a).save(tmp_path / "a.png")
    Image.fromarray(b).save(tmp_path / "b.png")
    for shave, args in ((0, ()), (4, ("--shave", "4"))):
        p = run_cnn("quality", "-i", str(tmp_path / "a.png"), "--ref", str(tmp_path / "b.png"), *args)  # no -c, no -o
        assert "Quality mode, shave: %d" % shave in p.stdout
        got = {k: float(v) for k, v in re.findall(r"^(psnr|ssim|mse): (\S+)", p.stdout, re.M)}
        want = gpu_quality(S, a, b, shave)
        assert [got["mse"], got["psnr"], got["ssim"]] == want.tolist(), (p.stdout, want)
    p = run_cnn("quality", "-i", str(tmp_path / "a.png"), "--ref", str(tmp_path / "a.png"))
    assert "psnr: inf dB" in p.stdout and re.search(r"^ssim: 1$", p.stdout, re.M) and re.search(r"^mse: 0$", p.stdout, re.M)
    Image.fromarray(a[:40]).save(tmp_path / "c.png")
    p = subprocess.run([CNN, "quality", "-i", str(tmp_path / "a.png"), "--ref", str(tmp_path / "c.png")],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 1 and "differ in size" in p.stdout


def test_cli_evaluate(S, tmp_path):
    from PIL import Image
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
    d = tmp_path / "images"
    d.mkdir()
    images = {"a.png": truth_rgba(67, 50, 1)[..., :3], "b.png": truth_rgba(48, 40, 2)[..., :3]}
    for name, img in images.items():
        Image.fromarray(np.ascontiguousarray(img)).save(d / name)
    Image.fromarray(truth_rgba(12, 30, 3)[..., :3].copy()).save(d / "c_tiny.png")  # Wc - 2 shave = 12 - 4 < 11
    (d / "notes.txt").write_text("not an image")
    report = tmp_path / "report.json"
    p = run_cnn("evaluate", "-c", str(tmp_path / "config.json"), "-i", str(d), "--scale", "2", "-o", str(report))
    assert "Evaluate mode, scale: 2, shave: 2" in p.stdout
    assert "'c_tiny.png' (12x30) is too small" in p.stdout and "Skipping image" in p.stdout
    assert "'notes.txt' does not decode" in p.stdout
    pd = torch.from_numpy(params).cuda()
    want = {}
    for name, img in images.items():
        Hh, W = img.shape[:2]
        rgba = np.concatenate([img, np.full((Hh, W, 1), 255, np.uint8)], axis=-1)
        nbytes = S.evaluate_workspace_bytes(net, W, Hh, 2)
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        res = torch.full((6,), float("nan"), dtype=torch.float64, device="cuda")
        S.evaluate(net, torch.from_numpy(rgba).cuda(), W, Hh, 2, 2, pd, res, ws, nbytes)
        want[name] = H(res)
    rep = json.loads(report.read_text())
    assert rep["scale"] == 2 and rep["shave"] == 2 and [r["name"] for r in rep["images"]] == ["a.png", "b.png"]
    for r in rep["images"]:
        w6 = want[r["name"]]
        assert [r["net"]["mse"], r["net"]["psnr"], r["net"]["ssim"]] == w6[:3].tolist()
        assert [r["bicubic"]["mse"], r["bicubic"]["psnr"], r["bicubic"]["ssim"]] == w6[3:].tolist()
        assert r["gain_db"] == w6[1] - w6[4]
        line = re.search(r"^'%s' \(\d+x\d+\): net psnr (\S+) dB ssim (\S+) \| bicubic psnr (\S+) dB ssim (\S+) \| "
                         r"gain (\S+) dB$" % re.escape(r["name"]), p.stdout, re.M)
        assert line and [float(v) for v in line.groups()] == [w6[1], w6[2], w6[4], w6[5], w6[1] - w6[4]], p.stdout
    m = rep["mean"]
    assert m["count"] == 2 and "mean over 2 images: net psnr" in p.stdout
    assert abs(m["net"]["psnr"] - np.mean([want[n][1] for n in want])) <= 1e-12 * m["net"]["psnr"]
    assert abs(m["bicubic"]["ssim"] - np.mean([want[n][5] for n in want])) <= 1e-12
    assert abs(m["gain_db"] - (m["net"]["psnr"] - m["bicubic"]["psnr"])) <= 1e-12
    # a single file, no report
    p = run_cnn("evaluate", "-c", str(tmp_path / "config.json"), "-i", str(d / "a.png"), "--scale", "2")
    assert "mean over 1 images" in p.stdout
