"""Training pairs from full-size images on the GPU (csrc/hip/pairs.hip):
srcnn_downscale_rgba and srcnn_gather_tiles against the float64 restatement of
the spec (tests/pairs_ref.py), the alignment of the down and up resampling on
the device, srcnn_make_pairs against its five calls and under the memory
contract of include/srcnn.h, and the `cnn` modes built on them."""
import functools
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

import hip_util
import pairs_ref as P
from conftest import ROOT
from hip_util import H, guarded, guards_intact, same_bits
from step_util import S, _settings  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CNN = os.path.join(ROOT, "cnn-super-resolution_amd", "bin", "cnn")
# A workgroup of downscale_rgba owns 32 x 16 output pixels at scale 1 and 2 and
# 32 x 8 at scale 3 and 4 (pairs.hip, struct Tile), so 135 x 37 spans five
# tiles across and three or five down, with a ragged last one (7 columns, 5
# rows); the other shapes: every tap clamped (1 x 1), smaller than the
# support, odd, and (37 x 23) more than one tile.
SHAPES = [(1, 1), (2, 3), (5, 4), (17, 9), (37, 23), (135, 37)]
EXEMPT_BAND = 1e-3  # distance of the reference's unrounded value from a half-integer
EXEMPT_CAP = 0.01


def random_rgba(W, Hh, seed):
    return np.random.default_rng(seed).integers(0, 256, (Hh, W, 4), dtype=np.uint8)


def ramp_rgba(W, Hh, ax, ay):
    y, x = np.mgrid[0:Hh, 0:W]
    v = ax * x + ay * y + 1
    assert v.max() <= 255
    return np.stack([v, v, v, np.full_like(v, 255)], axis=-1).astype(np.uint8)


def gpu_downscale(S, rgba, s):
    Hh, W = rgba.shape[:2]
    w, h = W // s, Hh // s
    src = torch.from_numpy(rgba.copy()).cuda()
    out = torch.full((h * w * 4,), 0x5A, dtype=torch.uint8, device="cuda")  # 0x5A: an unwritten alpha shows
    S.downscale_rgba(src, out, W, Hh, s)
    return H(out).reshape(h, w, 4)


# ---- 1: downscale_rgba against the float64 reference ----
@pytest.mark.parametrize("ragged", [False, True], ids=["exact", "ragged"])
@pytest.mark.parametrize("s", [2, 3, 4])
@pytest.mark.parametrize("w,h", SHAPES)
def test_downscale_vs_reference(S, w, h, s, ragged):
    """Within 1 everywhere; exactly equal wherever the reference's unrounded
    value is further than 1e-3 from a half-integer: the fp32 chain is at most
    68 roundings of half an ulp at magnitude < 512 (1.5e-5 each), so only there
    can the rounding go the other way.  The weights at s = 2, 4 are dyadic and
    real ties occur, so each case takes the first source seed in 0..7 for which
    the reference alone keeps the exempt share within 1 %."""
    W, Hh = (s * w + s - 1, s * h + s - 1) if ragged else (s * w, s * h)
    for seed in range(8):
        rgba = random_rgba(W, Hh, seed)
        ref, raw = P.down_rgba(rgba, s)
        near = np.abs(raw - np.floor(raw) - 0.5) <= EXEMPT_BAND
        if near.mean() <= EXEMPT_CAP:
            break
    else:
        pytest.fail("no seed in 0..7 keeps the reference's near-ties within 1 %")
    assert ref.shape == (h, w, 4)
    got = gpu_downscale(S, rgba, s)
    d = np.abs(got[..., :3].astype(np.int16) - ref[..., :3].astype(np.int16))
    print("downscale_rgba %dx%d -> %dx%d /%d seed %d: %d of %d exempt, %d differ by 1, max diff %d"
          % (W, Hh, w, h, s, seed, near.sum(), near.size, (d == 1).sum(), d.max()))
    hip_util.log_record({"what": "downscale_rgba %dx%d /%d" % (W, Hh, s), "seed": seed, "exempt": int(near.sum()),
                         "differ": int((d != 0).sum())})
    assert (got[..., 3] == 255).all(), "alpha is not 255 (or a pixel was left unwritten)"
    assert d.max() <= 1
    assert np.array_equal(got[..., :3][~near], ref[..., :3][~near])


# ---- 2: scale 1 returns the source's r, g, b ----
@pytest.mark.parametrize("w,h", SHAPES)
def test_downscale_scale_1_is_identity(S, w, h):
    rgba = random_rgba(w, h, 0)
    got = gpu_downscale(S, rgba, 1)
    assert np.array_equal(got[..., :3], rgba[..., :3])
    assert (got[..., 3] == 255).all()


# ---- 3: down then up is shift-free, on the device ----
@pytest.mark.parametrize("W,Hh,ax,ay", [(96, 64, 2, 1), (64, 96, 1, 2)])
@pytest.mark.parametrize("s", [1, 2, 3, 4])
def test_down_then_up_is_aligned(S, s, W, Hh, ax, ay):
    """|X - T| at least 4s pixels from every edge <= 2.1e-3: the references
    give <= 1.961e-3 (0.5 / 255, the rounding of the low-resolution bytes at
    s = 2, 4; tests/test_pairs_cpu.py) and upscale_luma's own 4e-6 bound sits
    on top.  A one-pixel shift would give >= 5.88e-3."""
    rgba = ramp_rgba(W, Hh, ax, ay)
    w, h = W // s, Hh // s
    src = torch.from_numpy(rgba.copy()).cuda()
    small = torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda")
    X = torch.full((s * h * s * w,), float("nan"), dtype=torch.float32, device="cuda")
    T = torch.full((Hh * W,), float("nan"), dtype=torch.float32, device="cuda")
    S.downscale_rgba(src, small, W, Hh, s)
    S.upscale_luma(small, X, w, h, s, 0)
    S.extract_luma(src, T, W, Hh, 1)
    X = H(X).reshape(s * h, s * w).astype(np.float64)
    T = H(T).reshape(Hh, W)[:s * h, :s * w].astype(np.float64)
    e = 4 * s
    d = np.abs(X - T)[e:-e, e:-e]
    print("down/up x%d on %dx%d: interior max |X - T| = %.4e" % (s, W, Hh, d.max()))
    assert d.size > 0 and d.max() <= 2.1e-3


# ---- 4: gather_tiles ----
# (pw, ph, x0, y0, stride, tw, th)
GRIDS = {
    "tile1": (23, 17, 0, 0, 1, 1, 1),
    "tile5_offset": (23, 17, 2, 1, 3, 5, 5),
    "tile33": (96, 64, 0, 0, 14, 33, 33),
    "tile128": (256, 128, 0, 0, 128, 128, 128),
    "tile7x3": (23, 17, 0, 0, 4, 7, 3),
    "whole_plane": (23, 17, 0, 0, 1, 23, 17),
}


@functools.lru_cache(maxsize=None)
def plane_of(pw, ph):
    a = np.random.default_rng(pw * 1000 + ph).uniform(-0.2, 1.2, (ph, pw)).astype(np.float32)
    a.setflags(write=False)
    return a


def grid_of(name):
    pw, ph, x0, y0, stride, tw, th = GRIDS[name]
    nx, ny = (pw - x0 - tw) // stride + 1, (ph - y0 - th) // stride + 1
    return pw, ph, x0, y0, stride, nx, ny, tw, th


def gpu_gather(S, plane, pw, ph, x0, y0, stride, nx, ny, tw, th, sub_mean, with_means=True):
    src = torch.from_numpy(plane.copy()).cuda()
    tiles = torch.full((nx * ny * th * tw,), float("nan"), dtype=torch.float32, device="cuda")
    means = torch.full((nx * ny,), float("nan"), dtype=torch.float32, device="cuda") if with_means else None
    S.gather_tiles(src, pw, ph, x0, y0, stride, nx, ny, tw, th, sub_mean, tiles, means)
    return H(tiles).reshape(nx * ny, th, tw), (H(means) if with_means else None)


@pytest.mark.parametrize("name", list(GRIDS))
def test_gather_tiles(S, name):
    """Without sub_mean the tiles are the plane's windows bit for bit (and
    means is not touched).  With it, means[i] is within the bound of the
    window's float64 mean and the tile is fp32(window - means[i]) bit for bit.

    The bound follows the kernel's summation order: thread t adds the tile's
    elements t, t + 256, ... in turn (ceil(tw*th / 256) additions), then the
    256 partial sums meet in a binary tree (six levels inside a wave, two over
    the four waves: 8 more), so the longest path has
    ceil(tw*th / 256) + 8 additions; each rounds by at most 2^-24 of a partial
    sum, which as a share of the final mean is at most 2^-24 x max|value|; the
    division and the final store add two more: 2^-24 x max|value| x (additions
    + 2), doubled."""
    pw, ph, x0, y0, stride, nx, ny, tw, th = grid_of(name)
    assert nx >= 1 and ny >= 1
    plane = plane_of(pw, ph)
    win = P.windows(plane, x0, y0, stride, nx, ny, tw, th)
    plain, untouched = gpu_gather(S, plane, pw, ph, x0, y0, stride, nx, ny, tw, th, 0)
    assert same_bits(plain, win)
    assert np.isnan(untouched).all(), "means written without sub_mean"
    tiles, means = gpu_gather(S, plane, pw, ph, x0, y0, stride, nx, ny, tw, th, 1)
    adds = math.ceil(tw * th / 256) + 8
    bound = 2.0 * 2.0 ** -24 * float(np.abs(plane).max()) * (adds + 2)
    err = np.abs(means.astype(np.float64) - win.astype(np.float64).mean(axis=(1, 2))).max()
    print("gather_tiles %s: %d tiles of %dx%d, max |mean err| %.3e (bound %.3e)" % (name, nx * ny, tw, th, err, bound))
    hip_util.log_record({"what": "gather_tiles " + name, "mean_err": float(err), "bound": bound})
    assert np.isfinite(means).all() and err <= bound
    assert same_bits(tiles, win - means[:, None, None])
    # means = NULL: the same tiles; a second run: the same bits
    no_means, _ = gpu_gather(S, plane, pw, ph, x0, y0, stride, nx, ny, tw, th, 1, with_means=False)
    assert same_bits(no_means, tiles)
    again, means2 = gpu_gather(S, plane, pw, ph, x0, y0, stride, nx, ny, tw, th, 1)
    assert same_bits(again, tiles) and same_bits(means2, means)
    # the last tile cut alone: the order does not depend on the grid
    ix, iy = nx - 1, ny - 1
    alone, mean1 = gpu_gather(S, plane, pw, ph, x0 + ix * stride, y0 + iy * stride, stride, 1, 1, tw, th, 1)
    assert same_bits(alone[0], tiles[iy * nx + ix]) and same_bits(mean1, means[iy * nx + ix:])


# ---- 5: make_pairs is its five calls ----
def five_calls(S, src, W, Hh, s, tile, stride):
    w, h = W // s, Hh // s
    Wc, Hc = s * w, s * h
    n, nx, ny = S.make_pairs_count(W, Hh, s, tile, stride)
    small = torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda")
    xp = torch.empty(Hc * Wc, dtype=torch.float32, device="cuda")
    tp = torch.empty(Hh * W, dtype=torch.float32, device="cuda")
    X = torch.full((n * tile * tile,), float("nan"), dtype=torch.float32, device="cuda")
    T = torch.full((n * tile * tile,), float("nan"), dtype=torch.float32, device="cuda")
    S.downscale_rgba(src, small, W, Hh, s)
    S.upscale_luma(small, xp, w, h, s, 0)
    S.extract_luma(src, tp, W, Hh, 1)
    S.gather_tiles(xp, Wc, Hc, 0, 0, stride, nx, ny, tile, tile, 1, X, None)
    S.gather_tiles(tp, W, Hh, 0, 0, stride, nx, ny, tile, tile, 0, T, None)
    return H(X), H(T), xp, (Wc, Hc, nx, ny)


def one_call(S, src, W, Hh, s, tile, stride):
    n, _, _ = S.make_pairs_count(W, Hh, s, tile, stride)
    nbytes = S.make_pairs_workspace_bytes(W, Hh, s)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    X = torch.full((n * tile * tile,), float("nan"), dtype=torch.float32, device="cuda")
    T = torch.full((n * tile * tile,), float("nan"), dtype=torch.float32, device="cuda")
    S.make_pairs(src, W, Hh, s, tile, stride, X, T, ws, nbytes)
    return H(X), H(T), (X, T, ws, nbytes)


@pytest.mark.parametrize("W,Hh,s,tile,stride", [(96, 64, 2, 33, 14), (67, 50, 3, 9, 4)])
def test_make_pairs_is_its_five_calls(S, W, Hh, s, tile, stride):
    rgba = random_rgba(W, Hh, 0)
    src = torch.from_numpy(rgba.copy()).cuda()
    Xo, To, _, (Wc, Hc, nx, ny) = five_calls(S, src, W, Hh, s, tile, stride)
    before = S.last_path()
    X, T, (Xd, Td, ws, nbytes) = one_call(S, src, W, Hh, s, tile, stride)
    assert S.last_path() == before  # (left as the luma ops leave it)
    assert np.isfinite(X).all() and np.isfinite(T).all()
    assert same_bits(X, Xo) and same_bits(T, To)
    assert X.size == nx * ny * tile * tile and len(np.unique(T)) > 8, "degenerate result"
    # T is the image's own luma; X is mean-free per tile
    assert np.abs(X.reshape(nx * ny, -1).astype(np.float64).mean(axis=1)).max() <= 1e-6
    with pytest.raises(S.SrcnnError) as e:
        S.make_pairs(src, W, Hh, s, tile, stride, Xd, Td, ws, nbytes - 1)
    assert e.value.code == S.ERR_WORKSPACE


def test_make_pairs_scale_1_input_is_the_ground_truth(S):
    """At s = 1 nothing is degraded: the X plane gathered without the mean is T."""
    W, Hh, tile, stride = 40, 30, 9, 4
    src = torch.from_numpy(random_rgba(W, Hh, 0).copy()).cuda()
    _, To, xp, (Wc, Hc, nx, ny) = five_calls(S, src, W, Hh, 1, tile, stride)
    _, T, _ = one_call(S, src, W, Hh, 1, tile, stride)
    raw = torch.full((nx * ny * tile * tile,), float("nan"), dtype=torch.float32, device="cuda")
    S.gather_tiles(xp, Wc, Hc, 0, 0, stride, nx, ny, tile, tile, 0, raw, None)
    assert same_bits(H(raw), T) and same_bits(T, To)


# ---- 6: the memory contract ----
@pytest.mark.parametrize("W,Hh,s,tile,stride", [(2, 2, 2, 2, 1), (67, 50, 3, 9, 4)])
def test_make_pairs_memory(S, W, Hh, s, tile, stride):
    """srcnn_make_pairs on an exact-size workspace holding zeros, NaN and
    +1e30, guard bands around rgba, X, T and ws.  The rgba bytes are a view of a
    guarded float buffer (W*H floats = 4*W*H bytes); X and T start as NaN and
    every float of them must come out finite."""
    n, nx, ny = S.make_pairs_count(W, Hh, s, tile, stride)
    assert n >= 1
    rgba = random_rgba(W, Hh, 1)
    rgba_f = rgba.copy().view(np.float32).ravel()
    nbytes = S.make_pairs_workspace_bytes(W, Hh, s)
    assert nbytes % 256 == 0
    runs = []
    for fill in (0.0,) + hip_util.POISONS:
        src = guarded(rgba_f, fill)
        assert np.array_equal(H(src.view(torch.uint8)), rgba.ravel())  # (bits survive the float view)
        X = guarded(n * tile * tile, fill, inner=float("nan"))
        T = guarded(n * tile * tile, fill, inner=float("nan"))
        ws = guarded(nbytes // 4, fill)
        S.make_pairs(src, W, Hh, s, tile, stride, X, T, ws, nbytes)
        x, t = H(X), H(T)
        assert np.isfinite(x).all() and np.isfinite(t).all(), "a float of X or T was left unwritten"
        runs.append((x, t))
        guards_intact(src, X, T, ws)
        assert np.array_equal(H(src.view(torch.uint8)), rgba.ravel())
    for x, t in runs[1:]:
        assert same_bits(x, runs[0][0]) and same_bits(t, runs[0][1]), \
            "result depends on the workspace's previous contents"


# ---- 7, 8: the command line ----
def run_cnn(*args):
    p = subprocess.run([CNN, *args], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    return p


def write_config(tmp_path):
    cfg = tmp_path / "config.json"
    conf = {"n1": 64, "n2": 32, "f1": 9, "f2": 1, "f3": 5, "momentum": 0.9, "weight_decay_parameter": 0.001,
            "learning_rates": [0.001, 0.001, 0.0001], "parameters_file": ""}
    for i in (1, 2, 3):
        conf["parameters_distribution_%d" % i] = {"mean_w": 0.0, "mean_b": 0.0, "std_deviation_w": 0.01,
                                                  "std_deviation_b": 0.0}
    cfg.write_text(json.dumps(conf))
    return cfg


def smooth_rgb(w, h, seed):
    """a smooth synthetic picture: three channels of a random low-resolution grid, upsampled"""
    ch = hip_util.smooth_patches(np.random.default_rng(seed), 3, w, h)
    return (ch.transpose(1, 2, 0) * 255.0 + 0.5).astype(np.uint8)


def test_cli_downscale(S, tmp_path):
    from PIL import Image
    rgb = np.random.default_rng(5).integers(0, 256, (41, 49, 3), dtype=np.uint8)  # 49 x 41: ragged at s = 2
    src = tmp_path / "in.png"
    Image.fromarray(rgb).save(src)
    small, back = tmp_path / "small.png", tmp_path / "back.png"
    p = run_cnn("downscale", "-i", str(src), "-o", str(small), "--scale", "2")  # (no -c)
    assert "Downscale mode, scale: 2" in p.stdout
    img = Image.open(small)
    assert img.size == (24, 20) and img.mode == "RGB"
    rgba = np.concatenate([rgb, np.full((41, 49, 1), 255, np.uint8)], axis=-1)
    assert np.array_equal(np.asarray(img), gpu_downscale(S, rgba, 2)[..., :3])
    run_cnn("upscale", "-c", str(write_config(tmp_path)), "-i", str(small), "-o", str(back), "--seed", "7",
            "--scale", "2")
    assert Image.open(back).size == (48, 40)
    # an image whose size is a multiple of the scale comes back at its own size
    Image.fromarray(rgb[:40, :48]).save(src)
    run_cnn("downscale", "-i", str(src), "-o", str(small), "--scale", "2")
    run_cnn("upscale", "-c", str(write_config(tmp_path)), "-i", str(small), "-o", str(back), "--seed", "7",
            "--scale", "2")
    assert Image.open(back).size == (48, 40)


def test_cli_train_from_images(S, tmp_path):
    from PIL import Image
    cfg = write_config(tmp_path)
    d = tmp_path / "images"
    d.mkdir()
    Image.fromarray(smooth_rgb(80, 60, 1)).save(d / "a.png")
    Image.fromarray(smooth_rgb(64, 64, 2)).save(d / "b.png")
    Image.fromarray(smooth_rgb(20, 20, 3)).save(d / "c_tiny.png")
    want = S.make_pairs_count(80, 60, 2, 33, 14)[0] + S.make_pairs_count(64, 64, 2, 33, 14)[0]
    assert want == 8 + 9
    outs = []
    for name in ("p1.json", "p2.json"):
        out = tmp_path / name
        p = run_cnn("train", "--from-images", "-c", str(cfg), "-i", str(d), "-o", str(out), "--scale", "2",
                    "--tile", "33", "--stride", "14", "-e", "2", "--seed", "7")
        assert "created %d sample pairs from 2 images" % want in p.stdout, p.stdout
        assert "'c_tiny.png' (20x20) is too small for one 33x33 tile at scale 2. Skipping image" in p.stdout
        errs = re.findall(r"mean validation error: (\S+)", p.stdout)
        assert errs and all(math.isfinite(float(v)) for v in errs), p.stdout
        assert "DONE" in p.stdout
        outs.append(out.read_bytes())
        params = json.loads(outs[-1])
        assert params["epochs"] == 2 and len(params["layer1"]["weights"]) == 9 * 9 * 64
    assert outs[0] == outs[1]
