"""srcnn_gather_batch on the GPU (csrc/hip/pairs.hip): every
record's X tile against srcnn_gather_tiles on its footprint and its T tile
against the plane, bit for bit through tests/batch_ref.py's orientation map;
the grid records against srcnn_make_pairs; the memory contract; invalid
records; the host's argument checks; and the `cnn train --from-images` modes
built on it.  Nothing here has a tolerance: the existing kernel is the
yardstick."""
import functools
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

import batch_ref as B
import hip_util
from conftest import ROOT
from hip_util import H, guarded, guards_intact, same_bits
from step_util import S, _settings  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CNN = os.path.join(ROOT, "cnn-super-resolution_amd", "bin", "cnn")
SCALE = 2
# gather_batch stages a footprint of sw x sh in LDS while sh * (sw | 1) <= 2048
# floats (pairs.hip, kStage) and reads the plane through the permutation
# beyond: 45 x 44 is staged in both orientations (44 * 45 and 45 * 45), 47 x 46
# in neither (46 * 47 and 47 * 47).  13 x 9 and 9 x 13 are not square, so a
# footprint that is not swapped when it should be is another window.
STAGE_FLOATS = 2048
SHAPES = [(33, 33), (1, 1), (13, 9), (9, 13), (45, 44), (47, 46)]  # (tw, th)


def random_rgba(W, Hh, seed):
    return np.random.default_rng(seed).integers(0, 256, (Hh, W, 4), dtype=np.uint8)


class Planes:
    """The two planes of one image, made by the calls srcnn_make_pairs starts
    with: x [Hc][Wc] (pitch Wc), t [H][W] (pitch W); tiles come from Wc x Hc."""

    def __init__(self, S, W, Hh, seed):
        s = SCALE
        self.W, self.Hh, self.rgba = W, Hh, random_rgba(W, Hh, seed)
        w, h = W // s, Hh // s
        self.w, self.h = s * w, s * h  # Wc, Hc
        self.x_pitch, self.t_pitch = self.w, W
        self.src = torch.from_numpy(self.rgba.copy()).cuda()
        small = torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda")
        self.x = torch.full((self.h * self.w,), float("nan"), dtype=torch.float32, device="cuda")
        self.t = torch.full((Hh * W,), float("nan"), dtype=torch.float32, device="cuda")
        S.downscale_rgba(self.src, small, W, Hh, s)
        S.upscale_luma(small, self.x, w, h, s, 0)
        S.extract_luma(self.src, self.t, W, Hh, 1)
        self.x_host = H(self.x).reshape(self.h, self.w)
        self.t_host = H(self.t).reshape(Hh, W)
        self.x_host.setflags(write=False)
        self.t_host.setflags(write=False)
        assert np.isfinite(self.x_host).all() and np.isfinite(self.t_host).all()
        self._ref = {}

    def entry(self, x=None, t=None, w=None, h=None):
        return (self.x if x is None else x, self.t if t is None else t, self.x_pitch, self.t_pitch,
                self.w if w is None else w, self.h if h is None else h)

    def reference(self, S, x, y, sw, sh):
        """(X footprint minus its mean, mean) as srcnn_gather_tiles forms them; computed once per footprint"""
        key = (x, y, sw, sh)
        if key not in self._ref:
            tiles = torch.full((sw * sh,), float("nan"), dtype=torch.float32, device="cuda")
            mean = torch.full((1,), float("nan"), dtype=torch.float32, device="cuda")
            S.gather_tiles(self.x, self.x_pitch, self.h, x, y, 1, 1, 1, sw, sh, 1, tiles, mean)
            a, m = H(tiles).reshape(sh, sw), H(mean)
            a.setflags(write=False)
            self._ref[key] = (a, m)
        return self._ref[key]


@pytest.fixture(scope="module")
def images(S):
    """80 x 60: equal pitches.  83 x 61: cropped to 82 x 60, x_pitch 82, t_pitch 83."""
    a, b = Planes(S, 80, 60, 11), Planes(S, 83, 61, 12)
    assert (a.w, a.h, a.x_pitch, a.t_pitch) == (80, 60, 80, 80)
    assert (b.w, b.h, b.x_pitch, b.t_pitch) == (82, 60, 82, 83)
    return [a, b]


def records_for(images, tw, th, seed=5):
    """all eight ops x {origin (0, 0), the largest legal x, the largest legal y,
    an interior point} x both planes, shuffled, one of them twice"""
    recs = []
    for p, im in enumerate(images):
        for op in B.OPS:
            sw, sh = B.footprint(tw, th, op)
            mx, my = im.w - sw, im.h - sh
            assert mx >= 0 and my >= 0
            for x, y in ((0, 0), (mx, 0), (0, my), (mx // 2 | (mx > 0), my // 3 | (my > 0))):
                recs.append((p, x, y, op))
    recs = np.array(recs, dtype=np.int64)
    rng = np.random.default_rng(seed)
    recs = recs[rng.permutation(len(recs))]
    return np.concatenate([recs, recs[3:4]])


def run_batch(S, table, n_planes, recs, tw, th, X=None, T=None, means="own"):
    n = len(recs)
    refs = torch.from_numpy(S.pack_tile_refs(recs)).cuda()
    tab = torch.from_numpy(S.pack_plane_table(table)).cuda()
    nan = float("nan")
    if X is None:
        X = torch.full((n * tw * th,), nan, dtype=torch.float32, device="cuda")
    if T is None:
        T = torch.full((n * tw * th,), nan, dtype=torch.float32, device="cuda")
    if isinstance(means, str):
        means = torch.full((n,), nan, dtype=torch.float32, device="cuda")
    S.gather_batch(tab, n_planes, refs, n, tw, th, X, T, means)
    return H(X).reshape(n, th, tw), H(T).reshape(n, th, tw), (None if means is None else H(means))


def expected(S, images, recs, tw, th):
    X = np.empty((len(recs), th, tw), np.float32)
    T = np.empty_like(X)
    M = np.empty(len(recs), np.float32)
    for i, (p, x, y, op) in enumerate(recs.tolist()):
        im = images[p]
        sw, sh = B.footprint(tw, th, op)
        ref, mean = im.reference(S, x, y, sw, sh)
        X[i] = B.orient(ref, op)
        T[i] = B.orient(B.window(im.t_host, x, y, tw, th, op), op)
        M[i] = mean[0]
    return X, T, M


# ---- 1: bit identity ----
@pytest.mark.parametrize("tw,th", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_bit_identity(S, images, tw, th):
    """The X tile is batch_ref's permutation of what srcnn_gather_tiles(nx = ny
    = 1, tw = sw, th = sh, sub_mean = 1) writes at that origin, the T tile the
    permutation of the plane, means gather_tiles' means: same_bits throughout."""
    for op in (0, 4):
        sw, sh = B.footprint(tw, th, op)
        staged = sh * (sw | 1) <= STAGE_FLOATS
        assert staged == ((tw, th) != (47, 46)), (tw, th, op)
    recs = records_for(images, tw, th)
    assert len(recs) == 8 * 4 * 2 + 1
    X, T, M = run_batch(S, [im.entry() for im in images], 2, recs, tw, th)
    eX, eT, eM = expected(S, images, recs, tw, th)
    assert np.isfinite(X).all() and np.isfinite(T).all() and np.isfinite(M).all()
    for i in range(len(recs)):
        assert same_bits(X[i], eX[i]), ("X", i, recs[i].tolist())
        assert same_bits(T[i], eT[i]), ("T", i, recs[i].tolist())
    assert same_bits(M, eM)
    assert same_bits(X[-1], X[3]) and same_bits(T[-1], T[3])  # (the duplicate)
    if tw * th > 1:
        assert len({X[i].tobytes() for i in range(len(recs))}) > 32, "degenerate result"


# ---- 2: the grid records are srcnn_make_pairs ----
def test_grid_records_reproduce_make_pairs(S, images):
    im = images[0]
    tile, stride = 33, 14
    n, nx, ny = S.make_pairs_count(im.W, im.Hh, SCALE, tile, stride)
    assert (n, nx, ny) == (8, 4, 2)
    nbytes = S.make_pairs_workspace_bytes(im.W, im.Hh, SCALE)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    Xp = torch.full((n * tile * tile,), float("nan"), dtype=torch.float32, device="cuda")
    Tp = torch.full((n * tile * tile,), float("nan"), dtype=torch.float32, device="cuda")
    S.make_pairs(im.src, im.W, im.Hh, SCALE, tile, stride, Xp, Tp, ws, nbytes)
    Xp, Tp = H(Xp).reshape(n, tile, tile), H(Tp).reshape(n, tile, tile)
    grid = np.array([(0, i % nx * stride, i // nx * stride, 0) for i in range(n)], dtype=np.int64)
    X, T, _ = run_batch(S, [im.entry()], 1, grid, tile, tile)
    assert same_bits(X, Xp) and same_bits(T, Tp)
    perm = np.random.default_rng(3).permutation(n)
    assert (perm != np.arange(n)).any()
    X, T, _ = run_batch(S, [im.entry()], 1, grid[perm], tile, tile)
    for row, i in enumerate(perm):
        assert same_bits(X[row], Xp[i]) and same_bits(T[row], Tp[i]), (row, i)


# ---- 3: the memory contract ----
@pytest.mark.parametrize("tw,th", [(13, 9), (47, 46)], ids=["staged", "direct"])
def test_memory(S, images, tw, th):
    """X, T, means and both planes of both images inside guard bands of zeros,
    NaN and +1e30; the outputs start as NaN and every float of them must come
    out finite; the same bits under all three fills; means = None changes
    nothing."""
    recs = records_for(images, tw, th)
    n = len(recs)
    runs = []
    for fill in (0.0,) + hip_util.POISONS:
        planes = [(guarded(im.x_host, fill), guarded(im.t_host, fill)) for im in images]
        table = [im.entry(x=px, t=pt) for im, (px, pt) in zip(images, planes)]
        X = guarded(n * tw * th, fill, inner=float("nan"))
        T = guarded(n * tw * th, fill, inner=float("nan"))
        M = guarded(n, fill, inner=float("nan"))
        x, t, m = run_batch(S, table, 2, recs, tw, th, X, T, M)
        assert np.isfinite(x).all() and np.isfinite(t).all() and np.isfinite(m).all(), \
            "a float of X, T or means was left unwritten"
        X2 = guarded(n * tw * th, fill, inner=float("nan"))
        T2 = guarded(n * tw * th, fill, inner=float("nan"))
        x2, t2, _ = run_batch(S, table, 2, recs, tw, th, X2, T2, None)
        assert same_bits(x2, x) and same_bits(t2, t), "means = None changes the tiles"
        for im, (px, pt) in zip(images, planes):
            assert same_bits(H(px), im.x_host.ravel()) and same_bits(H(pt), im.t_host.ravel())
        guards_intact(X, T, M, X2, T2, *[b for pair in planes for b in pair])
        runs.append((x, t, m))
    eX, eT, eM = expected(S, images, recs, tw, th)
    assert same_bits(runs[0][0], eX) and same_bits(runs[0][1], eT) and same_bits(runs[0][2], eM)
    for x, t, m in runs[1:]:
        assert same_bits(x, runs[0][0]) and same_bits(t, runs[0][1]) and same_bits(m, runs[0][2]), \
            "result depends on what lies around the buffers"


# ---- 4: invalid records ----
@pytest.mark.parametrize("tw,th", [(13, 9), (47, 46)], ids=["staged", "direct"])
def test_invalid_records_give_nan_tiles(S, images, tw, th):
    """Every invalid record is built so that even a kernel without the check
    stays inside allocated memory: the table declares w, h two pixels smaller
    than the planes are and the records overrun into that rim only; the bad
    plane index points at a real entry past n_planes; op = 8 has an in-range
    origin.  (A record whose x + sw wraps 32 bits cannot be made safe that way
    and is left to the code's reading: the sums are 64-bit.)"""
    im = images[1]
    w, h = im.w - 2, im.h - 2
    table = [im.entry(w=w, h=h), images[0].entry()]  # n_planes = 1: entry 1 is real but out of range
    bad = []
    for op in (0, 3, 5, 6):
        sw, sh = B.footprint(tw, th, op)
        bad += [(0, w - sw + 1, 0, op), (0, w - sw + 2, h - sh, op), (0, 0, h - sh + 1, op),
                (0, w - sw, h - sh + 2, op)]
    bad += [(1, 0, 0, 0), (1, 1, 1, 7), (0, 0, 0, 8), (0, 1, 2, 8)]
    good = []
    for op in B.OPS:
        sw, sh = B.footprint(tw, th, op)
        good += [(0, w - sw, h - sh, op), (0, 0, 0, op)]  # (the largest origins the declared extent allows)
    recs, is_bad = [], []
    for i, g in enumerate(good):  # bad records between the good ones, and at both ends
        if i < len(bad):
            recs.append(bad[i]), is_bad.append(True)
        recs.append(g), is_bad.append(False)
    recs += bad[len(good):]
    is_bad += [True] * len(bad[len(good):])
    assert sum(is_bad) == len(bad) and is_bad[0] and is_bad[-1]
    recs, is_bad = np.array(recs, dtype=np.int64), np.array(is_bad)
    n = len(recs)
    X = guarded(n * tw * th, 0.0, inner=1e30)
    T = guarded(n * tw * th, 0.0, inner=1e30)
    M = guarded(n, 0.0, inner=1e30)
    x, t, m = run_batch(S, table, 1, recs, tw, th, X, T, M)
    guards_intact(X, T, M)
    assert np.isnan(x[is_bad]).all() and np.isnan(t[is_bad]).all() and np.isnan(m[is_bad]).all()
    eX, eT, eM = expected(S, [im], recs[~is_bad], tw, th)
    assert same_bits(x[~is_bad], eX) and same_bits(t[~is_bad], eT) and same_bits(m[~is_bad], eM)


# ---- 5: the host's checks ----
def test_host_validation(S, images):
    im = images[0]
    tab = torch.from_numpy(S.pack_plane_table([im.entry()])).cuda()
    refs = torch.from_numpy(S.pack_tile_refs(np.array([[0, 0, 0, 0]]))).cuda()
    X = torch.full((64,), -3.0, dtype=torch.float32, device="cuda")
    T = torch.full((64,), -3.0, dtype=torch.float32, device="cuda")
    M = torch.full((4,), -3.0, dtype=torch.float32, device="cuda")
    rejected = {
        "null planes": (None, 1, refs, 1, 3, 3, X, T, M),
        "null refs": (tab, 1, None, 1, 3, 3, X, T, M),
        "null X": (tab, 1, refs, 1, 3, 3, None, T, M),
        "null T": (tab, 1, refs, 1, 3, 3, X, None, M),
        "n_planes 0": (tab, 0, refs, 1, 3, 3, X, T, M),
        "tw 0": (tab, 1, refs, 1, 0, 3, X, T, M),
        "th 0": (tab, 1, refs, 1, 3, 0, X, T, M),
        "tile beyond 2^31-1": (tab, 1, refs, 1, 65536, 32768, X, T, M),
    }
    for what, args in rejected.items():
        with pytest.raises(S.SrcnnError) as e:
            S.gather_batch(*args)
        assert e.value.code == S.ERR_INVALID, what
        assert "gather_batch" in S.last_error(), what
    S.gather_batch(tab, 1, refs, 0, 3, 3, X, T, M)  # n = 0: OK, no launch
    S.gather_batch(tab, 1, refs, 1, 3, 3, X, T, None)  # (and a call that does run, so the stream is not idle)
    x, t, m = H(X), H(T), H(M)
    assert (x[9:] == -3.0).all() and (t[9:] == -3.0).all() and (m == -3.0).all()
    assert np.isfinite(x[:9]).all() and (x[:9] != -3.0).all()
    X.fill_(-3.0)
    S.gather_batch(tab, 1, refs, 0, 3, 3, X, T, M)
    assert (H(X) == -3.0).all()


# ---- 6: the command line ----
def write_config(d):
    cfg = d / "config.json"
    conf = {"n1": 64, "n2": 32, "f1": 9, "f2": 1, "f3": 5, "momentum": 0.9, "weight_decay_parameter": 0.001,
            "learning_rates": [0.001, 0.001, 0.0001], "parameters_file": ""}
    for i in (1, 2, 3):
        conf["parameters_distribution_%d" % i] = {"mean_w": 0.0, "mean_b": 0.0, "std_deviation_w": 0.01,
                                                  "std_deviation_b": 0.0}
    cfg.write_text(json.dumps(conf))
    return cfg


def smooth_rgb(w, h, seed):
    ch = hip_util.smooth_patches(np.random.default_rng(seed), 3, w, h)
    return (ch.transpose(1, 2, 0) * 255.0 + 0.5).astype(np.uint8)


CASES = {"two_images": (17, 2), "three_images": (17 + 8, 3)}  # samples, images that hold a tile


@pytest.fixture(scope="module")
def cli(S, tmp_path_factory):
    """run(case, *flags) -> (stdout, parameters file bytes), each distinct run
    made once; again=True is the same command a second time"""
    from PIL import Image
    root = tmp_path_factory.mktemp("batch_cli")
    cfg = write_config(root)
    dirs = {}
    for case in CASES:
        d = root / case
        d.mkdir()
        Image.fromarray(smooth_rgb(80, 60, 1)).save(d / "a.png")
        Image.fromarray(smooth_rgb(64, 64, 2)).save(d / "b.png")
        Image.fromarray(smooth_rgb(20, 20, 3)).save(d / "c_tiny.png")
        if case == "three_images":
            Image.fromarray(smooth_rgb(83, 61, 4)).save(d / "d.png")
        dirs[case] = d
    assert S.make_pairs_count(80, 60, 2, 33, 14)[0] + S.make_pairs_count(64, 64, 2, 33, 14)[0] == 17
    assert S.make_pairs_count(83, 61, 2, 33, 14)[0] == 8
    count = [0]

    @functools.lru_cache(maxsize=None)
    def run(case, *flags, again=False):
        count[0] += 1
        out = root / ("p%d.json" % count[0])
        p = subprocess.run([CNN, "train", "--from-images", "-c", str(cfg), "-i", str(dirs[case]), "-o", str(out),
                            "--scale", "2", "--tile", "33", "--stride", "14", "-e", "2", "--seed", "7", *flags],
                           capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stdout + p.stderr
        return p.stdout, out.read_bytes()

    return run


def healthy(stdout, case):
    samples, n_images = CASES[case]
    assert "created %d sample pairs from %d images" % (samples, n_images) in stdout, stdout
    assert "'c_tiny.png' (20x20) is too small for one 33x33 tile at scale 2. Skipping image" in stdout
    errs = re.findall(r"mean validation error: (\S+)", stdout)
    assert errs and all(math.isfinite(float(v)) for v in errs), stdout
    assert "DONE" in stdout


@pytest.mark.parametrize("case", list(CASES))
def test_cli_device_batches_is_byte_identical(cli, case):
    plain_out, plain = cli(case)
    out, params = cli(case, "--device-batches")
    healthy(plain_out, case)
    healthy(out, case)
    assert "resident planes" in out and "resident planes" not in plain_out
    assert re.findall(r"mean validation error: .*", out) == re.findall(r"mean validation error: .*", plain_out)
    assert params == plain
    assert json.loads(params)["epochs"] == 2


@pytest.mark.parametrize("flag", ["--augment", "--random-origins"])
@pytest.mark.parametrize("case", list(CASES))
def test_cli_augmented_runs_are_reproducible(cli, case, flag):
    _, plain = cli(case)
    out, params = cli(case, flag)
    out2, params2 = cli(case, flag, again=True)
    healthy(out, case)
    healthy(out2, case)
    assert params == params2, "two runs with the same seed differ"
    assert params != plain, flag + " changed nothing"
    assert ("random orientations" in out) == (flag == "--augment")
    assert ("random origins" in out) == (flag == "--random-origins")


def test_cli_both_kinds_of_draw_together(cli):
    out, params = cli("two_images", "--augment", "--random-origins")
    healthy(out, "two_images")
    assert params != cli("two_images", "--augment")[1] and params != cli("two_images", "--random-origins")[1]


@pytest.mark.parametrize("case", list(CASES))
def test_cli_one_device_data_parallel_equals_single(cli, case):
    out, params = cli(case, "--augment", "--devices", "1")
    healthy(out, case)
    assert params == cli(case, "--augment")[1]


@pytest.mark.parametrize("flag", ["--augment", "--random-origins", "--device-batches"])
def test_cli_flags_need_from_images(S, tmp_path, flag):
    p = subprocess.run([CNN, "train", "-c", str(write_config(tmp_path)), "-i", str(tmp_path), "-o",
                        str(tmp_path / "p.json"), "-e", "1", flag], capture_output=True, text=True, timeout=60)
    assert p.returncode != 0
    assert "need train --from-images" in p.stdout
