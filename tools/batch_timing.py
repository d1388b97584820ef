"""Timing of srcnn_gather_batch against the two srcnn_gather_tiles launches it
stands in for, on the planes of one full-size image.

  One 1920 x 1080 image at scale 2, tile 33, stride 14: 10,125 records.
    gather_tiles_pair   srcnn_gather_tiles on the X plane (with the mean) and
                        on the T plane (copy), the grid of srcnn_make_pairs
    batch_grid          srcnn_gather_batch, the same grid as records, op 0
    batch_shuffled      the same records in a random order
    batch_shuffled_ops  ... each with a random op of 0..7
    batch_random        random origins and random ops

All run in this process, alternating, timed with device events after a
warm-up: windows of --iters calls, --rounds windows per variant, medians with
min - max (tools/pairs_timing.py's protocol).  Prints one JSON line: the times,
the bytes each variant moves (computed from the shapes: one read of each plane,
since overlapping tiles re-read it from cache, plus the tile writes; the
records add 16 bytes each), that model's share of the 8 TB/s HBM roof, and
batch_grid over gather_tiles_pair against the 1.10 bar.  Fails without a GPU.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cnn-super-resolution_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_BYTES_PER_S = 8e12  # MI355X HBM3E peak
BAR = 1.10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20, help="timed windows per variant")
    ap.add_argument("--iters", type=int, default=20, help="calls per window")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--scale", type=int, default=2)
    ap.add_argument("--tile", type=int, default=33)
    ap.add_argument("--stride", type=int, default=14)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("batch_timing: no GPU found")
    import srcnn_amd as S

    torch.cuda.set_device(0)
    W, H, s, tile, stride = a.width, a.height, a.scale, a.tile, a.stride
    w, h = W // s, H // s
    Wc, Hc = s * w, s * h
    count, nx, ny = S.make_pairs_count(W, H, s, tile, stride)
    if count == 0:
        sys.exit("batch_timing: the image holds no tile")
    rng = np.random.default_rng(0)
    cuda = lambda x: torch.from_numpy(x).cuda()
    full = cuda(rng.integers(0, 256, (H, W, 4), dtype=np.uint8))
    small = torch.empty(h * w * 4, dtype=torch.uint8, device="cuda")
    xplane = torch.empty(Hc * Wc, dtype=torch.float32, device="cuda")
    tplane = torch.empty(H * W, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    S.preload(S.Net(64, 32, 9, 1, 5))
    S.downscale_rgba(full, small, W, H, s, stream)
    S.upscale_luma(small, xplane, w, h, s, 0, stream)
    S.extract_luma(full, tplane, W, H, 1, stream)
    X = torch.empty(count * tile * tile, dtype=torch.float32, device="cuda")
    T = torch.empty(count * tile * tile, dtype=torch.float32, device="cuda")
    X2, T2 = torch.empty_like(X), torch.empty_like(T)

    table = cuda(S.pack_plane_table([(xplane, tplane, Wc, W, Wc, Hc)]))
    i = np.arange(count)
    grid = np.stack([np.zeros(count, np.int64), i % nx * stride, i // nx * stride, np.zeros(count, np.int64)], axis=1)
    shuffled = grid[rng.permutation(count)]
    with_ops = shuffled.copy()
    with_ops[:, 3] = rng.integers(0, 8, count)
    random = with_ops.copy()
    random[:, 1] = rng.integers(0, Wc - tile + 1, count)
    random[:, 2] = rng.integers(0, Hc - tile + 1, count)
    refs = {k: cuda(S.pack_tile_refs(v)) for k, v in
            (("batch_grid", grid), ("batch_shuffled", shuffled), ("batch_shuffled_ops", with_ops),
             ("batch_random", random))}

    def pair():
        S.gather_tiles(xplane, Wc, Hc, 0, 0, stride, nx, ny, tile, tile, 1, X, None, stream)
        S.gather_tiles(tplane, W, H, 0, 0, stride, nx, ny, tile, tile, 0, T, None, stream)

    variants = {"gather_tiles_pair": pair}
    for k, r in refs.items():
        variants[k] = (lambda r: lambda: S.gather_batch(table, 1, r, count, tile, tile, X2, T2, None, stream))(r)

    # the grid records are the two launches, bit for bit
    pair()
    variants["batch_grid"]()
    torch.cuda.synchronize()
    if not (torch.equal(X.view(torch.int32), X2.view(torch.int32)) and
            torch.equal(T.view(torch.int32), T2.view(torch.int32))):
        sys.exit("batch_timing: gather_batch in grid order differs from the two gather_tiles launches")

    e0, e1 = S.event_create(), S.event_create()

    def window(fn):
        S.event_record(e0, stream)
        for _ in range(a.iters):
            fn()
        S.event_record(e1, stream)
        S.event_sync(e1)
        return S.event_elapsed_ms(e0, e1) / a.iters

    for fn in variants.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, fn in variants.items():
            times[k].append(window(fn))
    S.event_destroy(e0)
    S.event_destroy(e1)
    res = {k: {"ms_median": statistics.median(v), "ms_min": min(v), "ms_max": max(v)} for k, v in times.items()}

    tiles_bytes = 4 * count * tile * tile
    model = 4 * Wc * Hc + 4 * W * H + 2 * tiles_bytes
    for k in res:
        b = model + (16 * count if k != "gather_tiles_pair" else 0)
        res[k].update(bytes=b, share_of_hbm_roof=b / HBM_BYTES_PER_S / (res[k]["ms_median"] * 1e-3))
    ratio = res["batch_grid"]["ms_median"] / res["gather_tiles_pair"]["ms_median"]
    print(json.dumps({
        "what": "batch_timing", "device": S.device_name(), "source": [W, H], "scale": s, "tile": tile,
        "stride": stride, "grid": [nx, ny], "records": count, "rounds": a.rounds, "iters": a.iters,
        "variants": res, "batch_grid_over_gather_tiles_pair": ratio, "bar": BAR,
        "bar_met": bool(ratio <= BAR),
    }))


if __name__ == "__main__":
    main()
