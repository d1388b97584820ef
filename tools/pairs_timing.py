"""Timing of the device-side training-pair path for one full-size image.

  srcnn_downscale_rgba, both srcnn_gather_tiles (X: with the mean, T: without)
  and srcnn_make_pairs on one 1920 x 1080 RGBA image at scale 2, tile 33,
  stride 14, and srcnn_extract_luma on the same source as the streaming
  yardstick.

All run in this process, alternating, timed with device events after a
warm-up: windows of --iters calls, --rounds windows per variant, medians with
min - max.  Prints one JSON line: the times, the bytes each kernel moves
(computed from the shapes; overlapping tiles re-read the plane from cache, so
a gather's model is one read of the plane plus the tile writes) and its share
of the 8 TB/s HBM roof.  Fails without a GPU.  The event time of a single
kernel includes the launch gap between back-to-back calls.
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
        sys.exit("pairs_timing: no GPU found")
    import srcnn_amd as S

    torch.cuda.set_device(0)
    W, H, s, tile, stride = a.width, a.height, a.scale, a.tile, a.stride
    w, h = W // s, H // s
    Wc, Hc = s * w, s * h
    count, nx, ny = S.make_pairs_count(W, H, s, tile, stride)
    if count == 0:
        sys.exit("pairs_timing: the image holds no tile")
    rng = np.random.default_rng(0)
    cuda = lambda x: torch.from_numpy(x).cuda()
    full = cuda(rng.integers(0, 256, (H, W, 4), dtype=np.uint8))
    small = torch.empty(h * w * 4, dtype=torch.uint8, device="cuda")
    xplane = cuda(rng.uniform(0, 1, Hc * Wc).astype(np.float32))
    tplane = torch.empty(H * W, dtype=torch.float32, device="cuda")
    X = torch.empty(count * tile * tile, dtype=torch.float32, device="cuda")
    T = torch.empty(count * tile * tile, dtype=torch.float32, device="cuda")
    ws_bytes = S.make_pairs_workspace_bytes(W, H, s)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    S.preload(S.Net(64, 32, 9, 1, 5))
    S.extract_luma(full, tplane, W, H, 1, stream)

    variants = {
        "downscale_rgba": lambda: S.downscale_rgba(full, small, W, H, s, stream),
        "gather_tiles_X": lambda: S.gather_tiles(xplane, Wc, Hc, 0, 0, stride, nx, ny, tile, tile, 1, X, None, stream),
        "gather_tiles_T": lambda: S.gather_tiles(tplane, W, H, 0, 0, stride, nx, ny, tile, tile, 0, T, None, stream),
        "extract_luma": lambda: S.extract_luma(full, tplane, W, H, 1, stream),
        "make_pairs": lambda: S.make_pairs(full, W, H, s, tile, stride, X, T, ws, ws_bytes, stream),
    }

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
    bytes_model = {
        "downscale_rgba": 4 * W * H + 4 * w * h,
        "gather_tiles_X": 4 * Wc * Hc + tiles_bytes,
        "gather_tiles_T": 4 * W * H + tiles_bytes,
        "extract_luma": 4 * W * H + 4 * W * H,
    }
    bytes_model["make_pairs"] = (bytes_model["downscale_rgba"] + (4 * w * h + 4 * Wc * Hc) + bytes_model["extract_luma"] +
                                 bytes_model["gather_tiles_X"] + bytes_model["gather_tiles_T"])
    for k, b in bytes_model.items():
        t = res[k]["ms_median"] * 1e-3
        res[k].update(bytes=b, share_of_hbm_roof=b / HBM_BYTES_PER_S / t)
    print(json.dumps({
        "what": "pairs_timing", "device": S.device_name(), "source": [W, H], "scale": s, "tile": tile,
        "stride": stride, "grid": [nx, ny], "pairs": count, "rounds": a.rounds, "iters": a.iters,
        "launches_per_image": 5, "launches_file_pair_path": 6 * count, "kernels": res,
    }))


if __name__ == "__main__":
    main()
