"""Timing of the device-side quality report.

  srcnn_quality on two 3840 x 2160 images, RGB8 (what srcnn_upscale writes)
  against RGBA8 (the decoded ground truth), shave 2;
  srcnn_evaluate of the default net on one 1920 x 1080 ground truth at scale 2;
  and, as the streaming yardstick, srcnn_extract_luma over each of the two
  images: the cost of merely reading them (and writing a float per pixel).
  srcnn_extract_luma takes 4-byte pixels, so the RGB8 image's 3 W H bytes are
  read as 3 W H / 4 of them.

All run in this process, alternating, timed with device events after a
warm-up: windows of --iters calls, --rounds windows per variant, medians with
min - max.  Prints one JSON line: the times, the bytes srcnn_quality must move
(each image once; the halo re-reads and the partial sums are left out), its
share of the 8 TB/s HBM roof and its ratio to the yardstick.  Fails without a
GPU.  The event time of a single kernel includes the launch gap between
back-to-back calls.
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
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--shave", type=int, default=2)
    ap.add_argument("--eval-width", type=int, default=1920)
    ap.add_argument("--eval-height", type=int, default=1080)
    ap.add_argument("--scale", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("quality_timing: no GPU found")
    import srcnn_amd as S

    torch.cuda.set_device(0)
    W, H, shave = a.width, a.height, a.shave
    if (3 * W * H) % 4:
        sys.exit("quality_timing: 3 * width * height must be a multiple of 4 (the yardstick reads 4-byte pixels)")
    rng = np.random.default_rng(0)
    cuda = lambda x: torch.from_numpy(x).cuda()
    truth = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    rgb = np.clip(truth[..., :3].astype(np.int16) + rng.integers(-6, 7, (H, W, 3)), 0, 255).astype(np.uint8)
    truth_d, rgb_d = cuda(truth), cuda(rgb)
    luma = torch.empty(H * W, dtype=torch.float32, device="cuda")
    res = torch.zeros(6, dtype=torch.float64, device="cuda")
    q_bytes = S.quality_workspace_bytes(W, H, shave)
    q_ws = torch.empty(q_bytes, dtype=torch.uint8, device="cuda")

    net = S.Net(64, 32, 9, 1, 5)
    EW, EH, s = a.eval_width, a.eval_height, a.scale
    etruth_d = cuda(rng.integers(0, 256, (EH, EW, 4), dtype=np.uint8))
    params = cuda((0.05 * rng.standard_normal(S.net_param_count(net))).astype(np.float32))
    e_bytes = S.evaluate_workspace_bytes(net, EW, EH, s)
    e_ws = torch.empty(e_bytes, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    S.preload(net)

    variants = {
        "quality": lambda: S.quality(rgb_d, S.PIX_RGB8, W, truth_d, S.PIX_RGBA8, W, W, H, shave, res, q_ws, q_bytes,
                                     stream),
        "extract_luma_rgba8": lambda: S.extract_luma(truth_d, luma, W, H, 1, stream),
        "extract_luma_rgb8_bytes": lambda: S.extract_luma(rgb_d, luma, W, 3 * H // 4, 1, stream),
        "evaluate": lambda: S.evaluate(net, etruth_d, EW, EH, s, s, params, res, e_ws, e_bytes, stream),
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
    out = {k: {"ms_median": statistics.median(v), "ms_min": min(v), "ms_max": max(v)} for k, v in times.items()}

    bytes_model = {"quality": 3 * W * H + 4 * W * H, "extract_luma_rgba8": 4 * W * H + 4 * W * H,
                   "extract_luma_rgb8_bytes": 3 * W * H + 3 * W * H}
    for k, b in bytes_model.items():
        out[k].update(bytes=b, share_of_hbm_roof=b / HBM_BYTES_PER_S / (out[k]["ms_median"] * 1e-3))
    yard = out["extract_luma_rgba8"]["ms_median"] + out["extract_luma_rgb8_bytes"]["ms_median"]
    out["quality"]["ratio_to_yardstick"] = out["quality"]["ms_median"] / yard
    torch.cuda.synchronize()
    print(json.dumps({
        "what": "quality_timing", "device": S.device_name(), "images": [W, H], "shave": shave,
        "evaluate": {"truth": [EW, EH], "scale": s, "net": [64, 32, 9, 1, 5]}, "rounds": a.rounds, "iters": a.iters,
        "yardstick_ms": yard, "kernels": out,
    }))


if __name__ == "__main__":
    main()
