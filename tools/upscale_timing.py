"""Timing of srcnn_upscale against today's chain at the same output size.

  new:   srcnn_upscale, 1920 x 1080 RGBA x2 -> 3840 x 2160 RGB (default net)
  chain: srcnn_extract_luma + srcnn_sub_mean + srcnn_forward + srcnn_swap_luma
         on a 3840 x 2160 RGBA that was scaled elsewhere (output 3828 x 2148
         inside an un-enhanced frame)

Both run in this process, alternating, timed with device events after a
warm-up; then the four luma kernels alone, alternating in the same way.
Prints one JSON line: the median and the spread of each, the bytes each new
kernel moves (computed from the shapes) and its share of the 8 TB/s HBM roof.
Fails without a GPU.  Kernel times are better taken from a profiler run of
this script (rocprofv3 --kernel-trace --stats -- python tools/upscale_timing.py
--rounds 3); the event times of single kernels here include the launch gap.
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
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("upscale_timing: no GPU found")
    import srcnn_amd as S

    torch.cuda.set_device(0)
    cfg = (64, 32, 9, 1, 5)
    net = S.Net(*cfg)
    pad = cfg[2] + cfg[3] + cfg[4] - 3
    w, h, s = a.width, a.height, a.scale
    W, H = s * w, s * h
    rng = np.random.default_rng(0)
    cuda = lambda x: torch.from_numpy(x).cuda()
    params = cuda((0.05 * rng.standard_normal(S.net_param_count(net))).astype(np.float32))
    small = cuda(rng.integers(0, 256, (h, w, 4), dtype=np.uint8))
    large = cuda(rng.integers(0, 256, (H, W, 4), dtype=np.uint8))
    S.preload(net)

    # new path
    up_bytes = S.upscale_workspace_bytes(net, w, h, s)
    up_ws = torch.empty(up_bytes, dtype=torch.uint8, device="cuda")
    rgb_new = torch.empty(3 * W * H, dtype=torch.uint8, device="cuda")
    # today's chain on the already scaled image
    luma = torch.empty(W * H, dtype=torch.float32, device="cuda")
    out = torch.empty((W - pad) * (H - pad), dtype=torch.float32, device="cuda")
    red_bytes = S.reduce_workspace_bytes(W * H)
    red = torch.empty(red_bytes, dtype=torch.uint8, device="cuda")
    fwd_bytes = S.forward_workspace_bytes(net, W, H, 1)
    fwd_ws = torch.empty(fwd_bytes, dtype=torch.uint8, device="cuda")
    rgb_old = torch.empty(3 * W * H, dtype=torch.uint8, device="cuda")
    # op-level buffers of the new kernels
    plane = torch.empty((W + pad) * (H + pad), dtype=torch.float32, device="cuda")
    new_luma = cuda(rng.uniform(0, 1, W * H).astype(np.float32))
    stream = torch.cuda.current_stream().cuda_stream

    def new():
        S.upscale(net, small, w, h, s, params, rgb_new, up_ws, up_bytes, stream)

    def chain():
        S.extract_luma(large, luma, W, H, 1, stream)
        S.sub_mean(luma, W * H, None, red, red_bytes, stream)
        S.forward(net, luma, W, H, 1, params, out, fwd_ws, fwd_bytes, stream)
        S.swap_luma(large, out, rgb_old, W, H, W - pad, H - pad, stream)

    kernels = {
        "upscale_luma": lambda: S.upscale_luma(small, plane, w, h, s, pad, stream),
        "extract_luma": lambda: S.extract_luma(large, luma, W, H, 1, stream),
        "upscale_compose": lambda: S.upscale_compose(small, new_luma, rgb_new, w, h, s, stream),
        "swap_luma": lambda: S.swap_luma(large, new_luma, rgb_old, W, H, W, H, stream),
    }

    e0, e1 = S.event_create(), S.event_create()

    def window(fn):
        S.event_record(e0, stream)
        for _ in range(a.iters):
            fn()
        S.event_record(e1, stream)
        S.event_sync(e1)
        return S.event_elapsed_ms(e0, e1) / a.iters

    def alternate(variants):
        for fn in variants.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for _ in range(a.rounds):
            for k, fn in variants.items():
                times[k].append(window(fn))
        return {k: {"ms_median": statistics.median(v), "ms_min": min(v), "ms_max": max(v)}
                for k, v in times.items()}

    end_to_end = alternate({"upscale": new, "chain": chain})
    per_kernel = alternate(kernels)
    S.event_destroy(e0)
    S.event_destroy(e1)

    bytes_model = {
        "upscale_luma": 4 * w * h + 4 * (W + pad) * (H + pad),
        "upscale_compose": 4 * w * h + 4 * W * H + 3 * W * H,
        "extract_luma": 4 * W * H + 4 * W * H,
        "swap_luma": 4 * W * H + 4 * W * H + 3 * W * H,
    }
    for k, b in bytes_model.items():
        t = per_kernel[k]["ms_median"] * 1e-3
        per_kernel[k].update(bytes=b, share_of_hbm_roof=b / HBM_BYTES_PER_S / t)
    print(json.dumps({
        "what": "upscale_timing", "device": S.device_name(), "source": [w, h], "scale": s,
        "output": [W, H], "net": list(cfg), "rounds": a.rounds, "iters": a.iters,
        "end_to_end": end_to_end, "kernels": per_kernel,
        "bars": {
            "upscale_luma_over_extract_luma": per_kernel["upscale_luma"]["ms_median"] /
            per_kernel["extract_luma"]["ms_median"],
            "upscale_compose_over_swap_luma": per_kernel["upscale_compose"]["ms_median"] /
            per_kernel["swap_luma"]["ms_median"],
            "limit": 1.10},
    }))


if __name__ == "__main__":
    main()
