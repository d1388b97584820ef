"""Timing of the downscale of Y'CbCr frames.

  srcnn_downscale_planes on one 3840 x 2160 luma plane at scale 2: 8-bit,
  10-bit planar, and the same number of samples as P010 (U, V) pairs
  (1920 x 2160 pairs, msb 1); srcnn_downscale_frame on a 4:2:0 frame of that
  size, 8-bit and P010; srcnn_make_pairs_frame on one 1920 x 1080 frame (tile
  33, stride 14); srcnn_evaluate_frame on a 1920 x 1080 truth at scale 2; and
  srcnn_downscale_rgba on a 3840 x 2160 RGBA image at the same scale as the
  yardstick: the kernel that was there before, with the same taps per output
  and four times the bytes of the 8-bit plane.

All run in this process, alternating, timed with device events after a
warm-up: windows of --iters calls, --rounds windows per variant, medians with
min - max.  Prints one JSON line: the times, the bytes each call must move
(computed from the shapes; the composite calls: the sum over their kernels,
the net's forward left out) and their share of the 8 TB/s HBM roof.  Fails
without a GPU.  The event time of a single kernel includes the launch gap
between back-to-back calls.
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
    ap.add_argument("--scale", type=int, default=2)
    ap.add_argument("--tile", type=int, default=33)
    ap.add_argument("--stride", type=int, default=14)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("frame_down_timing: no GPU found")
    import srcnn_amd as S

    torch.cuda.set_device(0)
    W, H, s = a.width, a.height, a.scale
    w, h = W // s, H // s
    CW, CH, cw, ch = (W + 1) // 2, (H + 1) // 2, (w + 1) // 2, (h + 1) // 2
    hw, hh = W // 2, H // 2  # the frame of make_pairs_frame and evaluate_frame
    rng = np.random.default_rng(0)
    cuda = lambda x: torch.from_numpy(x).cuda()
    buf = lambda n: torch.empty(n, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    net = S.Net(64, 32, 9, 1, 5)
    S.preload(net)

    rgba, small_rgba = cuda(rng.integers(0, 256, (H, W, 4), dtype=np.uint8)), buf(h * w * 4)
    y8, u8, v8 = (cuda(rng.integers(0, 256, n, dtype=np.uint8)) for n in (H * W, CH * CW, CH * CW))
    y10 = cuda(rng.integers(0, 1024, H * W).astype(np.uint16))
    uv10 = cuda((rng.integers(0, 1024, 2 * CH * CW) << 6).astype(np.uint16))  # P010 pairs
    p010 = cuda((rng.integers(0, 1024, H * W) << 6).astype(np.uint16))        # a plane of W / 2 x H pairs
    o8, o8u, o8v, o16, o16c = buf(h * w), buf(ch * cw), buf(ch * cw), buf(2 * h * w), buf(4 * ch * cw)

    f8 = S.yuv_format(8, 0, S.YUV_PLANAR, 2, 2, S.YUV_LIMITED)
    fp = S.yuv_format(10, 1, S.YUV_SEMIPLANAR, 2, 2, S.YUV_LIMITED)
    src8, dst8 = S.yuv_frame(y8, u8, v8, W, CW), S.yuv_frame(o8, o8u, o8v, w, cw)
    srcp, dstp = S.yuv_frame(p010, uv10, None, 2 * W, 4 * CW), S.yuv_frame(o16, o16c, None, 2 * w, 4 * cw)

    tile, stride = a.tile, a.stride
    count, nx, ny = S.make_pairs_count(hw, hh, s, tile, stride)
    X, T = (torch.empty(count * tile * tile, dtype=torch.float32, device="cuda") for _ in range(2))
    half = S.yuv_frame(y8, u8, v8, hw, (hw + 1) // 2)  # a 1080p frame in the first bytes of the 8-bit planes, tight
    pw_bytes = S.make_pairs_frame_workspace_bytes(f8, hw, hh, s)
    ew_bytes = S.evaluate_frame_workspace_bytes(net, f8, hw, hh, s)
    pws, ews = buf(pw_bytes), buf(ew_bytes)
    params = cuda((0.05 * rng.standard_normal(S.net_param_count(net))).astype(np.float32))
    result = torch.empty(16, dtype=torch.float64, device="cuda")

    variants = {
        "downscale_rgba": lambda: S.downscale_rgba(rgba, small_rgba, W, H, s, stream),
        "downscale_planes_y8": lambda: S.downscale_planes(y8, None, W, W, H, o8, None, w, w, h, s, 8, 0, 0, stream),
        "downscale_planes_y10": lambda: S.downscale_planes(y10, None, 2 * W, W, H, o16, None, 2 * w, w, h, s, 10, 0, 0,
                                                           stream),
        "downscale_planes_p010": lambda: S.downscale_planes(p010, None, 2 * W, W // 2, H, o16, None, 2 * w, w // 2, h, s,
                                                            10, 1, 1, stream),
        "downscale_frame_420_8": lambda: S.downscale_frame(f8, src8, dst8, W, H, s, stream),
        "downscale_frame_p010": lambda: S.downscale_frame(fp, srcp, dstp, W, H, s, stream),
        "make_pairs_frame_1080p": lambda: S.make_pairs_frame(f8, half, hw, hh, s, tile, stride, X, T, pws, pw_bytes,
                                                             stream),
        "evaluate_frame_1080p": lambda: S.evaluate_frame(net, f8, half, hw, hh, s, s, params, result, ews, ew_bytes,
                                                         stream),
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

    qw, qh = hw // s, hh // s
    tiles_bytes = 4 * count * tile * tile
    bytes_model = {
        "downscale_rgba": 4 * W * H + 4 * w * h,
        "downscale_planes_y8": W * H + w * h,
        "downscale_planes_y10": 2 * (W * H + w * h),
        "downscale_planes_p010": 2 * (W * H + w * h),
        "downscale_frame_420_8": W * H + w * h + 2 * (CW * CH + cw * ch),
        "downscale_frame_p010": 2 * (W * H + w * h + 2 * (CW * CH + cw * ch)),
        # down, luma16 of the small plane, luma16 of Y, the two gathers
        "make_pairs_frame_1080p": (hw * hh + qw * qh) + (qw * qh + 4 * s * qw * s * qh) + (hw * hh + 4 * hw * hh) +
                                  (4 * s * qw * s * qh + tiles_bytes) + (4 * hw * hh + tiles_bytes),
    }
    for k, b in bytes_model.items():
        t = res[k]["ms_median"] * 1e-3
        res[k].update(bytes=b, share_of_hbm_roof=b / HBM_BYTES_PER_S / t)
    yard = res["downscale_rgba"]
    allowed = yard["ms_median"] + (yard["ms_max"] - yard["ms_min"])
    print(json.dumps({
        "what": "frame_down_timing", "device": S.device_name(), "source": [W, H], "scale": s, "rounds": a.rounds,
        "iters": a.iters, "pairs_1080p": count, "kernels": res,
        "y8_against_rgba": {"ms_allowed": allowed, "ms_y8": res["downscale_planes_y8"]["ms_median"],
                            "no_slower": res["downscale_planes_y8"]["ms_median"] <= allowed},
    }))


if __name__ == "__main__":
    main()
