"""Timing of the any-size resampling kernels (csrc/hip/resize.hip).

  target:      the general kernels, srcnn_upscale_frame_to (8-bit 4:2:0) and
               srcnn_upscale_to at 1280 x 720 -> 1920 x 1080
  generality:  the general kernels at 1920 x 1080 -> 3840 x 2160 against the
               templated upscale_luma<2>, upscale_compose<2>,
               yuv_upscale_luma<2> and upscale_planes_u8<2> at the same shape,
               and srcnn_upscale_to against srcnn_upscale end to end

Everything runs in this process, the variants of a group alternating, timed
with device events after a warm-up (tools/upscale_timing.py's method).  Prints
one JSON line: the median and the spread of each, the bytes each kernel moves
(computed from the shapes), its share of the 8 TB/s HBM roof, and each
general / templated ratio beside the bar (1.5 per kernel, 1.03 end to end).
Fails without a GPU.  The event times of single kernels include the launch gap.
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
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("resize_timing: no GPU found")
    import srcnn_amd as S

    torch.cuda.set_device(0)
    cfg = (64, 32, 9, 1, 5)
    net = S.Net(*cfg)
    pad = cfg[2] + cfg[3] + cfg[4] - 3
    rng = np.random.default_rng(0)
    cuda = lambda x: torch.from_numpy(x).cuda()
    u8 = lambda n: torch.empty(n, dtype=torch.uint8, device="cuda")
    params = cuda((0.05 * rng.standard_normal(S.net_param_count(net))).astype(np.float32))
    S.preload(net)
    stream = torch.cuda.current_stream().cuda_stream
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

    def shape(w, h, W, H, scale):
        """the calls at w x h -> W x H (scale: the templated ones too)"""
        cw, ch, CW, CH = (w + 1) // 2, (h + 1) // 2, (W + 1) // 2, (H + 1) // 2
        rgba = cuda(rng.integers(0, 256, (h, w, 4), dtype=np.uint8))
        y, u, v = (cuda(rng.integers(0, 256, n, dtype=np.uint8)) for n in (w * h, cw * ch, cw * ch))
        Y, U, V = u8(W * H), u8(CW * CH), u8(CW * CH)
        plane = torch.empty((W + pad) * (H + pad), dtype=torch.float32, device="cuda")
        new_luma = cuda(rng.uniform(0, 1, W * H).astype(np.float32))
        rgb = u8(3 * W * H)
        nb = S.upscale_to_workspace_bytes(net, w, h, W, H)
        ws = u8(nb)
        f8 = S.yuv_format(8, 0, S.YUV_PLANAR, 2, 2, S.YUV_LIMITED)
        src, dst = S.yuv_frame(y, u, v, w, cw), S.yuv_frame(Y, U, V, W, CW)
        kernels = {
            "resize_luma": lambda: S.resize_luma(rgba, plane, w, h, W, H, pad, stream),
            "resize_compose": lambda: S.resize_compose(rgba, new_luma, rgb, w, h, W, H, stream),
            "yuv_resize_luma": lambda: S.yuv_resize_luma(y, w, plane, w, h, W, H, pad, 8, 0, S.YUV_LIMITED, stream),
            "resize_planes": lambda: S.resize_planes(u, v, cw, cw, ch, U, V, CW, CW, CH, w, W, h, H, 8, 0,
                                                     S.YUV_PLANAR, stream),
        }
        nets = {
            "upscale_to": lambda: S.upscale_to(net, rgba, w, h, W, H, params, rgb, ws, nb, stream),
            "upscale_frame_to": lambda: S.upscale_frame_to(net, f8, src, dst, w, h, W, H, params, ws, nb, stream),
        }
        if scale:
            kernels.update({
                "upscale_luma": lambda: S.upscale_luma(rgba, plane, w, h, scale, pad, stream),
                "upscale_compose": lambda: S.upscale_compose(rgba, new_luma, rgb, w, h, scale, stream),
                "yuv_upscale_luma": lambda: S.yuv_upscale_luma(y, w, plane, w, h, scale, pad, S.YUV_LIMITED, stream),
                "upscale_planes_u8": lambda: S.upscale_planes_u8(u, v, cw, cw, ch, U, V, CW, CW, CH, scale, stream),
            })
            nets.update({
                "upscale": lambda: S.upscale(net, rgba, w, h, scale, params, rgb, ws, nb, stream),
                "upscale_frame": lambda: S.upscale_frame(net, f8, src, dst, w, h, scale, params, ws, nb, stream),
            })
        plane_b = 4 * (W + pad) * (H + pad)
        model = {"resize_luma": 4 * w * h + plane_b, "resize_compose": 4 * w * h + 7 * W * H,
                 "yuv_resize_luma": w * h + plane_b, "resize_planes": 2 * (cw * ch + CW * CH)}
        model.update(upscale_luma=model["resize_luma"], upscale_compose=model["resize_compose"],
                     yuv_upscale_luma=model["yuv_resize_luma"], upscale_planes_u8=model["resize_planes"])
        per_kernel, end_to_end = alternate(kernels), alternate(nets)
        for k, t in per_kernel.items():
            t.update(bytes=model[k], share_of_hbm_roof=model[k] / HBM_BYTES_PER_S / (t["ms_median"] * 1e-3))
        return {"source": [w, h], "output": [W, H], "kernels": per_kernel, "end_to_end": end_to_end}

    target = shape(1280, 720, 1920, 1080, 0)
    general = shape(1920, 1080, 3840, 2160, 2)
    S.event_destroy(e0)
    S.event_destroy(e1)
    k, n = general["kernels"], general["end_to_end"]
    ratio = lambda d, g, t: d[g]["ms_median"] / d[t]["ms_median"]
    bars = {"resize_luma_over_upscale_luma": ratio(k, "resize_luma", "upscale_luma"),
            "resize_compose_over_upscale_compose": ratio(k, "resize_compose", "upscale_compose"),
            "yuv_resize_luma_over_yuv_upscale_luma": ratio(k, "yuv_resize_luma", "yuv_upscale_luma"),
            "resize_planes_over_upscale_planes_u8": ratio(k, "resize_planes", "upscale_planes_u8"),
            "kernel_limit": 1.5,
            "upscale_to_over_upscale": ratio(n, "upscale_to", "upscale"),
            "upscale_frame_to_over_upscale_frame": ratio(n, "upscale_frame_to", "upscale_frame"),
            "end_to_end_limit": 1.03}
    print(json.dumps({"what": "resize_timing", "device": S.device_name(), "net": list(cfg), "rounds": a.rounds,
                      "iters": a.iters, "target": target, "generality": general, "bars": bars}))


if __name__ == "__main__":
    main()
