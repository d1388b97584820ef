"""Timing of the Y'CbCr frame paths against the RGBA path at the same size
(DESIGN.md 14.4 and 15.4).

  yuv:   srcnn_upscale_yuv, 1920 x 1080 4:2:0 full range x2 -> 3840 x 2160
  rgba:  srcnn_upscale, 1920 x 1080 RGBA x2 -> 3840 x 2160 RGB (default net)
  p10:   srcnn_upscale_frame, the same frame at 10 bits, planar (values in the
         low bits of two-byte words)
  P010:  srcnn_upscale_frame, 10 bits in the high bits, chroma as (U, V) pairs

All run in this process, alternating, timed with device events after a
warm-up; then the op-level kernels of all, alternating in the same way.
Prints one JSON line: the median and the min - max of each, the bytes each
kernel moves (computed from the shapes), its share of the 8 TB/s HBM roof, and
the bars.  The three of DESIGN.md 14.4: a new median must not exceed the old
median plus the old variant's own min - max spread in this run.  Those of
DESIGN.md 15.4, one per deep kernel: its median must not exceed its 8-bit
counterpart's median times the ratio of the two byte models, plus the
counterpart's own min - max spread; the deep end-to-end times are reported
beside srcnn_upscale_yuv's without a bar.  Fails without a GPU.  The event
times of single kernels include the launch gap.
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
        sys.exit("video_timing: no GPU found")
    import srcnn_amd as S

    torch.cuda.set_device(0)
    cfg = (64, 32, 9, 1, 5)
    net = S.Net(*cfg)
    pad = cfg[2] + cfg[3] + cfg[4] - 3
    w, h, s = a.width, a.height, a.scale
    W, H = s * w, s * h
    cw, ch, CW, CH = (w + 1) // 2, (h + 1) // 2, (W + 1) // 2, (H + 1) // 2
    rng = np.random.default_rng(0)
    cuda = lambda x: torch.from_numpy(x).cuda()
    byt = lambda n: cuda(rng.integers(0, 256, n, dtype=np.uint8))
    params = cuda((0.05 * rng.standard_normal(S.net_param_count(net))).astype(np.float32))
    S.preload(net)

    rgba = byt(4 * w * h)
    rgb = torch.empty(3 * W * H, dtype=torch.uint8, device="cuda")
    y, u, v = byt(w * h), byt(cw * ch), byt(cw * ch)
    Y, U, V = (torch.empty(n, dtype=torch.uint8, device="cuda") for n in (W * H, CW * CH, CW * CH))
    src, dst = S.yuv_frame(y, u, v, w, cw), S.yuv_frame(Y, U, V, W, CW)
    nb_rgba = S.upscale_workspace_bytes(net, w, h, s)
    nb_yuv = S.upscale_yuv_workspace_bytes(net, w, h, s)
    ws_rgba = torch.empty(nb_rgba, dtype=torch.uint8, device="cuda")
    ws_yuv = torch.empty(nb_yuv, dtype=torch.uint8, device="cuda")
    plane = torch.empty((W + pad) * (H + pad), dtype=torch.float32, device="cuda")
    new_luma = cuda(rng.uniform(0, 1, W * H).astype(np.float32))
    stream = torch.cuda.current_stream().cuda_stream
    # the same frame at 10 bits: planar with the values in the low bits, and
    # P010 (high bits, chroma interleaved); pitches in bytes
    wrd = lambda n, sh: cuda((rng.integers(0, 1024, n) << sh).astype("<u2").view(np.uint8))
    y10, u10, v10 = wrd(w * h, 0), wrd(cw * ch, 0), wrd(cw * ch, 0)
    yP, uvP = wrd(w * h, 6), wrd(2 * cw * ch, 6)
    Y10, U10, V10, UV10 = (torch.empty(2 * n, dtype=torch.uint8, device="cuda")
                           for n in (W * H, CW * CH, CW * CH, 2 * CW * CH))
    src10, dst10 = S.yuv_frame(y10, u10, v10, 2 * w, 2 * cw), S.yuv_frame(Y10, U10, V10, 2 * W, 2 * CW)
    srcP, dstP = S.yuv_frame(yP, uvP, None, 2 * w, 4 * cw), S.yuv_frame(Y10, UV10, None, 2 * W, 4 * CW)
    f10 = S.yuv_format(10, 0, S.YUV_PLANAR, 2, 2, S.YUV_FULL)
    fP = S.yuv_format(10, 1, S.YUV_SEMIPLANAR, 2, 2, S.YUV_FULL)

    def back_end_yuv():
        S.yuv_compose_luma(new_luma, Y, W, W, H, S.YUV_FULL, stream)
        S.upscale_planes_u8(u, v, cw, cw, ch, U, V, CW, CW, CH, s, stream)

    end_to_end = {
        "upscale_yuv": lambda: S.upscale_yuv(net, src, dst, w, h, 2, 2, s, S.YUV_FULL, params, ws_yuv, nb_yuv, stream),
        "upscale": lambda: S.upscale(net, rgba, w, h, s, params, rgb, ws_rgba, nb_rgba, stream),
        "upscale_frame_p10": lambda: S.upscale_frame(net, f10, src10, dst10, w, h, s, params, ws_yuv, nb_yuv, stream),
        "upscale_frame_P010": lambda: S.upscale_frame(net, fP, srcP, dstP, w, h, s, params, ws_yuv, nb_yuv, stream),
    }
    kernels = {
        "yuv_upscale_luma": lambda: S.yuv_upscale_luma(y, w, plane, w, h, s, pad, S.YUV_FULL, stream),
        "upscale_luma": lambda: S.upscale_luma(rgba, plane, w, h, s, pad, stream),
        "yuv_back_end": back_end_yuv,
        "upscale_compose": lambda: S.upscale_compose(rgba, new_luma, rgb, w, h, s, stream),
        "yuv_compose_luma": lambda: S.yuv_compose_luma(new_luma, Y, W, W, H, S.YUV_FULL, stream),
        "upscale_planes_u8": lambda: S.upscale_planes_u8(u, v, cw, cw, ch, U, V, CW, CW, CH, s, stream),
        "yuv_upscale_luma16_p10": lambda: S.yuv_upscale_luma16(y10, 2 * w, plane, w, h, s, pad, 10, 0, S.YUV_FULL, stream),
        "yuv_upscale_luma16_P010": lambda: S.yuv_upscale_luma16(yP, 2 * w, plane, w, h, s, pad, 10, 1, S.YUV_FULL, stream),
        "yuv_compose_luma16_p10": lambda: S.yuv_compose_luma16(new_luma, Y10, 2 * W, W, H, 10, 0, S.YUV_FULL, stream),
        "yuv_compose_luma16_P010": lambda: S.yuv_compose_luma16(new_luma, Y10, 2 * W, W, H, 10, 1, S.YUV_FULL, stream),
        "upscale_planes_p10": lambda: S.upscale_planes(u10, v10, 2 * cw, cw, ch, U10, V10, 2 * CW, CW, CH, s, 10, 0,
                                                       S.YUV_PLANAR, stream),
        "upscale_planes_P010": lambda: S.upscale_planes(uvP, None, 4 * cw, cw, ch, UV10, None, 4 * CW, CW, CH, s, 10, 1,
                                                        S.YUV_SEMIPLANAR, stream),
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
        return {k: {"ms_median": statistics.median(t), "ms_min": min(t), "ms_max": max(t)} for k, t in times.items()}

    e2e = alternate(end_to_end)
    per_kernel = alternate(kernels)
    S.event_destroy(e0)
    S.event_destroy(e1)

    bytes_model = {
        "yuv_upscale_luma": w * h + 4 * (W + pad) * (H + pad),
        "upscale_planes_u8": 2 * cw * ch + 2 * CW * CH,
        "yuv_compose_luma": 4 * W * H + W * H,
        "upscale_luma": 4 * w * h + 4 * (W + pad) * (H + pad),
        "upscale_compose": 4 * w * h + 4 * W * H + 3 * W * H,
    }
    # a deep kernel and its 8-bit counterpart
    deep = {"yuv_upscale_luma16": "yuv_upscale_luma", "upscale_planes": "upscale_planes_u8",
            "yuv_compose_luma16": "yuv_compose_luma"}
    deep_bytes = {"yuv_upscale_luma16": 2 * w * h + 4 * (W + pad) * (H + pad),
                  "upscale_planes": 2 * (2 * cw * ch + 2 * CW * CH), "yuv_compose_luma16": 4 * W * H + 2 * W * H}
    for k, b in deep_bytes.items():
        for f in ("p10", "P010"):
            bytes_model[k + "_" + f] = b
    for k, b in bytes_model.items():
        t = per_kernel[k]["ms_median"] * 1e-3
        per_kernel[k].update(bytes=b, share_of_hbm_roof=b / HBM_BYTES_PER_S / t)

    def bar(new, old):
        limit = old["ms_median"] + (old["ms_max"] - old["ms_min"])
        return {"new_ms": new["ms_median"], "old_ms": old["ms_median"], "limit_ms": limit,
                "met": new["ms_median"] <= limit}

    def deep_bar(k, f):
        new, old = per_kernel[k + "_" + f], per_kernel[deep[k]]
        ratio = deep_bytes[k] / bytes_model[deep[k]]
        limit = old["ms_median"] * ratio + (old["ms_max"] - old["ms_min"])
        return {"new_ms": new["ms_median"], "old_ms": old["ms_median"], "bytes_ratio": ratio, "limit_ms": limit,
                "met": new["ms_median"] <= limit}

    print(json.dumps({
        "what": "video_timing", "device": S.device_name(), "source": [w, h], "chroma": "4:2:0", "range": "full",
        "scale": s, "output": [W, H], "net": list(cfg), "rounds": a.rounds, "iters": a.iters,
        "end_to_end": e2e, "kernels": per_kernel,
        "bars": {
            "yuv_upscale_luma_vs_upscale_luma": bar(per_kernel["yuv_upscale_luma"], per_kernel["upscale_luma"]),
            "yuv_back_end_vs_upscale_compose": bar(per_kernel["yuv_back_end"], per_kernel["upscale_compose"]),
            "upscale_yuv_vs_upscale": bar(e2e["upscale_yuv"], e2e["upscale"])},
        "deep_bars": {"%s_%s_vs_%s" % (k, f, deep[k]): deep_bar(k, f) for k in deep for f in ("p10", "P010")},
    }))


if __name__ == "__main__":
    main()
