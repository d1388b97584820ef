"""Timing of srcnn_quality_frame.

  srcnn_quality_frame on a pair of 3840 x 2160 4:2:0 frames, shave 2: 8-bit
  planar, 10-bit planar, and P010 (10 bits in the high bits, semi-planar)
  against 10-bit planar;
  and, as the same-session yardstick, srcnn_quality on two LUMA_F32 planes of
  that size: quality_tiles' arithmetic on 4-byte samples and no chroma.

All run in this process, alternating, timed with device events after a
warm-up: windows of --iters calls, --rounds windows per variant, medians with
min - max.  Prints one JSON line: the times, the bytes each call must move
(both frames once; the halo re-reads and the partial sums are left out), its
share of the 8 TB/s HBM roof and its ratio to the yardstick.  Fails without a
GPU.  The event time of a call includes the launch gaps between its kernels
and between back-to-back calls.
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
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("quality_frame_timing: no GPU found")
    import srcnn_amd as S

    torch.cuda.set_device(0)
    W, H, shave = a.width, a.height, a.shave
    cw, ch = (W + 1) // 2, (H + 1) // 2
    rng = np.random.default_rng(0)
    cuda = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    keep = []

    def frame(bits, msb, semi, like=None):
        """a random frame (or `like`'s values plus noise) on the device: (YuvFormat, YuvFrame, the values)"""
        dt, B = (np.uint8, 1) if bits == 8 else (np.uint16, 2)
        if like is None:
            vals = [rng.integers(0, 2 ** bits, s) for s in ((H, W), (ch, cw), (ch, cw))]
        else:
            vals = [np.clip(v + rng.integers(-6, 7, v.shape) * 2 ** (bits - 8), 0, 2 ** bits - 1) for v in like]
        y, u, v = ((x << ((16 - bits) if msb else 0)).astype(dt) for x in vals)
        planes = [cuda(y), cuda(np.stack([u, v], axis=-1))] if semi else [cuda(y), cuda(u), cuda(v)]
        keep.extend(planes)
        fr = S.yuv_frame(planes[0], planes[1], None if semi else planes[2], W * B, cw * B * (2 if semi else 1))
        return S.yuv_format(bits, msb, S.YUV_SEMIPLANAR if semi else S.YUV_PLANAR, 2, 2, S.YUV_LIMITED), fr, vals

    fa8, a8, v8 = frame(8, 0, False)
    fb8, b8, _ = frame(8, 0, False, v8)
    fa10, a10, v10 = frame(10, 0, False)
    fb10, b10, _ = frame(10, 0, False, v10)
    fp10, p10, _ = frame(10, 1, True, v10)
    la = cuda(rng.random((H, W), dtype=np.float32))
    lb = cuda(np.clip(la.cpu().numpy() + 0.02 * rng.standard_normal((H, W)).astype(np.float32), 0, 1))
    res = torch.zeros(8, dtype=torch.float64, device="cuda")
    f_bytes = S.quality_frame_workspace_bytes(W, H, 2, 2, shave)
    f_ws = torch.empty(f_bytes, dtype=torch.uint8, device="cuda")
    q_bytes = S.quality_workspace_bytes(W, H, shave)
    q_ws = torch.empty(q_bytes, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    S.preload(S.Net(64, 32, 9, 1, 5))

    qf = lambda fa, x, fb, y: (lambda: S.quality_frame(fa, x, fb, y, W, H, shave, res, f_ws, f_bytes, stream))
    variants = {
        "quality_frame_8bit_planar": qf(fa8, a8, fb8, b8),
        "quality_frame_10bit_planar": qf(fa10, a10, fb10, b10),
        "quality_frame_p010_vs_planar": qf(fp10, p10, fa10, a10),
        "quality_luma_f32": lambda: S.quality(la, S.PIX_LUMA_F32, W, lb, S.PIX_LUMA_F32, W, W, H, shave, res, q_ws,
                                              q_bytes, stream),
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

    samples = W * H + 2 * cw * ch
    bytes_model = {"quality_frame_8bit_planar": 2 * samples, "quality_frame_10bit_planar": 4 * samples,
                   "quality_frame_p010_vs_planar": 4 * samples, "quality_luma_f32": 8 * W * H}
    yard = out["quality_luma_f32"]["ms_median"]
    for k, b in bytes_model.items():
        out[k].update(bytes=b, share_of_hbm_roof=b / HBM_BYTES_PER_S / (out[k]["ms_median"] * 1e-3),
                      ratio_to_yardstick=out[k]["ms_median"] / yard)
    torch.cuda.synchronize()
    print(json.dumps({
        "what": "quality_frame_timing", "device": S.device_name(), "frames": [W, H], "chroma": "4:2:0",
        "shave": shave, "rounds": a.rounds, "iters": a.iters, "yardstick_ms": yard, "kernels": out,
    }))


if __name__ == "__main__":
    main()
