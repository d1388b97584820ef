"""Two builds of libsrcnn_hip.so alternating in one process: the five end-to-end
calls of the upscale family (srcnn_upscale and srcnn_upscale_frame at 1920 x
1080 x2, srcnn_upscale_to and srcnn_upscale_frame_to at 1280 x 720 -> 1920 x
1080, srcnn_evaluate on a 3840 x 2160 truth at x2), for a change to the host
side that the kernels should not see.

  tools/upscale_flow_ab.py --parent PATH/libsrcnn_hip.so [--new PATH]

Timed with device events after a warm-up, as tools/upscale_timing.py and
tools/resize_timing.py time their variants.  Prints one JSON line: per call the
median and the min-max of each library, whether the new median lies within the
parent's own min-max, and whether both wrote the same bytes.  Fails without a
GPU."""
import argparse
import ctypes
import importlib.util
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cnn-super-resolution_amd")
import numpy as np  # noqa: E402
import torch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--parent", required=True, help="the library to compare against")
ap.add_argument("--new", default=os.path.join(PKG, "lib", "libsrcnn_hip.so"))
ap.add_argument("--rounds", type=int, default=30, help="timed windows per call and library")
ap.add_argument("--iters", type=int, default=20, help="calls per window")
ap.add_argument("--warmup", type=int, default=5)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("upscale_flow_ab: no GPU found")
ROUNDS, ITERS, WARMUP = a.rounds, a.iters, a.warmup


def load(name, lib):
    """srcnn_amd bound to `lib`, as a module of its own"""
    os.environ["SRCNN_HIP_LIB"] = lib
    spec = importlib.util.spec_from_file_location(name, os.path.join(PKG, "srcnn_amd", "__init__.py"))
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    assert m.LIB_PATH == lib
    return m


LIBS = {"parent": load("srcnn_parent", os.path.abspath(a.parent)), "new": load("srcnn_new", os.path.abspath(a.new))}
addr = lambda m: ctypes.cast(m.lib().srcnn_upscale, ctypes.c_void_p).value
assert addr(LIBS["parent"]) != addr(LIBS["new"]), "one library loaded twice"

torch.cuda.set_device(0)
cfg = (64, 32, 9, 1, 5)
rng = np.random.default_rng(0)
cuda = lambda x: torch.from_numpy(x).cuda()
u8 = lambda n: torch.empty(n, dtype=torch.uint8, device="cuda")
stream = torch.cuda.current_stream().cuda_stream
S0 = LIBS["new"]
params = cuda((0.05 * rng.standard_normal(S0.net_param_count(S0.Net(*cfg)))).astype(np.float32))


def rows(S, out):
    net = S.Net(*cfg)
    S.preload(net)
    r = {}

    def shape(w, h, W, H, scale):
        cw, ch, CW, CH = (w + 1) // 2, (h + 1) // 2, (W + 1) // 2, (H + 1) // 2
        rgba = cuda(rng.integers(0, 256, (h, w, 4), dtype=np.uint8))
        y, u, v = (cuda(rng.integers(0, 256, n, dtype=np.uint8)) for n in (w * h, cw * ch, cw * ch))
        Y, U, V = u8(W * H), u8(CW * CH), u8(CW * CH)
        rgb = u8(3 * W * H)
        f8 = S.yuv_format(8, 0, S.YUV_PLANAR, 2, 2, S.YUV_LIMITED)
        src, dst = S.yuv_frame(y, u, v, w, cw), S.yuv_frame(Y, U, V, W, CW)
        keep = (rgba, y, u, v, Y, U, V, rgb)
        if scale:
            nb = S.upscale_workspace_bytes(net, w, h, scale)
            assert nb == S.upscale_yuv_workspace_bytes(net, w, h, scale)
            ws = u8(nb)
            r["srcnn_upscale"] = lambda k=keep: S.upscale(net, rgba, w, h, scale, params, rgb, ws, nb, stream)
            r["srcnn_upscale_frame"] = lambda k=keep: S.upscale_frame(net, f8, src, dst, w, h, scale, params, ws, nb, stream)
            out["rgb"], out["Y"], out["U"] = rgb, Y, U
        else:
            nb = S.upscale_to_workspace_bytes(net, w, h, W, H)
            assert nb == S.upscale_frame_to_workspace_bytes(net, w, h, W, H)
            ws = u8(nb)
            r["srcnn_upscale_to"] = lambda k=keep: S.upscale_to(net, rgba, w, h, W, H, params, rgb, ws, nb, stream)
            r["srcnn_upscale_frame_to"] = lambda k=keep: S.upscale_frame_to(net, f8, src, dst, w, h, W, H, params, ws, nb, stream)
            out["rgb_to"], out["Y_to"], out["U_to"] = rgb, Y, U

    shape(1920, 1080, 3840, 2160, 2)
    shape(1280, 720, 1920, 1080, 0)
    W, H = 3840, 2160
    truth = cuda(rng.integers(0, 256, (H, W, 4), dtype=np.uint8))
    nb = S.evaluate_workspace_bytes(net, W, H, 2)
    ws, res = u8(nb), torch.zeros(6, dtype=torch.float64, device="cuda")
    r["srcnn_evaluate"] = lambda: S.evaluate(net, truth, W, H, 2, 4, params, res, ws, nb, stream)
    out["evaluate"] = res
    return r


# the same inputs for both: reseed
outs, variants = {}, {}
for name, S in LIBS.items():
    rng = np.random.default_rng(1)
    outs[name] = {}
    for k, fn in rows(S, outs[name]).items():
        variants[(k, name)] = fn

e0, e1 = S0.event_create(), S0.event_create()


def window(fn):
    S0.event_record(e0, stream)
    for _ in range(ITERS):
        fn()
    S0.event_record(e1, stream)
    S0.event_sync(e1)
    return S0.event_elapsed_ms(e0, e1) / ITERS


for fn in variants.values():
    for _ in range(WARMUP):
        fn()
torch.cuda.synchronize()
# what both computed, byte for byte
same = {k: bool(torch.equal(outs["parent"][k], outs["new"][k])) for k in outs["new"]}
times = {k: [] for k in variants}
keys = sorted({k for k, _ in variants})
for _ in range(ROUNDS):
    for k in keys:
        for name in ("parent", "new"):
            times[(k, name)].append(window(variants[(k, name)]))
torch.cuda.synchronize()
table = {}
for k in keys:
    p, n = times[(k, "parent")], times[(k, "new")]
    table[k] = {"parent_median": statistics.median(p), "parent_min": min(p), "parent_max": max(p),
                "new_median": statistics.median(n), "new_min": min(n), "new_max": max(n),
                "new_median_within_parent_spread": min(p) <= statistics.median(n) <= max(p)}
res = {"what": "upscale_flow_ab", "device": S0.device_name(), "rounds": ROUNDS, "iters": ITERS, "ms": table,
       "outputs_equal": same}
print(json.dumps(res))
