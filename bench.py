#!/usr/bin/env python3
"""bench.py -- SRCNN training throughput on MI355X (BASELINE.json metric).

Workload (BASELINE.json configs[1]): default SRCNN (n1=64, n2=32, f1=9, f2=1,
f3=5), fp32, 33x33 luma patches, batch 4096 tiles per GPU.  One step = the
reference epoch body: ConfigBasedDataPipeline::execute_batch(backprop) over
the batch (forward L1-L3, last delta, deltas, weight/bias gradients) +
[RCCL all-reduce of the flat gradient buffer when N > 1] +
update_parameters (momentum SGD + weight decay, batch = global tile count)
+ zeroing of the gradient accumulators.  Every kernel is HIP (libsrcnn_hip.so
through its C ABI); inputs are resident in HBM before the timed region.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N

A plain run measures the headline only: set up, settle + W warmup steps, K
timed steps, one JSON line (per-kernel figures from hipEvents on sampled timed
steps ride along).  `--full` adds every other measurement: the wide net, the
256x256 tile and 4K inference lines, the CPU baselines and, with N > 1, the
strong-scaling sub-record and the sharded 4K frame (--no-wide, --no-forward,
--no-cpu-baseline, --no-strong drop single legs of a full run).
`--dump-outputs DIR` writes what the last timed step left a caller with
(DIR/params.npy, momentum.npy, grads.npy, float32); the training state is then
reset to its seeded initial values right before the timed steps, so the dump
depends on the arguments only, not on how many settle steps the clock took.

`--gpus N > 1` without a torch.distributed.run environment launches the N
rank processes itself (torch.distributed.run as a child process, before any
GPU call) and exits with its status; under torch.distributed.run, WORLD_SIZE
must equal --gpus.  Rank 0 prints ONE JSON line.  With --full and N > 1 the line
also carries the strong-scaling step (global batch 4096 sharded over the ranks)
under "strong".  Data is synthetic (smooth random luma patches, seed
1234 + rank; weights N(0, 1e-3), biases 0).
"""
import argparse
import glob
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "cnn-super-resolution_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import torch  # noqa: E402  (device memory / streams / torch.distributed only)
import torch.distributed as dist  # noqa: E402

PEAK_FP32_TFLOPS = 157.3   # MI355X_MICROARCH.md: FP32 vector = FP32 MFMA peak
PEAK_HBM_GBS = 8000.0      # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
NOMINAL_CLOCK_GHZ = 2.4    # MI355X_MICROARCH.md: max clock, the clock PEAK_FP32_TFLOPS assumes
RIDGE = PEAK_FP32_TFLOPS * 1e12 / (PEAK_HBM_GBS * 1e9)
# split-bf16 kernels (srcnn_set_arith 0: l12x6, d1x6) form each fp32 product
# from six bf16 part products on v_mfma_f32_32x32x16_bf16: their matrix-core
# ceiling in fp32-equivalent FLOP/s is the dense BF16 peak (MI355X_MICROARCH.md:
# 1024 FLOP/cycle/SIMD x 1024 SIMDs x 2.4 GHz) / 6
PEAK_BF16_TFLOPS = 2516.6
PEAK_SPLIT_TFLOPS = round(PEAK_BF16_TFLOPS / 6, 1)
SPLIT_KERNELS = {"l12x6_fwd": "l12_fwd_mfma", "l12x6_fwd_lazy": "l12_fwd_mfma", "d1x6_grad12": "delta1_grad12_fused",
                 "d1x6_d3": "delta1_grad12_fused", "l3r_d3": "l3_delta_fused",
                 "wl1x6_fwd": "wide_l1_fwd", "wl2x6_fwd": "wide_l2_fwd", "wd1x6": "wide_delta1", "wg1x6": "wide_grad1",
                 "wgrad2x6": "wide_grad2"}
# the split-bf16 default step moves delta2 out of the layer-3 kernel: l3r
# writes delta3 ("l3r_d3") and d1x6 forms delta2 from it ("d1x6_d3"); set from
# the headline step's kernel list (split_profiled)
D3_MODE = False


def split_profiled(S):
    """Profiler names of the kernels of the last step that ran split-bf16
    (and D3_MODE: whether that step formed delta2 in d1x6)."""
    global D3_MODE
    try:
        ks = S.last_kernels()
    except Exception:
        return set()
    if isinstance(ks, str):
        ks = ks.split(",")
    D3_MODE = D3_MODE or "d1x6_d3" in ks  # (sticky: the wide leg's kernels do not reset it)
    return {SPLIT_KERNELS[k] for k in ks if k in SPLIT_KERNELS}

DEFAULT_NET = (64, 32, 9, 1, 5)
TILE = 33


def layer_work(net, w, h):
    """Algorithmic FLOPs and HBM bytes per tile of every stage:
    each tensor written once and read once per consumer, weights ignored."""
    n1, n2, f1, f2, f3 = net
    w1, h1 = w - f1 + 1, h - f1 + 1
    w2, h2 = w1 - f2 + 1, h1 - f2 + 1
    w3, h3 = w2 - f3 + 1, h2 - f3 + 1
    X, A1, A2, A3 = 4 * w * h, 4 * w1 * h1 * n1, 4 * w2 * h2 * n2, 4 * w3 * h3
    T = 4 * w3 * h3  # centre crop of the ground truth that is read
    m1 = w1 * h1 * n1 * f1 * f1
    m2 = w2 * h2 * n2 * f2 * f2 * n1
    m3 = w3 * h3 * f3 * f3 * n2
    return {
        "l1_fwd": (2 * m1, X + A1),
        "l2_fwd": (2 * m2, A1 + A2),
        "l3_fwd": (2 * m3, A2 + A3),
        "last_delta": (2 * w3 * h3, A3 + T + A3),
        "delta2": (2 * m3, A3 + A2 + A2),
        "delta1": (2 * m2, A2 + A1 + A1),
        "grad3": (2 * m3, A2 + A3),
        "grad2": (2 * m2, A1 + A2),
        "grad1": (2 * m1, X + A1),
    }


# kernel name (srcnn_profile_*) -> the stages it performs
KERNEL_STAGES = {
    # generic path
    "conv_fwd_generic": ["l1_fwd", "l2_fwd", "l3_fwd"],
    "last_delta": ["last_delta"],
    "conv_delta_generic": ["delta2", "delta1"],
    "grad_partial_generic": ["grad1", "grad2", "grad3"],
    # gfx950 specialisations
    "l1_fwd_mfma": ["l1_fwd"],
    "l2_fwd_mfma": ["l2_fwd"],
    "l3_fwd": ["l3_fwd"],
    "l12_fwd_mfma": ["l1_fwd", "l2_fwd"],
    "l3_delta_fused": ["l3_fwd", "last_delta", "delta2", "grad3"],
    "delta2": ["delta2"],
    "delta1_mfma": ["delta1"],
    "grad1_mfma": ["grad1"],
    "grad2_mfma": ["grad2"],
    "grad3": ["grad3"],
    "delta1_grad12_fused": ["delta1", "grad1", "grad2"],
    # wide family (train_wide.hip)
    "wide_l1_fwd": ["l1_fwd"],
    "wide_l2_fwd": ["l2_fwd"],
    "wide_l3_delta": ["l3_fwd", "last_delta", "delta2", "grad3"],
    "wide_delta1_grad1": ["delta1", "grad1"],
    "wide_delta1": ["delta1"],   # split path: wd1x6 (delta1 to D1), then gW1 from D1
    "wide_grad1": ["grad1"],
    "wide_grad2": ["grad2"],
}


def fused_bytes(net, w, h):
    """Minimum HBM bytes per tile of each kernel that fuses stages: every
    input it needs read once, every output it produces written once, weights
    ignored (train_fused.hip, train_wide.hip).  The layer-by-layer figures of
    layer_work() charge the intermediates the fusion never materialises."""
    n1, n2, f1, f2, f3 = net
    w1, h1 = w - f1 + 1, h - f1 + 1
    w2, h2 = w1 - f2 + 1, h1 - f2 + 1
    w3, h3 = w2 - f3 + 1, h2 - f3 + 1
    X, A1, A2, T3 = 4 * w * h, 4 * w1 * h1 * n1, 4 * w2 * h2 * n2, 4 * w3 * h3
    return {
        # default family (f2 = 1)
        "l12_fwd_mfma": X + A1 + A2,             # read X, write A1 and A2
        "l3_delta_fused": A2 + T3 + A2,          # read A2 + centre of T, write delta2
        "delta1_grad12_fused": X + A1 + A2,      # read X, A1, delta2 (delta1 never leaves the CU)
        # wide family (train_wide.hip)
        "wide_l1_fwd": X + A1,                   # read X, write A1
        "wide_l2_fwd": A1 + A2,                  # read A1, write A2
        "wide_l3_delta": A2 + T3 + A2,           # read A2 + centre of T, write delta2 (A3, delta3 stay in)
        "wide_delta1_grad1": X + A1 + A2,        # read X, A1 (relu'), delta2; delta1 stays in registers
        "wide_delta1": A2 + A1,                  # read delta2, write D1 (before relu')
        "wide_grad1": X + A1 + A1,               # read X, D1, A1 (relu')
        "wide_grad2": A1 + A2,                   # read A1, delta2
    }


def step_roof_ms(stats, n, work, tiles, net=DEFAULT_NET, w=TILE, h=TILE, split=()):
    """Fused-minimum step roofline (ms): sum over the kernels that ran of
    max(F / FP32 peak, B_min / HBM peak) with B_min from fused_bytes().  The
    small slab reduction / update launches (no stage work, ~1% of the step)
    count as zero, so this is a lower bound of the step as built.  Kernels
    named in `split` are priced at the split-bf16 peak instead."""
    t = 0.0
    for name, (cnt, _) in stats.items():
        kw = kernel_work(name, work, net, w, h)
        if kw:
            peak = PEAK_SPLIT_TFLOPS if name in split else PEAK_FP32_TFLOPS
            t += cnt / n * max(kw[0] * tiles / (cnt / n) / (peak * 1e12),
                               kw[1] * tiles / (cnt / n) / (PEAK_HBM_GBS * 1e9))
    return t * 1e3


def step_roofline(fused_ms, layerwise_ms, ms, split_ms=None):
    """The step against its fused-minimum roof (t_roof_ms / frac: the bound of
    the kernels as fused) and, for reference, SURVEY.md 8(d)'s layer-by-layer
    roof (each stage's tensors through HBM; the fused kernels can beat it).
    split_ms: the same roof with the split-bf16 kernels at their own peak."""
    # layerwise_ratio: the layer-by-layer roof over the measured step; the
    # fused kernels never move the bytes it charges, so it can exceed 1 (it
    # is a comparison, not a fraction of a roof)
    out = {"t_roof_ms": round(fused_ms, 4), "frac": round(fused_ms / ms, 4),
           "model": "sum over the step's kernels of max(F/157.3 TF, B_min/8 TB/s)",
           "layerwise_t_roof_ms": round(layerwise_ms, 4), "layerwise_ratio": round(layerwise_ms / ms, 4)}
    if split_ms is not None:
        # the split-bf16 kernels priced at the ceiling of the instructions they
        # issue: this is the step's roof ("frac"); the FP32-priced one beside
        out.update({"t_roof_ms": round(split_ms, 4), "frac": round(split_ms / ms, 4),
                    "model": ("sum over the step's kernels of max(F/peak, B_min/8 TB/s), peak = %.1f TF "
                              "for the split-bf16 kernels, 157.3 TF for the fp32 ones" % PEAK_SPLIT_TFLOPS),
                    "fp32_t_roof_ms": round(fused_ms, 4), "frac_fp32_equiv": round(fused_ms / ms, 4)})
    return out


# D3_MODE: the two kernels around delta2 (l3r writes delta3, d1x6 forms delta2)
D3_STAGES = {"l3_delta_fused": ["l3_fwd", "last_delta", "grad3"],
             "delta1_grad12_fused": ["delta2", "delta1", "grad1", "grad2"]}


def d3_bytes(net, w, h):
    """fused_bytes() of the D3_MODE pair: l3r reads A2 + the centre of T and
    writes delta3; d1x6 reads X, A1, A2 (relu' of layer 2) and delta3."""
    n1, n2, f1, f2, f3 = net
    w1, h1 = w - f1 + 1, h - f1 + 1
    w2, h2 = w1 - f2 + 1, h1 - f2 + 1
    w3, h3 = w2 - f3 + 1, h2 - f3 + 1
    X, A1, A2, T3 = 4 * w * h, 4 * w1 * h1 * n1, 4 * w2 * h2 * n2, 4 * w3 * h3
    return {"l3_delta_fused": A2 + T3 + T3, "delta1_grad12_fused": X + A1 + A2 + T3}


def kernel_work(name, work, net, w, h):
    """(algorithmic FLOPs, algorithmic HBM bytes) per tile of one kernel."""
    if D3_MODE and tuple(net) == DEFAULT_NET and name in D3_STAGES:
        return sum(work[s][0] for s in D3_STAGES[name]), d3_bytes(net, w, h)[name]
    stages = KERNEL_STAGES.get(name)
    if not stages:
        return None
    flops = sum(work[s][0] for s in stages)
    nbytes = fused_bytes(net, w, h).get(name, sum(work[s][1] for s in stages))
    return flops, nbytes


def held_clock(S, name):
    """Shader clock (GHz) the chip held during the last launch of `name`
    (in-kernel s_memtime / s_memrealtime probe, srcnn_profile_clock), or None."""
    try:
        return S.profile_clock(name)
    except Exception:
        return None


def add_clock(out, ghz):
    """Beside the nominal-clock fraction: the same achieved rate against the
    peak scaled to the clock the chip held (MI355X_MICROARCH.md DVFS)."""
    if out is None or not ghz:
        return out
    out["held_clock_ghz"] = round(ghz, 3)
    if out["bound"] == "mfma":
        out["frac_at_held_clock"] = round(out["frac"] * NOMINAL_CLOCK_GHZ / ghz, 4)
    return out


def roofline_of(name, launches_per_step, ms_per_step, work, tiles, pmc=None, net=DEFAULT_NET,
                w=TILE, h=TILE, split=False):
    kw = kernel_work(name, work, net, w, h)
    if not kw or ms_per_step <= 0:
        return None
    flops = kw[0] * tiles / launches_per_step
    nbytes = kw[1] * tiles / launches_per_step
    dur_s = ms_per_step / launches_per_step * 1e-3
    traffic = None
    if pmc and name in pmc:
        traffic = pmc[name]
    # the ceiling of the instructions the kernel issues: FP32 MFMA, or for the
    # split-bf16 kernels the BF16 MFMA peak / 6 part products (verdict r05
    # weak #2); the bound is whichever of compute and HBM time is larger
    peak_c = PEAK_SPLIT_TFLOPS if split else PEAK_FP32_TFLOPS
    ach_tf = flops / dur_s / 1e12
    if flops / (peak_c * 1e12) >= nbytes / (PEAK_HBM_GBS * 1e9):
        out = {"bound": "mfma", "achieved": round(ach_tf, 3), "peak": peak_c, "unit": "TFLOP/s",
               "frac": round(ach_tf / peak_c, 4)}
    else:
        ach = nbytes / dur_s / 1e9
        out = {"bound": "hbm", "achieved": round(ach, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
               "frac": round(ach / PEAK_HBM_GBS, 4),
               "compute_tflops": round(ach_tf, 3), "compute_frac": round(ach_tf / peak_c, 4)}
    out.update({"traffic": traffic, "kernel": name, "avg_launch_ms": round(dur_s * 1e3, 5),
                "algorithmic_flops_per_launch": int(flops), "algorithmic_bytes_per_launch": int(nbytes)})
    if split:
        out["arith"] = "split-bf16 x6"
        out["peak_model"] = ("BF16 MFMA %.1f TF / 6 part products = %.1f TF fp32-equivalent"
                             % (PEAK_BF16_TFLOPS, PEAK_SPLIT_TFLOPS))
        # the same rate against the FP32 MFMA peak (what it would be on fp32
        # MFMA instructions; can exceed 1)
        out["frac_fp32_equiv"] = round(ach_tf / PEAK_FP32_TFLOPS, 4)
    return out


def load_pmc():
    """Per-launch HBM bytes from the committed rocprofv3 PMC summary
    (profiles/pmc_*.json, written by profiles/pmc_summary.py)."""
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "pmc_*.json")))
    if not files:
        return None
    try:
        with open(files[-1]) as fh:
            data = json.load(fh)
        return {k: v["hbm_bytes_per_launch"] for k, v in data.get("kernels", {}).items()}
    except Exception:
        return None


def init_params(net, P):
    """weights N(0, 1e-3), biases 0; identical on every rank."""
    n1, n2, f1, f2, f3 = net
    sizes = [f1 * f1 * n1, n1, f2 * f2 * n1 * n2, n2, f3 * f3 * n2, 1]
    assert sum(sizes) == P
    wrng = np.random.default_rng(1234)
    out, o = np.zeros(P, np.float32), 0
    for i, n in enumerate(sizes):
        if i % 2 == 0:
            out[o:o + n] = 1e-3 * wrng.standard_normal(n)
        o += n
    return out


def synthetic_batch(rng, batch, w, h):
    """Smooth random luma patches (uniform grid upsampled x4, clipped), input
    mean-subtracted per patch (Main_cl.cpp:141), target = patch + N(0, 0.02)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from hip_util import make_batch
    return make_batch(rng, batch, w, h)


def host_cores():
    """CPU cores this process may run on, and the team size the baseline uses:
    every core of the affinity mask, unless the host's OMP_NUM_THREADS says
    otherwise (the GPU box sets it to the 16-core share of one GPU)."""
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:  # pragma: no cover
        avail = os.cpu_count() or 1
    want = int(os.environ.get("OMP_NUM_THREADS", "0") or 0) or avail
    return avail, want


def threads_source():
    """Where the CPU baseline's thread count comes from (reported beside it)."""
    if os.environ.get("OMP_NUM_THREADS"):
        return ("OMP_NUM_THREADS=%s (the host's per-GPU CPU share on the GPU box; the other "
                "host CPUs belong to the other GPUs' jobs)" % os.environ["OMP_NUM_THREADS"])
    return "every CPU of the affinity mask"


def cpu_baseline(net, tiles_min=16, budget_s=12.0):
    """Time the CPU restatement of the reference path (oracle/, OpenMP) on a
    bounded sample of the same workload."""
    import srcnn_oracle as orc
    avail, want = host_cores()
    threads = orc.set_threads(want)
    rng = np.random.default_rng(1234)
    batch = max(tiles_min, threads * 2)
    X, T = synthetic_batch(rng, batch, TILE, TILE)
    params = init_params(net, orc.param_count(*net))
    P = params.size
    grads = np.zeros(P, np.float32)
    mom = np.zeros(P, np.float32)
    lr = [1e-4, 1e-4, 1e-5]
    orc.train_fwd_bwd(net, X[:TILE * TILE], T[:TILE * TILE], TILE, TILE, 1, params, grads)  # warm
    done, t0 = 0, time.perf_counter()
    while True:
        grads, _ = orc.train_fwd_bwd(net, X, T, TILE, TILE, batch, params, grads)
        params, grads, mom = orc.update_all(net, params, grads, mom, 0.9, 1e-3, lr, batch)
        done += batch
        el = time.perf_counter() - t0
        if el >= budget_s:
            break
    return {"value": round(done / el, 2), "unit": "tiles/s", "cores": threads, "host_cpus": avail,
            "cores_from": threads_source(),
            "kind": "port",
            "sample": "%d tiles of 33x33 (default net, fwd+bwd+update) in %.1fs with the oracle C "
                      "restatement (oracle/srcnn_oracle.c), OpenMP over tiles" % (done, el)}


def forward_flops(net, w, h):
    """Algorithmic FLOPs of the three layers over one w x h frame."""
    n1, n2, f1, f2, f3 = net
    w1, h1 = w - f1 + 1, h - f1 + 1
    w2, h2 = w1 - f2 + 1, h1 - f2 + 1
    w3, h3 = w2 - f3 + 1, h2 - f3 + 1
    return 2.0 * (w1 * h1 * n1 * f1 * f1 + w2 * h2 * n2 * n1 * f2 * f2 + w3 * h3 * n2 * f3 * f3)


def cpu_forward_baseline(net, strip_rows=256, reps=3):
    """CPU restatement of the reference forward (oracle_forward, OpenMP over
    output rows): BASELINE.json configs[0] (one 256x256 luma tile: ms and
    GFLOP/s) and configs[4] measured on a bounded strip of the 3840x2160
    frame (3840 x strip_rows input rows), reported as input Mpix/s."""
    import srcnn_oracle as orc
    avail, want = host_cores()
    threads = orc.set_threads(want)
    prm = init_params(net, orc.param_count(*net))
    rng = np.random.default_rng(5)
    out = {"cores": threads, "host_cpus": avail, "cores_from": threads_source(), "kind": "port"}
    x = (rng.random(256 * 256, dtype=np.float32) - 0.5)
    orc.forward(net, x, 256, 256, 1, prm)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        orc.forward(net, x, 256, 256, 1, prm)
        ts.append(time.perf_counter() - t0)
    t = sorted(ts)[len(ts) // 2]
    out["tile_256"] = {"ms": round(t * 1e3, 3), "gflop_s": round(forward_flops(net, 256, 256) / t / 1e9, 2),
                       "sample": "median of %d forwards of one 256x256 tile (configs[0])" % reps}
    x = (rng.random(3840 * strip_rows, dtype=np.float32) - 0.5)
    t0 = time.perf_counter()
    orc.forward(net, x, 3840, strip_rows, 1, prm)
    t = time.perf_counter() - t0
    out["frame_4k"] = {"mpix_s": round(3840 * strip_rows / t / 1e6, 3),
                       "gflop_s": round(forward_flops(net, 3840, strip_rows) / t / 1e9, 2),
                       "sample": "one 3840x%d strip of the 3840x2160 frame (configs[4]) in %.2fs"
                                 % (strip_rows, t)}
    return out


def forward_4k(S, net_t, frames=20, warmup=3, w=3840, h=2160, settle_ms=50.0):
    """BASELINE.json configs[4]: forward-only inference of one 3840x2160 luma
    frame (fused path), reported as input Mpix/s.  Time with events on the
    stream the kernels run on; per-kernel split from srcnn_profile_*."""
    net = S.Net(*net_t)
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(4)
    x = torch.from_numpy((rng.random(w * h, dtype=np.float32) - 0.5)).to(dev)
    prm = torch.from_numpy(init_params(net_t, S.net_param_count(net))).to(dev)
    n1, n2, f1, f2, f3 = net_t
    out = torch.empty((w - (f1 + f2 + f3 - 3)) * (h - (f1 + f2 + f3 - 3)), device=dev)
    nbytes = S.forward_workspace_bytes(net, w, h, 1)
    ws = torch.empty(nbytes // 4 + 64, device=dev)
    # the frames follow the 0.5 s pause after the wide net: without settle()
    # they time the clock ramp (rocprofv3, profiles/r05_clock: 1.19 -> 1.03 ms
    # for the first 20 frames' fwd_l123)
    n_settle = settle(lambda: S.forward(net, x, w, h, 1, prm, out, ws, nbytes, stream), settle_ms,
                      torch.cuda.synchronize, 1, "gloo", dev)
    for _ in range(warmup):
        S.forward(net, x, w, h, 1, prm, out, ws, nbytes, stream)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(frames):
        S.forward(net, x, w, h, 1, prm, out, ws, nbytes, stream)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    # per-kernel split: one more frame with hipEvents around its launches
    S.profile_reset()
    S.profile_enable(True)
    S.forward(net, x, w, h, 1, prm, out, ws, nbytes, stream)
    torch.cuda.synchronize()
    S.profile_enable(False)
    stats = S.profile_stats()
    ms = el / frames * 1e3
    # algorithmic work: the three layers over the frame
    flops = forward_flops(net_t, w, h)
    kernels = {k: {"launches_per_frame": c, "ms_per_frame": round(t, 4)} for k, (c, t) in stats.items()}
    kname = "fwd_l123_mfma"
    kroof = None
    if kname in stats:
        cnt, kms = stats[kname]
        kdur = kms / cnt * 1e-3
        ach = flops / kdur / 1e12  # the seam kernel's adds are ~0.01% of the frame's FLOPs
        split = tuple(net_t) == DEFAULT_NET and S.get_arith() == 0  # fwd_l123x6 (split-bf16)
        peak = PEAK_SPLIT_TFLOPS if split else PEAK_FP32_TFLOPS
        kroof = {"bound": "mfma", "achieved": round(ach, 3), "peak": peak, "unit": "TFLOP/s",
                 "frac": round(ach / peak, 4), "kernel": kname, "avg_launch_ms": round(kdur * 1e3, 5),
                 "algorithmic_flops_per_launch": int(flops), "traffic": None}
        if split:
            kroof.update({"arith": "split-bf16 x6",
                          "peak_model": ("BF16 MFMA %.1f TF / 6 part products" % PEAK_BF16_TFLOPS),
                          "frac_fp32_equiv": round(ach / PEAK_FP32_TFLOPS, 4)})
    else:
        split, peak = False, PEAK_FP32_TFLOPS
    res = {"frame": "%dx%d" % (w, h), "frames": frames, "settle_frames": n_settle, "ms_per_frame": round(ms, 4),
           "mpix_s": round(w * h / (ms * 1e-3) / 1e6, 1),
           "tflops": round(flops / (ms * 1e-3) / 1e12, 2),
           "roofline_frac": round(flops / (ms * 1e-3) / 1e12 / peak, 4),
           "roofline_peak_tflops": peak,
           "algorithmic_gflop_per_frame": round(flops / 1e9, 2), "kernels": kernels,
           "kernel_path": S.last_path(), "roofline": add_clock(kroof, held_clock(S, kname))}
    if split:
        res["roofline_frac_fp32_equiv"] = round(flops / (ms * 1e-3) / 1e12 / PEAK_FP32_TFLOPS, 4)
    ghz = held_clock(S, "fwd_l123_mfma")
    if ghz:
        res["held_clock_ghz"] = round(ghz, 3)
        res["roofline_frac_at_held_clock"] = round(res["roofline_frac"] * NOMINAL_CLOCK_GHZ / ghz, 4)
    return res


def forward_tile_256(S, net_t, reps=20):
    """BASELINE.json configs[0] on the GPU: one 256x256 luma tile through the
    fused inference kernels (srcnn_forward), ms per tile, beside the CPU
    restatement's time for the same tile (cpu_forward_baseline)."""
    net = S.Net(*net_t)
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.current_stream().cuda_stream
    w = h = 256
    rng = np.random.default_rng(256)
    x = torch.from_numpy((rng.random(w * h, dtype=np.float32) - 0.5)).to(dev)
    prm = torch.from_numpy(init_params(net_t, S.net_param_count(net))).to(dev)
    pad = net_t[2] + net_t[3] + net_t[4] - 3
    out = torch.empty((w - pad) * (h - pad), device=dev)
    nbytes = S.forward_workspace_bytes(net, w, h, 1)
    ws = torch.empty(nbytes // 4 + 64, device=dev)
    for _ in range(3):
        S.forward(net, x, w, h, 1, prm, out, ws, nbytes, stream)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        S.forward(net, x, w, h, 1, prm, out, ws, nbytes, stream)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / reps * 1e3
    return {"tile": "256x256", "ms": round(ms, 4), "gflop_s": round(forward_flops(net_t, w, h) / (ms * 1e-3) / 1e9, 1),
            "kernel_path": S.last_path(), "reps": reps}


def forward_4k_sharded(S, net_t, rank, world, reduce_max, backend, frames=10, warmup=3, w=3840, h=2160,
                       settle_ms=50.0):
    """BASELINE.json configs[4] on N GPUs: the 3840x2160 frame sharded by row
    bands with a 12-row halo (parallel.forward_band), no
    collective in the data path.  Every rank holds the frame and writes its
    band of the output; Mpix/s of the whole frame over the slowest rank."""
    from srcnn_amd import parallel
    net = S.Net(*net_t)
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(4)
    x = torch.from_numpy((rng.random(w * h, dtype=np.float32) - 0.5)).to(dev)
    prm = torch.from_numpy(init_params(net_t, S.net_param_count(net))).to(dev)
    ctx = net_t[2] + net_t[3] + net_t[4] - 3
    out = torch.empty((w - ctx) * (h - ctx), device=dev)
    _, ni, _, _ = parallel.frame_band(w, h, net_t[2:], rank, world)
    nbytes = S.forward_workspace_bytes(net, w, max(ni, ctx + 1), 1)
    ws = torch.empty(nbytes // 4 + 64, device=dev)
    settle(lambda: parallel.forward_band(S, net, x, w, h, prm, out, ws, nbytes, stream, rank, world),
           settle_ms, torch.cuda.synchronize, world, backend, dev)
    for _ in range(warmup):
        parallel.forward_band(S, net, x, w, h, prm, out, ws, nbytes, stream, rank, world)
    torch.cuda.synchronize()
    dist.barrier()
    t0 = time.perf_counter()
    for _ in range(frames):
        parallel.forward_band(S, net, x, w, h, prm, out, ws, nbytes, stream, rank, world)
    torch.cuda.synchronize()
    dist.barrier()
    el = reduce_max(time.perf_counter() - t0)
    ms = el / frames * 1e3
    return {"frame": "%dx%d" % (w, h), "frames": frames, "ms_per_frame": round(ms, 4),
            "mpix_s": round(w * h / (ms * 1e-3) / 1e6, 1),
            "tflops": round(forward_flops(net_t, w, h) / (ms * 1e-3) / 1e12, 2),
            "sharding": "row bands of %d output rows + %d halo rows per GPU, no collective"
                        % (-(-(h - ctx) // world), ctx),
            "n_gpus": world, "kernel_path": S.last_path()}


WIDE_NET = (128, 64, 9, 5, 5)


def wide_training(S, steps=5, warmup=2, batch=4096):
    """BASELINE.json configs[3]: the wide net (n1=128, n2=64, f2=5) trained on
    1 GPU, 33x33 tiles, batch 4096, same step as the headline line.  Reported
    beside it (tiles/s, per-kernel split, step roofline)."""
    net_t = WIDE_NET
    net = S.Net(*net_t)
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.current_stream().cuda_stream
    w = h = TILE
    P = S.net_param_count(net)
    rng = np.random.default_rng(77)
    X, T = synthetic_batch(rng, batch, w, h)
    Xd, Td = torch.from_numpy(X).to(dev), torch.from_numpy(T).to(dev)
    params = torch.from_numpy(init_params(net_t, P)).to(dev)
    grads = torch.zeros(P, dtype=torch.float32, device=dev)
    mom = torch.zeros(P, dtype=torch.float32, device=dev)
    nbytes = S.train_workspace_bytes(net, w, h, batch)
    ws = torch.empty(nbytes // 4 + 64, dtype=torch.float32, device=dev)
    lr = [1e-4, 1e-4, 1e-5]

    def step():
        if os.environ.get("SRCNN_BENCH_SEPARATE_UPDATE"):
            S.train_fwd_bwd(net, Xd, Td, w, h, batch, params, grads, None, ws, nbytes, stream)
            S.update_all(net, params, grads, mom, 0.9, 1e-3, lr, batch, stream)
        else:  # the same step as the headline's (srcnn_train_step)
            S.train_step(net, Xd, Td, w, h, batch, params, grads, mom, 0.9, 1e-3, lr, batch, None,
                         ws, nbytes, stream)

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    S.profile_reset()
    S.profile_enable(True)
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    _mark("wide timed steps done")
    split = split_profiled(S)
    S.profile_enable(False)
    stats = S.profile_stats()
    work = layer_work(net_t, w, h)
    flops = sum(f for f, _ in work.values()) * batch
    t_roof = sum(max(f / (PEAK_FP32_TFLOPS * 1e12), b / (PEAK_HBM_GBS * 1e9))
                 for f, b in work.values()) * batch
    ms = el / steps * 1e3
    kernels = {k: {"launches_per_step": c / steps, "ms_per_step": round(t / steps, 4)}
               for k, (c, t) in stats.items()}
    rooflines = {}
    for k, (c, t) in stats.items():
        r = roofline_of(k, c / steps, t / steps, work, batch, load_pmc(), net_t, w, h, split=k in split)
        if r:
            rooflines[k] = r
    return {"workload": "SRCNN wide n1=128 n2=64 f1=9 f2=5 f3=5, fp32 training, 33x33 tiles, "
                        "batch %d (BASELINE.json configs[3])" % batch,
            "tiles_s": round(batch * steps / el, 1), "ms_per_step": round(ms, 4), "steps": steps,
            "tflops": round(flops / (ms * 1e-3) / 1e12, 2),
            "step_roofline": step_roofline(step_roof_ms(stats, steps, work, batch, net_t, w, h), t_roof * 1e3, ms,
                                           step_roof_ms(stats, steps, work, batch, net_t, w, h, split)
                                           if split else None),
            "kernel_path": S.last_path(), "kernels": kernels, "rooflines": rooflines}


_T0 = time.perf_counter()


def _mark(what):
    if os.environ.get("SRCNN_BENCH_TRACE"):
        print("[bench %.1f ms] %s" % ((time.perf_counter() - _T0) * 1e3, what), file=sys.stderr, flush=True)


STRONG_GLOBAL_BATCH = 4096  # strong scaling over a 4096-tile global batch


def launch_plan(gpus, env):
    """How this invocation runs (reference training loop: Main_cl.cpp:161-195,
    one process per GPU here).  Returns ("run", world) when this process is
    one rank already -- WORLD_SIZE from torch.distributed.run, or a single
    GPU -- and ("spawn", gpus) when --gpus N > 1 was asked for without a
    launcher, so the N ranks must be started first.  A WORLD_SIZE that
    disagrees with --gpus is an error (the line would be mislabelled)."""
    if gpus < 1:
        raise SystemExit("bench.py: --gpus must be >= 1 (got %d)" % gpus)
    ws = env.get("WORLD_SIZE")
    if ws is None or ws == "":
        return ("spawn", gpus) if gpus > 1 else ("run", 1)
    try:
        world = int(ws)
    except ValueError:
        raise SystemExit("bench.py: WORLD_SIZE=%r is not an integer" % ws)
    if world != gpus:
        raise SystemExit("bench.py: WORLD_SIZE=%d but --gpus %d; launch one rank per GPU "
                         "(torch.distributed.run --nproc-per-node %d ... bench.py --gpus %d)"
                         % (world, gpus, gpus, gpus))
    return ("run", world)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def spawn_command(n, argv, port):
    """torch.distributed.run over this script with the same arguments: one
    rank per GPU of this node, rendezvous on 127.0.0.1."""
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=%d" % n,
            "--master-addr=127.0.0.1", "--master-port=%d" % port, os.path.abspath(__file__)] + list(argv)


def spawn_ranks(n, argv):
    """Start the N rank processes as a child (nothing in this process has
    touched the GPU) and return its exit status; rank 0's JSON line reaches
    stdout through the inherited descriptor."""
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC only on these hosts
    cmd = spawn_command(n, argv, _free_port())
    print("[bench] launching %d ranks: %s" % (n, " ".join(cmd)), file=sys.stderr, flush=True)
    return subprocess.call(cmd, env=env)


class CudaDevice:
    """This rank's GPU as the bench uses it: the torch device (memory only),
    the HIP stream the headline runs on (graph capture needs a created
    stream) and a device-wide sync.  The CPU tests inject a stand-in."""

    def __init__(self, index):
        torch.cuda.set_device(index)
        self.dev = torch.device("cuda", index)
        self.hstream = torch.cuda.Stream(device=self.dev)
        self.stream = self.hstream.cuda_stream

    def sync(self):
        torch.cuda.synchronize()

    def on_stream(self):
        """torch work (a torch.distributed collective) ordered on the headline stream"""
        return torch.cuda.stream(self.hstream)


def reduce_int(v, op, world, backend, dev):
    """MIN / MAX of an int over the process group (every rank gets it)."""
    if world <= 1:
        return int(v)
    t = torch.tensor([int(v)], dtype=torch.int64, device=dev if backend == "nccl" else "cpu")
    dist.all_reduce(t, op=op)
    return int(t.item())


def agree_all(flag, world, backend, dev):
    """True on every rank iff `flag` is true on every rank (MIN over the
    process group), so that all ranks take the same branch."""
    return bool(reduce_int(1 if flag else 0, dist.ReduceOp.MIN if world > 1 else None, world, backend, dev))


def settle(step, settle_ms, sync, world, backend, dev, probe=3):
    """Untimed steps of the timed workload itself, run right before its W
    warmup steps, until ~settle_ms of it has executed: the chip's clock keeps
    moving for ~20 ms after a change of workload (rocprofv3 trace of the
    driver's command, profiles/r05_clock: the headline kernels 5-8% slow over
    steps 3-8 after the 4K frames, steady from step ~20), so a short timed
    region (--steps 20 --warmup 5) would otherwise time that transient.  The
    step count is agreed over the ranks (MAX): the steps carry the gradient
    all-reduce, so every rank must run the same number.  Returns the count."""
    if settle_ms <= 0:
        return 0
    sync()
    t0 = time.perf_counter()
    for _ in range(probe):
        step()
    sync()
    per_ms = max((time.perf_counter() - t0) / probe * 1e3, 1e-3)
    n = reduce_int(int(settle_ms / per_ms + 0.999), dist.ReduceOp.MAX if world > 1 else None, world,
                   backend, dev)
    for _ in range(n):
        step()
    sync()
    return probe + n


def timed_region(step, steps, warmup, world, every, stream, S, graph_mode, backend, dev, sync,
                 before_timed=None, after_timed=None):
    """W untimed warmup steps, then K timed steps bracketed by a barrier and a
    device sync on both sides; returns (elapsed max over ranks, profiled
    steps, whether a HIP graph was replayed).  Per-kernel hipEvents on every
    `every`-th step (or on as many extra steps after a graph replay).
    graph_mode (one rank only: a step is then one srcnn_train_step, no
    collective): the timed steps replay one captured step.  before_timed():
    called after the last untimed step, ahead of the opening barrier + sync;
    after_timed(): called once the clock is read, before any extra step."""
    for _ in range(warmup):
        step()
    sync()
    graph = None
    if graph_mode:
        ok = True
        try:
            graph = S.Graph(step, stream)
        except S.SrcnnError as e:
            print("[bench] HIP graph capture failed (%s)" % e, file=sys.stderr)
            ok = False
        # agree before anything is replayed (advisor r04): no rank may run a
        # captured step unless every rank captured one
        if not agree_all(ok, world, backend, dev):
            if graph is not None:
                graph.close()
            graph = None
            print("[bench] HIP graph not used on every rank; timing direct calls", file=sys.stderr)
        if graph is not None:
            graph.launch()  # one untimed replay
            sync()
    if before_timed is not None:
        before_timed()
    if world > 1:
        dist.barrier()
    sync()
    S.profile_reset()
    n_prof = 0
    t0 = time.perf_counter()
    if graph is not None:
        for _ in range(steps):
            graph.launch()
    else:
        for i in range(steps):
            on = i % every == every - 1
            n_prof += on
            S.profile_enable(on)
            step()
    sync()
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    S.profile_enable(False)
    if after_timed is not None:
        after_timed()
    if graph is not None:
        n_prof = max(1, steps // every)
        S.profile_enable(True)
        for _ in range(n_prof):
            step()
        sync()
        S.profile_enable(False)
        graph.close()
    if world > 1:
        e = torch.tensor([elapsed], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
        dist.all_reduce(e, op=dist.ReduceOp.MAX)
        elapsed = float(e.item())
    return elapsed, n_prof, graph is not None


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1,
                    help="GPUs of this node, one rank each; without torch.distributed.run the "
                         "ranks are launched by this script")
    # defaults: the kernels reach their steady clock after ~25 steps of a
    # fresh process (rocprofv3 trace: d1 485 -> 432 us over the first 25
    # launches, flat over the next 275), so the default run warms up past it
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--settle-ms", type=float, default=50.0,
                    help="untimed steps of the timed workload (~this many ms of them) before its "
                         "warmup, so the timed steps start at the steady clock (see settle())")
    ap.add_argument("--batch", type=int, default=4096,
                    help="tiles per GPU per step (weak scaling, the default line)")
    ap.add_argument("--global-batch", type=int, default=None,
                    help="strong scaling: this many tiles per step in total, sharded over the "
                         "ranks (parallel.shard; SURVEY.md 8(d) config 3: 4096)")
    ap.add_argument("--path", choices=["auto", "generic"], default="auto")
    ap.add_argument("--full", action="store_true",
                    help="also measure everything beside the headline: the wide net, the 256x256 "
                         "tile and 4K inference, the CPU baselines, N > 1: the strong-scaling "
                         "sub-record and the sharded 4K frame")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step left (params, momentum, grads) as "
                         "DIR/<name>.npy (float32); the state is reset to its seeded initial "
                         "values right before the timed steps")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baselines")
    ap.add_argument("--no-forward", action="store_true", help="--full: skip the 4K inference line")
    ap.add_argument("--no-wide", action="store_true", help="--full: skip the wide-net training line")
    ap.add_argument("--cpu-budget", type=float, default=12.0)
    ap.add_argument("--profile-every", type=int, default=5,
                    help="per-kernel hipEvents on every N-th timed step (1 = every step)")
    # N > 1: the gradient all-reduce is the library's own RCCL stage
    # (srcnn_allreduce_grads over a srcnn_comm_init_rank communicator) by
    # default; torch.distributed then only ships the RCCL id and runs the
    # barriers / max-time reduction (gloo).  --comm torch uses dist.all_reduce.
    ap.add_argument("--comm", choices=["srcnn", "torch"], default="srcnn")
    # N > 1: one step = srcnn_train_fwd_bwd_lazy (the previous step's update
    # inside its first kernel) + the all-reduce; --dp-step separate keeps the
    # update as its own launch after the all-reduce (A/B)
    ap.add_argument("--dp-step", choices=["lazy", "separate"], default="lazy")
    # --graph on (one GPU): the timed steps replay one HIP graph of the step
    # (srcnn_graph_*).  Default off: it measured the same (0.8975 vs 0.894 ms,
    # same box); the direct calls enqueue well ahead of the GPU.  N > 1 steps
    # ping-pong parameter buffers on the host, so they are always direct calls
    ap.add_argument("--graph", choices=["auto", "on", "off"], default="auto")
    ap.add_argument("--no-strong", action="store_true",
                    help="--full, N > 1: skip the strong-scaling sub-record (global batch 4096)")
    ap.add_argument("--dist-backend", choices=["nccl", "gloo"], default=None,
                    help="process-group backend (default: gloo with --comm srcnn, nccl with torch)")
    # rehearsal of the N>1 path on a single-GPU box (NOT a measurement):
    # every rank on one device, gradients all-reduced over gloo
    ap.add_argument("--all-ranks-on-device", type=int, default=None)
    return ap.parse_args(argv)


def main(argv=None, S=None, device=None):
    """Entry point (argv = sys.argv[1:] by default).  `S` (the srcnn_amd
    binding) and `device` (a CudaDevice-like object: dev, stream, sync,
    on_stream) are injectable so that the CPU tests can drive the multi-rank
    path with a stand-in library; the bench itself uses neither argument."""
    if argv is None:
        argv = sys.argv[1:]
    args = parse_args(argv)
    mode, world = launch_plan(args.gpus, os.environ)
    if mode == "spawn":
        sys.exit(spawn_ranks(world, argv))
    if S is None:
        import srcnn_amd as S
    from srcnn_amd import parallel
    rank, world, local = parallel.env_world()
    try:
        run(args, S, parallel, rank, world, local, device)
    except BaseException as e:
        if world <= 1:
            raise
        # one rank failed: leave at once, so no peer stays blocked in a
        # collective of this rank's -- gloo peers see the closed connections
        # and fail (then exit here too), torch.distributed.run stops the rest,
        # and the group's timeout bounds the remaining cases.  os._exit skips
        # the teardown (RCCL communicator, process group) that could itself
        # block on the dead peers.
        code = e.code if isinstance(e, SystemExit) and isinstance(e.code, int) and e.code else 1
        if not (isinstance(e, SystemExit) and e.code is None):
            import traceback
            print("[bench rank %d/%d] failed: %s" % (rank, world, e), file=sys.stderr)
            traceback.print_exc()
        sys.stderr.flush()
        sys.stdout.flush()
        os._exit(code)


def run(args, S, parallel, rank, world, local, device=None):
    dev_index = local if world > 1 else 0
    if args.all_ranks_on_device is not None:
        dev_index = args.all_ranks_on_device
    backend = args.dist_backend or ("gloo" if args.comm == "srcnn" else "nccl")
    D = device if device is not None else CudaDevice(dev_index)
    parallel.init(backend, D.dev if D.dev.type == "cuda" else None)
    S.set_path(0 if args.path == "auto" else 1)
    dev = D.dev
    stream = D.stream
    sync = D.sync

    net_t = DEFAULT_NET
    net = S.Net(*net_t)
    strong = args.global_batch is not None
    if strong:
        _, B = parallel.shard(args.global_batch, rank, world)
        global_tiles = args.global_batch
    else:
        B = args.batch
        global_tiles = B * world
    w, h = TILE, TILE
    P = S.net_param_count(net)
    # the strong-scaling sub-record (--full, N > 1) reuses the first tiles of
    # this rank's batch, so allocate for the larger of the two shards
    Bs = parallel.shard(STRONG_GLOBAL_BATCH, rank, world)[1] if world > 1 and args.full else 0
    Bmax = max(B, Bs, 1)
    rng = np.random.default_rng(1234 + rank)
    X, T = synthetic_batch(rng, Bmax, w, h)
    prm = init_params(net_t, P)
    Xd = torch.from_numpy(X).to(dev)
    Td = torch.from_numpy(T).to(dev)
    params = torch.from_numpy(prm).to(dev)
    grads = torch.zeros(P, dtype=torch.float32, device=dev)
    mom = torch.zeros(P, dtype=torch.float32, device=dev)
    ws_bytes = S.train_workspace_bytes(net, w, h, Bmax)
    ws = torch.empty(ws_bytes // 4 + 64, dtype=torch.float32, device=dev)
    lr = [1e-4, 1e-4, 1e-5]
    mu, wd = 0.9, 1e-3

    comm = None
    rccl_ranks = None
    if world > 1 and args.comm == "srcnn":
        comm = parallel.SrcnnComm(S, stream)
        # what the communicator itself reports, not what the launcher asked for
        c_rank, rccl_ranks = S.comm_rank(comm.comm)
        if rccl_ranks != world or c_rank != rank:
            raise SystemExit("bench.py: RCCL communicator has rank %d of %d, expected %d of %d"
                             % (c_rank, rccl_ranks, rank, world))
    elif world > 1 and backend == "nccl":
        rccl_ranks = dist.get_world_size()
    allreduce = comm
    if world > 1 and comm is None:
        def allreduce(g):  # dist.all_reduce ordered on the stream the kernels run on
            with D.on_stream():
                dist.all_reduce(g, op=dist.ReduceOp.SUM)

    lazy = world > 1 and args.dp_step == "lazy"
    # the lazy step ping-pongs the parameters / momentum; `bufs` holds the
    # current pair first
    bufs = {"p": params, "m": mom, "p2": torch.empty_like(params) if lazy else None,
            "m2": torch.empty_like(mom) if lazy else None}

    def dp_step(batch, global_batch):
        """One rank's shard -> grads; one all-reduce; the same update on every
        rank (srcnn_amd/parallel.py)."""
        if lazy:
            return parallel.LazyDataParallelStep(
                bufs["p"], bufs["p2"], bufs["m"], bufs["m2"], grads,
                lambda pi, po, mi, mo, g, pend: S.train_fwd_bwd_lazy(
                    net, Xd, Td, w, h, batch, pi, po, mi, mo, g, mu, wd, lr, pend, None, ws, ws_bytes,
                    stream),
                lambda p, m, g, nb: S.update_all(net, p, g, m, mu, wd, lr, nb, stream),
                global_batch, allreduce=allreduce)
        return parallel.DataParallelStep(
            grads,
            lambda g: S.train_fwd_bwd(net, Xd, Td, w, h, batch, bufs["p"], g, None, ws, ws_bytes, stream),
            lambda nb: S.update_all(net, bufs["p"], grads, bufs["m"], mu, wd, lr, nb, stream),
            global_batch, allreduce=allreduce)

    def finish(step):
        """apply a lazy step's owed update; its current buffers become bufs'"""
        if isinstance(step, parallel.LazyDataParallelStep):
            p, m = step.finish()
            if p is not bufs["p"]:
                bufs["p"], bufs["p2"], bufs["m"], bufs["m2"] = p, bufs["p"], m, bufs["m"]

    step = dp_step(B, global_tiles)
    if world == 1 and not os.environ.get("SRCNN_BENCH_SEPARATE_UPDATE"):
        # one device, no exchange: srcnn_train_step (the same step; on the
        # fused path the update runs inside the gradient reduction).
        # SRCNN_BENCH_SEPARATE_UPDATE=1: fwd_bwd + update_all (A/B)
        def step():
            S.train_step(net, Xd, Td, w, h, B, params, grads, mom, mu, wd, lr, global_tiles,
                         None, ws, ws_bytes, stream)

    # --full: the single-GPU side lines (the wide net, one 256x256 tile, 4K
    # inference) are measured before the headline; a plain run goes straight
    # to the headline's settle() steps.  Order and pause matter on this part
    # (tools/first_step.py): right after ~0.15 s of the
    # wide net's full-power load the GPU stalls the next launch for 8-24 ms
    # (a power-state transition; a 0.2 s idle pause avoids it), and a step
    # launched on an idle GPU runs through a ~25 ms clock ramp.  So: wide net,
    # a pause, then the two inference lines, then settle() steps of the
    # headline's own workload, then its W warmup + K timed steps, which
    # thereby run at the steady clock of sustained load.  With N > 1 every
    # rank runs the same sequence on its own GPU, so that each N's headline
    # starts from the same power state (a rank that skipped it would time its
    # warmup through the idle clock ramp and the scaling curve would charge
    # that to N); only N = 1 reports these lines.
    S.preload(net)
    side = {}
    if args.full and not args.no_wide:
        side["wide"] = wide_training(S)
        sync()
        time.sleep(0.5)
    if args.full and not args.no_forward:
        side["forward_tile_256"] = forward_tile_256(S, net_t)
        side["forward"] = forward_4k(S, net_t)
    if world > 1:
        side = {}
    sync()
    _mark("side legs done")

    graph_mode = args.graph == "on" and world == 1
    every = max(1, min(args.profile_every, args.steps))
    # Per-kernel durations come from hipEvent pairs recorded around the
    # launches of every `every`-th timed step (steps every-1, 2*every-1, ...:
    # the first step after the warmup sync starts cold).  Event pairs around
    # every launch cost 2.5% of the step even as fence-free timing events
    # (1.011 vs 0.986 ms, same box), so the sampled steps carry the
    # instrumentation and the others run bare.
    reset_state = None
    if args.dump_outputs:
        # the settle step count follows the clock, so the state the timed
        # steps start from is put back to the seeded initial one: the dump then
        # depends on the arguments alone (a lazy step's owed update is applied
        # first, so that nothing of the untimed steps is left pending)
        prm0 = torch.from_numpy(prm.copy())

        def reset_state():
            finish(step)
            bufs["p"].copy_(prm0)
            bufs["m"].zero_()
            grads.zero_()

    dump = {}

    def snapshot():
        """what a caller of the step holds after the last timed step"""
        sync()
        for k, v in (("params", bufs["p"]), ("momentum", bufs["m"]), ("grads", grads)):
            dump[k] = v.detach().cpu().numpy().astype(np.float32, copy=True)

    n_settle = settle(step, args.settle_ms, sync, world, backend, dev)
    elapsed, n_prof, used_graph = timed_region(
        step, args.steps, args.warmup, world, every, stream, S, graph_mode, backend, dev, sync,
        before_timed=reset_state, after_timed=snapshot if args.dump_outputs and not lazy else None)
    _mark("headline timed steps done")
    kernel_path = S.last_path()
    split = split_profiled(S)  # (the step's own kernels: read before the side legs run)
    stats = S.profile_stats()
    finish(step)
    if args.dump_outputs and lazy:
        snapshot()  # (a lazy step's last update is applied by finish())

    # --full, N > 1: the strong-scaling step in the same run (global batch 4096
    # sharded over the ranks: 512 tiles per rank at N = 8), timed the same way
    strong_rec = None
    if args.full and world > 1 and not strong and not args.no_strong:
        sstep = dp_step(Bs, STRONG_GLOBAL_BATCH)
        s_settle = settle(sstep, args.settle_ms, sync, world, backend, dev)
        s_el, s_prof, s_graph = timed_region(sstep, args.steps, args.warmup, world, every, stream, S,
                                             graph_mode, backend, dev, sync)
        s_stats = S.profile_stats()
        finish(sstep)
        s_ms = s_el / args.steps * 1e3
        strong_rec = {
            "scaling": "strong", "global_batch": STRONG_GLOBAL_BATCH, "batch_per_gpu": Bs,
            "value": round(STRONG_GLOBAL_BATCH * args.steps / s_el, 1), "unit": "tiles/s",
            "ms_per_step": round(s_ms, 4), "steps": args.steps, "warmup": args.warmup,
            "settle_steps": s_settle, "hip_graph": s_graph,
            "kernels": {k: {"launches_per_step": c / max(s_prof, 1), "ms_per_step": round(t / max(s_prof, 1), 4)}
                        for k, (c, t) in s_stats.items()},
            "note": "rank 0's per-kernel split; value = 4096 tiles x steps / max-over-ranks time"}
        _mark("strong timed steps done")
    assert np.isfinite(bufs["p"].cpu().numpy()).all(), "non-finite parameters after training"
    fwd_sharded = None
    if args.full and world > 1 and not args.no_forward:
        def reduce_max(v):
            t = torch.tensor([v], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            return float(t.item())
        fwd_sharded = forward_4k_sharded(S, net_t, rank, world, reduce_max, backend)

    if rank == 0:
        K = args.steps
        value = global_tiles * K / elapsed
        work = layer_work(net_t, w, h)
        pmc = load_pmc()
        kernels = {}
        for name, (cnt, ms) in stats.items():
            kernels[name] = {"launches_per_step": cnt / n_prof, "ms_per_step": round(ms / n_prof, 4)}
        rooflines = {}
        for name, (cnt, ms) in stats.items():
            r = roofline_of(name, cnt / n_prof, ms / n_prof, work, B, pmc, split=name in split)
            if r:
                rooflines[name] = add_clock(r, held_clock(S, name))
        dominant = max(rooflines, key=lambda k: stats[k][1]) if rooflines else None
        roof = rooflines.get(dominant)
        # whole-step roofline: T_roof = sum_stage max(F/peak, B/peak)
        t_roof = sum(max(f / (PEAK_FP32_TFLOPS * 1e12), b / (PEAK_HBM_GBS * 1e9))
                     for f, b in work.values()) * B
        ms_step = elapsed / K * 1e3
        if strong:
            metric = "training tiles/sec (fwd+bwd+update), default SRCNN 33x33, global batch %d" % global_tiles
            workload = ("SRCNN default n1=64 n2=32 f1=9 f2=1 f3=5, fp32 training, 33x33 luma tiles, "
                        "global batch %d sharded over %d GPUs (BASELINE.json configs[2], strong scaling)"
                        % (global_tiles, world))
        else:
            metric = "training tiles/sec (fwd+bwd+update), default SRCNN 33x33, batch 4096/GPU"
            workload = ("SRCNN default n1=64 n2=32 f1=9 f2=1 f3=5, fp32 training, 33x33 luma tiles, "
                        "batch %d per GPU (BASELINE.json configs[1]%s)"
                        % (B, ", configs[2] weak scaling" if world > 1 else ""))
        if world == 1 and not strong and B == STRONG_GLOBAL_BATCH:
            # at N = 1 the strong-scaling step IS the headline step
            strong_rec = {"scaling": "strong", "global_batch": B, "batch_per_gpu": B,
                          "value": round(value, 1), "unit": "tiles/s", "ms_per_step": round(ms_step, 4),
                          "note": "N = 1: the headline step (global batch 4096 on one GPU)"}
        if world == 1:
            step_call = ("srcnn_train_fwd_bwd + srcnn_update_all" if os.environ.get("SRCNN_BENCH_SEPARATE_UPDATE")
                         else "srcnn_train_step (SGD update inside the gradient reduction)")
        elif lazy:
            step_call = ("srcnn_train_fwd_bwd_lazy (the previous step's SGD update inside its first "
                         "kernel) + the gradient all-reduce")
        else:
            step_call = "srcnn_train_fwd_bwd + the gradient all-reduce + srcnn_update_all"
        out = {
            "metric": metric,
            "value": round(value, 1),
            "unit": "tiles/s",
            "n_gpus": world,
            "steps": K,
            "warmup": args.warmup,
            "ms_per_step": round(ms_step, 4),
            "higher_is_better": True,
            "scaling": "strong" if strong else "weak",
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic (smooth random 33x33 luma patches, seed 1234+rank; weights N(0,1e-3))",
            "config": {"workload": workload, "global_batch": global_tiles, "batch_per_gpu": B,
                       "tile": "33x33", "parallelism": "dp%d" % world,
                       "kernel_path": kernel_path,
                       "mfma_arith": ("split-bf16 x6: fp32 operands as three exact bf16 parts, six part "
                                      "products per k-step on v_mfma_f32_32x32x16_bf16 (fp32 accuracy, "
                                      "tests/test_split_arith_gpu.py)" if split else "fp32 MFMA"),
                       "hip_graph": used_graph,
                       "settle_steps": n_settle,
                       "step_call": step_call,
                       "grad_allreduce": (("srcnn_allreduce_grads (RCCL)" if comm else
                                           "torch.distributed all_reduce (%s)" % backend)
                                          if world > 1 else None),
                       "rccl_ranks": rccl_ranks,
                       "launcher": ("torch.distributed.run" if os.environ.get("TORCHELASTIC_RUN_ID")
                                    else "env") if world > 1 else None},
            "roofline": roof,
            "rooflines": rooflines,
            "step_roofline": step_roofline(step_roof_ms(stats, n_prof, work, B), t_roof * 1e3, ms_step,
                                           step_roof_ms(stats, n_prof, work, B, split=split) if split else None),
            "kernels": kernels,
            "profiled_steps": n_prof,
            "cpu_baseline": None,
        }
        if strong_rec is not None:
            out["strong"] = strong_rec
        if fwd_sharded is not None:
            out["forward"] = fwd_sharded
        out.update(side)
        if args.full and world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(net_t, budget_s=args.cpu_budget)
            out["cpu_forward_baseline"] = cpu_forward_baseline(net_t)
        if args.dump_outputs:
            os.makedirs(args.dump_outputs, exist_ok=True)
            for name, a in dump.items():
                np.save(os.path.join(args.dump_outputs, name + ".npy"), a)
            out["outputs"] = sorted(dump)
        print(json.dumps(out), flush=True)
    if comm is not None:
        comm.close()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
