#!/usr/bin/env python3
"""Print what the net-level calls dispatch to on the MI355X, as JSON: for a
fixed list of nets and tiles under both arithmetics, srcnn_last_path() and the
srcnn_last_kernels() list after srcnn_train_fwd_bwd, and for three of them
also after srcnn_train_step, two consecutive srcnn_train_fwd_bwd_lazy calls
and srcnn_forward.  Needs the GPU (the calls run).

  tools/record_dispatch_table.py > tests/golden/dispatch_table.json
  SRCNN_HIP_LIB=.../libsrcnn_hip_<name>.so tools/record_dispatch_table.py   # another build

tests/test_dispatch_table_gpu.py compares the current build against the
committed table, list for list.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NETS = {"default": (64, 32, 9, 1, 5), "example": (32, 16, 9, 1, 5), "default_f3": (64, 32, 9, 1, 3),
        "wide": (128, 64, 9, 5, 5), "tiny": (8, 4, 5, 1, 3)}
# (net, tile, srcnn_set_path)
CASES = [("default", 33, 0), ("default", 21, 0), ("default", 13, 0), ("default", 36, 0),
         ("default", 39, 0), ("default", 40, 0), ("default_f3", 33, 0), ("example", 33, 0),
         ("wide", 33, 0), ("wide", 34, 0), ("tiny", 15, 0), ("default", 33, 1)]
# these also record train_step, the lazy pair and the forward
FULL = [("default", 33, 0), ("wide", 33, 0), ("default", 39, 0)]
BATCH = 3  # (kernel names do not depend on the batch)
FRAME = (64, 48)
LR = [1e-4, 1e-4, 1e-5]


def case_id(name, size, path, arith):
    return "%s-%d-%s-arith%d" % (name, size, "generic" if path else "auto", arith)


def run_case(S, torch, name, size, path, arith):
    """{call: {"path": srcnn_last_path, "kernels": srcnn_last_kernels}} of one case."""
    net = S.Net(*NETS[name])
    P = S.net_param_count(net)
    gen = torch.Generator(device="cuda").manual_seed(5)
    rand = lambda n, sd=1.0: sd * torch.randn(n, device="cuda", generator=gen)
    out = {}

    def seen(call):
        torch.cuda.synchronize()
        out[call] = {"path": S.last_path(), "kernels": S.last_kernels()}

    arith0, path0 = S.get_arith(), S.get_path()
    try:
        S.set_arith(arith)
        S.set_path(path)
        X, T = rand(BATCH * size * size), rand(BATCH * size * size)
        nbytes = S.train_workspace_bytes(net, size, size, BATCH)
        ws = torch.zeros(nbytes // 4 + 64, device="cuda")
        p, g, m = rand(P, 0.05), torch.zeros(P, device="cuda"), torch.zeros(P, device="cuda")
        S.train_fwd_bwd(net, X, T, size, size, BATCH, p, g, None, ws, nbytes)
        seen("train_fwd_bwd")
        if (name, size, path) in FULL:
            S.train_step(net, X, T, size, size, BATCH, p, g, m, 0.9, 1e-3, LR, BATCH, None, ws, nbytes)
            seen("train_step")
            p2, m2 = torch.zeros(P, device="cuda"), torch.zeros(P, device="cuda")
            S.train_fwd_bwd_lazy(net, X, T, size, size, BATCH, p, p2, m, m2, g, 0.9, 1e-3, LR, 0, None,
                                 ws, nbytes)
            seen("lazy_first")
            S.train_fwd_bwd_lazy(net, X, T, size, size, BATCH, p, p2, m, m2, g, 0.9, 1e-3, LR, BATCH,
                                 None, ws, nbytes)
            seen("lazy_second")
            # (srcnn_forward notes no kernels: the list stays the lazy step's)
            w, h = FRAME
            pad = sum(NETS[name][2:]) - 3
            fbytes = S.forward_workspace_bytes(net, w, h, 1)
            fws = torch.zeros(fbytes // 4 + 64, device="cuda")
            res = torch.zeros((w - pad) * (h - pad), device="cuda")
            S.forward(net, rand(w * h), w, h, 1, p2, res, fws, fbytes)
            seen("forward")
    finally:
        S.set_arith(arith0)
        S.set_path(path0)
    return out


def record(S, torch):
    return {case_id(n, s, p, a): run_case(S, torch, n, s, p, a) for n, s, p in CASES for a in (0, 1)}


def main():
    sys.path.insert(0, os.path.join(ROOT, "cnn-super-resolution_amd"))
    import torch
    import srcnn_amd as S
    table = record(S, torch)
    print("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in table.items()) + "\n}")


if __name__ == "__main__":
    main()
