#!/usr/bin/env python3
"""Print srcnn_train_workspace_bytes and srcnn_forward_workspace_bytes for a
fixed table of nets, tiles, batches, arithmetics and kernel paths, as JSON.
The queries are host-only, so this runs without a GPU.

  tools/record_workspace_table.py > tests/golden/workspace_table.json
  SRCNN_HIP_LIB=.../libsrcnn_hip_<name>.so tools/record_workspace_table.py   # another build

tests/test_workspace_table_cpu.py compares the current build against the
committed table, row for row: a change of any byte count is a change of the
dispatch (which kernels serve a shape, their grids and slabs).
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NETS = {"default": (64, 32, 9, 1, 5), "example": (32, 16, 9, 1, 5), "default_f3": (64, 32, 9, 1, 3),
        "example_f3": (32, 16, 9, 1, 3), "wide": (128, 64, 9, 5, 5), "tiny": (8, 4, 5, 1, 3),
        "invalid": (64, 32, 9, 2, 5)}  # even f2
TILES = [(s, s) for s in (13, 14, 17, 21, 25, 33, 34, 36, 39, 40, 48)] + [(33, 25), (25, 33)]
BATCHES = [1, 2, 3, 255, 256, 257, 511, 512, 513, 1024, 1025, 4096]
FRAMES = [(256, 256), (3840, 2160)]  # forward only, batch 1


def record(S):
    """The table of the library behind the srcnn_amd module S, as a list of rows."""
    rows = []
    arith0, path0 = S.get_arith(), S.get_path()
    try:
        for name, cfg in NETS.items():
            net = S.Net(*cfg)
            for arith in (0, 1):
                S.set_arith(arith)
                for path in (0, 1):
                    S.set_path(path)
                    for w, h in TILES:
                        rows.append({"net": name, "w": w, "h": h, "arith": arith, "path": path,
                                     "batches": BATCHES,
                                     "train": [S.train_workspace_bytes(net, w, h, b) for b in BATCHES],
                                     "forward": [S.forward_workspace_bytes(net, w, h, b) for b in BATCHES]})
                    for w, h in FRAMES:
                        rows.append({"net": name, "w": w, "h": h, "arith": arith, "path": path,
                                     "batches": [1], "forward": [S.forward_workspace_bytes(net, w, h, 1)]})
    finally:
        S.set_arith(arith0)
        S.set_path(path0)
    return rows


def main():
    sys.path.insert(0, os.path.join(ROOT, "cnn-super-resolution_amd"))
    import srcnn_amd as S
    rows = record(S)
    print("[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in rows) + "\n]")


if __name__ == "__main__":
    main()
