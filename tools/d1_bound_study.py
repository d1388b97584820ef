#!/usr/bin/env python3
"""How loose is the per-sample bound on delta1 that a two-part fp16 split of
gW1's operand would take its scale from (split.hpp)?

On bench.py's own data (smooth patches, seed 1234; weights N(0, 1e-3)) and,
for comparison, on weights N(0, 0.05) as the parity tests use, the CPU oracle
forms delta3, delta2 and delta1 of the default net per sample, and this prints
the distribution of log2(bound / max |delta1|) for three bounds:

  norm    max|delta3| . max_n sum_tap |W3[tap][n]| . max_c sum_n |W2[c][n]|
  d2max   max|delta2| . max_c sum_n |W2[c][n]|          (needs a pass over delta2)
  d2chan  max_c sum_n |W2[c][n]| max_p |delta2[p][n]|   (per-channel maxima)

The fp16 form keeps the six-product form's accuracy while the bound is within
about 2^8 of the true maximum (tests/test_split_f16_cpu.py).  CPU only.

usage: d1_bound_study.py [tiles]      (default 256)
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("oracle", "tests", "."):
    sys.path.insert(0, os.path.join(ROOT, p))

import srcnn_oracle as orc  # noqa: E402
from hip_util import make_batch, make_params  # noqa: E402
from bench import init_params  # noqa: E402

NET = (64, 32, 9, 1, 5)
SIZE = 33


def deltas(X, T, params, batch):
    n1, n2, f1, f2, f3 = NET
    o = orc.ORACLE
    sizes = [f1 * f1 * n1, n1, f2 * f2 * n1 * n2, n2, f3 * f3 * n2, 1]
    W1, B1, W2, B2, W3, B3 = np.split(params, np.cumsum(sizes)[:-1])
    w1 = SIZE - f1 + 1
    w2 = w1 - f2 + 1
    w3 = w2 - f3 + 1
    A1 = o.conv_fwd(X, W1, B1, SIZE, SIZE, 1, n1, f1, True, batch)
    A2 = o.conv_fwd(A1, W2, B2, w1, w1, n1, n2, f2, True, batch)
    A3 = o.conv_fwd(A2, W3, B3, w2, w2, n2, 1, f3, False, batch)
    d3 = o.last_delta(T, A3, SIZE, SIZE, w3, w3, batch)
    d2 = o.conv_delta(d3, A2, W3, f3, n2, 1, w2, w2, batch)
    d1 = o.conv_delta(d2, A1, W2, f2, n1, n2, w1, w1, batch)
    return (d3.reshape(batch, -1), d2.reshape(batch, -1, n2), d1.reshape(batch, -1, n1),
            np.abs(W2.reshape(n1, n2)), np.abs(W3.reshape(f3 * f3, n2)))


def study(tag, params, tiles):
    rng = np.random.default_rng(1234)
    X, T = make_batch(rng, tiles, SIZE, SIZE)
    d3, d2, d1, aW2, aW3 = deltas(X, T, params, tiles)
    m1 = np.abs(d1).max(axis=(1, 2))
    m3 = np.abs(d3).max(axis=1)
    n3, n2 = aW3.sum(axis=0).max(), aW2.sum(axis=1).max()
    bounds = {
        "norm": m3 * n3 * n2,
        "d2max": np.abs(d2).max(axis=(1, 2)) * n2,
        "d2chan": (aW2[None] * np.abs(d2).max(axis=1)[:, None, :]).sum(axis=2).max(axis=1),
    }
    ok = m1 > 0
    out = {"data": tag, "tiles": int(tiles), "tiles_with_zero_delta1": int((~ok).sum())}
    for k, b in bounds.items():
        assert (b[ok] >= m1[ok] * (1 - 1e-5)).all(), k  # a bound
        r = np.log2(b[ok] / m1[ok])
        out[k] = {"log2_min": round(float(r.min()), 2), "log2_median": round(float(np.median(r)), 2),
                  "log2_p95": round(float(np.percentile(r, 95)), 2), "log2_max": round(float(r.max()), 2)}
    return out


def main():
    tiles = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    P = orc.ORACLE.param_count(*NET)
    print(json.dumps(study("bench.py weights N(0, 1e-3)", init_params(NET, P), tiles)))
    print(json.dumps(study("weights N(0, 0.05)", make_params(np.random.default_rng(1234), NET, sd=0.05), tiles)))


if __name__ == "__main__":
    main()
