#!/usr/bin/env python3
"""How loose is the per-sample bound on A1 that l12x6's layer 2 takes its
two-part fp16 scale from (l12x6.hpp)?

  bound = max |X_sample| . max_c sum_tap |W1[tap][c]| + max |B1|

On bench.py's own data (smooth patches, seed 1234; weights N(0, 1e-3)) and on
weights N(0, 0.05) as the parity tests use, the CPU oracle forms A1 of the
default net per sample and this prints the distribution of
log2(bound / max |A1|).  The fp16 form keeps the six-product form's accuracy
while the bound is within about 2^8 of the true maximum
(tests/test_split_f16_cpu.py).  CPU only.

usage: a1_bound_study.py [tiles]      (default 256)
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
from bench import init_params, synthetic_batch  # noqa: E402

NET = (64, 32, 9, 1, 5)
SIZE = 33


def study(tag, X, params, tiles):
    n1, n2, f1, f2, f3 = NET
    W1, B1 = params[:f1 * f1 * n1], params[f1 * f1 * n1:f1 * f1 * n1 + n1]
    A1 = orc.ORACLE.conv_fwd(X, W1, B1, SIZE, SIZE, 1, n1, f1, True, tiles).reshape(tiles, -1)
    m = np.abs(A1).max(axis=1)
    wnorm = np.abs(W1.reshape(f1 * f1, n1)).sum(axis=0).max()
    b = np.abs(X.reshape(tiles, -1)).max(axis=1) * wnorm + np.abs(B1).max()
    ok = m > 0
    assert (b[ok] >= m[ok] * (1 - 1e-5)).all()
    r = np.log2(b[ok] / m[ok])
    return {"data": tag, "tiles": int(tiles), "tiles_with_zero_a1": int((~ok).sum()),
            "log2_min": round(float(r.min()), 2), "log2_median": round(float(np.median(r)), 2),
            "log2_p95": round(float(np.percentile(r, 95)), 2), "log2_max": round(float(r.max()), 2)}


def main():
    tiles = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    P = orc.ORACLE.param_count(*NET)
    Xb, _ = synthetic_batch(np.random.default_rng(1234), tiles, SIZE, SIZE)
    print(json.dumps(study("bench.py data, weights N(0, 1e-3)", Xb, init_params(NET, P), tiles)))
    Xt, _ = make_batch(np.random.default_rng(1234), tiles, SIZE, SIZE)
    print(json.dumps(study("make_batch, weights N(0, 0.05)", Xt,
                           make_params(np.random.default_rng(1234), NET, sd=0.05), tiles)))


if __name__ == "__main__":
    main()
