"""bench.py --dump-outputs on the GPU: the dumped training state of a plain
`--gpus 1` run is the state the CPU oracle reaches from the same seeded inputs
after the same K steps, whatever the number of untimed steps before them.

bench.main runs in this process (64 tiles per step, 3 timed steps); the
oracle runs the reference step (train_fwd_bwd + update_all) 3 times on the
batch bench.py builds (seed 1234, weights N(0, 1e-3)).  Tolerance: hip_util's
RTOL, normwise, as for one step's gradients -- three steps of lr <= 1e-4 move
the parameters by ~1e-7, far too little for the later steps' gradients to
drift apart by more than their own rounding.
"""
import json
import sys

import numpy as np
import pytest

import srcnn_oracle as orc
from conftest import ROOT
from hip_util import RTOL, assert_close, max_rel_err
from step_util import S, _settings  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, ROOT)
import bench  # noqa: E402

BATCH, STEPS = 64, 3


@pytest.fixture(scope="module")
def oracle_state():
    cfg = bench.DEFAULT_NET
    rng = np.random.default_rng(1234)
    X, T = bench.synthetic_batch(rng, BATCH, bench.TILE, bench.TILE)
    params = bench.init_params(cfg, orc.param_count(*cfg))
    grads = np.zeros(params.size, np.float32)
    mom = np.zeros(params.size, np.float32)
    for _ in range(STEPS):
        grads, _ = orc.train_fwd_bwd(cfg, X, T, bench.TILE, bench.TILE, BATCH, params, grads)
        params, grads, mom = orc.update_all(cfg, params, grads, mom, 0.9, 1e-3, [1e-4, 1e-4, 1e-5], BATCH)
    return {"params": params, "momentum": mom, "grads": grads}


@pytest.mark.parametrize("warmup,settle_ms", [(0, "0"), (4, "1")])
def test_dump_matches_oracle(tmp_path, capsys, monkeypatch, oracle_state, warmup, settle_ms):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    out = tmp_path / "dump"
    bench.main(["--gpus", "1", "--batch", str(BATCH), "--steps", str(STEPS), "--warmup", str(warmup),
                "--settle-ms", settle_ms, "--dump-outputs", str(out)])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["steps"] == STEPS and line["ms_per_step"] > 0
    assert line["config"]["kernel_path"] == "fused"  # the HIP path of the headline, not a fall-back
    assert "wide" not in line and "forward" not in line and line["cpu_baseline"] is None
    for name in ("params", "momentum", "grads"):
        got = np.load(out / (name + ".npy"))
        assert got.dtype == np.float32
        print(name, "normwise err vs oracle:", max_rel_err(got, oracle_state[name]))
    for name in ("params", "momentum", "grads"):
        assert_close(np.load(out / (name + ".npy")), oracle_state[name], rtol=RTOL,
                     what="bench dump " + name)
    assert np.abs(np.load(out / "momentum.npy")).max() > 0
