"""bench.py's plain run, `--full` and `--dump-outputs` (CPU, stand-in library).

`bench.main` runs in this process as the one rank of `--gpus 1`, with the
recording stand-in of test_bench_multirank_cpu.py in place of srcnn_amd and a
CPU device object.  Its train_step adds 1 to every parameter and 2 to every
momentum element, which makes the dump of K timed steps known exactly.
"""
import json
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_bench_multirank_cpu import CpuDevice, P_DEFAULT, StubS

sys.path.insert(0, ROOT)
import bench  # noqa: E402  (module import touches no GPU)


class CountingS(StubS):
    def train_step(self, net, X, T, w, h, batch, params, grads, mom, *rest):
        super().train_step(net, X, T, w, h, batch, params, grads, mom, *rest)
        params.add_(1.0)
        mom.add_(2.0)


def _run(tmp_path, capsys, argv, monkeypatch):
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    S = CountingS(0, str(tmp_path / "log.json"))
    bench.main(["--gpus", "1", "--batch", "8"] + argv, S=S, device=CpuDevice())
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 1  # ONE JSON line
    return json.loads(lines[0]), S


def test_plain_run_times_only_the_headline(tmp_path, capsys, monkeypatch):
    steps, warmup = 4, 2
    line, S = _run(tmp_path, capsys, ["--steps", str(steps), "--warmup", str(warmup), "--settle-ms", "0"],
                   monkeypatch)
    # --steps sets the number of timed steps: W + K calls of the step in all
    assert len([e for e in S.log if e[0] == "train_step"]) == steps + warmup
    assert line["steps"] == steps and line["warmup"] == warmup and line["n_gpus"] == 1
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line
    assert line["unit"] == "tiles/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["ms_per_step"] > 0
    # value and ms_per_step describe the same K steps of 8 tiles
    assert line["value"] == pytest.approx(8 / (line["ms_per_step"] * 1e-3), rel=1e-2)
    # nothing of the side legs
    for key in ("wide", "forward", "forward_tile_256", "cpu_forward_baseline"):
        assert key not in line
    assert line["cpu_baseline"] is None


def test_full_reaches_the_side_legs(tmp_path, capsys, monkeypatch):
    """With the side legs replaced by recorders: --full runs every one of them
    and puts their records into the line, a plain run calls none, and the
    --no-* options drop single legs of a full run."""
    legs = ("wide_training", "forward_tile_256", "forward_4k", "cpu_baseline", "cpu_forward_baseline")
    called = []
    for leg in legs:
        monkeypatch.setattr(bench, leg, lambda *a, _leg=leg, **kw: called.append(_leg) or {"leg": _leg})
    monkeypatch.setattr(bench.time, "sleep", lambda s: None)  # the pause after the wide net
    base = ["--steps", "2", "--warmup", "1", "--settle-ms", "0"]
    line, _ = _run(tmp_path, capsys, base, monkeypatch)
    assert called == []
    line, _ = _run(tmp_path, capsys, base + ["--full"], monkeypatch)
    assert called == list(legs)
    assert line["wide"] == {"leg": "wide_training"} and line["forward"] == {"leg": "forward_4k"}
    assert line["forward_tile_256"] == {"leg": "forward_tile_256"}
    assert line["cpu_baseline"] == {"leg": "cpu_baseline"}
    assert line["cpu_forward_baseline"] == {"leg": "cpu_forward_baseline"}
    del called[:]
    line, _ = _run(tmp_path, capsys, base + ["--full", "--no-wide", "--no-cpu-baseline"], monkeypatch)
    assert called == ["forward_tile_256", "forward_4k"]
    assert "wide" not in line and line["cpu_baseline"] is None


@pytest.mark.parametrize("warmup,settle_ms", [(0, "0"), (3, "0"), (1, "0.5")])
def test_dump_outputs_depend_on_the_arguments_only(tmp_path, capsys, monkeypatch, warmup, settle_ms):
    steps = 3
    out = tmp_path / "dump"
    line, S = _run(tmp_path, capsys, ["--steps", str(steps), "--warmup", str(warmup), "--settle-ms", settle_ms,
                                      "--dump-outputs", str(out)], monkeypatch)
    assert line["outputs"] == ["grads", "momentum", "params"]
    assert sorted(p.name for p in out.iterdir()) == ["grads.npy", "momentum.npy", "params.npy"]
    arrs = {k: np.load(out / (k + ".npy")) for k in line["outputs"]}
    for a in arrs.values():
        assert a.dtype == np.float32 and a.shape == (P_DEFAULT,)
    # the state is back at its seeded initial values when the timed steps
    # begin, however many untimed steps ran before them
    want = bench.init_params(bench.DEFAULT_NET, P_DEFAULT)
    for _ in range(steps):
        want = want + np.float32(1.0)
    np.testing.assert_array_equal(arrs["params"], want)
    np.testing.assert_array_equal(arrs["momentum"], np.full(P_DEFAULT, 2.0 * steps, np.float32))
    np.testing.assert_array_equal(arrs["grads"], np.zeros(P_DEFAULT, np.float32))
    assert sum(a.nbytes for a in arrs.values()) <= 64 << 20
