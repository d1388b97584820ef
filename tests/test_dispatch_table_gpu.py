"""Dispatch of the net-level calls against a recorded table: which kernel
family (srcnn_last_path) and which kernel variants, in launch order
(srcnn_last_kernels), serve each net / tile under either arithmetic.  The
table, tests/golden/dispatch_table.json, is recorded on the MI355X by
tools/record_dispatch_table.py; the comparison is exact list equality.  The
plans that decide all of this are plan_step of fused_plan.hpp (the fused
family, train_fused.hip; its names are compared with the table on the host
too, tests/test_fused_plan_cpu.py), plan_step of wide_plan.hpp (the wide
family, train_wide.hip) and plan_forward of fwd_plan.hpp (forward_fused.hip)."""
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN, ROOT
from step_util import S, _settings  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def load_tool():
    spec = importlib.util.spec_from_file_location(
        "record_dispatch_table", os.path.join(ROOT, "tools", "record_dispatch_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


tool = load_tool()


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "dispatch_table.json")) as fh:
        return json.load(fh)


def test_golden_holds_every_case(golden):
    ids = [tool.case_id(n, s, p, a) for n, s, p in tool.CASES for a in (0, 1)]
    assert sorted(golden) == sorted(ids)
    for n, s, p in tool.CASES:
        calls = ["train_fwd_bwd"]
        if (n, s, p) in tool.FULL:
            calls += ["train_step", "lazy_first", "lazy_second", "forward"]
        for a in (0, 1):
            assert list(golden[tool.case_id(n, s, p, a)]) == calls


@pytest.mark.parametrize("arith", [0, 1])
@pytest.mark.parametrize("name,size,path", tool.CASES,
                         ids=["%s-%d-%s" % (n, s, "generic" if p else "auto") for n, s, p in tool.CASES])
def test_dispatch_is_the_recorded_one(S, golden, name, size, path, arith):
    want = golden[tool.case_id(name, size, path, arith)]
    got = tool.run_case(S, torch, name, size, path, arith)  # (restores arith and path in a finally)
    assert S.get_arith() == 0 and S.get_path() == 0
    assert list(got) == list(want)
    for call in want:
        print(call, got[call])
        assert got[call]["path"] == want[call]["path"], call
        assert got[call]["kernels"] == want[call]["kernels"], call


@pytest.mark.parametrize("arith", [0, 1])
def test_wide_step_profiles_one_launch_per_kernel(S, arith):
    """Every profile name of the wide step (and the slab reduction) reports
    one launch per step, under either arithmetic."""
    net = S.Net(*tool.NETS["wide"])
    size, batch = 33, tool.BATCH
    P = S.net_param_count(net)
    X, T = torch.randn(batch * size * size, device="cuda"), torch.randn(batch * size * size, device="cuda")
    p, g = 0.05 * torch.randn(P, device="cuda"), torch.zeros(P, device="cuda")
    nbytes = S.train_workspace_bytes(net, size, size, batch)
    ws = torch.zeros(nbytes // 4 + 64, device="cuda")
    S.set_arith(arith)
    try:
        S.profile_reset()
        S.profile_enable(True)
        S.train_fwd_bwd(net, X, T, size, size, batch, p, g, None, ws, nbytes)
        torch.cuda.synchronize()
        assert S.last_path() == "wide"
        S.profile_enable(False)
        stats = S.profile_stats()
    finally:
        S.profile_enable(False)
        S.profile_reset()
    print(stats)
    wide = sorted(k for k in stats if k.startswith("wide_"))
    # prepack, the three forwards, delta1 (+ grad1 where they are two kernels), grad2
    assert len(wide) >= 6 and "slab_reduce" in stats, stats
    for k in wide + ["slab_reduce"]:
        assert stats[k][0] == 1, (k, stats[k])
