"""The workspace queries against a recorded table (no GPU: the queries are
host-only).  srcnn_train_workspace_bytes and srcnn_forward_workspace_bytes
follow from the dispatch plans (which family serves a shape, its grids and
slab regions), so every byte count of tests/golden/workspace_table.json,
recorded by tools/record_workspace_table.py, must come out unchanged."""
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN, ROOT


@pytest.fixture(scope="module")
def S():
    import srcnn_amd
    return srcnn_amd


def load_tool():
    spec = importlib.util.spec_from_file_location(
        "record_workspace_table", os.path.join(ROOT, "tools", "record_workspace_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_workspace_table_is_unchanged(S):
    tool = load_tool()
    with open(os.path.join(GOLDEN, "workspace_table.json")) as fh:
        golden = json.load(fh)
    got = tool.record(S)
    # the golden file holds the whole table of the tool: no row missing or skipped
    nets, shapes = len(tool.NETS), len(tool.TILES) + len(tool.FRAMES)
    assert len(golden) == len(got) == nets * 2 * 2 * shapes
    key = lambda r: (r["net"], r["w"], r["h"], r["arith"], r["path"])
    assert [key(r) for r in got] == [key(r) for r in golden]
    bad = [(key(g), what, b, want, have)
           for g, r in zip(golden, got) for what in ("train", "forward") if what in g
           for b, want, have in zip(g["batches"], g[what], r[what]) if want != have]
    assert not bad, "%d byte counts differ, first: %s" % (len(bad), bad[:5])
    assert got == golden
    # the table is not trivially empty: the served shapes ask for workspace
    assert sum(v > 0 for r in golden for v in r.get("train", [])) > 2000
    assert S.get_arith() == 0 and S.get_path() == 0
