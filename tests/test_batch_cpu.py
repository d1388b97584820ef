"""srcnn_gather_batch without a GPU: the orientation map of tests/batch_ref.py
is the dihedral group, the binding packs the two device tables in the layout
include/srcnn.h documents, and the symbol is declared and bound."""
import ctypes
import os
import re

import numpy as np
import pytest

import batch_ref as B
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "srcnn.h")


@pytest.fixture(scope="module")
def S():
    import srcnn_amd
    return srcnn_amd


def asymmetric():
    return np.arange(15, dtype=np.float32).reshape(3, 5)  # sh = 3 rows of sw = 5


def test_eight_ops_are_distinct_and_closed_under_composition():
    foot = asymmetric()
    tiles = [B.orient(foot, op) for op in B.OPS]
    keys = [(t.shape, t.tobytes()) for t in tiles]
    assert len(set(keys)) == 8
    for op in B.OPS:
        assert np.array_equal(tiles[op], B.orient_by_index(foot, op)), op
    # applying q to the result of p is again one of the eight, and the table is a
    # group's: every row and every column of it is a permutation of the eight
    table = np.empty((8, 8), int)
    for p_ in B.OPS:
        for q in B.OPS:
            t = B.orient(tiles[p_], q)
            hit = [k for k in B.OPS if keys[k] == (t.shape, t.tobytes())]
            assert len(hit) == 1, (p_, q)
            table[p_, q] = hit[0]
    assert (np.sort(table, axis=0) == np.arange(8)[:, None]).all()
    assert (np.sort(table, axis=1) == np.arange(8)[None, :]).all()
    assert (table[0] == np.arange(8)).all() and (table[:, 0] == np.arange(8)).all()  # op 0 is the identity


@pytest.mark.parametrize("op", B.OPS)
def test_transposing_ops_swap_the_shape(op):
    foot = asymmetric()
    t = B.orient(foot, op)
    assert t.shape == ((5, 3) if op >= 4 else (3, 5))
    th, tw = t.shape
    assert B.footprint(tw, th, op) == (5, 3)  # (sw, sh) of the footprint it came from
    assert B.footprint(7, 4, op) == ((4, 7) if op >= 4 else (7, 4))
    plane = np.arange(200, dtype=np.float32).reshape(10, 20)
    w = B.window(plane, 2, 1, 7, 4, op)
    assert w.shape == ((7, 4) if op >= 4 else (4, 7)) and w[0, 0] == plane[1, 2]


class PlanePair(ctypes.Structure):
    _fields_ = [("x", ctypes.c_uint64), ("t", ctypes.c_uint64), ("x_pitch", ctypes.c_uint32),
                ("t_pitch", ctypes.c_uint32), ("w", ctypes.c_uint32), ("h", ctypes.c_uint32)]


class TileRef(ctypes.Structure):
    _fields_ = [("plane", ctypes.c_uint32), ("x", ctypes.c_uint32), ("y", ctypes.c_uint32),
                ("op", ctypes.c_uint32)]


def test_pack_plane_table_layout(S):
    assert ctypes.sizeof(PlanePair) == 32
    assert [getattr(PlanePair, f).offset for f, _ in PlanePair._fields_] == [0, 8, 16, 20, 24, 28]
    rows = [(0x1122334455667788, 0x0102030405060708, 82, 83, 81, 60), (4096, 8192, 1920, 1921, 1920, 1080)]
    raw = S.pack_plane_table(rows)
    assert raw.dtype == np.uint8 and raw.shape == (64,)
    got = (PlanePair * 2).from_buffer_copy(raw.tobytes())
    for g, r in zip(got, rows):
        assert (g.x, g.t, g.x_pitch, g.t_pitch, g.w, g.h) == r
    assert raw[:8].tolist() == [0x88, 0x77, 0x66, 0x55, 0x44, 0x33, 0x22, 0x11]  # little-endian
    assert S.pack_plane_table([]).size == 0


def test_pack_tile_refs_layout(S):
    assert ctypes.sizeof(TileRef) == 16
    assert [getattr(TileRef, f).offset for f, _ in TileRef._fields_] == [0, 4, 8, 12]
    rows = np.array([[1, 2, 3, 4], [0, 0xffffffff, 7, 5], [9, 47, 27, 0]], dtype=np.int64)
    raw = S.pack_tile_refs(rows)
    assert raw.dtype == np.uint8 and raw.shape == (48,)
    got = (TileRef * 3).from_buffer_copy(raw.tobytes())
    assert [[g.plane, g.x, g.y, g.op] for g in got] == rows.tolist()
    assert raw[:4].tolist() == [1, 0, 0, 0]
    assert S.pack_tile_refs(np.zeros((0, 4), np.int64)).size == 0
    with pytest.raises(ValueError):
        S.pack_tile_refs(np.zeros((3, 3), np.int64))
    with pytest.raises(ValueError):
        S.pack_tile_refs(np.array([[0, -1, 0, 0]]))


def test_symbol_is_declared_and_bound(S):
    src = open(HEADER).read()
    assert re.search(r"SRCNN_API\s+int\s+srcnn_gather_batch\s*\(\s*const\s+srcnn_plane_pair\s*\*", src)
    assert "} srcnn_plane_pair;" in src and "} srcnn_tile_ref;" in src
    assert re.search(r"#define\s+SRCNN_ABI_VERSION\s+1\b", src)
    res, args = S.SIGNATURES["srcnn_gather_batch"]
    assert res is ctypes.c_int and len(args) == 10
    assert callable(S.gather_batch)
