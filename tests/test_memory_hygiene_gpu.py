"""Memory hygiene of the HIP path: what the kernels read and write beyond
their data (include/srcnn.h, "Memory contract").

Every call here runs three times on the same inputs, with
  - a workspace of EXACTLY *_workspace_bytes() bytes (no slack), pre-filled
    with zeros, then NaN, then +1e30: the workspace needs no initialisation,
    so no kernel may consume a region that no kernel of the same call wrote;
  - every buffer the call writes (workspace, gradients, squared error,
    parameters, momenta, outputs) between guard bands that must stay intact;
  - every buffer the call only reads (X, T, parameters) between guard bands
    holding the same three fills: an over-read that is discarded passes, one
    that reaches arithmetic does not.
The results must be BIT-IDENTICAL across the three runs: the library is
deterministic by design (test_full_batch_gradients_vs_oracle asserts
run-to-run bit-determinism), so any difference is foreign memory reaching a
result.  No oracle here: HIP against HIP.

+1e30 matters beside NaN: a ReLU' mask read from foreign memory lets a
positive finite value through, while NaN > 0 is false and hides that.

The delta3-mode run-geometry sweep at the end compares the split-bf16 step
with the oracles at tiles of every column / row remainder class.
"""
import numpy as np
import pytest

import srcnn_oracle as orc
import hip_util
from hip_util import (H, RTOL, act_sizes, assert_close, check_gradients, dims, guarded, guards_intact, make_batch,
                      make_params, same_bits, segments)
from step_util import S, _settings, run_step  # noqa: F401

pytestmark = pytest.mark.gpu

NETS = {"default": (64, 32, 9, 1, 5), "wide": (128, 64, 9, 5, 5), "tiny": (8, 4, 5, 1, 3),
        "example": (32, 16, 9, 1, 5), "default_f3": (64, 32, 9, 1, 3)}
FILLS = (0.0,) + hip_util.POISONS  # zeros, NaN, +1e30
LR = [1e-4, 2e-4, 1e-5]


def assert_runs_identical(runs, what):
    """runs: one dict of host arrays per fill; all bit-identical to the first."""
    names = list(runs[0])
    for fill, r in zip(FILLS[1:], runs[1:]):
        for nm in names:
            a, b = runs[0][nm], r[nm]
            assert np.isfinite(b).all(), "%s: %s not finite with fill %r" % (what, nm, fill)
            if not same_bits(a, b):
                d = np.flatnonzero(a.view(np.int32) != b.view(np.int32))
                raise AssertionError(
                    "%s: %s differs between fill 0 and fill %r at %d of %d elements (first %s: %r vs %r)"
                    % (what, nm, fill, d.size, a.size, d[:6].tolist(), a.ravel()[d[:3]].tolist(),
                       b.ravel()[d[:3]].tolist()))


def check_kernels(S, path, kernels):
    assert S.last_path() == path, (S.last_path(), path)
    ks = S.last_kernels()
    assert all(k in ks for k in kernels), (ks, kernels)


def live_params(rng, cfg, X, w, h, batch):
    """Random parameters whose layer-3 bias is shifted so that half of the
    outputs A3 are positive.  A3 of a random net on smooth patches has one
    sign almost everywhere, and last_layer_delta masks by A3 > 0: left as
    drawn, most seeds give delta3 = 0 and gradients that never change, which
    would pass every comparison here vacuously."""
    params = make_params(rng, cfg, sd=0.05)
    params[-1] -= np.median(orc.forward(cfg, X, w, h, batch, params))
    return params


_INPUTS = {}


def train_inputs(name, w, h, batch, seed=5):
    key = (name, w, h, batch, seed)
    if key not in _INPUTS:
        cfg = NETS[name]
        rng = np.random.default_rng(seed)
        X, T = make_batch(rng, batch, w, h)
        params = live_params(rng, cfg, X, w, h, batch)
        g0 = (1e-3 * rng.standard_normal(params.size)).astype(np.float32)
        m0 = (1e-3 * rng.standard_normal(params.size)).astype(np.float32)
        _INPUTS[key] = (cfg, X, T, params, g0, m0)
    return _INPUTS[key]


def assert_live(A3, grads, g0, what):
    """The step exercised its masks: a mixed layer-3 ReLU' decision and
    gradients that moved (dead channels of a small net leave some unchanged)."""
    pos = float((A3 > 0).mean())
    assert 0.2 < pos < 0.8, "%s: %.2f of A3 positive: delta3 mask not mixed" % (what, pos)
    moved = float((grads != g0).mean())
    assert moved > 0.5, "%s: only %.2f of the gradients changed" % (what, moved)


def read_activations(S, net, cfg, w, h, batch, ws, nbytes, fill):
    """A1 / A2 / A3 of the step that last wrote `ws`, into guarded outputs."""
    outs = [guarded(n, fill) for n in act_sizes(cfg, w, h, batch)]
    S.train_activations(net, w, h, batch, ws, nbytes, *outs)
    res = [H(o) for o in outs]
    guards_intact(*outs)
    return dict(zip(("A1", "A2", "A3"), res))


# (net, w, h, batch, arith, srcnn_last_path, kernels srcnn_last_kernels must name)
TRAIN_CASES = [
    # the default training path: split-bf16, delta3 mode.  Batches ragged
    # against the grids: l3r walks the batch from its end, two samples per
    # block (257); l12 at 512 blocks (513)
    ("default", 33, 33, 5, 0, "fused", ["l12x6_fwd", "l3r_d3", "d1x6_d3"]),
    ("default", 33, 33, 257, 0, "fused", ["l12x6_fwd", "l3r_d3", "d1x6_d3"]),
    ("default", 33, 33, 513, 0, "fused", ["l12x6_fwd", "l3r_d3", "d1x6_d3"]),
    ("default", 33, 33, 5, 1, "fused", ["l12_fwd", "l3r_delta", "d1c_grad12"]),
    ("default", 33, 33, 257, 1, "fused", ["l12_fwd", "l3r_delta", "d1c_grad12"]),
    ("default", 33, 33, 513, 1, "fused", ["l12_fwd", "l3r_delta", "d1c_grad12"]),
    ("example", 33, 33, 3, 0, "fused", ["l3_delta"]),
    ("default_f3", 33, 33, 3, 0, "fused", ["l3_delta"]),
    ("default", 39, 39, 3, 0, "fused", ["l3_op_level"]),
    ("default", 48, 48, 3, 0, "fast", []),
    ("wide", 33, 33, 3, 0, "wide", []),
    ("wide", 37, 37, 3, 0, "fast", []),
    ("tiny", 15, 15, 5, 0, "generic", []),
]


def case_id(c):
    return "%s_%dx%d_b%d_%s" % (c[0], c[1], c[2], c[3], "f32" if c[4] else "split")


@pytest.mark.parametrize("case", TRAIN_CASES, ids=case_id)
def test_train_fwd_bwd_memory(S, case):
    """srcnn_train_fwd_bwd + srcnn_train_activations: gradients, squared error
    and A1 / A2 / A3 do not depend on the workspace's previous contents or on
    the memory around X, T and the parameters; nothing is written outside the
    workspace, the gradients, the squared error and the activation outputs."""
    name, w, h, batch, arith, path, kernels = case
    cfg, X, T, params, g0, _ = train_inputs(name, w, h, batch)
    net = S.Net(*cfg)
    S.set_arith(arith)
    nbytes = S.train_workspace_bytes(net, w, h, batch)
    assert nbytes % 4 == 0
    runs = []
    for fill in FILLS:
        Xd, Td, pd = guarded(X, fill), guarded(T, fill), guarded(params, fill)
        g, err = guarded(g0, fill), guarded(np.array([0.5], np.float32), fill)
        ws = guarded(nbytes // 4, fill)
        S.train_fwd_bwd(net, Xd, Td, w, h, batch, pd, g, err, ws, nbytes)
        check_kernels(S, path, kernels)
        r = {"grads": H(g), "sq_err": H(err)}
        r.update(read_activations(S, net, cfg, w, h, batch, ws, nbytes, fill))
        guards_intact(Xd, Td, pd, g, err, ws)
        assert same_bits(H(Xd), X) and same_bits(H(Td), T) and same_bits(H(pd), params), "an input was written"
        runs.append(r)
    assert_runs_identical(runs, "train_fwd_bwd " + case_id(case))
    assert_live(runs[0]["A3"], runs[0]["grads"], g0, case_id(case))
    assert runs[0]["sq_err"][0] > 0.5


STEP_CASES = [
    # the fused update reads the slabs (slab_reduce_update)
    ("default", 33, 33, 5, 0, "fused", ["d1x6_d3", "slab_reduce_update"]),
    ("default", 33, 33, 257, 0, "fused", ["d1x6_d3", "slab_reduce_update"]),
    ("default", 33, 33, 5, 1, "fused", ["d1c_grad12", "slab_reduce_update"]),
    ("example", 33, 33, 3, 0, "fused", ["l3_delta", "slab_reduce_update"]),
    ("default", 39, 39, 3, 0, "fused", ["l3_op_level", "update_all"]),
    ("wide", 33, 33, 3, 0, "wide", []),
    ("tiny", 15, 15, 5, 0, "generic", ["update_all"]),
]


@pytest.mark.parametrize("case", STEP_CASES, ids=case_id)
def test_train_step_memory(S, case):
    """srcnn_train_step: parameters, momenta, the zeroed gradients and the
    squared error, with every one of them and the workspace guarded."""
    name, w, h, batch, arith, path, kernels = case
    cfg, X, T, params, g0, m0 = train_inputs(name, w, h, batch, seed=6)
    net = S.Net(*cfg)
    S.set_arith(arith)
    nbytes = S.train_workspace_bytes(net, w, h, batch)
    runs = []
    for fill in FILLS:
        Xd, Td = guarded(X, fill), guarded(T, fill)
        p, g, m = guarded(params, fill), guarded(g0, fill), guarded(m0, fill)
        err = guarded(np.array([0.5], np.float32), fill)
        ws = guarded(nbytes // 4, fill)
        S.train_step(net, Xd, Td, w, h, batch, p, g, m, 0.9, 1e-3, LR, 3 * batch, err, ws, nbytes)
        check_kernels(S, path, kernels)
        runs.append({"params": H(p), "grads": H(g), "momentum": H(m), "sq_err": H(err)})
        guards_intact(Xd, Td, p, g, m, err, ws)
    assert_runs_identical(runs, "train_step " + case_id(case))
    assert not runs[0]["grads"].any() and (runs[0]["params"] != params).mean() > 0.9


@pytest.mark.parametrize("name,w,h,batch,path", [("default", 33, 33, 5, "fused"), ("tiny", 15, 15, 5, "generic")])
def test_train_fwd_bwd_lazy_memory(S, name, w, h, batch, path):
    """Two chained srcnn_train_fwd_bwd_lazy steps (the first with nothing
    pending, the second applying the first one's update out of place):
    params_out, mom_out, gradients and squared error."""
    cfg, X, T, params, _, m0 = train_inputs(name, w, h, batch, seed=7)
    net = S.Net(*cfg)
    P = params.size
    nbytes = S.train_workspace_bytes(net, w, h, batch)
    runs = []
    for fill in FILLS:
        Xd, Td = guarded(X, fill), guarded(T, fill)
        p_in, m_in = guarded(params, fill), guarded(m0, fill)
        p_out, m_out = guarded(P, fill), guarded(P, fill)
        g = guarded(P, fill)  # overwritten, not accumulated: starts as poison
        err = guarded(np.array([0.5], np.float32), fill)
        ws = guarded(nbytes // 4, fill)
        S.train_fwd_bwd_lazy(net, Xd, Td, w, h, batch, p_in, None, None, None, g, 0.9, 1e-3, LR, 0, err, ws,
                             nbytes)
        assert S.last_path() == path, S.last_path()
        g1 = H(g)
        S.train_fwd_bwd_lazy(net, Xd, Td, w, h, batch, p_in, p_out, m_in, m_out, g, 0.9, 1e-3, LR, batch, err,
                             ws, nbytes)
        assert S.last_path() == path, S.last_path()
        runs.append({"grads step 1": g1, "params_out": H(p_out), "mom_out": H(m_out), "grads step 2": H(g),
                     "sq_err": H(err)})
        guards_intact(Xd, Td, p_in, m_in, p_out, m_out, g, err, ws)
        assert same_bits(H(p_in), params) and same_bits(H(m_in), m0), "params_in / mom_in were written"
    assert_runs_identical(runs, "train_fwd_bwd_lazy %s" % name)
    assert (runs[0]["params_out"] != params).mean() > 0.9


# (net, w, h, batch, srcnn_set_path, srcnn_set_arith, srcnn_last_path)
FORWARD_CASES = [
    ("default", 77, 45, 3, 1, 0, "generic"),  # the layered path: conv_fwd x 3 through A1 / A2 in ws
    # the fused forward takes every frame with a 5 x 5 A2 (13 x 13 is the
    # smallest the net accepts at all: one output); 75 x 61 is ragged against
    # the split kernel's regions of 32 x 24 outputs (A2 67 x 53: 3 x 3 regions,
    # the last 3 wide and 5 high) and against the fp32 kernel's
    ("default", 13, 13, 1, 0, 0, "fused"),
    ("default", 75, 61, 2, 0, 0, "fused"),
    ("default", 75, 61, 2, 0, 1, "fused"),
    ("example", 45, 77, 2, 0, 0, "fused"),
    ("wide", 40, 31, 2, 0, 0, None),
]


@pytest.mark.parametrize("name,w,h,batch,path,arith,family", FORWARD_CASES,
                         ids=lambda v: str(v))
def test_forward_memory(S, name, w, h, batch, path, arith, family):
    """srcnn_forward on an exact-size poisoned workspace, guarded output."""
    cfg = NETS[name]
    net = S.Net(*cfg)
    rng = np.random.default_rng(w * 100 + h)
    X, _ = make_batch(rng, batch, w, h)
    params = make_params(rng, cfg, sd=0.05)
    n_out = act_sizes(cfg, w, h, batch)[2]
    S.set_path(path)
    S.set_arith(arith)
    nbytes = S.forward_workspace_bytes(net, w, h, batch)
    runs = []
    for fill in FILLS:
        Xd, pd = guarded(X, fill), guarded(params, fill)
        out = guarded(n_out, fill, inner=float("nan"))  # every output must be written
        ws = guarded(nbytes // 4, fill)
        S.forward(net, Xd, w, h, batch, pd, out, ws, nbytes)
        if family is not None:
            assert S.last_path() == family, S.last_path()
        runs.append({"out": H(out)})
        guards_intact(Xd, pd, out, ws)
    assert np.isfinite(runs[0]["out"]).all()
    assert_runs_identical(runs, "forward %s %dx%d" % (name, w, h))
    assert runs[0]["out"].any()


def test_forward_smallest_frame(S):
    """13 x 13 is the smallest frame the default net accepts (12 x 12 has no
    output); FORWARD_CASES asserts that it already runs the fused kernel."""
    net = S.Net(*NETS["default"])
    assert S.forward_workspace_bytes(net, 12, 12, 1) == 0
    assert S.forward_workspace_bytes(net, 13, 13, 1) > 0


# ----------------------------------------------------------------------------
# op-level calls with a workspace
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("shape,path,family", [((1, 64, 9, 25, 25, 6), 0, "fast"),    # GRAD_SHAPES: default gW1
                                               ((64, 32, 1, 25, 25, 6), 0, "fast"),   # default gW2
                                               ((3, 5, 3, 7, 6, 3), 1, "generic")],  # ragged, generic
                         ids=["gW1_auto", "gW2_auto", "ragged_generic"])
def test_conv_grad_acc_memory(S, shape, path, family):
    n_prev, n_cur, f, ow, oh, b = shape
    rng = np.random.default_rng(3)
    iw, ih = ow + f - 1, oh + f - 1
    inp = rng.standard_normal(b * iw * ih * n_prev).astype(np.float32)
    dl = rng.standard_normal(b * ow * oh * n_cur).astype(np.float32)
    gW0 = rng.standard_normal(f * f * n_prev * n_cur).astype(np.float32)
    gB0 = rng.standard_normal(n_cur).astype(np.float32)
    S.set_path(path)
    nbytes = S.conv_grad_workspace_bytes(n_prev, n_cur, f, ow, oh, b)
    runs = []
    for fill in FILLS:
        i_d, d_d = guarded(inp, fill), guarded(dl, fill)
        gW, gB = guarded(gW0, fill), guarded(gB0, fill)
        ws = guarded(max(nbytes // 4, 1), fill)
        S.conv_grad_acc(i_d, d_d, gW, gB, n_prev, n_cur, f, ow, oh, b, ws, nbytes)
        assert S.last_path() == family, S.last_path()
        runs.append({"gW": H(gW), "gB": H(gB)})
        guards_intact(i_d, d_d, gW, gB, ws)
    assert_runs_identical(runs, "conv_grad_acc %s" % (shape,))
    assert (runs[0]["gW"] != gW0).all()


@pytest.mark.parametrize("n", [900, 100003])
def test_reductions_memory(S, n):
    """srcnn_sum, srcnn_sq_err and srcnn_sub_mean at an odd length: poisoned
    exact-size workspace, guarded result / data / mean."""
    rng = np.random.default_rng(n)
    data = rng.standard_normal(n).astype(np.float32)
    aw, ah, pad = (30, 30, 4) if n == 900 else (n, 1, 0)
    gt = rng.standard_normal((ah + 2 * pad) * (aw + 2 * pad)).astype(np.float32)
    nb = S.reduce_workspace_bytes(n)
    runs = []
    for fill in FILLS:
        r = {}
        for squared in (0, 1):
            d, res, ws = guarded(data, fill), guarded(1, fill), guarded(nb // 4, fill)
            S.buf_sum(d, n, squared, res, ws, nb)
            r["sum%d" % squared] = H(res)
            guards_intact(d, res, ws)
        g_d, y_d, res, ws = guarded(gt, fill), guarded(data, fill), guarded(1, fill), guarded(nb // 4, fill)
        S.sq_err(g_d, y_d, res, aw + 2 * pad, ah + 2 * pad, aw, ah, 1, ws, nb)
        r["sq_err"] = H(res)
        guards_intact(g_d, y_d, res, ws)
        d, mean, ws = guarded(data, fill), guarded(1, fill), guarded(nb // 4, fill)
        S.sub_mean(d, n, mean, ws, nb)
        r["mean"], r["centred"] = H(mean), H(d)
        guards_intact(d, mean, ws)
        runs.append(r)
    assert_runs_identical(runs, "reductions n=%d" % n)
    assert abs(float(runs[0]["sum0"][0]) - float(data.astype(np.float64).sum())) <= 1e-3 * np.sqrt(n)
    assert abs(float(runs[0]["centred"].astype(np.float64).mean())) < 1e-4


# ----------------------------------------------------------------------------
# delta3-mode run geometry (runs.hpp) against the oracles
# ----------------------------------------------------------------------------
# Tiles of the default net that reach l3r_d3 + d1x6_d3 under split arithmetic,
# chosen from d1x6_fits(w, h, true) (w <= 57, <= 160 KB of LDS, at least 4
# chunks), l3r_fits (A2 of at most 640 pixels, at most 512 outputs) and
# l3r_d3_fits: every column remainder ow % 4 (ow = w - 8; the remainder
# columns are cut into column runs) with oh % 4 == 0 and != 0 (column runs cut
# at the tile's last row: dummy slots inside a run), w < h and w > h.
#   (w, h, delta3 mode)                ow x oh   ow%4 oh%4
D3_TILES = [
    (32, 32, True),   # 24 x 24: 0 0; 144 runs, 18 chunks, NO dummy slot
    (20, 21, True),   # 12 x 13: 0 1; row runs only, 1 dummy run
    (33, 32, True),   # 25 x 24: 1 0; column runs without dummy slots
    (17, 19, True),   #  9 x 11: 1 3; 25 runs: the smallest tile delta3 mode takes
                      #          (4 chunks; 17 x 18 has 23 runs = 3 chunks); w < h
    (34, 28, True),   # 26 x 20: 2 0; w > h
    (30, 30, True),   # 22 x 22: 2 2; six dummy runs, two dummy slots per column
                      #          run: the geometry of 34 x 34 inside delta3 mode
    (27, 36, True),   # 19 x 28: 3 0; w < h
    (19, 19, True),   # 11 x 11: 3 3
    (18, 18, True),   # 10 x 10: 2 2; the smallest square tile of delta3 mode
    # 34 x 34 (26 x 26: 2 2, six dummy runs, two dummy slots per column run)
    # cannot reach delta3 mode: its A2 has 676 pixels, past l3r's 640 (40
    # 16-pixel units), so layer 3 runs on the op-level kernels and d1x6 takes
    # delta2 from HBM (d1x6_grad12).  Kept in the sweep on that path: the same
    # run geometry through l12x6 and the other d1x6 instantiation
    (34, 34, False),
]
_D3_REF = {}


def d3_reference(w, h, batch):
    """Inputs and both oracles' results for a sweep tile, computed once and
    shared by the two arithmetics (read-only)."""
    key = (w, h, batch)
    if key not in _D3_REF:
        cfg = NETS["default"]
        n1, n2, f1, f2, f3 = cfg
        rng = np.random.default_rng(1000 * w + h)
        X, T = make_batch(rng, batch, w, h)
        params = live_params(rng, cfg, X, w, h, batch)
        g0 = (1e-3 * rng.standard_normal(params.size)).astype(np.float32)
        rg, _ = orc.train_fwd_bwd(cfg, X, T, w, h, batch, params, g0)
        xg, _ = orc.f64.train_fwd_bwd(cfg, X, T, w, h, batch, params, g0)
        W1, B1, W2, B2, W3, B3 = segments(cfg, params)
        w1, h1, w2, h2, w3, h3 = dims(cfg, w, h)
        acts = []
        for m in (orc, orc.f64):  # (fp32 oracle, fp64 oracle): A1, A2 after ReLU, A3 linear
            A1 = m.conv_fwd(X, W1, B1, w, h, 1, n1, f1, 1, batch)
            A2 = m.conv_fwd(A1, W2, B2, w1, h1, n1, n2, f2, 1, batch)
            A3 = m.conv_fwd(A2, W3, B3, w2, h2, n2, 1, f3, 0, batch)
            acts.append({"A1": A1, "A2": A2, "A3": A3})
        ref_err = orc.sq_err(T, acts[0]["A3"], w, h, w3, h3, batch)
        assert_live(acts[0]["A3"], rg, g0, "sweep reference %dx%d" % (w, h))
        ref = (X, T, params, g0, rg, xg, acts, ref_err)
        for a in ref[:6] + tuple(acts[0].values()) + tuple(acts[1].values()):
            a.setflags(write=False)
        _D3_REF[key] = ref
    return _D3_REF[key]


@pytest.mark.parametrize("arith", [0, 1], ids=["split", "f32"])
@pytest.mark.parametrize("w,h,d3", D3_TILES, ids=lambda v: str(v))
def test_d3_mode_run_geometry_sweep(S, w, h, d3, arith):
    """Gradients, squared error, A1, A2 and A3 of the default net at batch 3
    against the fp32 and fp64 oracles, on tiles of every run-geometry class;
    under split arithmetic through l3r_d3 + d1x6_d3 (asserted), under fp32
    through d1c.  Exact-size NaN-poisoned workspace."""
    cfg = NETS["default"]
    batch = 3
    X, T, params, g0, rg, xg, acts, ref_err = d3_reference(w, h, batch)
    if arith == 0:
        want = ["l12x6_fwd", "l3r_d3", "d1x6_d3"] if d3 else ["l12x6_fwd", "l3_op_level", "d1x6_grad12"]
    else:
        want = ["l12_fwd", "l3r_delta" if d3 else "l3_op_level", "d1c_grad12"]

    def expect(path, ks):
        assert path == "fused", path
        assert all(k in ks for k in want), (ks, want)
        assert ("d1x6_d3" in ks) == (d3 and arith == 0), ks
    st = run_step(S, cfg, w, h, batch, X, T, params, g0, arith=arith, guard=True, hold=True, expect=expect)
    tag = "d3 sweep %dx%d %s " % (w, h, "f32" if arith else "split")
    check_gradients(cfg, st.grads, rg, xg, tag)
    assert st.sq_err == pytest.approx(ref_err, rel=1e-4)
    a = dict(zip(("A1", "A2", "A3"), st.activations()))
    for nm in ("A1", "A2", "A3"):
        assert_close(a[nm], acts[0][nm], RTOL, tag + nm, acts[1][nm])
