"""d1x6's delta3 forms with one pair of gW1 scales per launch: delta1 and X are
scaled by powers of two from the launch's own maxima (max |delta3| per l3r
block, max |X| per l12x6 block, left behind the relu' mask in the D2 region
and reduced in d1x6's prologue), and a sample's top is one barrier.

Default net, split arithmetic, through the C ABI; every case asserts the
kernels l12x6_fwd, l3r_d3 and its form of d1x6.  Cases (w, h, batch):
  - "below", 33 x 33 x 5: a batch below every grid, so most maxima slots are
    never written and must never be read;
  - "many", 19 x 17 x 770: three to four samples per d1x6 block;
  - "scratch", 27 x 37 x 3: d1x6_d3_sc takes the same prologue;
  - "outlier", 33 x 33 x 520 with the target of sample OUTLIER scaled by 2^20:
    every other sample lies 2^20 below the launch's scale;
  - "tiny", the same with X of samples 256-511 scaled by 2^-20;
  - "zero_bound", 33 x 33 x 5 with every target the step's own output: all
    delta3 zero;
  - "zero_x", 33 x 33 x 5 with X all zero.
The first five hold gW1 and gB1 (the outlier cases gW2 as well) to a normwise
error against the fp64 oracle of at most 1.5 x the larger error of the
fp32-arithmetic step (srcnn_set_arith(1)) on the same inputs, as
tests/test_d1x6_gw1_f16_gpu.py states it, and check all six gradients with
hip_util.check_gradients on an exact-size NaN-poisoned guarded workspace.  The
zero cases ask for finite gradients and gW1 = 0.  Two more tests: the "many"
case twice for equal bits, and stale maxima slots (NaN poison would hide
behind fmaxf there, so that one fills the slots with large finite values): a
5-sample step on a workspace that a 520-sample step with targets x 2^40 has
used, and on one filled with 1e30, gives the bytes of the same step on a
zeroed workspace.
"""
import functools

import numpy as np
import pytest

import srcnn_oracle as orc
from hip_util import NAMES, check_gradients, dims, make_batch, make_params, normwise, same_bits, segments
from step_util import S, _settings, no_x6, ran, run_step  # noqa: F401

pytestmark = pytest.mark.gpu

CFG = (64, 32, 9, 1, 5)
OUTLIER = 100  # outside the tiny samples 256-511
CASES = {  # name -> (w, h, batch, d1x6 form, seed, segments under the normwise bound)
    "below": (33, 33, 5, "d1x6_d3", 41, 2),
    "many": (19, 17, 770, "d1x6_d3", 42, 2),
    "scratch": (27, 37, 3, "d1x6_d3_sc", 43, 2),
    "outlier": (33, 33, 520, "d1x6_d3", 44, 3),
    "tiny": (33, 33, 520, "d1x6_d3", 44, 3),
}


def grads(S, arith, w, h, batch, X, T, params, form=None, **kw):
    """The step's gradients; under split arithmetic (a `form` given) l12x6_fwd,
    l3r_d3 and that form of d1x6 must have run, under fp32 arithmetic no split
    kernel."""
    expect = ran("fused", ["l12x6_fwd", "l3r_d3"], form) if form is not None else no_x6
    kw.setdefault("guard", True)
    return run_step(S, CFG, w, h, batch, X, T, params, arith=arith, expect=expect, **kw).grads


@functools.lru_cache(maxsize=None)
def inputs(name):
    w, h, batch, _, seed, _ = CASES[name]
    rng = np.random.default_rng(seed)
    X, T = make_batch(rng, batch, w, h)
    params = make_params(rng, CFG, sd=0.05)
    if name in ("outlier", "tiny"):
        T = T.reshape(batch, -1).copy()
        T[OUTLIER] *= np.float32(2.0 ** 20)
        T = T.ravel()
    if name == "tiny":
        X = X.reshape(batch, -1).copy()
        X[256:512] *= np.float32(2.0 ** -20)
        X = X.ravel()
    return X, T, params  # (shared between tests: nobody writes to them)


def own_output_targets(S, w, h, batch, X, T, params):
    """T with every sample's inner region set to the step's own output there,
    so that delta3 = 0 throughout."""
    a3 = run_step(S, CFG, w, h, batch, X, T, params, guard=True, hold=True).activations()[2]
    w3, h3 = dims(CFG, w, h)[4:]
    py, px = (h - h3) // 2, (w - w3) // 2
    t = T.reshape(batch, h, w).copy()
    t[:, py:py + h3, px:px + w3] = a3.reshape(batch, h3, w3)
    return t.ravel()


@pytest.mark.parametrize("name", list(CASES))
def test_launch_scale_gradients(S, name):
    w, h, batch, form, _, nseg = CASES[name]
    X, T, params = inputs(name)
    g0 = np.zeros(params.size, np.float32)
    rg, _ = orc.train_fwd_bwd(CFG, X, T, w, h, batch, params, g0)
    xg, _ = orc.f64.train_fwd_bwd(CFG, X, T, w, h, batch, params, g0)
    got = grads(S, 0, w, h, batch, X, T, params, form)
    f32 = grads(S, 1, w, h, batch, X, T, params)
    errs = {}
    for nm, g, f, x in list(zip(NAMES, segments(CFG, got), segments(CFG, f32), segments(CFG, xg)))[:nseg]:
        errs[nm] = (normwise(g, x), normwise(f, x))
        print("%s g%s: f16 x3, launch scales %.3e  fp32 arithmetic %.3e" % (name, nm, *errs[nm]))
    bar = 1.5 * max(e[1] for e in errs.values())
    for nm, (es, _) in errs.items():
        assert es <= bar, (name, nm, es, bar)
    check_gradients(CFG, got, rg, xg, "launch scale %s " % name)


def test_zero_bound(S):
    """All delta3 zero: the bound is zero, any finite scale does."""
    w, h, batch = 33, 33, 5
    X, T, params = inputs("below")
    T0 = own_output_targets(S, w, h, batch, X, T, params)
    got = grads(S, 0, w, h, batch, X, T0, params, "d1x6_d3")
    assert np.isfinite(got).all()
    assert not got.any(), [nm for nm, g in zip(NAMES, segments(CFG, got)) if g.any()]


def test_zero_x(S):
    """X all zero: finite gradients, gW1 = 0, the rest as the oracles have it."""
    w, h, batch = 33, 33, 5
    X, T, params = inputs("below")
    X0 = np.zeros_like(X)
    g0 = np.zeros(params.size, np.float32)
    rg, _ = orc.train_fwd_bwd(CFG, X0, T, w, h, batch, params, g0)
    xg, _ = orc.f64.train_fwd_bwd(CFG, X0, T, w, h, batch, params, g0)
    got = grads(S, 0, w, h, batch, X0, T, params, "d1x6_d3")
    assert np.isfinite(got).all()
    assert not segments(CFG, got)[0].any()
    assert segments(CFG, got)[1].any()  # (gB1 is not zero: the step did run)
    check_gradients(CFG, got, rg, xg, "launch scale zero x ")


def test_determinism(S):
    w, h, batch, form, _, _ = CASES["many"]
    X, T, params = inputs("many")
    a = grads(S, 0, w, h, batch, X, T, params, form)
    b = grads(S, 0, w, h, batch, X, T, params, form)
    assert same_bits(a, b), "two runs differ"


def test_stale_slots(S):
    """The maxima slots past the batch are never read: what an earlier, larger
    step (or anyone) left in the workspace does not reach a 5-sample step."""
    import torch
    w, h, big, small = 33, 33, 520, 5
    Xb, Tb = make_batch(np.random.default_rng(45), big, w, h)
    Xs, Ts, params = inputs("below")
    net = S.Net(*CFG)
    nbytes = S.train_workspace_bytes(net, w, h, big)
    assert nbytes >= S.train_workspace_bytes(net, w, h, small)

    def small_step(ws):
        return grads(S, 0, w, h, small, Xs, Ts, params, "d1x6_d3", guard=False, ws=(ws, nbytes))
    fresh = small_step(torch.zeros(nbytes // 4 + 64, dtype=torch.float32, device="cuda"))
    used = torch.zeros(nbytes // 4 + 64, dtype=torch.float32, device="cuda")
    grads(S, 0, w, h, big, Xb, (Tb * np.float32(2.0 ** 40)).astype(np.float32), params, "d1x6_d3", guard=False,
          ws=(used, nbytes))
    assert same_bits(small_step(used), fresh), "a stale slot of the larger step was read"
    filled = torch.full((nbytes // 4 + 64,), 1e30, dtype=torch.float32, device="cuda")
    assert same_bits(small_step(filled), fresh), "a slot past the batch was read"
