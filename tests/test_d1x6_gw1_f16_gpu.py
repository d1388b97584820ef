"""gW1 / gB1 of d1x6's delta3 forms on two-part fp16 split products (three
v_mfma_f32_32x32x16_f16 per k-step, split.hpp; delta1 and X scaled per sample
by powers of two, the accumulators' exponent kept in the kernel).

Default net, split arithmetic, through the C ABI on an exact-size NaN-poisoned
guarded workspace.  Cases (w, h, batch):
  - 33 x 33 x 5: one sample per block;
  - 19 x 17 x 770: three to four samples per block;
  - 27 x 37 x 3: the scratch form (d1x6_d3_sc);
  - 33 x 33 x 520, "jumps": the targets of samples 256-511 are scaled by 2^10,
    so every block's second sample has a delta3 2^10 above its first (blocks
    0-7 come back down with a third), and the target of sample 515 is the
    step's own output there, so block 3 meets delta3 = 0 (a zero bound) after
    the jump.
Each case asserts the kernel names, holds gW1 and gB1 to a normwise error
against the fp64 oracle of at most 1.5 x the larger of the two errors of the
fp32-arithmetic path (srcnn_set_arith(1)) on the same inputs, checks all six
gradients with hip_util.assert_close as it stands, and runs twice for equal
bits.  With SRCNN_GW1_DUMP set to a directory every case also saves its
gradients there (<case>.npy), so runs of two libraries (SRCNN_HIP_LIB) can be
compared byte for byte outside W1 | B1.
"""
import os

import numpy as np
import pytest

import srcnn_oracle as orc
from hip_util import NAMES, check_gradients, dims, make_batch, make_params, normwise, same_bits, segments
from step_util import S, _settings, no_x6, ran, run_step  # noqa: F401

pytestmark = pytest.mark.gpu

CFG = (64, 32, 9, 1, 5)
CASES = [("one", 33, 33, 5, "d1x6_d3", 31), ("many", 19, 17, 770, "d1x6_d3", 32), ("scratch", 27, 37, 3, "d1x6_d3_sc", 33),
         ("jumps", 33, 33, 520, "d1x6_d3", 34)]
ZERO_SAMPLE = 515


def grads(S, arith, w, h, batch, X, T, params, form=None):
    """The step's gradients on guarded buffers; under split arithmetic (a
    `form` given) l12x6_fwd, l3r_d3 and that form of d1x6 must have run, under
    fp32 arithmetic no split kernel."""
    expect = ran("fused", ["l12x6_fwd", "l3r_d3"], form) if form is not None else no_x6
    return run_step(S, CFG, w, h, batch, X, T, params, arith=arith, guard=True, expect=expect).grads


def inputs(S, name, w, h, batch, seed):
    rng = np.random.default_rng(seed)
    X, T = make_batch(rng, batch, w, h)
    params = make_params(rng, CFG, sd=0.05)
    if name == "jumps":
        # a first step for the net's own output of the zero sample
        a3 = run_step(S, CFG, w, h, batch, X, T, params, guard=True, hold=True).activations()[2]
        w3, h3 = dims(CFG, w, h)[4:]
        a3 = a3.reshape(batch, h3, w3)
        t = T.reshape(batch, h, w).copy()
        t[256:512] *= np.float32(1024.0)
        t[ZERO_SAMPLE, 6:h - 6, 6:w - 6] = a3[ZERO_SAMPLE]
        T = t.ravel()
    return X, T, params


@pytest.mark.parametrize("name,w,h,batch,form,seed", CASES, ids=[c[0] for c in CASES])
def test_gw1_two_part_f16(S, name, w, h, batch, form, seed):
    X, T, params = inputs(S, name, w, h, batch, seed)
    g0 = np.zeros(params.size, np.float32)
    rg, _ = orc.train_fwd_bwd(CFG, X, T, w, h, batch, params, g0)
    xg, _ = orc.f64.train_fwd_bwd(CFG, X, T, w, h, batch, params, g0)
    got = grads(S, 0, w, h, batch, X, T, params, form)
    f32 = grads(S, 1, w, h, batch, X, T, params)
    dump = os.environ.get("SRCNN_GW1_DUMP")
    if dump:
        os.makedirs(dump, exist_ok=True)
        np.save(os.path.join(dump, name + ".npy"), got)
    errs = {}
    for nm, g, f, x in zip(NAMES[:2], segments(CFG, got), segments(CFG, f32), segments(CFG, xg)):
        errs[nm] = (normwise(g, x), normwise(f, x))
        print("%s g%s: f16 x3 %.3e  fp32 arithmetic %.3e" % (name, nm, *errs[nm]))
    bar = 1.5 * max(e[1] for e in errs.values())
    for nm, (es, _) in errs.items():
        assert es <= bar, (name, nm, es, bar)
    check_gradients(CFG, got, rg, xg, "gw1 f16 %s " % name)
    got2 = grads(S, 0, w, h, batch, X, T, params, form)
    assert same_bits(got, got2), "two runs differ"
