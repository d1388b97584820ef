"""gW2's delta2 operand and gB2 in d1x6's delta3 form with the part images
(csrc/hip/d6tr.hpp): the split parts of delta1's delta2 operand go through a
per-wave bf16 image and come back transposed as gW2's operand; gB2 is summed
per lane in the row layout and reduced across lanes after the loop.

Default net, split arithmetic, exact-size NaN-poisoned guarded workspace, and
every case asserts that l12x6_fwd, l3r_d3 and d1x6's delta3 form ran, and
which: d1x6_d3 is the form with the part images, d1x6_d3_sc the one with the
fp32 transpose scratch that the plan takes where the images do not fit the
LDS (D6Lds::tr).

Shapes (w, h, batch):
  - 19 x 17 x 3 and 17 x 19 x 3: the delta3 form needs at least 4 chunks, 25
    runs of 4 pixels; over all (ow, oh) the least w x h with 25 runs is 323,
    reached by 9 x 11 outputs (2 row runs per row + 3 runs in the one remainder
    column) and by 11 x 9 (2 per row + 3 remainder columns of 3 runs, the last
    run of each with 3 dummy slots).  d1x6_fits(w, h, true) holds for both.
  - 30 x 30 x 3: two dummy slots at the end of every column run.
  - 33 x 33 x 258: the headline tile; d1x6's blocks 0 and 1 take two samples
    each, so a wave's image and its gB2 sums cross a sample boundary, every
    other block takes one.
  - 19 x 17 x 770: every block takes three samples (blocks 0 and 1 four), so
    the item a wave forms past its block's last sample reads the delta3 image
    of a sample three back, not zeros, and must stay out of gB2 (at fewer
    samples per block that image is still all zero).
  - 27 x 37 x 3: the part images with padded delta3 rows are past 160 KB of
    LDS, so the plan keeps the scratch form (with padded rows, 163,568 B): the
    same run-code table, per-item X addresses and slot loads in the kernel's
    other delta3 instantiation.  Of the shapes in that case it is one of the
    three the fused step takes at all (w h <= 1536, h <= 40, A2 of at most 640
    pixels: 19 x 29 here, 15 x 25 outputs); the others are 29 x 37 and 30 x 36.
Checks:
  - all six gradients against the fp64 oracle (hip_util.assert_close), two
    runs bit-equal;
  - gB2 with delta3 nonzero at a single output pixel, in turn at the four
    corners of the output: the target equals the step's own A3 (from a first
    step, layer 3's bias raised until every A3 is positive, since delta3 is
    masked by A3 > 0) except at that pixel, where it is A3 - 1.  The 5 x 5 patch
    of delta2 then lies in a corner of the A2 tile: on the first slots of chunk
    0, at row ends, in the remainder columns' runs beside their dummy slots and
    on the last chunk.  All six gradients, gB2 among them, against the oracle.
Seeds were chosen on the CPU so that for every case the fp32 oracle alone
passes assert_close against the fp64 one with the same bounds (for the
single-pixel cases with the fp32 oracle's A3 standing in for the step's); each
case asserts that of its own reference again before the GPU result is trusted.
Layer 2's biases are centred per channel (as in test_d3_mask_gpu.py) so every
channel's ReLU' mask is mixed and every gB2 element has terms.
"""
import numpy as np
import pytest

import srcnn_oracle as orc
from hip_util import check_gradients, dims, make_batch, make_params, offsets, same_bits
from step_util import S, _settings, centre_params, ran, run_step  # noqa: F401

pytestmark = pytest.mark.gpu

CFG = (64, 32, 9, 1, 5)
N1, N2, F1, F2, F3 = CFG
OFF = offsets(CFG)
SCRATCH_FORM = {(27, 37, 3)}  # shapes whose part images do not fit: the rest take them
SHAPES = [(19, 17, 3), (17, 19, 3), (30, 30, 3), (33, 33, 258), (19, 17, 770), (27, 37, 3)]
SPIKE_SHAPES = [(30, 30, 3), (19, 17, 3)]
CORNERS = ["top_left", "top_right", "bottom_left", "bottom_right"]
SEEDS = {(19, 17, 3): 21, (17, 19, 3): 22, (30, 30, 3): 23, (33, 33, 258): 24, (19, 17, 770): 25,
         (27, 37, 3): 26}

_BASE = {}
_REF = {}


def base_inputs(w, h, batch, all_positive=False):
    """X, T and parameters, computed once per shape (read-only): layer 2's
    biases centred per channel, layer 3's bias so that half of A3 is positive,
    or (all_positive) every A3 by at least 0.1."""
    key = (w, h, batch, all_positive)
    if key not in _BASE:
        rng = np.random.default_rng(SEEDS[(w, h, batch)])
        X, T = make_batch(rng, batch, w, h)
        params = make_params(rng, CFG, sd=0.05)
        centre_params(CFG, X, w, h, batch, params, all_positive=all_positive)
        for a in (X, T, params):
            a.setflags(write=False)
        _BASE[key] = (X, T, params)
    return _BASE[key]


def oracles(w, h, batch, X, T, params, tag):
    """Both oracles' gradients for these inputs; the fp32 one alone must pass
    the bounds the GPU result is held to."""
    g0 = np.zeros(params.size, np.float32)
    rg, _ = orc.train_fwd_bwd(CFG, X, T, w, h, batch, params, g0)
    xg, _ = orc.f64.train_fwd_bwd(CFG, X, T, w, h, batch, params, g0)
    check_gradients(CFG, rg, rg, xg, tag + "fp32 oracle alone: ")
    return rg, xg


def reference(w, h, batch):
    key = (w, h, batch)
    if key not in _REF:
        X, T, params = base_inputs(w, h, batch)
        rg, xg = oracles(w, h, batch, X, T, params, "%dx%d b%d " % key)
        w1, h1 = dims(CFG, w, h)[:2]
        a1 = orc.conv_fwd(X, params[OFF[0]:OFF[1]], params[OFF[1]:OFF[2]], w, h, 1, N1, F1, 1, batch)
        a2 = np.asarray(orc.conv_fwd(a1, params[OFF[2]:OFF[3]], params[OFF[3]:OFF[4]], w1, h1, N1, N2, F2, 1, batch))
        share = (a2.reshape(-1, N2) > 0).mean(axis=0)
        assert share.min() >= 0.2 and share.max() <= 0.8, "%s: a channel's mask is not mixed: %s" % (key, share)
        for a in (rg, xg):
            a.setflags(write=False)
        _REF[key] = (rg, xg)
    return _REF[key]


def step(S, w, h, batch, X, T, params, hold=False):
    """One step on guarded buffers; l12x6_fwd, l3r_d3 and the shape's form of
    d1x6 must have run."""
    form = "d1x6_d3_sc" if (w, h, batch) in SCRATCH_FORM else "d1x6_d3"
    return run_step(S, CFG, w, h, batch, X, T, params, guard=True, hold=hold,
                    expect=ran("fused", ["l12x6_fwd", "l3r_d3"], form))


@pytest.mark.parametrize("w,h,batch", SHAPES, ids=["%dx%d_b%d" % s for s in SHAPES])
def test_gradients(S, w, h, batch):
    """All six gradients against both oracles; two runs bit-identical."""
    rg, xg = reference(w, h, batch)
    X, T, params = base_inputs(w, h, batch)
    got = step(S, w, h, batch, X, T, params).grads
    check_gradients(CFG, got, rg, xg, "gw2 operand %dx%d b%d " % (w, h, batch))
    got2 = step(S, w, h, batch, X, T, params).grads
    assert same_bits(got, got2), "two runs differ"


def spiked_target(T, a3, w, h, batch, corner):
    """T with the step's A3 in the output window, less 1 at the corner pixel."""
    (w3, h3), pad = dims(CFG, w, h)[4:], 6
    t = np.array(T, np.float32).reshape(batch, h, w)
    t[:, pad:pad + h3, pad:pad + w3] = np.asarray(a3, np.float32).reshape(batch, h3, w3)
    y3 = 0 if corner.startswith("top") else h3 - 1
    x3 = 0 if corner.endswith("left") else w3 - 1
    t[:, pad + y3, pad + x3] -= 1.0
    return t.ravel()


_A3 = {}


def own_a3(S, w, h, batch):
    """The step's own A3 for the all-positive parameters, once per shape."""
    key = (w, h, batch)
    if key not in _A3:
        X, T, params = base_inputs(w, h, batch, all_positive=True)
        a3 = step(S, w, h, batch, X, T, params, hold=True).activations()[2]
        assert a3.min() > 0.0, "A3 not positive everywhere: %g" % a3.min()
        a3.setflags(write=False)
        _A3[key] = a3
    return _A3[key]


@pytest.mark.parametrize("corner", CORNERS)
@pytest.mark.parametrize("w,h,batch", SPIKE_SHAPES, ids=["%dx%d_b%d" % s for s in SPIKE_SHAPES])
def test_gb2_single_pixel(S, w, h, batch, corner):
    """delta3 = 1 at one corner pixel of every sample's output and 0 elsewhere:
    gB2 (and the other gradients) against both oracles."""
    X, T, params = base_inputs(w, h, batch, all_positive=True)
    T1 = spiked_target(T, own_a3(S, w, h, batch), w, h, batch, corner)
    tag = "gw2 operand %dx%d b%d %s " % (w, h, batch, corner)
    rg, xg = oracles(w, h, batch, X, T1, params, tag)
    assert np.abs(rg[OFF[3]:OFF[4]]).min() > 0.0, "oracle: a gB2 element without terms"
    got = step(S, w, h, batch, X, T1, params).grads
    print(tag + "gB2 max |got - fp64| %g of max |gB2| %g"
          % (np.abs(got[OFF[3]:OFF[4]] - xg[OFF[3]:OFF[4]]).max(), np.abs(xg[OFF[3]:OFF[4]]).max()))
    check_gradients(CFG, got, rg, xg, tag)
