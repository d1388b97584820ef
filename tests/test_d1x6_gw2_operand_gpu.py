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
import hip_util
from hip_util import FLIP_FLOOR, RTOL, assert_close, guarded, guards_intact, make_batch, make_params, same_bits

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CFG = (64, 32, 9, 1, 5)
N1, N2, F1, F2, F3 = CFG
OFF = np.cumsum([0, F1 * F1 * N1, N1, N1 * N2, N2, F3 * F3 * N2, 1])
NAMES = ["W1", "B1", "W2", "B2", "W3", "B3"]
KERNELS = ["l12x6_fwd", "l3r_d3"]
D1X6_FORMS = ("d1x6_d3", "d1x6_d3_sc")
SCRATCH_FORM = {(27, 37, 3)}  # shapes whose part images do not fit: the rest take them
SHAPES = [(19, 17, 3), (17, 19, 3), (30, 30, 3), (33, 33, 258), (19, 17, 770), (27, 37, 3)]
SPIKE_SHAPES = [(30, 30, 3), (19, 17, 3)]
CORNERS = ["top_left", "top_right", "bottom_left", "bottom_right"]
SEEDS = {(19, 17, 3): 21, (17, 19, 3): 22, (30, 30, 3): 23, (33, 33, 258): 24, (19, 17, 770): 25,
         (27, 37, 3): 26}


@pytest.fixture(scope="module")
def S():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import srcnn_amd
    return srcnn_amd


@pytest.fixture(autouse=True)
def _settings(S):
    try:
        yield
    finally:
        S.set_arith(0)
        S.set_path(0)
        hip_util._GUARDS.clear()


def H(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().copy()


_BASE = {}
_REF = {}


def mid(a):
    """Midway between the two middle values (at the median itself one value
    would be 0 up to rounding and its ReLU decision a coin toss)."""
    s = np.sort(np.asarray(a, np.float64), axis=0)
    k = s.shape[0] // 2
    return 0.5 * (s[k - 1] + s[k])


def base_inputs(w, h, batch, all_positive=False):
    """X, T and parameters, computed once per shape (read-only): layer 2's
    biases centred per channel, layer 3's bias so that half of A3 is positive,
    or (all_positive) every A3 by at least 0.1."""
    key = (w, h, batch, all_positive)
    if key not in _BASE:
        rng = np.random.default_rng(SEEDS[(w, h, batch)])
        X, T = make_batch(rng, batch, w, h)
        params = make_params(rng, CFG, sd=0.05)
        A1 = orc.conv_fwd(X, params[OFF[0]:OFF[1]], params[OFF[1]:OFF[2]], w, h, 1, N1, F1, 1, batch)
        Z = orc.conv_fwd(A1, params[OFF[2]:OFF[3]], np.zeros(N2, np.float32), w - 8, h - 8, N1, N2, F2, 0, batch)
        params[OFF[3]:OFF[4]] = (-mid(np.asarray(Z).reshape(-1, N2))).astype(np.float32)
        a3 = np.asarray(orc.forward(CFG, X, w, h, batch, params), np.float64).ravel()
        params[-1] -= np.float32(a3.min() - 0.1 if all_positive else mid(a3))
        for a in (X, T, params):
            a.setflags(write=False)
        _BASE[key] = (X, T, params)
    return _BASE[key]


def check_gradients(got, rg, xg, tag):
    for i, nm in enumerate(NAMES):
        sl = slice(OFF[i], OFF[i + 1])
        assert_close(got[sl], rg[sl], RTOL, tag + "grad " + nm, xg[sl], FLIP_FLOOR)


def oracles(w, h, batch, X, T, params, tag):
    """Both oracles' gradients for these inputs; the fp32 one alone must pass
    the bounds the GPU result is held to."""
    g0 = np.zeros(params.size, np.float32)
    rg, _ = orc.train_fwd_bwd(CFG, X, T, w, h, batch, params, g0)
    xg, _ = orc.f64.train_fwd_bwd(CFG, X, T, w, h, batch, params, g0)
    check_gradients(rg, rg, xg, tag + "fp32 oracle alone: ")
    return rg, xg


def reference(w, h, batch):
    key = (w, h, batch)
    if key not in _REF:
        X, T, params = base_inputs(w, h, batch)
        rg, xg = oracles(w, h, batch, X, T, params, "%dx%d b%d " % key)
        a1 = orc.conv_fwd(X, params[OFF[0]:OFF[1]], params[OFF[1]:OFF[2]], w, h, 1, N1, F1, 1, batch)
        a2 = np.asarray(orc.conv_fwd(a1, params[OFF[2]:OFF[3]], params[OFF[3]:OFF[4]], w - 8, h - 8, N1, N2, F2, 1, batch))
        share = (a2.reshape(-1, N2) > 0).mean(axis=0)
        assert share.min() >= 0.2 and share.max() <= 0.8, "%s: a channel's mask is not mixed: %s" % (key, share)
        for a in (rg, xg):
            a.setflags(write=False)
        _REF[key] = (rg, xg)
    return _REF[key]


def run_step(S, w, h, batch, X, T, params, keep=False):
    """One step on an exact-size NaN workspace: gradients (from zero) and what
    srcnn_train_activations needs.  keep: the guarded views stay registered and
    come back last, for the caller's guards_intact."""
    net = S.Net(*CFG)
    S.set_arith(0)
    nbytes = S.train_workspace_bytes(net, w, h, batch)
    ws = guarded(nbytes // 4, float("nan"))
    g, err = guarded(np.zeros(params.size, np.float32), 1e30), guarded(1, 1e30, inner=0.0)
    S.train_fwd_bwd(net, guarded(X, 1e30), guarded(T, 1e30), w, h, batch, guarded(params, 1e30), g, err, ws, nbytes)
    assert S.last_path() == "fused", S.last_path()
    ks = S.last_kernels()
    assert all(k in ks for k in KERNELS), ks
    form = D1X6_FORMS[(w, h, batch) in SCRATCH_FORM]
    assert [k for k in ks if k in D1X6_FORMS] == [form], ks
    got = H(g)
    if keep:
        return net, got, ws, nbytes, (g, err, ws)
    guards_intact(g, err, ws)
    return net, got, ws, nbytes


@pytest.mark.parametrize("w,h,batch", SHAPES, ids=["%dx%d_b%d" % s for s in SHAPES])
def test_gradients(S, w, h, batch):
    """All six gradients against both oracles; two runs bit-identical."""
    rg, xg = reference(w, h, batch)
    X, T, params = base_inputs(w, h, batch)
    _, got, _, _ = run_step(S, w, h, batch, X, T, params)
    check_gradients(got, rg, xg, "gw2 operand %dx%d b%d " % (w, h, batch))
    _, got2, _, _ = run_step(S, w, h, batch, X, T, params)
    assert same_bits(got, got2), "two runs differ"


def spiked_target(T, a3, w, h, batch, corner):
    """T with the step's A3 in the output window, less 1 at the corner pixel."""
    w3, h3, pad = w - 12, h - 12, 6
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
        net, _, ws, nbytes, views = run_step(S, w, h, batch, X, T, params, keep=True)
        sizes = (batch * (w - 8) * (h - 8) * N1, batch * (w - 8) * (h - 8) * N2, batch * (w - 12) * (h - 12))
        outs = [guarded(n, 1e30) for n in sizes]
        S.train_activations(net, w, h, batch, ws, nbytes, *outs)
        a3 = H(outs[2])
        guards_intact(*views, *outs)
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
    _, got, _, _ = run_step(S, w, h, batch, X, T1, params)
    print(tag + "gB2 max |got - fp64| %g of max |gB2| %g"
          % (np.abs(got[OFF[3]:OFF[4]] - xg[OFF[3]:OFF[4]]).max(), np.abs(xg[OFF[3]:OFF[4]]).max()))
    check_gradients(got, rg, xg, tag)
