"""Layer 2's ReLU' as a bit mask in the delta3-mode step (l3r_d3 writes one
dword per A2 pixel after delta3 in the D2 region, bit n = A2[pixel][n] > 0;
d1x6_d3 reads that dword instead of the A2 row).

Default net, split arithmetic, exact-size NaN-poisoned workspace, and every
case asserts that l3r_d3 and d1x6_d3 ran.
  - Dead channels: with B2[n] = -1e3 the channel's A2 is exactly 0, so gW2[:, n]
    and gB2[n] must be exactly 0, and nonzero for every live n.  An irregular
    set and each single channel pin bit <-> channel through both lane halves
    and the crow register order.
  - Several samples per block: at batch 600 d1x6's 256 blocks take 2-3 samples
    each, so the triple-buffered delta3 image and the mask loads cross sample
    boundaries; 30 x 30 has two dummy slots per column run (mask 0 there).
Before a pass is trusted, the fp32 oracle's A2 must be genuinely mixed: the
share of positive elements in [0.2, 0.8] (seeds chosen on the CPU).  The
dead-channel cases also centre the live channels' B2 (see reference()), and
require of the oracle alone that every live channel's mask is mixed and its
gradient nonzero.
"""
import numpy as np
import pytest

import srcnn_oracle as orc
from hip_util import RTOL, assert_close, check_gradients, dims, make_batch, make_params, offsets, same_bits, segments
from step_util import S, _settings, centre_params, ran, run_step  # noqa: F401

pytestmark = pytest.mark.gpu

CFG = (64, 32, 9, 1, 5)
N1, N2, F1, F2, F3 = CFG
OFF = offsets(CFG)
KERNELS = ["l12x6_fwd", "l3r_d3", "d1x6_d3"]
DEAD_SET = (1, 4, 7, 10, 13, 18, 21, 27, 30)
# (w, h, batch) -> the seed of its inputs: chosen on the CPU so that the fp32
# oracle's A2 is mixed for every case below
SEEDS = {(17, 19, 3): 11, (33, 33, 600): 12, (30, 30, 3): 13}


_BASE = {}
_REF = {}


def base_inputs(w, h, batch):
    """X, T and parameters whose layer-3 bias makes half of A3 positive
    (delta3 is masked by A3 > 0), computed once per shape (read-only)."""
    key = (w, h, batch)
    if key not in _BASE:
        rng = np.random.default_rng(SEEDS[key])
        X, T = make_batch(rng, batch, w, h)
        params = make_params(rng, CFG, sd=0.05)
        params[-1] -= np.median(orc.forward(CFG, X, w, h, batch, params))
        for a in (X, T, params):
            a.setflags(write=False)
        _BASE[key] = (X, T, params)
    return _BASE[key]


def reference(w, h, batch, dead=(), centre=False):
    """Both oracles' gradients, activations and squared error for the shape's
    inputs with the channels `dead` of layer 2 switched off, computed once.
    centre: every other channel's B2 is first centred and layer 3's bias
    after it (step_util.centre_params); otherwise "a gradient on every live
    channel" would not hold and no channel's mask would be mixed."""
    key = (w, h, batch, tuple(dead), centre)
    if key not in _REF:
        X, T, params = base_inputs(w, h, batch)
        params = params.copy()
        assert centre or not dead
        if centre:
            centre_params(CFG, X, w, h, batch, params, dead)
        g0 = np.zeros(params.size, np.float32)
        rg, _ = orc.train_fwd_bwd(CFG, X, T, w, h, batch, params, g0)
        xg, _ = orc.f64.train_fwd_bwd(CFG, X, T, w, h, batch, params, g0)
        W1, B1, W2, B2, W3, B3 = segments(CFG, params)
        w1, h1, w2, h2, w3, h3 = dims(CFG, w, h)
        acts = []
        for m in (orc, orc.f64):
            A1 = m.conv_fwd(X, W1, B1, w, h, 1, N1, F1, 1, batch)
            A2 = m.conv_fwd(A1, W2, B2, w1, h1, N1, N2, F2, 1, batch)
            A3 = m.conv_fwd(A2, W3, B3, w2, h2, N2, 1, F3, 0, batch)
            acts.append({"A1": A1, "A2": A2, "A3": A3})
        ref_err = orc.sq_err(T, acts[0]["A3"], w, h, w3, h3, batch)
        # the masks are exercised: layer 2's (the bit mask) and layer 3's
        a2 = np.asarray(acts[0]["A2"]).reshape(-1, N2)
        pos2 = float((a2 > 0).mean())
        assert 0.2 <= pos2 <= 0.8, "%s: %.3f of the oracle's A2 positive: the mask is not mixed" % (key, pos2)
        for n in dead:
            assert not a2[:, n].any(), "channel %d is not dead in the oracle" % n
        pos3 = float((np.asarray(acts[0]["A3"]) > 0).mean())
        assert 0.2 < pos3 < 0.8, "%s: %.3f of A3 positive: delta3 mask not mixed" % (key, pos3)
        for a in (params, rg, xg):
            a.setflags(write=False)
        _REF[key] = (params, rg, xg, acts, ref_err)
    return _REF[key]


def step(S, w, h, batch, params, hold=False):
    """One step of the shape's inputs on guarded buffers; KERNELS must have run."""
    X, T, _ = base_inputs(w, h, batch)
    return run_step(S, CFG, w, h, batch, X, T, params, guard=True, hold=hold, expect=ran("fused", KERNELS))


@pytest.mark.parametrize("dead", [DEAD_SET] + [(n,) for n in range(N2)],
                         ids=["set"] + ["ch%d" % n for n in range(N2)])
def test_dead_channels(S, dead):
    """17 x 19, the smallest delta3-mode tile (4 chunks, column runs, dummy
    slots), batch 3: gW2[:, n] and gB2[n] are exactly 0 for the dead channels
    and nonzero for every live one; all gradients against both oracles."""
    w, h, batch = 17, 19, 3
    params, rg, xg, acts, ref_err = reference(w, h, batch, dead, centre=True)
    # the oracle alone: every live channel has a mixed mask and a gradient
    a2 = np.asarray(acts[0]["A2"]).reshape(-1, N2)
    for n in range(N2):
        if n not in dead:
            share = float((a2[:, n] > 0).mean())
            assert 0.2 <= share <= 0.8, "oracle: %.3f of live channel %d positive" % (share, n)
            assert rg[OFF[2]:OFF[3]].reshape(N1, N2)[:, n].any() and rg[OFF[3] + n] != 0.0
    st = step(S, w, h, batch, params)
    got, err = st.grads, st.sq_err
    gW2 = got[OFF[2]:OFF[3]].reshape(N1, N2)
    gB2 = got[OFF[3]:OFF[4]]
    print("dead %s: max |gW2[:, dead]| %g, max |gB2[dead]| %g, min live max|gW2[:, n]| %g, min live |gB2| %g"
          % (dead, np.abs(gW2[:, list(dead)]).max(), np.abs(gB2[list(dead)]).max(),
             min(np.abs(gW2[:, n]).max() for n in range(N2) if n not in dead),
             min(abs(gB2[n]) for n in range(N2) if n not in dead)))
    for n in range(N2):
        if n in dead:
            assert not gW2[:, n].any() and gB2[n] == 0.0, "dead channel %d has a gradient" % n
        else:
            assert gW2[:, n].any() and gB2[n] != 0.0, "live channel %d has no gradient" % n
    check_gradients(CFG, got, rg, xg, "d3 mask %dx%d dead %s " % (w, h, "set" if len(dead) > 1 else dead[0]))
    assert err == pytest.approx(ref_err, rel=1e-4)


@pytest.mark.parametrize("w,h,batch", [(33, 33, 600), (30, 30, 3)], ids=["33x33_b600", "30x30_b3"])
def test_samples_per_block(S, w, h, batch):
    """Gradients, squared error and A1 / A2 / A3 against both oracles; two runs
    bit-identical."""
    params, rg, xg, acts, ref_err = reference(w, h, batch)
    st = step(S, w, h, batch, params, hold=True)
    got, err = st.grads, st.sq_err
    tag = "d3 mask %dx%d b%d " % (w, h, batch)
    check_gradients(CFG, got, rg, xg, tag)
    assert err == pytest.approx(ref_err, rel=1e-4)
    a = dict(zip(("A1", "A2", "A3"), st.activations()))
    for nm in ("A1", "A2", "A3"):
        assert_close(a[nm], acts[0][nm], RTOL, tag + nm, acts[1][nm])
    again = step(S, w, h, batch, params)
    assert same_bits(got, again.grads) and err == again.sq_err, "two runs differ"
