"""l12x6's layer 1 on two-part fp16 split products (three
v_mfma_f32_32x32x16_f16 per k-step, split.hpp; W1 scaled once per launch by
2^ew, X once per sample by 2^ex, the fp32 MFMA that starts the accumulator
carrying 2^ew on its A side and 2^ex on its B side, the accumulator unscaled
ahead of the ReLU).

Default net, split arithmetic, through the C ABI on exact-size NaN-poisoned
guarded buffers; A1, A2 and A3 read back with train_activations.  Cases
(w, h, batch):
  - 33 x 33 x 5: one sample per block;
  - 17 x 19 x 1030: the grid is 512, so blocks 0-5 run three samples and the
    rest two; 99 output pixels, so the last chunk is ragged;
  - "jumps", 17 x 19 x 1030: samples 512-1023 have X x 2^12, sample 1024 is all
    zero and sample 1025 has X x 2^-30, so every block meets a jump up and
    blocks 0 and 1 then a zero or a tiny sample;
  - 21 x 23 x 3 and 35 x 35 x 3: X6Lds's padded stride and its 3 w fallback
    (the rule is restated below and asserted for both tiles);
  - the lazy kernel at 33 x 33 x 5 with a pending update that takes max |W1|
    from about 2^-2 to about 2^2: with the old maximum the scaled weights
    would pass fp16's range.
Per sample, A1's and A2's normwise error against the fp64 oracle's forward is
at most 1.5 x the fp32-arithmetic path's (set_arith(1)) on that sample +
2^-24; the zero sample's A1 is relu(B1) bit for bit and its A2 the same row at
every pixel.  All six gradient segments pass hip_util.assert_close as it
stands, the guards are intact and two runs give equal bits.  Containment: one
+inf pixel in sample 3 of 17 x 19 x 1030 leaves A1 and A2 of every other
sample as they were, bit for bit (samples 515 and 1027 share its block).
"""
import numpy as np
import pytest

import srcnn_oracle as orc
from hip_util import check_gradients, dims, make_batch, make_params, offsets, same_bits, segments
from step_util import S, _settings, no_x6, ran, run_step  # noqa: F401

pytestmark = pytest.mark.gpu

CFG = (64, 32, 9, 1, 5)
N1, N2, F1, F2, F3 = CFG
OFF = offsets(CFG)
LR = [1.0, 1e-4, 1e-5]  # the lazy case: layer 1's rate moves W1 by whole units
ZERO, TINY = 1024, 1025
CASES = [("one", 33, 33, 5, 41), ("many", 17, 19, 1030, 42), ("jumps", 17, 19, 1030, 42), ("padded", 21, 23, 3, 43),
         ("fallback", 35, 35, 3, 44)]


def x6lds_padded(w, h):
    """X6Lds (l12x6.hpp): whether the tile's pair image takes the padded row
    stride (it fits 80 KB on the three-part sizes) or the 3 w fallback."""
    base = (5 * 2 * 3 * 512 + 4 * 3 * 512) * 2 + (128 + 32) * 4
    a4 = (4 * ((w - 8) // 4)) % 32
    rs3 = 3 * w + (a4 - 3 * w) % 32
    xs = base + (rs3 * h + 1) * 4
    return ((xs + w * h * 4 + 15) & ~15) + 4 * (32 * 32 + 32) * 4 <= 80 * 1024


def test_stride_branches_of_the_cases():
    assert x6lds_padded(21, 23) and x6lds_padded(33, 33) and x6lds_padded(17, 19)
    assert not x6lds_padded(35, 35)


def step(S, arith, w, h, batch, X, T, params, lazy=None, finite=True):
    """-> (grads, A1, A2, A3, params the step ran on) of a step on guarded
    buffers.  lazy: (pending grads, momentum) of a pending update, applied by
    train_fwd_bwd_lazy."""
    expect = no_x6 if arith else ran("fused", ["l12x6_fwd" if lazy is None else "l12x6_fwd_lazy"])
    st = run_step(S, CFG, w, h, batch, X, T, params, arith=arith, guard=True, hold=True, expect=expect,
                  lazy=None if lazy is None else lazy + (LR,))
    acts = st.activations()
    if finite:
        assert all(np.isfinite(a).all() for a in acts)
    return st.grads, acts[0], acts[1], acts[2], st.params


_INPUTS = {}


def inputs(name, w, h, batch, seed):
    if name not in _INPUTS:
        rng = np.random.default_rng(seed)
        X, T = make_batch(rng, batch, w, h)
        params = make_params(rng, CFG, sd=0.05)
        if name == "jumps":
            x = X.reshape(batch, -1).copy()
            x[512:1024] *= np.float32(4096.0)
            x[ZERO] = 0.0
            x[TINY] *= np.float32(2.0 ** -30)
            X = x.ravel()
        for a in (X, T, params):
            a.setflags(write=False)
        _INPUTS[name] = (X, T, params)
    return _INPUTS[name]


def forward64(X, params, w, h, batch):
    ow, oh = dims(CFG, w, h)[:2]
    seg = segments(CFG, params)
    a1 = orc.f64.conv_fwd(X, seg[0], seg[1], w, h, 1, N1, F1, True, batch)
    a2 = orc.f64.conv_fwd(a1, seg[2], seg[3], ow, oh, N1, N2, F2, True, batch)
    return a1.reshape(batch, -1), a2.reshape(batch, -1)


def per_sample_err(a, ref):
    d = np.linalg.norm(a.reshape(ref.shape).astype(np.float64) - ref, axis=1)
    n = np.linalg.norm(ref, axis=1)
    return np.where(n > 0, d / np.where(n > 0, n, 1.0), d)


def check_activations(name, got, f32, X, p_got, p_f32, w, h, batch):
    r1, r2 = forward64(X, p_got, w, h, batch)
    q1, q2 = (r1, r2) if p_f32 is p_got else forward64(X, p_f32, w, h, batch)
    for nm, a, b, ra, rb in (("A1", got[1], f32[1], r1, q1), ("A2", got[2], f32[2], r2, q2)):
        es, ef = per_sample_err(a, ra), per_sample_err(b, rb)
        k = int(np.argmax(es - (1.5 * ef + 2.0 ** -24)))
        print("%s %s: f16 x3 worst sample %d %.3e (fp32 arithmetic there %.3e); means %.3e / %.3e"
              % (name, nm, k, es[k], ef[k], es.mean(), ef.mean()))
        assert np.all(es <= 1.5 * ef + 2.0 ** -24), (name, nm, k, es[k], ef[k])


def check_grads(name, got, X, T, params, w, h, batch):
    g0 = np.zeros(params.size, np.float32)
    rg, _ = orc.train_fwd_bwd(CFG, X, T, w, h, batch, params, g0)
    xg, _ = orc.f64.train_fwd_bwd(CFG, X, T, w, h, batch, params, g0)
    check_gradients(CFG, got, rg, xg, "l12x6 f16 %s " % name)


@pytest.mark.parametrize("name,w,h,batch,seed", CASES, ids=[c[0] for c in CASES])
def test_l12x6_two_part_f16(S, name, w, h, batch, seed):
    X, T, params = inputs(name, w, h, batch, seed)
    got = step(S, 0, w, h, batch, X, T, params)
    f32 = step(S, 1, w, h, batch, X, T, params)
    check_activations(name, got, f32, X, params, params, w, h, batch)
    if name == "jumps":
        ow, oh = dims(CFG, w, h)[:2]
        a1 = got[1].reshape(batch, ow * oh, N1)[ZERO]
        b1 = np.maximum(params[OFF[1]:OFF[2]], np.float32(0))
        assert same_bits(a1, np.broadcast_to(b1, a1.shape)), "the zero sample's A1 is not relu(B1)"
        a2 = got[2].reshape(batch, ow * oh, N2)[ZERO]
        assert same_bits(a2, np.broadcast_to(a2[0], a2.shape)), "the zero sample's A2 differs between pixels"
    check_grads(name, got[0], X, T, params, w, h, batch)
    again = step(S, 0, w, h, batch, X, T, params)
    assert all(same_bits(a, b) for a, b in zip(got[:4], again[:4])), "two runs differ"


def test_l12x6_lazy_scale_of_the_updated_weights(S):
    w, h, batch = 33, 33, 5
    X, T, params = inputs("one", w, h, batch, 41)
    rng = np.random.default_rng(45)
    pend = np.zeros(params.size, np.float32)
    # lr = 1 on layer 1: the update moves every W1 weight by about N(0, 1)
    pend[OFF[0]:OFF[1]] = (batch * rng.standard_normal(OFF[1])).astype(np.float32)
    mom = np.zeros(params.size, np.float32)
    got = step(S, 0, w, h, batch, X, T, params, lazy=(pend, mom))
    f32 = step(S, 1, w, h, batch, X, T, params, lazy=(pend, mom))
    w_old, w_new = np.abs(params[OFF[0]:OFF[1]]).max(), np.abs(got[4][OFF[0]:OFF[1]]).max()
    print("lazy: max |W1| %.3g -> %.3g" % (w_old, w_new))
    assert w_new >= 8 * w_old  # under the old scale (max to [2^14, 2^15)) these pass fp16's 65504
    check_activations("lazy", got, f32, X, got[4], f32[4], w, h, batch)
    check_grads("lazy", got[0], X, T, got[4], w, h, batch)
    again = step(S, 0, w, h, batch, X, T, params, lazy=(pend, mom))
    assert all(same_bits(a, b) for a, b in zip(got, again)), "two runs differ"


def test_l12x6_non_finite_pixel_stays_in_its_sample(S):
    name, w, h, batch, seed = CASES[1]
    X, T, params = inputs(name, w, h, batch, seed)
    clean = step(S, 0, w, h, batch, X, T, params)
    x = X.reshape(batch, -1).copy()
    x[3, (h // 2) * w + w // 2] = np.inf
    dirty = step(S, 0, w, h, batch, x.ravel(), T, params, finite=False)
    keep = np.arange(batch) != 3
    for nm, a, b in (("A1", clean[1], dirty[1]), ("A2", clean[2], dirty[2])):
        a, b = a.reshape(batch, -1), b.reshape(batch, -1)
        assert same_bits(a[keep], b[keep]), nm + " of another sample changed"
