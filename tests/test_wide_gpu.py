"""GPU parity of the wide-net training step (BASELINE.json configs[3]:
n1=128, n2=64, f1=9, f2=5, f3=5; train_wide.hip) against the CPU oracle.

Every intermediate the step leaves in the workspace (A1, A2, D2, in the
reference HWC layout, src/kernel/layer_uber_kernel.cl:51-56; delta1 stays
inside the delta1+gW1 kernel and is checked through gW1 / gB1) and the
accumulated gradients are compared with oracle/srcnn_oracle.c at
north_star's 1e-4 normwise tolerance (hip_util.RTOL), on square, ragged
and non-square tiles; the profile stats prove the MFMA kernels ran.
"""
import numpy as np
import pytest

import srcnn_oracle as orc
from hip_util import (FLIP_FLOOR, H, NAMES, RTOL, act_sizes, assert_close, check_gradients, dims, make_batch,
                      make_params, offsets, segments)
from step_util import S, _settings, check_flips, decisions, run_step  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

WIDE = (128, 64, 9, 5, 5)


def align(n):
    return (n + 255) & ~255


def wide_step(S, w, h, batch, seed, sd=0.05, g0=None, want_acts=False):
    """The step on seeded inputs, a zero-filled workspace (read back whole for
    split_ws) and the profile on."""
    net = S.Net(*WIDE)
    rng = np.random.default_rng(seed)
    X, T = make_batch(rng, batch, w, h)
    params = make_params(rng, WIDE, sd=sd)
    if g0 is None:
        g0 = np.zeros(params.size, np.float32)
    nbytes = S.train_workspace_bytes(net, w, h, batch)
    ws = torch.zeros(nbytes // 4 + 64, dtype=torch.float32, device="cuda")
    S.profile_reset()
    S.profile_enable(True)
    st = run_step(S, WIDE, w, h, batch, X, T, params, g0, ws=(ws, nbytes))
    S.profile_enable(False)
    out = (X, T, params, g0, st.grads, st.sq_err, H(ws), S.profile_stats())
    if want_acts:
        # the activations the step left (srcnn_train_activations): its own
        # ReLU decisions
        out += (tuple(st.activations()),)
    return out


def split_ws(ws, w, h, batch):
    n1 = WIDE[0]
    w1, h1 = dims(WIDE, w, h)[:2]
    s1, s2 = act_sizes(WIDE, w, h, batch)[:2]
    # the A1 region holds whole 32-pixel chunks per sample (abi.cpp NetDims::s1p)
    s1p = (w1 * h1 + 31) // 32 * 32 * n1 * batch
    o = 0
    out = {}
    for name, n, room in (("A1", s1, s1p), ("D1", s1, s1), ("A2", s2, s2), ("D2", s2, s2)):
        out[name] = ws[o // 4:o // 4 + n]
        o += align(4 * room)
    return out


# batch 8: the smallest batch whose d1g16 (16 blocks) and wgrad2 (32 blocks)
# grids take the XCD-aware block mapping; the other small batches run the
# plain mapping, batch 64 / 300 / 4096 (below) the mapped one at full grids
@pytest.mark.parametrize("w,h,batch", [(33, 33, 1), (33, 33, 6), (29, 29, 3), (33, 27, 2),
                                       (25, 31, 3), (33, 33, 8)])
def test_wide_step_stages_vs_oracle(S, w, h, batch):
    X, T, params, g0, got, err, ws, stats, hacts = wide_step(S, w, h, batch, seed=7 + w + h + batch,
                                                            want_acts=True)
    assert "wide_l2_fwd" in stats and "wide_grad2" in stats, stats.keys()
    ref_g, acts = orc.train_fwd_bwd(WIDE, X, T, w, h, batch, params, g0, want_acts=True)
    x_g, xacts = orc.f64.train_fwd_bwd(WIDE, X, T, w, h, batch, params, g0, want_acts=True)
    n1, n2, f1, f2, f3 = WIDE
    w1, h1, w2, h2, w3, h3 = dims(WIDE, w, h)
    s1, s2, s3 = act_sizes(WIDE, w, h, batch)
    rA1 = acts[:s1]
    rA2 = acts[s1:s1 + s2]
    rD2 = acts[s1 + s2 + 2 * s3:s1 + 2 * s2 + 2 * s3]
    st = split_ws(ws, w, h, batch)
    assert_close(st["A1"], rA1, RTOL, "A1", xacts[:s1])
    assert_close(st["A2"], rA2, RTOL, "A2", xacts[s1:s1 + s2])
    assert_close(st["D2"], rD2, RTOL, "D2", xacts[s1 + s2 + 2 * s3:s1 + 2 * s2 + 2 * s3])
    # gradients against both oracles under the step's own ReLU decisions:
    # a pre-activation within fp32 rounding of zero can go either way in any
    # summation order (33x33 batch 6: one of 480,000 layer-1 decisions,
    # |exact| = 1.7e-8 of its terms' magnitude, under the split-bf16 L1) and
    # its whole delta then enters the gradients, far past FLIP_FLOOR; every
    # decision that differs from the exact sign must lie in the rounding band
    # (step_util.check_flips)
    m1, m2, m3 = (a > 0 for a in hacts)
    ref_m, _ = orc.train_fwd_bwd_masked(WIDE, X, T, w, h, batch, params, g0, m1, m2, m3)
    x_m, xacts_m = orc.f64.train_fwd_bwd_masked(WIDE, X, T, w, h, batch, params, np.asarray(g0, np.float64),
                                                m1, m2, m3, want_acts=True)
    pre1, mag1, pre2, mag2 = decisions(WIDE, X, w, h, batch, params, xacts_m[:s1])
    W3_, B3_ = segments(WIDE, np.asarray(params, np.float64))[4:]
    pre3 = xacts_m[s1 + s2:s1 + s2 + s3]
    mag3 = orc.f64.conv_fwd(np.abs(xacts_m[s1:s1 + s2]), np.abs(W3_), np.abs(B3_), w2, h2, n2, 1, f3, 0, batch)
    for k, (m, p, mg) in enumerate(((m1, pre1, mag1), (m2, pre2, mag2), (m3, pre3, mag3))):
        check_flips("wide A%d" % (k + 1), m, p, mg)
    check_gradients(WIDE, got, ref_m, x_m, "")
    A3 = orc.forward(WIDE, X, w, h, batch, params)
    ref_err = orc.sq_err(T, A3, w, h, w3, h3, batch)
    assert err == pytest.approx(ref_err, rel=1e-4)


def test_wide_step_accumulates_and_is_deterministic(S):
    w = h = 33
    batch = 300
    rng = np.random.default_rng(3)
    g0 = (1e-3 * rng.standard_normal(orc.param_count(*WIDE))).astype(np.float32)
    X, T, params, _, got, _, _, _ = wide_step(S, w, h, batch, seed=11, g0=g0)
    ref_g, _ = orc.train_fwd_bwd(WIDE, X, T, w, h, batch, params, g0)
    x_g, _ = orc.f64.train_fwd_bwd(WIDE, X, T, w, h, batch, params, g0)
    assert_close(got, ref_g, RTOL, "wide gradients (accumulated onto g0)", x_g, FLIP_FLOOR)
    _, _, _, _, got2, _, _, _ = wide_step(S, w, h, batch, seed=11, g0=g0)
    np.testing.assert_array_equal(got2, got)


def test_wide_fast_matches_generic_path(S):
    w = h = 33
    batch = 64
    fast = wide_step(S, w, h, batch, seed=5)
    S.set_path(1)
    gen = wide_step(S, w, h, batch, seed=5)
    assert "wide_l2_fwd" not in gen[7]
    assert_close(fast[4], gen[4], RTOL, "fast vs generic gradients")
    assert fast[5] == pytest.approx(gen[5], rel=1e-4)


def test_wide_full_batch_4096_vs_oracle(S):
    """BASELINE.json configs[3] at its own size (batch 4096 of 33x33 tiles).
    The oracle needs ~2.3 TFLOP for 4096 wide tiles (about a minute), so the
    batch is 64 distinct tiles, each repeated 64 times: the gradient of the
    4096-tile step is then 64 x the oracle's 64-tile gradient (the sums
    differ only in order), and every tile's A2 / D2 equals its source tile's.
    This runs the full-size grids, slab counts and tails of every wide kernel."""
    w = h = 33
    distinct, rep = 64, 64
    batch = distinct * rep
    net = S.Net(*WIDE)
    rng = np.random.default_rng(4096)
    X, T = make_batch(rng, distinct, w, h)
    params = make_params(rng, WIDE, sd=0.05)
    P = params.size
    Xb, Tb = np.tile(X, rep), np.tile(T, rep)
    nbytes = S.train_workspace_bytes(net, w, h, batch)
    ws = torch.zeros(nbytes // 4 + 64, dtype=torch.float32, device="cuda")
    step = run_step(S, WIDE, w, h, batch, Xb, Tb, params, sq_err=False, ws=(ws, nbytes))
    assert step.path == "wide"
    got = step.grads
    ref_g, acts = orc.train_fwd_bwd(WIDE, X, T, w, h, distinct, params, np.zeros(P, np.float32),
                                    want_acts=True)
    x_g, xacts = orc.f64.train_fwd_bwd(WIDE, X, T, w, h, distinct, params, np.zeros(P), want_acts=True)
    off = offsets(WIDE)
    # 2.6M-term fp32 sums (64x the oracle's 64-tile sums): 2e-4 normwise, as
    # for the other >1M-term sums (test_backpropagation_big_data), and the
    # same as the elementwise floor (7M ReLU decisions of A1 / A2 feed these
    # gradients, so a few fall within fp32 rounding of zero, hip_util.FLIP_FLOOR)
    for i, nm in enumerate(NAMES):
        sl = slice(off[i], off[i + 1])
        assert_close(got[sl], rep * ref_g[sl], 2e-4, "batch-4096 grad " + nm, rep * x_g[sl], 2e-4)
    # sampled activation slices: tiles 0, 1000, 4095 (sources 0, 1000 % 64, 63)
    s1, s2, s3 = act_sizes(WIDE, w, h, 1)
    a2 = slice(s1 * distinct, (s1 + s2) * distinct)
    d2 = slice((s1 + s2 + 2 * s3) * distinct, (s1 + 2 * s2 + 2 * s3) * distinct)
    st = split_ws(H(ws), w, h, batch)
    for t in (0, 1000, batch - 1):
        src = slice((t % distinct) * s2, (t % distinct + 1) * s2)
        mine = slice(t * s2, (t + 1) * s2)
        assert_close(st["A2"][mine], acts[a2][src], RTOL, "A2 tile %d" % t, xacts[a2][src])
        assert_close(st["D2"][mine], acts[d2][src], RTOL, "D2 tile %d" % t, xacts[d2][src])
