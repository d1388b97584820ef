"""GPU parity: the HIP path (called through the C ABI) against the CPU oracle
and the reference's golden vectors.

Tolerance: fp32, normwise 1e-4 (hip_util.RTOL) unless a fixture's own
printed precision is coarser (then that precision, as in
test_oracle_golden.py).  Integer / byte outputs (swap_luma) are exact.
Every parametrised op-level case runs on both kernel paths: "auto" (the
ops_fast.hip gfx950 kernels where the shape matches, asserted through
srcnn_last_path) and "generic".
"""
import json
import os

import numpy as np
import pytest

import srcnn_oracle as orc
from conftest import GOLDEN
from hip_util import (D, H, RTOL, act_sizes, assert_close, check_gradients, dims, make_batch, make_params, ran_x6,
                      segments)
from step_util import S, _settings, run_step  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(params=[0, 1], ids=["auto", "generic"])
def path(request, S):
    S.set_path(request.param)
    yield request.param
    S.set_path(0)


def load(name):
    with open(os.path.join(GOLDEN, name)) as fh:
        return json.load(fh)


def zeros(n, dtype=torch.float32):
    return torch.zeros(int(n), dtype=dtype, device="cuda")


# ----------------------------------------------------------------------------
# the reference's own specs, through the HIP path
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(load("layer_test_cases.json").keys()))
def test_layer_spec(S, path, case):
    d = load("layer_test_cases.json")[case]
    f, k, n = d["f_spatial_size"], d["n_prev_filter_cnt"], d["current_filter_count"]
    ow, oh = d["input_w"] - f + 1, d["input_h"] - f + 1
    out = zeros(ow * oh * n)
    S.conv_fwd(D(d["input"]), out, D(d["weights"]), D(d["bias"]), d["input_w"], d["input_h"], k, n,
               f, 1, 1)
    np.testing.assert_allclose(H(out), d["output"], rtol=0, atol=5e-4)


def test_layer_deltas_spec(S, path):
    d = load("layer_deltas.json")
    y = np.maximum(np.array(d["input_x"], np.float32), 0)
    out = zeros(50)
    S.conv_delta(D(d["deltas"]), D(y), out, D(d["weights"]), d["f_next"], d["n_prev_layer"],
                 d["n_next"], d["curr_w"], d["curr_h"], 1)
    np.testing.assert_allclose(H(out), d["expected"], rtol=0, atol=2e-6)


def test_backpropagation_spec(S, path):
    d = load("backprop.json")
    gW = D(np.full(54, d["grad_w_init"], np.float32))
    gB = zeros(3)
    ow = d["in_w"] - d["f"] + 1
    nbytes = S.conv_grad_workspace_bytes(2, 3, 3, ow, ow, 1)
    ws = zeros(nbytes // 4 + 1)
    S.conv_grad_acc(D(d["input"]), D(d["deltas"]), gW, gB, 2, 3, 3, ow, ow, 1, ws, nbytes)
    np.testing.assert_allclose(H(gW), d["expected_grad_w"], rtol=0, atol=6e-5)
    np.testing.assert_allclose(H(gB), d["expected_grad_b"], rtol=0, atol=6e-4)


def test_backpropagation_big_data(S, path):
    """BackpropagationTest.cpp:160-170 (1024x1024, 32->16, f=3): crash-only in
    the reference; here checked against the oracle on random data."""
    rng = np.random.default_rng(11)
    n_prev, n_cur, f, iw = 32, 16, 3, 1024
    ow = iw - f + 1
    inp = rng.standard_normal(iw * iw * n_prev).astype(np.float32)
    dl = rng.standard_normal(ow * ow * n_cur).astype(np.float32)
    nbytes = S.conv_grad_workspace_bytes(n_prev, n_cur, f, ow, ow, 1)
    ws = zeros(nbytes // 4 + 1)
    gW, gB = zeros(f * f * n_prev * n_cur), zeros(n_cur)
    S.conv_grad_acc(D(inp), D(dl), gW, gB, n_prev, n_cur, f, ow, ow, 1, ws, nbytes)
    rW, rB = orc.conv_grad_acc(inp, dl, np.zeros(f * f * n_prev * n_cur), np.zeros(n_cur), n_prev,
                               n_cur, f, ow, ow, 1)
    xW, xB = orc.f64.conv_grad_acc(inp, dl, np.zeros(f * f * n_prev * n_cur), np.zeros(n_cur), n_prev,
                                   n_cur, f, ow, ow, 1)
    assert_close(H(gW), rW, 2e-4, "gW big data", xW)   # 1M-term fp32 sums
    assert_close(H(gB), rB, 2e-4, "gB big data", xB)


def test_update_parameters_spec(S):
    rng = np.random.default_rng(1234)
    nW, nB, batch = 5 * 5 * 2 * 400, 400, 2
    vals = {}
    for key, size in (("w", nW), ("b", nB)):
        cur = (rng.integers(0, 2560, size) / 10.0).astype(np.float32)
        grad = (rng.integers(0, 2560, size) / 100.0).astype(np.float32)
        prev = (rng.integers(0, 2560, size) / 10.0).astype(np.float32)
        vals[key] = (cur, grad, prev)
    W, B = D(vals["w"][0]), D(vals["b"][0])
    dW, dB = D(vals["w"][2]), D(vals["b"][2])
    S.sgd_update(W, B, D(vals["w"][1]), D(vals["b"][1]), dW, dB, 0.8, 0.0, 0.001, batch, nW, nB)
    for key, got_v, got_d in (("w", W, dW), ("b", B, dB)):
        cur, grad, prev = vals[key]
        deltas = np.float32(0.8) * prev + np.float32(0.001) * grad
        np.testing.assert_allclose(H(got_v), cur - deltas / np.float32(batch), rtol=1e-6, atol=1e-4)
        np.testing.assert_allclose(H(got_d), deltas, rtol=1e-6, atol=1e-4)


def test_update_parameters_weight_decay(S):
    rng = np.random.default_rng(5)
    nW, nB = 777, 13
    W0, B0 = rng.standard_normal(nW).astype(np.float32), rng.standard_normal(nB).astype(np.float32)
    gW0, gB0 = rng.standard_normal(nW).astype(np.float32), rng.standard_normal(nB).astype(np.float32)
    dW0, dB0 = rng.standard_normal(nW).astype(np.float32), rng.standard_normal(nB).astype(np.float32)
    rW, rB, rdW, rdB = orc.sgd_update(W0, B0, gW0, gB0, dW0, dB0, 0.9, 1e-3, 1e-4, 37)
    W, B, dW, dB = D(W0), D(B0), D(dW0), D(dB0)
    S.sgd_update(W, B, D(gW0), D(gB0), dW, dB, 0.9, 1e-3, 1e-4, 37, nW, nB)
    for got, ref in ((W, rW), (B, rB), (dW, rdW), (dB, rdB)):
        np.testing.assert_allclose(H(got), ref, rtol=2e-7, atol=1e-7)


def test_last_layer_delta_spec(S):
    rng = np.random.default_rng(7)
    aw = ah = 6
    pad = 4
    gw, gh = aw + 2 * pad, ah + 2 * pad
    gt = np.full((gh, gw), 99999.0, np.float32)
    t = (rng.integers(0, 256, (ah, aw)) / 100.0).astype(np.float32)
    x = (rng.integers(0, 2560, (ah, aw)) / 1000.0).astype(np.float32) - np.float32(1.28)
    y = np.maximum(x, 0)
    gt[pad:pad + ah, pad:pad + aw] = t
    exp = (y - t) * (x > 0)
    out = zeros(aw * ah)
    S.last_delta(D(gt), D(y), out, gw, gh, aw, ah, 1)
    np.testing.assert_array_equal(H(out), exp.ravel())


def test_squared_error_spec(S):
    rng = np.random.default_rng(3)
    aw, ah, pad = 1000, 2000, 4
    gw, gh = aw + 2 * pad, ah + 2 * pad
    gt = np.full((gh, gw), 99999.0, np.float32)
    gt[pad:pad + ah, pad:pad + aw] = rng.integers(0, 256, (ah, aw))
    algo = (rng.integers(0, 2560, (ah, aw)) / 10.0).astype(np.float32)
    d = gt[pad:pad + ah, pad:pad + aw].astype(np.float64) - algo
    expected = float(np.sum(d * d))
    nb = S.reduce_workspace_bytes(aw * ah)
    ws, res = zeros(nb // 4 + 1), zeros(1)
    S.sq_err(D(gt), D(algo), res, gw, gh, aw, ah, 1, ws, nb)
    assert abs(float(H(res)[0]) - expected) <= 1e-5 * expected


@pytest.mark.parametrize("squared", [False, True])
def test_sum_spec(S, squared):
    data = np.arange(900, dtype=np.float32)
    expected = sum(i * i if squared else i for i in range(900))
    nb = S.reduce_workspace_bytes(900)
    ws, res = zeros(nb // 4 + 1), zeros(1)
    S.buf_sum(D(data), 900, squared, res, ws, nb)
    assert abs(float(H(res)[0]) - expected) <= 20  # SumTest.cpp:47


def test_subtract_from_all_and_mean(S):
    data = np.arange(900, dtype=np.float32)
    t = D(data)
    S.sub_scalar(t, 450.0, 900)
    np.testing.assert_array_equal(H(t), data - 450.0)
    t = D(data)
    nb = S.reduce_workspace_bytes(900)
    ws, mean = zeros(nb // 4 + 1), zeros(1)
    S.sub_mean(t, 900, mean, ws, nb)
    assert float(H(mean)[0]) == pytest.approx(449.5, abs=1e-3)
    np.testing.assert_allclose(H(t), data - np.float32(449.5), atol=1e-3)


@pytest.mark.parametrize("normalize", [True, False])
def test_extract_luma_spec(S, normalize):
    d = load("extract_luma.json")
    rgba = np.array(d["rgba"], np.uint8)
    out = zeros(d["w"] * d["h"])
    S.extract_luma(D(rgba, np.uint8), out, d["w"], d["h"], normalize)
    ref = orc.extract_luma(rgba, d["w"], d["h"], normalize)
    np.testing.assert_allclose(H(out), ref, rtol=1e-6, atol=1e-6)
    exp = np.array(d["expected_normalized"], np.float32) * (1 if normalize else 255)
    np.testing.assert_allclose(H(out), exp, rtol=0, atol=5e-3 * (1 if normalize else 255))


def test_swap_luma_spec(S):
    d = load("swap_luma.json")
    w, h, pad = d["w"], d["h"], d["padding"]
    lw, lh = w - 2 * pad, h - 2 * pad
    n = lw * lw
    new_luma = (np.arange(n, dtype=np.float32) * np.float32(1.0)) / np.float32(n)
    rgba = np.array(d["rgba"], np.uint8)
    out = zeros(w * h * 3, torch.uint8)
    S.swap_luma(D(rgba, np.uint8), D(new_luma), out, w, h, lw, lh)
    np.testing.assert_array_equal(H(out), orc.swap_luma(rgba, new_luma, w, h, lw, lh))


# ----------------------------------------------------------------------------
# random shapes vs the oracle (including the SRCNN default / wide layers)
# ----------------------------------------------------------------------------
FWD_SHAPES = [
    # (n_prev, n_cur, f, in_w, in_h, batch, relu, served by ops_fast.hip on the auto path)
    (1, 64, 9, 33, 33, 5, 1, True),     # default L1
    (64, 32, 1, 25, 25, 5, 1, True),    # default L2
    (32, 1, 5, 25, 25, 5, 0, True),     # default L3 (SKIP_RELU)
    (1, 128, 9, 33, 33, 2, 1, True),    # wide L1
    (128, 64, 5, 25, 25, 2, 1, True),   # wide L2
    (64, 1, 5, 21, 21, 2, 0, True),     # wide L3
    (3, 7, 3, 11, 9, 3, 1, False),      # ragged
    (1, 1, 1, 1, 1, 1, 0, False),       # minimal
    (1, 64, 9, 40, 37, 3, 1, True),     # non-square, not a 33 tile
    (1, 32, 9, 33, 33, 3, 1, True),     # example L1
    (32, 16, 1, 25, 25, 3, 1, True),    # example L2
    (16, 1, 5, 25, 25, 3, 0, True),     # example L3
    (64, 32, 1, 7, 5, 1, 0, True),      # pointwise: ragged pixel count, no ReLU
    (1, 64, 9, 41, 41, 2, 1, True),     # past one 40x40 input window: 2x2 windows
    (1, 64, 9, 100, 71, 2, 1, True),    # 4x2 windows, ragged right / bottom ones
    (1, 32, 5, 77, 45, 1, 1, True),     # f1 = 5: 36x36 output windows
    (1, 128, 9, 128, 128, 1, 1, True),  # the reference's 128 px samples (wide L1)
    (32, 1, 5, 64, 50, 2, 0, True),     # layer 3 past one 25x25 A2 window, ragged
    (16, 1, 3, 90, 47, 1, 0, True),     # f3 = 3: 39x39 output windows
    (32, 1, 5, 120, 120, 1, 0, True),   # A2 of a 128 px sample
    (128, 64, 5, 60, 45, 1, 1, True),   # wide L2 in 21x21 output windows, ragged
    (128, 64, 5, 25, 25, 1, 0, False),  # wide L2 without ReLU: generic
    # the wide net on 25x25 tiles (host spec geometry)
    (1, 128, 9, 25, 25, 3, 1, True),
    (128, 64, 5, 17, 17, 3, 1, True),
    (64, 1, 5, 13, 13, 3, 0, True),
]


def check_path(S, path, fast):
    """The op-level call ran the gfx950 kernel it was meant to (auto path)."""
    want = "fast" if (path == 0 and fast) else "generic"
    assert S.last_path() == want, (S.last_path(), want)


@pytest.mark.parametrize("shape", FWD_SHAPES, ids=lambda s: "k%d_n%d_f%d_%dx%d_b%d" % s[:6])
def test_conv_fwd_vs_oracle(S, path, shape):
    n_prev, n_cur, f, iw, ih, b, relu, fast = shape
    rng = np.random.default_rng(hash(shape) & 0xFFFF)
    x = rng.standard_normal(b * iw * ih * n_prev).astype(np.float32)
    W = (rng.standard_normal(f * f * n_prev * n_cur) / np.sqrt(f * f * n_prev)).astype(np.float32)
    B = (0.1 * rng.standard_normal(n_cur)).astype(np.float32)
    ref = orc.conv_fwd(x, W, B, iw, ih, n_prev, n_cur, f, relu, b)
    out = zeros(ref.size)
    S.conv_fwd(D(x), out, D(W), D(B), iw, ih, n_prev, n_cur, f, relu, b)
    check_path(S, path, fast)
    assert_close(H(out), ref, RTOL, "conv_fwd", orc.f64.conv_fwd(x, W, B, iw, ih, n_prev, n_cur, f, relu, b))


DELTA_SHAPES = [
    # (n_curr, n_next, f_next, curr_w, curr_h, batch, served by ops_fast.hip on auto)
    (32, 1, 5, 25, 25, 4, True),     # default delta2 (through W3)
    (64, 32, 1, 25, 25, 4, True),    # default delta1 (through W2)
    (64, 1, 5, 21, 21, 2, True),     # wide delta2
    (128, 64, 5, 25, 25, 2, True),   # wide delta1
    (2, 3, 3, 5, 5, 1, False),       # LayerDeltasTest shape
    (5, 4, 3, 9, 7, 3, False),       # ragged
    (16, 1, 5, 25, 25, 3, True),     # example delta2
    (32, 16, 1, 25, 25, 3, True),    # example delta1
    (32, 1, 3, 9, 6, 2, True),       # f3 = 3, non-square
    (64, 1, 5, 13, 13, 3, True),     # wide net, 25x25 tiles
    (128, 64, 5, 17, 17, 3, True),
    (32, 1, 5, 140, 70, 1, True),    # delta2 in 64x64 A2 windows, ragged
    (128, 64, 5, 61, 40, 1, True),   # wide delta1 in 25x25 windows
    (16, 1, 3, 70, 130, 2, True),
]


@pytest.mark.parametrize("shape", DELTA_SHAPES, ids=lambda s: "n%d_k%d_f%d_%dx%d_b%d" % s[:6])
def test_conv_delta_vs_oracle(S, path, shape):
    n_curr, n_next, f, cw, ch, b, fast = shape
    rng = np.random.default_rng(hash(shape) & 0xFFFF)
    nw, nh = cw - f + 1, ch - f + 1
    d_next = rng.standard_normal(b * nw * nh * n_next).astype(np.float32)
    y = np.maximum(rng.standard_normal(b * cw * ch * n_curr), 0).astype(np.float32)
    W = rng.standard_normal(f * f * n_curr * n_next).astype(np.float32)
    ref = orc.conv_delta(d_next, y, W, f, n_curr, n_next, cw, ch, b)
    out = zeros(ref.size)
    S.conv_delta(D(d_next), D(y), out, D(W), f, n_curr, n_next, cw, ch, b)
    check_path(S, path, fast)
    assert_close(H(out), ref, RTOL, "conv_delta",
                 orc.f64.conv_delta(d_next, y, W, f, n_curr, n_next, cw, ch, b))


GRAD_SHAPES = [
    # (n_prev, n_cur, f, out_w, out_h, batch, served by ops_fast.hip on auto)
    (1, 64, 9, 25, 25, 6, True),     # default gW1
    (64, 32, 1, 25, 25, 6, True),    # default gW2
    (32, 1, 5, 21, 21, 6, True),     # default gW3
    (128, 64, 5, 21, 21, 2, True),   # wide gW2
    (3, 5, 3, 7, 6, 3, False),       # ragged
    (1, 128, 9, 25, 25, 3, True),    # wide gW1
    (64, 1, 5, 17, 17, 3, True),     # wide gW3
    (1, 32, 9, 25, 25, 3, True),     # example gW1
    (32, 16, 1, 25, 25, 3, True),    # example gW2
    (16, 1, 5, 21, 21, 3, True),     # example gW3
    (64, 32, 1, 5, 3, 1, True),      # pointwise, 15 pixels
    (64, 1, 5, 9, 9, 3, True),       # wide net, 25x25 tiles
    (128, 64, 5, 13, 13, 3, True),
    (1, 128, 9, 17, 17, 3, True),
    (1, 64, 9, 92, 63, 2, True),     # layer 1 in 32x32 output windows, ragged
    (1, 32, 5, 70, 40, 1, True),     # f1 = 5 windows
    (1, 64, 9, 120, 120, 1, True),   # a 128 px sample
    (32, 1, 5, 136, 66, 1, True),    # gW3 in 64x64 A2 windows, ragged
    (64, 1, 3, 70, 129, 2, True),
    (128, 64, 5, 50, 37, 1, True),   # wide gW2 in 16 x 4 output windows
]


@pytest.mark.parametrize("shape", GRAD_SHAPES, ids=lambda s: "k%d_n%d_f%d_%dx%d_b%d" % s[:6])
def test_conv_grad_vs_oracle(S, path, shape):
    n_prev, n_cur, f, ow, oh, b, fast = shape
    rng = np.random.default_rng(hash(shape) & 0xFFFF)
    iw, ih = ow + f - 1, oh + f - 1
    inp = rng.standard_normal(b * iw * ih * n_prev).astype(np.float32)
    dl = rng.standard_normal(b * ow * oh * n_cur).astype(np.float32)
    gW0 = rng.standard_normal(f * f * n_prev * n_cur).astype(np.float32)
    gB0 = rng.standard_normal(n_cur).astype(np.float32)
    rW, rB = orc.conv_grad_acc(inp, dl, gW0, gB0, n_prev, n_cur, f, ow, oh, b)
    nbytes = S.conv_grad_workspace_bytes(n_prev, n_cur, f, ow, oh, b)
    ws = zeros(nbytes // 4 + 1)
    gW, gB = D(gW0), D(gB0)
    S.conv_grad_acc(D(inp), D(dl), gW, gB, n_prev, n_cur, f, ow, oh, b, ws, nbytes)
    check_path(S, path, fast)
    xW, xB = orc.f64.conv_grad_acc(inp, dl, gW0, gB0, n_prev, n_cur, f, ow, oh, b)
    assert_close(H(gW), rW, RTOL, "gW", xW)
    assert_close(H(gB), rB, RTOL, "gB", xB)


# ----------------------------------------------------------------------------
# network level (ConfigBasedDataPipeline) vs the oracle
# ----------------------------------------------------------------------------
NETS = {"default": (64, 32, 9, 1, 5), "wide": (128, 64, 9, 5, 5), "tiny": (8, 4, 5, 1, 3),
        "example": (32, 16, 9, 1, 5), "default_f3": (64, 32, 9, 1, 3)}


def expected_train_path(name, size, path):
    """Kernel family srcnn_train_fwd_bwd must report (srcnn_last_path): the
    fused f2 == 1 kernels take tiles up to 39x39 (l12's and d1's LDS images;
    past 33x33 layer 3 runs on the op-level kernels between them); the wide
    step's kernels take tiles up to 33x33 (its L2 output, 21 x 21 = 441
    pixels, fills the 14 register tiles of 32 pixels of the L2 forward;
    wide_plan.hpp: plan_step(), the WidePlan); larger tiles run every conv on the windowed
    op-level gfx950 kernels ("fast"); nets outside the instantiated shapes
    (tiny: n1 = 8) on the generic ones."""
    if path == 1 or name == "tiny":
        return {"generic"}
    if name in ("default", "example", "default_f3"):
        return {"fused"} if size <= 39 else {"fast"}
    if name == "wide":
        return {"wide"} if size <= 33 else {"fast"}
    return {"generic", "fast"}


def test_preload_every_net(S):
    """srcnn_preload resolves the net-level kernels of every net family (and
    is a no-op for nets without specialised kernels); a step afterwards runs."""
    for cfg in NETS.values():
        S.preload(S.Net(*cfg))
    assert S.lib().srcnn_preload(None) != 0  # null net: SRCNN_ERR_INVALID, no crash


@pytest.mark.parametrize("name,batch,size", [("default", 16, 33), ("wide", 3, 33), ("tiny", 5, 15),
                                             ("default", 2, 48), ("example", 7, 33),
                                             ("default", 3, 21), ("default", 600, 33),
                                             # ragged against the grids: l3r / l12 (512 blocks; l3r
                                             # walks the batch from its end), d1c (1024)
                                             ("default", 257, 33), ("default", 513, 33),
                                             # the strong-scaling shard (512 tiles per rank) and its
                                             # neighbours; below 1024 samples d1c splits each
                                             # sample's chunks over 2 (511, 512) or 4 (100) blocks
                                             ("default", 511, 33), ("default", 512, 33), ("default", 100, 33),
                                             # d1c (1024 blocks, 4 samples each at batch 4096)
                                             ("default", 1025, 33), ("default", 5, 39),
                                             # tiles past l3_delta's LDS image (33x33): l12 +
                                             # op-level layer 3 + d1; 36x36 as the reference's
                                             # train_samples36 (profile.py:7)
                                             ("default", 9, 36), ("example", 5, 39),
                                             ("default", 300, 36), ("default_f3", 7, 33),
                                             ("default", 3, 40),
                                             # past the fused tiles: op-level windowed kernels,
                                             # e.g. the reference's 128 px samples
                                             # (generate_training_samples.py -s 128)
                                             ("default", 2, 128), ("example", 3, 64),
                                             ("wide", 2, 48)])
def test_train_step_vs_oracle(S, path, name, batch, size):
    cfg = NETS[name]
    net = S.Net(*cfg)
    rng = np.random.default_rng(42)
    X, T = make_batch(rng, batch, size, size)
    params = make_params(rng, cfg, sd=0.05)
    P = params.size
    g0 = (1e-3 * rng.standard_normal(P)).astype(np.float32)
    rg, acts = orc.train_fwd_bwd(cfg, X, T, size, size, batch, params, g0)
    xg, _ = orc.f64.train_fwd_bwd(cfg, X, T, size, size, batch, params, g0)
    st = run_step(S, cfg, size, size, batch, X, T, params, g0)
    assert st.path in expected_train_path(name, size, path), st.path
    check_gradients(cfg, st.grads, rg, xg, "")
    # validation metric over the same forward
    w3, h3 = dims(cfg, size, size)[4:]
    A3 = orc.forward(cfg, X, size, size, batch, params)
    ref_err = orc.sq_err(T, A3, size, size, w3, h3, batch)
    assert st.sq_err == pytest.approx(ref_err, rel=1e-4)
    # update
    mom0 = (1e-3 * rng.standard_normal(P)).astype(np.float32)
    lr = [1e-4, 1e-4, 1e-5]
    rp, rg2, rm = orc.update_all(cfg, params, rg, mom0, 0.9, 1e-3, lr, batch)
    p_dev, m_dev = D(params), D(mom0)
    g_ref_dev = D(rg)  # update from identical grads -> isolates the update kernel
    S.update_all(net, p_dev, g_ref_dev, m_dev, 0.9, 1e-3, lr, batch)
    np.testing.assert_allclose(H(p_dev), rp, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(H(m_dev), rm, rtol=1e-6, atol=1e-9)
    assert not H(g_ref_dev).any()


@pytest.mark.parametrize("name,batch,size,fused_update", [
    ("default", 16, 33, True), ("default", 513, 33, True), ("default", 4096, 33, True),
    ("example", 7, 33, True), ("default_f3", 7, 33, True),
    # layer 3 on the op-level kernels / generic kernels: update_all afterwards
    ("wide", 3, 33, True), ("default", 9, 36, False), ("tiny", 5, 15, False)])
def test_train_step_matches_fwd_bwd_then_update(S, path, name, batch, size, fused_update):
    """srcnn_train_step (the update fused into the slab reduction on the fused
    path) gives bit-identical parameters, momenta, zeroed gradients and
    squared error to srcnn_train_fwd_bwd followed by srcnn_update_all
    (src/Main_cl.cpp:161-175 with the batch in one chunk)."""
    cfg = NETS[name]
    net = S.Net(*cfg)
    rng = np.random.default_rng(11)
    X, T = make_batch(rng, batch, size, size)
    params = make_params(rng, cfg, sd=0.05)
    P = params.size
    g0 = (1e-3 * rng.standard_normal(P)).astype(np.float32)  # accumulated earlier chunks
    m0 = (1e-3 * rng.standard_normal(P)).astype(np.float32)
    lr = [1e-4, 2e-4, 1e-5]
    nbytes = S.train_workspace_bytes(net, size, size, batch)
    ws = torch.empty(nbytes // 4 + 64, dtype=torch.float32, device="cuda")
    Xd, Td = D(X), D(T)
    outs = []
    for fused in (False, True):
        p, g, m, err = D(params), D(g0), D(m0), zeros(1)
        if fused:
            S.train_step(net, Xd, Td, size, size, batch, p, g, m, 0.9, 1e-3, lr, 3 * batch, err, ws,
                         nbytes)
        else:
            S.train_fwd_bwd(net, Xd, Td, size, size, batch, p, g, err, ws, nbytes)
            S.update_all(net, p, g, m, 0.9, 1e-3, lr, 3 * batch)
        assert S.last_path() in expected_train_path(name, size, path), S.last_path()
        outs.append([H(p), H(g), H(m), H(err)])
    for a, b, what in zip(outs[0], outs[1], ["params", "grads", "momentum", "sq_err"]):
        np.testing.assert_array_equal(b, a, err_msg=what)
    assert not outs[1][1].any()
    assert (outs[1][0] != params).mean() > 0.9  # the step moved the parameters
    if path == 0 and fused_update:
        # the fused path launches no separate update kernel
        S.profile_enable(True)
        S.profile_reset()
        S.train_step(net, Xd, Td, size, size, batch, D(params), D(g0), D(m0), 0.9, 1e-3, lr, batch,
                     None, ws, nbytes)
        torch.cuda.synchronize()
        S.profile_enable(False)
        names = set(S.profile_stats())
        assert "update_all" not in names and "slab_reduce" in names, names


@pytest.mark.parametrize("w,h,batch", [(35, 31, 7), (29, 38, 5), (33, 17, 9)])
def test_train_step_nonsquare_tiles(S, w, h, batch):
    """Non-square training tiles through the fused kernels (l12, l3 / op-level
    layer 3, d1c: pixel -> X offsets and row clamps use ow != oh)."""
    cfg = NETS["default"]
    rng = np.random.default_rng(7)
    X, T = make_batch(rng, batch, w, h)
    params = make_params(rng, cfg, sd=0.05)
    P = params.size
    g0 = np.zeros(P, np.float32)
    rg, _ = orc.train_fwd_bwd(cfg, X, T, w, h, batch, params, g0)
    xg, _ = orc.f64.train_fwd_bwd(cfg, X, T, w, h, batch, params, g0)
    st = run_step(S, cfg, w, h, batch, X, T, params, sq_err=False)
    assert st.path == "fused", st.path
    check_gradients(cfg, st.grads, rg, xg, "")


@pytest.mark.parametrize("size", [34, 37, 40])
@pytest.mark.parametrize("arith", [0, 1], ids=["split", "f32"])
def test_wide_tiles_past_the_wide_step(S, size, arith):
    """Wide tiles of 34-40 px (past the wide step's 33 px, expected_train_path):
    every layer on the windowed op-level gfx950 kernels under either
    arithmetic, one srcnn_last_kernels entry per reference launcher
    (ConfigBasedDataPipeline.cpp:128-323: any tile size goes through
    execute_batch), gradients against the oracle."""
    cfg = NETS["wide"]
    rng = np.random.default_rng(size)
    batch = 3
    X, T = make_batch(rng, batch, size, size)
    params = make_params(rng, cfg, sd=0.05)
    P = params.size
    g0 = (1e-3 * rng.standard_normal(P)).astype(np.float32)
    rg, _ = orc.train_fwd_bwd(cfg, X, T, size, size, batch, params, g0)
    xg, _ = orc.f64.train_fwd_bwd(cfg, X, T, size, size, batch, params, g0)
    st = run_step(S, cfg, size, size, batch, X, T, params, g0, arith=arith)
    path, ks = st.path, st.kernels
    assert path == "fast", path
    assert path in expected_train_path("wide", size, 0)
    assert ks == ["conv_fwd_l1:fast", "conv_fwd_l2:fast", "conv_fwd_l3:fast", "conv_delta_l2:fast",
                  "conv_delta_l1:fast", "conv_grad_l3:fast", "conv_grad_l2:fast", "conv_grad_l1:fast"], ks
    check_gradients(cfg, st.grads, rg, xg, "wide %d " % size)
    w3, h3 = dims(cfg, size, size)[4:]
    A3 = orc.forward(cfg, X, size, size, batch, params)
    assert st.sq_err == pytest.approx(orc.sq_err(T, A3, size, size, w3, h3, batch), rel=1e-4)


def test_train_activations_follow_the_step_arith(S):
    """srcnn_train_activations converts A1 in the layout the step that wrote
    the workspace used (split-bf16: run order; fp32: blocked), even when
    srcnn_set_arith changed in between (advisor r05)."""
    cfg = NETS["default"]
    net = S.Net(*cfg)
    rng = np.random.default_rng(17)
    batch, size = 5, 33
    X, T = make_batch(rng, batch, size, size)
    params = make_params(rng, cfg, sd=0.05)
    P = params.size
    W1, B1 = segments(cfg, params)[:2]
    A1ref = orc.conv_fwd(X, W1, B1, size, size, 1, cfg[0], cfg[2], 1, batch)
    nbytes = S.train_workspace_bytes(net, size, size, batch)
    ws = torch.empty(nbytes // 4 + 64, dtype=torch.float32, device="cuda")
    for arith_step, arith_read in ((0, 1), (1, 0)):
        S.set_arith(arith_step)
        S.train_fwd_bwd(net, D(X), D(T), size, size, batch, D(params), zeros(P), None, ws, nbytes)
        step_kernels = S.last_kernels()
        S.set_arith(arith_read)
        A1d, A2d, A3d = (zeros(n) for n in act_sizes(cfg, size, size, batch))
        S.train_activations(net, size, size, batch, ws, nbytes, A1d, A2d, A3d)
        assert ran_x6(step_kernels) == (arith_step == 0), step_kernels
        assert_close(H(A1d), A1ref, RTOL, "A1 (step arith %d, read under %d)" % (arith_step, arith_read))


@pytest.mark.parametrize("arith", [0, 1], ids=["split", "f32"])
@pytest.mark.parametrize("name,batch,w,h,l3", [
    # l3r: one sample (256-1024 samples: two) per block.  Split arithmetic:
    # l3r writes delta3 and d1x6 forms delta2 ("l3r_d3" + "d1x6_d3"); fp32:
    # l3r writes delta2 for d1c ("l3r_delta")
    ("default", 16, 33, 33, "l3r"), ("default", 512, 33, 33, "l3r"),
    ("default", 257, 33, 33, "l3r"), ("default", 7, 35, 31, "l3r"),
    ("default", 2, 21, 21, "l3r"), ("default", 1537, 33, 33, "l3r"),
    # n2 = 16, and n2 = 32 past l3r's 512 A3 outputs (f3 = 3 on 33x33: 529):
    # l3_delta; past 640 A2 pixels: the op-level layer-3 kernels
    ("example", 16, 33, 33, "l3_delta"), ("default_f3", 7, 33, 33, "l3_delta"),
    ("default", 3, 39, 39, "l3_op_level")])
def test_train_step_sq_err_and_a3_vs_oracle(S, name, batch, w, h, l3, arith):
    """The fused step's layer-3 kernel -- which one ran is asserted per case
    (srcnn_last_kernels): gradients, squared error and the A3 it leaves in the
    workspace (srcnn_train_activations) against the oracle
    (last_layer_delta.cl, squared_error.cl, layer_deltas.cl, backpropagate.cl)."""
    cfg = NETS[name]
    rng = np.random.default_rng(31)
    X, T = make_batch(rng, batch, w, h)
    params = make_params(rng, cfg, sd=0.05)
    P = params.size
    g0 = (1e-3 * rng.standard_normal(P)).astype(np.float32)
    rg, _ = orc.train_fwd_bwd(cfg, X, T, w, h, batch, params, g0)
    xg, _ = orc.f64.train_fwd_bwd(cfg, X, T, w, h, batch, params, g0)
    st = run_step(S, cfg, w, h, batch, X, T, params, g0, arith=arith)
    S.set_arith(0)
    assert st.path == "fused", st.path
    ks = st.kernels
    if l3 == "l3r":
        x6 = ran_x6(ks)
        assert x6 == (arith == 0), ks
        want = ["l3r_d3", "d1x6_d3"] if x6 else ["l3r_delta"]
        assert all(k in ks for k in want), ks
    else:
        assert l3 in ks, ks
        assert "l3r_d3" not in ks and "d1x6_d3" not in ks, ks
    check_gradients(cfg, st.grads, rg, xg, "l3 ")
    w3, h3 = dims(cfg, w, h)[4:]
    A3 = orc.forward(cfg, X, w, h, batch, params)
    ref_err = orc.sq_err(T, A3, w, h, w3, h3, batch)
    assert st.sq_err == pytest.approx(ref_err, rel=1e-4)
    assert_close(st.activations()[2], A3, RTOL, "l3 A3")


def test_forward_vs_oracle(S, path):
    cfg = NETS["default"]
    net = S.Net(*cfg)
    rng = np.random.default_rng(9)
    w, h, b = 256, 256, 1   # BASELINE config 1: one 256x256 tile
    X, _ = make_batch(rng, b, w, h)
    params = make_params(rng, cfg, sd=0.05)
    ref = orc.forward(cfg, X, w, h, b, params)
    nbytes = S.forward_workspace_bytes(net, w, h, b)
    ws = torch.empty(nbytes // 4 + 64, dtype=torch.float32, device="cuda")
    out = zeros(ref.size)
    S.forward(net, D(X), w, h, b, D(params), out, ws, nbytes)
    assert_close(H(out), ref, RTOL, "forward 256x256", orc.f64.forward(cfg, X, w, h, b, params))


FWD_FRAMES = [("default", 77, 45, 3), ("default", 300, 210, 1), ("example", 96, 64, 2),
              ("default", 33, 33, 5), ("default", 41, 200, 1), ("wide", 64, 48, 1)]


@pytest.mark.parametrize("name,w,h,b", FWD_FRAMES, ids=lambda v: str(v))
def test_forward_frames_vs_oracle(S, path, name, w, h, b):
    """srcnn_forward on ragged frames: partial 32-wide regions / 16-row
    gather tiles at every edge, batches, both fused nets and a generic one."""
    cfg = NETS[name]
    net = S.Net(*cfg)
    rng = np.random.default_rng(w * 1000 + h)
    X, _ = make_batch(rng, b, w, h)
    params = make_params(rng, cfg, sd=0.05)
    ref = orc.forward(cfg, X, w, h, b, params)
    nbytes = S.forward_workspace_bytes(net, w, h, b)
    ws = torch.empty(nbytes // 4 + 64, dtype=torch.float32, device="cuda")
    out = torch.full((ref.size,), float("nan"), dtype=torch.float32, device="cuda")
    S.forward(net, D(X), w, h, b, D(params), out, ws, nbytes)
    got = H(out)
    assert np.isfinite(got).all()  # every output written
    assert_close(got, ref, RTOL, "forward %s %dx%d b%d" % (name, w, h, b),
                 orc.f64.forward(cfg, X, w, h, b, params))


def test_forward_4k_frame_vs_oracle(S):
    """BASELINE.json configs[4] at its own size: one 3840x2160 luma frame
    through the fused inference kernels against the oracle (OpenMP over
    output rows), every one of the 3828x2148 outputs checked."""
    cfg = NETS["default"]
    net = S.Net(*cfg)
    rng = np.random.default_rng(4096)
    w, h = 3840, 2160
    X, _ = make_batch(rng, 1, w, h)
    params = make_params(rng, cfg, sd=0.05)
    ref = orc.forward(cfg, X, w, h, 1, params)
    nbytes = S.forward_workspace_bytes(net, w, h, 1)
    ws = torch.empty(nbytes // 4 + 64, dtype=torch.float32, device="cuda")
    out = torch.full((ref.size,), float("nan"), dtype=torch.float32, device="cuda")
    S.forward(net, D(X), w, h, 1, D(params), out, ws, nbytes)
    assert S.last_path() == "fused"
    got = H(out)
    assert np.isfinite(got).all()  # every output written
    assert_close(got, ref, RTOL, "forward 3840x2160", orc.f64.forward(cfg, X, w, h, 1, params))


def test_forward_large_frame_fused_vs_generic(S):
    """A 1280x720 frame: the fused path and the generic layer-by-layer path,
    each against the oracle."""
    cfg = NETS["default"]
    net = S.Net(*cfg)
    rng = np.random.default_rng(720)
    w, h = 1280, 720
    X, _ = make_batch(rng, 1, w, h)
    params = make_params(rng, cfg, sd=0.05)
    n_out = (w - 12) * (h - 12)
    res = {}
    for p in (0, 1):
        S.set_path(p)
        nbytes = S.forward_workspace_bytes(net, w, h, 1)
        ws = torch.empty(nbytes // 4 + 64, dtype=torch.float32, device="cuda")
        out = torch.full((n_out,), float("nan"), dtype=torch.float32, device="cuda")
        S.forward(net, D(X), w, h, 1, D(params), out, ws, nbytes)
        res[p] = H(out)
    assert np.isfinite(res[0]).all()
    ref = orc.forward(cfg, X, w, h, 1, params)
    ref64 = orc.f64.forward(cfg, X, w, h, 1, params)
    assert_close(res[0], ref, RTOL, "forward 1280x720 fused", ref64)
    assert_close(res[1], ref, RTOL, "forward 1280x720 generic", ref64)


@pytest.mark.parametrize("world", [2, 3, 8])
def test_forward_row_bands_vs_oracle(S, world):
    """Inference sharded by row bands (parallel.forward_band):
    every rank's band run in turn on device 0 into one output buffer, each
    band a slice of the frame's own buffers.  The stitched frame covers every
    output and matches the oracle's whole-frame forward; the bands' region
    grids start at their own row 0, so the sums are grouped differently from
    the unsharded call (within RTOL of it, not bit-equal)."""
    from srcnn_amd import parallel
    cfg = NETS["default"]
    net = S.Net(*cfg)
    rng = np.random.default_rng(1000 + world)
    w, h = 640, 365
    X, _ = make_batch(rng, 1, w, h)
    params = make_params(rng, cfg, sd=0.05)
    n_out = (w - 12) * (h - 12)
    nbytes = S.forward_workspace_bytes(net, w, h, 1)
    ws = torch.empty(nbytes // 4 + 64, dtype=torch.float32, device="cuda")
    Xd, Pd = D(X), D(params)
    out = torch.full((n_out,), float("nan"), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    rows = 0
    for r in range(world):
        _, no = parallel.forward_band(S, net, Xd, w, h, Pd, out, ws, nbytes, stream, r, world)
        rows += no
    assert rows == h - 12
    whole = torch.full((n_out,), float("nan"), dtype=torch.float32, device="cuda")
    S.forward(net, Xd, w, h, 1, Pd, whole, ws, nbytes)
    got = H(out)
    assert np.isfinite(got).all()
    ref = orc.forward(cfg, X, w, h, 1, params)
    assert_close(got, ref, RTOL, "forward %d row bands" % world, orc.f64.forward(cfg, X, w, h, 1, params))
    assert_close(got, H(whole), RTOL, "row bands vs whole frame")


# ----------------------------------------------------------------------------
# full size (BASELINE config 2: default net, 33x33, batch 4096)
# ----------------------------------------------------------------------------
def test_full_batch_gradients_vs_oracle(S):
    cfg = NETS["default"]
    net = S.Net(*cfg)
    batch, size = 4096, 33
    rng = np.random.default_rng(2024)
    X, T = make_batch(rng, batch, size, size)
    params = make_params(rng, cfg, sd=0.05)
    P = params.size
    rg, _ = orc.train_fwd_bwd(cfg, X, T, size, size, batch, params, np.zeros(P, np.float32))
    xg, _ = orc.f64.train_fwd_bwd(cfg, X, T, size, size, batch, params, np.zeros(P))
    nbytes = S.train_workspace_bytes(net, size, size, batch)
    ws = torch.empty(nbytes // 4 + 64, dtype=torch.float32, device="cuda")
    Xd, Td, pd = D(X), D(T), D(params)
    g = zeros(P)
    S.train_fwd_bwd(net, Xd, Td, size, size, batch, pd, g, None, ws, nbytes)
    got = H(g)
    check_gradients(cfg, got, rg, xg, "full-batch ")
    # determinism: a second pass gives bit-identical gradients
    g2 = zeros(P)
    S.train_fwd_bwd(net, Xd, Td, size, size, batch, pd, g2, None, ws, nbytes)
    np.testing.assert_array_equal(H(g2), got)
    # chunk linearity: two 2048-tile chunks accumulate to the same gradient
    g3 = zeros(P)
    half = batch // 2
    n = size * size
    S.train_fwd_bwd(net, Xd[:half * n], Td[:half * n], size, size, half, pd, g3, None, ws, nbytes)
    S.train_fwd_bwd(net, Xd[half * n:], Td[half * n:], size, size, half, pd, g3, None, ws, nbytes)
    assert_close(H(g3), got, RTOL, "chunked accumulation")


def test_held_clock_probe(S):
    """srcnn_profile_clock: the production library carries no in-kernel probe
    and reports -1; a diagnostic build (make PROBE=1) reports a plausible
    shader clock after a launch (MI355X max 2.4 GHz; under MFMA load the chip
    holds less).  Other names are rejected either way."""
    cfg = NETS["default"]
    net = S.Net(*cfg)
    batch, size = 512, 33
    rng = np.random.default_rng(7)
    X, T = make_batch(rng, batch, size, size)
    params = make_params(rng, cfg, sd=0.05)
    nbytes = S.train_workspace_bytes(net, size, size, batch)
    ws = torch.empty(nbytes // 4 + 64, dtype=torch.float32, device="cuda")
    g = zeros(params.size)
    S.train_fwd_bwd(net, D(X), D(T), size, size, batch, D(params), g, None, ws, nbytes)
    torch.cuda.synchronize()
    probe = os.environ.get("SRCNN_EXPECT_CLOCK_PROBE") == "1"
    for k in ("l12_fwd_mfma", "l3_delta_fused", "delta1_grad12_fused"):
        ghz = S.profile_clock(k)
        if probe:
            assert ghz is not None and 0.3 < ghz < 3.0, (k, ghz)
        else:
            assert ghz is None, (k, ghz)
    with pytest.raises(S.SrcnnError):
        S.profile_clock("no_such_kernel")


# ----------------------------------------------------------------------------
# error behaviour (reference: std::runtime_error from the launchers)
# ----------------------------------------------------------------------------
def test_invalid_arguments_raise(S):
    with pytest.raises(S.SrcnnError) as e:
        S.conv_fwd(zeros(1), zeros(1), zeros(1), zeros(1), 3, 3, 1, 1, 5, 1, 1)  # f > input
    assert e.value.code == S.ERR_INVALID
    with pytest.raises(S.SrcnnError) as e:
        S.conv_grad_acc(zeros(81), zeros(81), zeros(81), zeros(1), 1, 1, 1, 9, 9, 1, zeros(1), 0)
    assert e.value.code in (S.ERR_WORKSPACE, S.ERR_INVALID)
    with pytest.raises(S.SrcnnError) as e:
        S.train_fwd_bwd(S.Net(64, 32, 9, 2, 5), zeros(1), zeros(1), 33, 33, 1, zeros(1), zeros(1),
                        None, zeros(1), 4)
    assert e.value.code == S.ERR_INVALID   # even f2 (Config.cpp:64-66)


# ----------------------------------------------------------------------------
# HIP graphs (srcnn_graph_*): a captured step replays to the same results
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [7, 512])
def test_graph_replay_matches_direct_steps(S, batch):
    """Three srcnn_train_step calls and three replays of one captured
    srcnn_train_step give bit-identical parameters, momenta and gradients; so
    do fwd_bwd + a one-rank RCCL all-reduce + update_all (the data-parallel
    step bench.py captures for N > 1) against the same calls made directly."""
    cfg = NETS["default"]
    net = S.Net(*cfg)
    rng = np.random.default_rng(5)
    X, T = make_batch(rng, batch, 33, 33)
    params = make_params(rng, cfg, sd=0.05)
    P = params.size
    lr = [1e-4, 2e-4, 1e-5]
    nbytes = S.train_workspace_bytes(net, 33, 33, batch)
    ws = torch.empty(nbytes // 4 + 64, dtype=torch.float32, device="cuda")
    st = torch.cuda.Stream()
    sh = st.cuda_stream
    Xd, Td = D(X), D(T)
    comms = S.comm_init_all([0])
    try:
        for mode in ("train_step", "dp"):
            outs = []
            for use_graph in (False, True):
                p, g, m = D(params), zeros(P), zeros(P)
                torch.cuda.synchronize()

                def step():
                    if mode == "train_step":
                        S.train_step(net, Xd, Td, 33, 33, batch, p, g, m, 0.9, 1e-3, lr, batch, None, ws,
                                     nbytes, sh)
                    else:
                        S.train_fwd_bwd(net, Xd, Td, 33, 33, batch, p, g, None, ws, nbytes, sh)
                        S.allreduce_grads(comms[0], g, P, sh)
                        S.update_all(net, p, g, m, 0.9, 1e-3, lr, batch, sh)
                if use_graph:
                    gr = S.Graph(step, sh)
                    for _ in range(3):
                        gr.launch()
                    torch.cuda.synchronize()
                    gr.close()
                else:
                    for _ in range(3):
                        step()
                outs.append([H(p), H(g), H(m)])
            for a, b, what in zip(outs[0], outs[1], ["params", "grads", "momentum"]):
                np.testing.assert_array_equal(b, a, err_msg="%s %s" % (mode, what))
            assert (outs[1][0] != params).mean() > 0.9  # the replays trained
    finally:
        S.comm_destroy(comms[0])
    with pytest.raises(ValueError):
        S.Graph(lambda: None, None)  # the NULL stream cannot be captured
