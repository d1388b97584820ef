"""Split-bf16 arithmetic (srcnn_set_arith 0, l12x6 / d1x6) against the fp32
MFMA kernels (srcnn_set_arith 1), both against the double-precision oracle.

The fused default-net step forms its layer-1/2 products from three exact
bf16 parts per fp32 operand and six part products (csrc/hip/split.hpp).  The
claim is fp32 accuracy: on the same inputs its normwise error against the
fp64 computation must stay within the fp32 kernels' own (x 1.5, plus a
2^-24 floor), gradient segment by segment, and the parameters after an SGD
step likewise.  The fp32 oracle's error is printed beside them."""
import numpy as np
import pytest

import srcnn_oracle as orc
from hip_util import D, H, NAMES, log_record, make_batch, make_params, normwise, ran_x6, segments
from step_util import S, _settings, run_step  # noqa: F401

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NET = (64, 32, 9, 1, 5)


def workspace(S, net, size, batch):
    """One query serves either arithmetic (the slab regions are sized for
    both), so the tests query once and run both on the same workspace."""
    nbytes = S.train_workspace_bytes(net, size, size, batch)
    return torch.empty(nbytes // 4 + 64, dtype=torch.float32, device="cuda"), nbytes


@pytest.mark.parametrize("batch,size,sd", [(64, 33, 0.05), (600, 33, 0.05), (256, 33, 1e-3), (7, 25, 0.05)])
def test_split_arith_within_fp32_error(S, batch, size, sd):
    rng = np.random.default_rng(7)
    X, T = make_batch(rng, batch, size, size)
    params = make_params(rng, NET, sd=sd)
    P = params.size
    g0 = np.zeros(P, np.float32)
    g32, _ = orc.train_fwd_bwd(NET, X, T, size, size, batch, params, g0)
    g64, _ = orc.f64.train_fwd_bwd(NET, X, T, size, size, batch, params, g0)
    wsn = workspace(S, S.Net(*NET), size, batch)
    split, f32 = (run_step(S, NET, size, size, batch, X, T, params, arith=arith, ws=wsn) for arith in (0, 1))
    ks, kf = split.kernels, f32.kernels
    # (l3r writes delta3 and d1x6 forms delta2 where l3r serves the tile)
    assert "l12x6_fwd" in ks and any(k in ks for k in ("d1x6_grad12", "d1x6_d3")), ks
    assert "l12_fwd" in kf and not ran_x6(kf), kf
    for nm, gs, gf, go, gx in zip(NAMES, *(segments(NET, g) for g in (split.grads, f32.grads, g32, g64))):
        es, ef, eo = normwise(gs, gx), normwise(gf, gx), normwise(go, gx)
        log_record({"test": "split_arith", "batch": batch, "size": size, "sd": sd, "seg": nm,
                    "err_split": es, "err_f32_mfma": ef, "err_f32_oracle": eo})
        print("%s batch %d: split %.3e  fp32 MFMA %.3e  fp32 oracle %.3e" % (nm, batch, es, ef, eo))
        assert es <= 1.5 * ef + 2.0 ** -24, (nm, es, ef)


@pytest.mark.parametrize("w,h", [(256, 256), (333, 197)])
def test_split_forward_within_fp32_error(S, w, h):
    """The inference path (fwd_l123x6 vs fwd_l123) likewise."""
    rng = np.random.default_rng(11)
    X = (rng.random(w * h, dtype=np.float32) - 0.5).astype(np.float32)
    params = make_params(rng, NET, sd=0.05)
    ref64 = orc.f64.forward(NET, X, w, h, 1, params)
    ref32 = orc.forward(NET, X, w, h, 1, params)
    net = S.Net(*NET)
    errs = {}
    # one query for both arithmetics (the partial sums are sized for the split
    # kernel's 24-row and the fp32 kernel's 28-row regions alike)
    nbytes = S.forward_workspace_bytes(net, w, h, 1)
    ws = torch.empty(nbytes // 4 + 64, dtype=torch.float32, device="cuda")
    for arith in (0, 1):
        S.set_arith(arith)
        out = torch.empty(ref32.size, dtype=torch.float32, device="cuda")
        S.forward(net, D(X), w, h, 1, D(params), out, ws, nbytes)
        errs[arith] = normwise(H(out), ref64)
    log_record({"test": "split_forward", "w": w, "h": h, "err_split": errs[0], "err_f32_mfma": errs[1],
                "err_f32_oracle": normwise(ref32, ref64)})
    print("forward %dx%d: split %.3e  fp32 MFMA %.3e  fp32 oracle %.3e"
          % (w, h, errs[0], errs[1], normwise(ref32, ref64)))
    assert errs[0] <= 1.5 * errs[1] + 2.0 ** -24, errs


WIDE = (128, 64, 9, 5, 5)


# (33 is the largest square tile of the fused wide step: its L2 output,
#  21 x 21, fills the 14 register tiles of 32 pixels)
@pytest.mark.parametrize("batch,size", [(3, 33), (16, 33), (5, 29), (4, 25), (3, 27)])
def test_split_wide_within_fp32_error(S, batch, size):
    """The wide net's split kernels (wl1x6_fwd, wl2x6_fwd, wd1x6 + wg1x6,
    wgrad2x6 against wl1_fwd, conv_mfma, d1g16, wgrad2): the whole gradient,
    segment by segment."""
    rng = np.random.default_rng(5)
    X, T = make_batch(rng, batch, size, size)
    params = make_params(rng, WIDE, sd=0.05)
    P = params.size
    g0 = np.zeros(P, np.float32)
    g64, _ = orc.f64.train_fwd_bwd(WIDE, X, T, size, size, batch, params, g0)
    g32, _ = orc.train_fwd_bwd(WIDE, X, T, size, size, batch, params, g0)
    wsn = workspace(S, S.Net(*WIDE), size, batch)
    split, f32 = (run_step(S, WIDE, size, size, batch, X, T, params, arith=arith, ws=wsn) for arith in (0, 1))
    assert all(k in split.kernels for k in ("wl1x6_fwd", "wl2x6_fwd", "wd1x6", "wg1x6", "wgrad2x6")), split.kernels
    assert not ran_x6(f32.kernels), f32.kernels
    for nm, gs, gf, go, gx in zip(NAMES, *(segments(WIDE, g) for g in (split.grads, f32.grads, g32, g64))):
        es, ef, eo = normwise(gs, gx), normwise(gf, gx), normwise(go, gx)
        log_record({"test": "split_wide", "batch": batch, "size": size, "seg": nm, "err_split": es,
                    "err_f32_mfma": ef, "err_f32_oracle": eo})
        print("wide %s batch %d size %d: split %.3e  fp32 MFMA %.3e  fp32 oracle %.3e" % (nm, batch, size, es, ef, eo))
        # (B3 is one sum over every delta3 with heavy cancellation: either fp32
        # computation can land far closer to the fp64 value by chance, so the
        # bound is the larger of the two fp32 errors.  The wide step chains
        # four split kernels -- L1, L2, delta1, gW2 -- against one in the
        # default net's stages, so its bound is 2x, not the 1.5x of
        # test_split_within_fp32_error: batch 3 / 33x33 measured W3 3.4e-7,
        # B1 3.5e-7 against 1.8e-7 / 2.0e-7 for the fp32 MFMA path, all
        # normwise against fp64 and 300x under the 1e-4 tolerance)
        assert es <= 2.0 * max(ef, eo) + 2.0 ** -24, (nm, es, ef, eo)
        # (the fp32 wide kernels, the fallback past the split kernels' image
        # limits, stay parity-checked here too)
        assert ef <= 1e-5, (nm, ef)


def test_non_finite_input_stays_in_its_window(S):
    """srcnn.h: the two arithmetics agree for finite operands below the bf16
    maximum; a non-finite input (here one +inf pixel) is where they may
    differ (split parts inf - inf = NaN, the split ReLU keeps a NaN).  Pinned
    here: in both arithmetics the non-finite outputs lie inside that pixel's
    13 x 13 output window, and every output outside it is bit-identical to the
    same arithmetic's run without the inf pixel."""
    w = h = 96
    rng = np.random.default_rng(23)
    X = (rng.random(w * h, dtype=np.float32) - 0.5).astype(np.float32)
    params = make_params(rng, NET, sd=0.05)
    net = S.Net(*NET)
    ctx = NET[2] + NET[3] + NET[4] - 3  # 12
    ow = w - ctx
    py, px = 40, 57
    Xi = X.copy()
    Xi[py * w + px] = np.inf
    win = np.zeros((ow, ow), bool)
    win[max(0, py - ctx):py + 1, max(0, px - ctx):px + 1] = True
    nbytes = S.forward_workspace_bytes(net, w, h, 1)
    ws = torch.empty(nbytes // 4 + 64, dtype=torch.float32, device="cuda")
    for arith in (0, 1):
        S.set_arith(arith)
        outs = []
        for x in (X, Xi):
            out = torch.empty(ow * ow, dtype=torch.float32, device="cuda")
            S.forward(net, D(x), w, h, 1, D(params), out, ws, nbytes)
            outs.append(H(out).reshape(ow, ow))
        clean, dirty = outs
        assert np.isfinite(clean).all()
        bad = ~np.isfinite(dirty)
        log_record({"test": "split_non_finite", "arith": arith, "non_finite_in_window": int(bad.sum()),
                    "window": int(win.sum())})
        print("arith %d: %d non-finite outputs, all inside the %d-output window" % (arith, bad.sum(), win.sum()))
        assert not (bad & ~win).any(), arith
        assert np.array_equal(dirty[~win], clean[~win]), arith
