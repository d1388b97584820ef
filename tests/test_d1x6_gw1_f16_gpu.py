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
import hip_util
from hip_util import FLIP_FLOOR, RTOL, assert_close, guarded, guards_intact, make_batch, make_params, same_bits

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CFG = (64, 32, 9, 1, 5)
N1, N2, F1, F2, F3 = CFG
OFF = np.cumsum([0, F1 * F1 * N1, N1, N1 * N2, N2, F3 * F3 * N2, 1])
NAMES = ["W1", "B1", "W2", "B2", "W3", "B3"]
CASES = [("one", 33, 33, 5, "d1x6_d3", 31), ("many", 19, 17, 770, "d1x6_d3", 32), ("scratch", 27, 37, 3, "d1x6_d3_sc", 33),
         ("jumps", 33, 33, 520, "d1x6_d3", 34)]
ZERO_SAMPLE = 515


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


def normwise(a, ref):
    return float(np.linalg.norm(np.asarray(a, np.float64) - ref) / np.linalg.norm(ref))


def run_step(S, arith, w, h, batch, X, T, params, form=None, keep_ws=False):
    net = S.Net(*CFG)
    S.set_arith(arith)
    nbytes = S.train_workspace_bytes(net, w, h, batch)
    ws = guarded(nbytes // 4, float("nan"))
    g, err = guarded(np.zeros(params.size, np.float32), 1e30), guarded(1, 1e30, inner=0.0)
    S.train_fwd_bwd(net, guarded(X, 1e30), guarded(T, 1e30), w, h, batch, guarded(params, 1e30), g, err, ws, nbytes)
    ks = S.last_kernels()
    if form is not None:
        assert S.last_path() == "fused", S.last_path()
        assert "l12x6_fwd" in ks and "l3r_d3" in ks, ks
        assert [k for k in ks if k in ("d1x6_d3", "d1x6_d3_sc")] == [form], ks
    else:
        assert "x6" not in ks, ks
    got = H(g)
    if keep_ws:
        return got, net, ws, nbytes
    guards_intact(g, err, ws)
    return got


def inputs(S, name, w, h, batch, seed):
    rng = np.random.default_rng(seed)
    X, T = make_batch(rng, batch, w, h)
    params = make_params(rng, CFG, sd=0.05)
    if name == "jumps":
        # a first step for the net's own output of the zero sample
        _, net, ws, nbytes = run_step(S, 0, w, h, batch, X, T, params, keep_ws=True)
        sizes = (batch * (w - 8) * (h - 8) * N1, batch * (w - 8) * (h - 8) * N2, batch * (w - 12) * (h - 12))
        outs = [guarded(n, 1e30) for n in sizes]
        S.train_activations(net, w, h, batch, ws, nbytes, *outs)
        a3 = H(outs[2]).reshape(batch, h - 12, w - 12)
        hip_util._GUARDS.clear()
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
    got = run_step(S, 0, w, h, batch, X, T, params, form)
    f32 = run_step(S, 1, w, h, batch, X, T, params)
    dump = os.environ.get("SRCNN_GW1_DUMP")
    if dump:
        os.makedirs(dump, exist_ok=True)
        np.save(os.path.join(dump, name + ".npy"), got)
    errs = {}
    for i, nm in enumerate(NAMES[:2]):
        sl = slice(OFF[i], OFF[i + 1])
        errs[nm] = (normwise(got[sl], xg[sl]), normwise(f32[sl], xg[sl]))
        print("%s g%s: f16 x3 %.3e  fp32 arithmetic %.3e" % (name, nm, *errs[nm]))
    bar = 1.5 * max(e[1] for e in errs.values())
    for nm, (es, _) in errs.items():
        assert es <= bar, (name, nm, es, bar)
    for i, nm in enumerate(NAMES):
        sl = slice(OFF[i], OFF[i + 1])
        assert_close(got[sl], rg[sl], RTOL, "gw1 f16 %s grad %s" % (name, nm), xg[sl], FLIP_FLOOR)
    got2 = run_step(S, 0, w, h, batch, X, T, params, form)
    assert same_bits(got, got2), "two runs differ"
