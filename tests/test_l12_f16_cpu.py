"""l12x6's layers 1 and 2 on two-part fp16 split products, emulated in numpy
as the kernel builds them (l12x6.hpp), against fp64.  Layer 1:

  - one scale for W1 per launch, ew = scale_exp_h(max |W1|) over all of its
    81 x 64 weights, and one for X per sample, ex = scale_exp_h(max |X|);
  - the accumulator starts from one fp32 32x32x2 MFMA of tap (8, 8) and the
    bias, 2^ew on its A side (W1's tap 80, B1) and 2^ex on its B side (x88, and
    2^ex where the bias column had 1.0);
  - taps 0-79 in five 16-slot k-steps of three fp16 part products each, small
    ones first;
  - the accumulator times 2^-(ew + ex) (exact, in two steps where the factor
    passes 2^127), then the ReLU.

Layer 2 (K = 64 channels in four k-steps, A1 after the ReLU as the B operand):

  - one scale for W2 per launch, ew2 = scale_exp_h(max |W2|), and one for A1
    per sample from a bound instead of a pass over it, ea = scale_exp_h(max
    |X| . max_c sum_tap |W1[tap][c]| + max |B1|), the bound formed in fp32;
  - the accumulator starts from zero: three part products per k-step, then
    B2 2^ew2 (rounded once per launch) times 2^ea is added to the finished
    sum, then 2^-(ea + ew2) and the ReLU.

The slot order within a k-step does not enter: the part products of a k-step
are exact and summed as one.  The k-steps hold taps (dy, dx < 8) of rows
0-7, then row 8 and column 8, as the kernel's; the emulation takes the taps
in a fixed permutation with the same grouping.

Criterion (test_split_arith_within_fp32_error's): the normwise error against
fp64 is at most 1.5 x the fp32 chain's on the same data + 2^-24.
"""
import numpy as np
import pytest

from hip_util import make_batch
from test_split_f16_cpu import E_MAX, E_MIN, gemm_f16_x3, mfma_chain, normwise, scale_exp, split_f16

N1, N2, F1 = 64, 32, 9
K = F1 * F1  # 81 taps; tap 80 = (8, 8) rides the fp32 MFMA with the bias


def tap_order():
    """Taps 0-79 in the kernel's k-step order: group g = dy for dx < 8 (rows
    0-8), group 9 = column 8 (dy 0-7); k-step s holds groups 2s and 2s + 1."""
    order = []
    for g in range(10):
        order += [g * F1 + j for j in range(8)] if g < 9 else [j * F1 + 8 for j in range(8)]
    assert sorted(order) == list(range(80))
    return np.array(order)


def windows(x, w, h):
    """[81, ow * oh]: the 9 x 9 windows of one sample (tap-major)."""
    img = x.reshape(h, w)
    ow, oh = w - F1 + 1, h - F1 + 1
    return np.stack([img[dy:dy + oh, dx:dx + ow].ravel() for dy in range(F1) for dx in range(F1)])


def pow2(e):
    assert -126 <= e <= 127, e  # pow2_h: a normal fp32
    return np.float32(2.0) ** np.float32(e)


def w_scale(W1):
    return scale_exp(np.abs(W1).max(), 14)


def layer1_as_built(W1, B1, x, w, h, ew):
    """W1 [81, 64] (tap-major, as the parameters lie), B1 [64], x one sample.
    -> relu'd A1 [64, ow * oh] as fp32, and the constants used."""
    Xw = windows(x, w, h)
    ex = scale_exp(np.abs(x).max(), 14)
    sw, sx = pow2(ew), pow2(ex)
    # the fp32 MFMA: two exact products, one rounding
    a88, b1 = (W1[80] * sw).astype(np.float32), (B1 * sw).astype(np.float32)
    x88 = (Xw[80] * sx).astype(np.float32)
    acc = (a88.astype(np.float64)[:, None] * x88.astype(np.float64)[None, :] +
           b1.astype(np.float64)[:, None] * np.float64(sx)).astype(np.float32)
    od = tap_order()
    A, B = W1[od].T.copy(), Xw[od].copy()  # [64, 80], [80, P]
    a0, a1 = (p.astype(np.float64) for p in split_f16(A, ew))
    b0, b1_ = (p.astype(np.float64) for p in split_f16(B, ex))
    parts = (a0, a1, b0, b1_)
    assert all(np.isfinite(p).all() for p in parts)
    acc = mfma_chain(acc, [(a1, b0), (a0, b1_), (a0, b0)], 80)
    eu = -(ew + ex)
    eu1 = min(eu, 127)
    with np.errstate(over="ignore"):
        acc = (acc * pow2(eu1)).astype(np.float32)
        if eu != eu1:
            acc = (acc * pow2(eu - eu1)).astype(np.float32)
    return np.maximum(acc, np.float32(0)), (sw, sx, pow2(eu1), pow2(eu - eu1))


def layer1_fp32_chain(W1, B1, x, w, h):
    """The fp32 MFMA path: tap 80 and the bias first, then 40 32x32x2 steps."""
    Xw = windows(x, w, h).astype(np.float64)
    W = W1.astype(np.float64)
    acc = (np.outer(W[80], Xw[80]) + B1.astype(np.float64)[:, None]).astype(np.float32)
    od = tap_order()
    A, B = W[od].T, Xw[od]
    for k in range(0, 80, 2):
        acc = (acc.astype(np.float64) + A[:, k:k + 2] @ B[k:k + 2]).astype(np.float32)
    return np.maximum(acc, np.float32(0))


def layer1_f64(W1, B1, x, w, h):
    return np.maximum(W1.astype(np.float64).T @ windows(x, w, h).astype(np.float64) + B1.astype(np.float64)[:, None], 0.0)


def samples(rng, w, h):
    X, _ = make_batch(rng, 3, w, h)
    X = X.reshape(3, -1)
    spike = X[2].copy()
    spike[(h // 2) * w + w // 2] = np.float32(np.abs(spike).max() * 2.0 ** 10)
    return {"plain": X[0], "x2^12": np.ldexp(X[1], 12), "x2^-30": np.ldexp(X[1], -30), "spike": spike}


@pytest.mark.parametrize("sd", [1e-3, 0.05])
@pytest.mark.parametrize("kind", ["plain", "x2^12", "x2^-30", "spike"])
def test_layer1_as_built_within_fp32_error(kind, sd):
    w, h = 19, 17
    rng = np.random.default_rng(77)
    W1 = (sd * rng.standard_normal((K, N1))).astype(np.float32)
    B1 = (sd * rng.standard_normal(N1)).astype(np.float32)
    x = samples(rng, w, h)[kind]
    ref = layer1_f64(W1, B1, x, w, h)
    got, _ = layer1_as_built(W1, B1, x, w, h, w_scale(W1))
    e3, ef = normwise(got, ref), normwise(layer1_fp32_chain(W1, B1, x, w, h), ref)
    print("layer 1 %s sd=%g: f16 x3 as built %.3e  fp32 chain %.3e" % (kind, sd, e3, ef))
    assert np.isfinite(got).all()
    assert e3 <= 1.5 * ef + 2.0 ** -24, (e3, ef)


def test_plain_gemm_form_agrees():
    """Without the fp32 start term the layer is test_split_f16_cpu's
    gemm_f16_x3 on the same scales, bit for bit."""
    w, h = 19, 17
    rng = np.random.default_rng(5)
    W1 = (0.05 * rng.standard_normal((K, N1))).astype(np.float32)
    W1[80] = 0.0
    x = samples(rng, w, h)["plain"]
    ew, ex = w_scale(W1), scale_exp(np.abs(x).max(), 14)
    od = tap_order()
    ref = gemm_f16_x3(W1[od].T.copy(), ew, windows(x, w, h)[od].copy(), ex)
    got, _ = layer1_as_built(W1, np.zeros(N1, np.float32), x, w, h, ew)
    assert np.array_equal(got, np.maximum(ref, np.float32(0)))


@pytest.mark.parametrize("sd", [1e-3, 0.05])
def test_zero_sample_is_relu_b1(sd):
    w, h = 19, 17
    rng = np.random.default_rng(8)
    W1 = (sd * rng.standard_normal((K, N1))).astype(np.float32)
    B1 = (sd * rng.standard_normal(N1)).astype(np.float32)
    got, _ = layer1_as_built(W1, B1, np.zeros(w * h, np.float32), w, h, w_scale(W1))
    assert np.array_equal(got, np.broadcast_to(np.maximum(B1, np.float32(0))[:, None], got.shape))


@pytest.mark.parametrize("ew", [E_MIN, E_MAX])
@pytest.mark.parametrize("ex", [E_MIN, E_MAX])
def test_constants_finite_at_the_ends(ew, ex):
    """Every pair of exponents at the ends of [kScaleMin, kScaleMax]: 2^ew,
    2^ex and the two unscale steps are finite, non-zero fp32 values whose
    product is 2^-(ew + ex)."""
    sw, sx = pow2(ew), pow2(ex)
    eu = -(ew + ex)
    eu1 = min(eu, 127)
    u1, u2 = pow2(eu1), pow2(eu - eu1)
    for c in (sw, sx, u1, u2):
        assert np.isfinite(c) and c > 0 and c.dtype == np.float32
    assert np.float64(u1) * np.float64(u2) * np.float64(sw) * np.float64(sx) == 1.0


def test_constants_over_all_exponents():
    for ew in range(E_MIN, E_MAX + 1):
        for ex in (E_MIN, -114, -20, 0, 17, E_MAX):
            eu = -(ew + ex)
            eu1 = min(eu, 127)
            assert -126 <= eu1 <= 127 and 0 <= eu - eu1 <= 127


def a1_bound(W1, B1, x):
    """The kernel's bound on |A1| of a sample, in fp32 as it forms it."""
    wnorm = np.abs(W1).sum(axis=0, dtype=np.float32).max()
    return np.float32(np.float32(np.abs(x).max() * wnorm) + np.abs(B1).max())


def layer2_as_built(A1, W2, B2, bound):
    """A1 [64, P] (fp32, after the ReLU), W2 [64, 32] (channel-major, as the
    parameters lie), B2 [32] -> A2 [32, P] after the ReLU."""
    ew2, ea = scale_exp(np.abs(W2).max(), 14), scale_exp(bound, 14)
    b2 = ((B2 * pow2(ew2)).astype(np.float32) * pow2(ea)).astype(np.float32)
    acc = np.zeros((N2, A1.shape[1]), np.float32)
    a0, a1 = (p.astype(np.float64) for p in split_f16(W2.T.copy(), ew2))
    b0, b1 = (p.astype(np.float64) for p in split_f16(A1, ea))
    assert all(np.isfinite(p).all() for p in (a0, a1, b0, b1))
    assert np.abs(b0).max() <= 2.0 ** 15
    acc = mfma_chain(acc, [(a1, b0), (a0, b1), (a0, b0)], N1)
    acc = (acc + b2[:, None]).astype(np.float32)
    ev = -(ea + ew2)
    ev1 = min(ev, 127)
    with np.errstate(over="ignore"):
        acc = (acc * pow2(ev1)).astype(np.float32)
        if ev != ev1:
            acc = (acc * pow2(ev - ev1)).astype(np.float32)
    return np.maximum(acc, np.float32(0))


def layer2_fp32_chain(A1, W2, B2):
    acc = np.broadcast_to(B2[:, None], (N2, A1.shape[1])).astype(np.float32)
    A, B = W2.T.astype(np.float64), A1.astype(np.float64)
    for k in range(0, N1, 2):
        acc = (acc.astype(np.float64) + A[:, k:k + 2] @ B[k:k + 2]).astype(np.float32)
    return np.maximum(acc, np.float32(0))


@pytest.mark.parametrize("sd", [1e-3, 0.05])
@pytest.mark.parametrize("kind", ["plain", "x2^12", "x2^-30", "spike"])
def test_layer2_as_built_within_fp32_error(kind, sd):
    w, h = 19, 17
    rng = np.random.default_rng(78)
    W1 = (sd * rng.standard_normal((K, N1))).astype(np.float32)
    B1 = (sd * rng.standard_normal(N1)).astype(np.float32)
    W2 = (sd * rng.standard_normal((N1, N2))).astype(np.float32)
    B2 = (sd * rng.standard_normal(N2)).astype(np.float32)
    x = samples(rng, w, h)[kind]
    A1, _ = layer1_as_built(W1, B1, x, w, h, w_scale(W1))
    bound = a1_bound(W1, B1, x)
    slack = np.log2(float(bound) / float(A1.max()))
    assert 0 <= slack <= 8, slack  # a bound, and within the 2^8 the form tolerates
    ref = np.maximum(W2.astype(np.float64).T @ A1.astype(np.float64) + B2.astype(np.float64)[:, None], 0.0)
    got = layer2_as_built(A1, W2, B2, bound)
    e3, ef = normwise(got, ref), normwise(layer2_fp32_chain(A1, W2, B2), ref)
    print("layer 2 %s sd=%g: f16 x3 as built %.3e  fp32 chain %.3e  (bound 2^%.2f above max A1)" % (kind, sd, e3, ef, slack))
    assert np.isfinite(got).all()
    assert e3 <= 1.5 * ef + 2.0 ** -24, (e3, ef)


def test_zero_sample_layer2():
    """The zero sample: the bound is max |B1|, A1 = relu(B1), and layer 2 of
    that is within the same rule."""
    rng = np.random.default_rng(9)
    W1 = (0.05 * rng.standard_normal((K, N1))).astype(np.float32)
    B1 = (0.05 * rng.standard_normal(N1)).astype(np.float32)
    W2 = (0.05 * rng.standard_normal((N1, N2))).astype(np.float32)
    B2 = (0.05 * rng.standard_normal(N2)).astype(np.float32)
    x = np.zeros(19 * 17, np.float32)
    assert a1_bound(W1, B1, x) == np.abs(B1).max()
    A1, _ = layer1_as_built(W1, B1, x, 19, 17, w_scale(W1))
    ref = np.maximum(W2.astype(np.float64).T @ A1.astype(np.float64) + B2.astype(np.float64)[:, None], 0.0)
    got = layer2_as_built(A1, W2, B2, a1_bound(W1, B1, x))
    assert normwise(got, ref) <= 1.5 * normwise(layer2_fp32_chain(A1, W2, B2), ref) + 2.0 ** -24
