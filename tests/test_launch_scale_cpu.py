"""gW1 on two-part fp16 split products with ONE pair of scales for a whole
launch (d1x6.hpp, the delta3 forms), restated in numpy.

Every sample's delta1 is scaled by 2^e1 and its X by 2^ex, with e1 from a bound
on the largest |delta1| of the launch and ex from the largest |X| of the
launch; the accumulators hold 2^(e1 + ex) x the sum over all samples and are
unscaled once.  A power of two leaves an operand's two fp16 parts as they are
while none is subnormal; a sample far below the launch's largest loses low
bits, at a size far below the fp32 rounding of the sum that the large samples
dominate.

The parts are rounded as the hardware rounds them (numpy's float16 is IEEE
binary16 with subnormals, round to nearest even), the part products of a
16-slot k-step are formed exactly (fp64) and rounded once per MFMA into the
fp32 accumulator, small terms first.  The criterion is the one
tests/test_split_f16_cpu.py states for the per-sample form: the normwise error
against the fp64 sum is at most 1.5 x that of an fp32 MFMA chain on the same
data (+ 2^-24).
"""
import numpy as np
import pytest

F16_TOP = 15            # a scale maps its bound into [2^14, 2^15]
E_MIN, E_MAX = -126, 60  # a scale's exponent: 2^e is a normal fp32


def normwise(a, ref):
    return float(np.linalg.norm(a.astype(np.float64) - ref) / np.linalg.norm(ref))


def scale_exp(bound):
    """e with bound 2^e in [2^14, 2^15); 0 for a zero bound; clamped."""
    if not np.isfinite(bound):
        return E_MIN
    if bound == 0.0:
        return 0
    _, ex = np.frexp(np.float32(bound))  # bound = m 2^ex, m in [0.5, 1)
    return int(np.clip(F16_TOP - int(ex), E_MIN, E_MAX))


def split_f16(x, e):
    """The two fp16 parts of x 2^e (the residual is exact in fp32)."""
    xs = np.ldexp(x.astype(np.float32), e).astype(np.float32)
    p0 = xs.astype(np.float16)
    p1 = (xs - p0.astype(np.float32)).astype(np.float32).astype(np.float16)
    return p0.astype(np.float64), p1.astype(np.float64)


def mfma_chain(acc, terms, K):
    """acc (fp32) += every term (a_part [M, K], b_part [K, N]) per 16-slot
    k-step, one fp32 rounding per MFMA, in the terms' order."""
    for k in range(0, K, 16):
        for a, b in terms:
            acc = (acc.astype(np.float64) + a[:, k:k + 16] @ b[k:k + 16]).astype(np.float32)
    return acc


def gemm_f32_chain(A, B):
    """v_mfma_f32_32x32x2_f32: two exact products and one rounding per MFMA."""
    acc = np.zeros((A.shape[0], B.shape[1]), np.float32)
    A64, B64 = A.astype(np.float64), B.astype(np.float64)
    for k in range(0, A.shape[1], 2):
        acc = (acc.astype(np.float64) + A64[:, k:k + 2] @ B64[k:k + 2]).astype(np.float32)
    return acc


def launch_sum(Ds, Xs, slack=1.0):
    """sum over the samples of D @ X under one scale pair; -> (sum, e1, ex)."""
    d_bound = np.float32(max(float(np.abs(D).max()) for D in Ds) * slack)
    x_max = np.float32(max(float(np.abs(X).max()) for X in Xs))
    e1 = scale_exp(d_bound) if d_bound > 0 else 0
    ex = scale_exp(x_max) if x_max > 0 else 0
    acc = np.zeros((Ds[0].shape[0], Xs[0].shape[1]), np.float32)
    for D, X in zip(Ds, Xs):
        d0, d1 = split_f16(D, e1)
        x0, x1 = split_f16(X, ex)
        parts = (d0, d1, x0, x1)
        assert all(np.isfinite(p).all() and np.abs(p).max() <= 2.0 ** F16_TOP for p in parts)
        acc = mfma_chain(acc, [(d1, x0), (d0, x1), (d0, x0)], D.shape[1])  # small terms first
        assert np.isfinite(acc).all()
    return np.ldexp(acc, -(e1 + ex)), e1, ex


def delta_like(rng, K, mag=1e-6):
    """delta1-like rows (lognormal sigma = 3 magnitudes, random signs, half of
    them zeroed by relu') against X-like windows (pixels in [0, 1))."""
    A = mag * rng.lognormal(0.0, 3.0, (64, K)) * rng.choice([-1.0, 1.0], (64, K))
    A[rng.random((64, K)) < 0.5] = 0.0
    return A.astype(np.float32), rng.random((K, 32)).astype(np.float32)


def samples(rng, d_jumps, x_jumps, K=96):
    """One (delta1, X) pair per entry: delta1 x 2^jump (None: all zero), X x
    2^jump."""
    Ds, Xs = [], []
    for dj, xj in zip(d_jumps, x_jumps):
        D, X = delta_like(rng, K)
        D = np.zeros_like(D) if dj is None else np.ldexp(D, dj)
        Ds.append(D.astype(np.float32))
        Xs.append(np.ldexp(X, xj).astype(np.float32))
    return Ds, Xs


def check(Ds, Xs, slack, what):
    Dcat, Xcat = np.concatenate(Ds, axis=1), np.concatenate(Xs, axis=0)
    ref = Dcat.astype(np.float64) @ Xcat.astype(np.float64)
    got, e1, ex = launch_sum(Ds, Xs, slack)
    e3, ef = normwise(got, ref), normwise(gemm_f32_chain(Dcat, Xcat), ref)
    print("%s, slack %g: e1 %d ex %d: f16 x3 %.3e  fp32 chain %.3e" % (what, slack, e1, ex, e3, ef))
    assert e3 <= 1.5 * ef + 2.0 ** -24, (what, e3, ef)


D_JUMPS = {
    "level": [0] * 8,
    "up_down_10": [0, 10, 0, -10, 0, None, 10, 0],
    "up_down_20": [0, 10, 0, -10, 0, None, 10, 20, 10, 0, -10, -20, 3, 0],
    "one_outlier_20": [0, 0, 0, 20, 0, 0, None, 0],
    "one_tiny_20": [0, 0, 0, -20, 0, 0, None, 0],
}


@pytest.mark.parametrize("slack", [1.0, 2.0 ** 7])
@pytest.mark.parametrize("name", sorted(D_JUMPS))
def test_one_scale_pair_delta_jumps(name, slack):
    """delta1's magnitude jumps by 0, +-10 and +-20 binary orders between the
    samples of a launch, one sample all zero.  slack: the bound over the true
    maximum of |delta1|."""
    rng = np.random.default_rng(99)
    dj = D_JUMPS[name]
    Ds, Xs = samples(rng, dj, [0] * len(dj))
    check(Ds, Xs, slack, name)


X_JUMPS = [
    # tiny samples beside normal ones, delta1 level or jumping the same way:
    # what a tiny sample loses is tiny in the sum
    ([0, -20, 0, -20, 0, 0], [0] * 6),
    ([-20, -20, 0, -20, -20, -20], [0] * 6),
    ([0, 10, -10, 20, 0, -20], [0] * 6),
    ([0, 10, -10, 20, 0, -20], [0, 10, -10, 20, None, -20]),
]


@pytest.mark.parametrize("xj,dj", X_JUMPS, ids=["tiny", "one_normal", "mixed", "with_delta"])
def test_one_scale_pair_x_jumps(xj, dj):
    """X's magnitude jumps too."""
    rng = np.random.default_rng(7)
    Ds, Xs = samples(rng, dj, xj)
    check(Ds, Xs, 1.0, "x %s d %s" % (xj, dj))


def test_what_one_scale_pair_does_not_serve():
    """The limit, stated: the two operands' ranges are not traded against each
    other any more.  A sample that is small in X and large in delta1 by the
    same factor has products of the other samples' size, and what its small
    operand loses under the launch's scale shows in the sum: with X against
    delta1 by 2^8 ([0, 8, -8, 8, 0, -8] against [0, -8, 8, -8, None, 8] on this
    file's data) the error is 2.7e-6 where the fp32 chain has 2.1e-7, and a
    sample whose X lies 2^40 below the launch's largest has no fp16 part left
    at all (2^15 2^-40 < 2^-24, the smallest subnormal).  The per-sample scales
    served both.  Training tiles (pixels in [0, 1], every sample's maximum near
    1) are far from either."""
    rng = np.random.default_rng(7)
    Ds, Xs = samples(rng, [0, 40], [0, -40])
    _, e1, ex = launch_sum(Ds, Xs)
    assert Xs[1].any() and not any(p.any() for p in split_f16(Xs[1], ex))


def test_all_zero_launch():
    """A zero bound (every delta1 zero) and zero X take finite scales and give
    an exact zero."""
    rng = np.random.default_rng(3)
    Ds, Xs = samples(rng, [None] * 3, [0] * 3)
    got, e1, ex = launch_sum(Ds, Xs)
    assert e1 == 0 and np.isfinite(got).all() and not got.any()
    Ds, Xs = samples(rng, [0] * 3, [0] * 3)
    got, e1, ex = launch_sum(Ds, [np.zeros_like(X) for X in Xs])
    assert ex == 0 and np.isfinite(got).all() and not got.any()


def test_largest_sample_keeps_its_parts():
    """The launch's scale pair is the largest sample's own: its parts, and so
    its part products, are those of the per-sample form."""
    rng = np.random.default_rng(11)
    Ds, Xs = samples(rng, [0, -10, -20], [0, 0, 0])
    _, e1, ex = launch_sum(Ds, Xs)
    assert e1 == scale_exp(np.float32(np.abs(Ds[0]).max()))
    # a sample 2^10 below: the same parts up to the power of two, where none is subnormal
    own = scale_exp(np.float32(np.abs(Ds[1]).max()))
    p_launch, p_own = split_f16(Ds[1], e1), split_f16(Ds[1], own)
    normal = np.abs(p_launch[1]) >= 2.0 ** -14
    assert normal.any()
    for a, b in zip(p_launch, p_own):
        assert np.array_equal(np.ldexp(a[normal], own - e1), b[normal])
