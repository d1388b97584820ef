"""The two-part fp16 split product (split.hpp: split8_h, mma_x3_h) emulated in
numpy beside the six-product bf16 form and an fp32 chain, against fp64.

An fp32 value scaled by a power of two, xs = x 2^e, splits into p0 =
rne16(xs) and p1 = rne16(xs - p0) (22-23 significant bits together); a
product keeps p0 q0, p0 q1 and p1 q0, one v_mfma_f32_32x32x16_f16 each.  The
emulation rounds the parts as the hardware does (numpy's float16 is IEEE
binary16 with subnormals, round to nearest even), forms the part products of
a 16-slot k-step exactly (in fp64: 11 x 11 bits and 16 terms fit) and rounds
once per MFMA into the fp32 accumulator, small terms first.

The criterion is the project's own (test_split_arith_within_fp32_error): the
form's normwise error against fp64 is at most 1.5 x the fp32 chain's on the
same data.
"""
import numpy as np
import pytest

F16_TOP = 15  # a scale maps its bound to 2^15 (fp16's largest finite: 65504)
E_MIN, E_MAX = -126, 60  # a scale's exponent: 2^e is a normal fp32, whatever the maximum (non-finite included)
ACC_TOP = 2.0 ** 100  # the accumulators' bound never passes this (fp32: 2^128)


def normwise(a, ref):
    return float(np.linalg.norm(a.astype(np.float64) - ref) / np.linalg.norm(ref))


def bf16_rne(x):
    u = x.astype(np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def split_bf16(x):
    p0 = bf16_rne(x)
    r = (x - p0).astype(np.float32)
    p1 = bf16_rne(r)
    p2 = bf16_rne((r - p1).astype(np.float32))
    return [p.astype(np.float64) for p in (p0, p1, p2)]


def split_f16(x, e):
    """The parts of x 2^e as fp16 (the residual is exact in fp32)."""
    xs = np.ldexp(x.astype(np.float32), e).astype(np.float32)
    p0 = xs.astype(np.float16)
    p1 = (xs - p0.astype(np.float32)).astype(np.float32).astype(np.float16)
    return p0, p1


def mfma_chain(acc, terms, K):
    """acc (fp32) += every term (a_part [M, K], b_part [K, N], fp64 values) per
    16-slot k-step, one fp32 rounding per MFMA, in the terms' order."""
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


def gemm_bf16_x6(A, B):
    a, b = split_bf16(A), split_bf16(B)
    terms = [(a[2], b[0]), (a[1], b[1]), (a[0], b[2]), (a[1], b[0]), (a[0], b[1]), (a[0], b[0])]
    return mfma_chain(np.zeros((A.shape[0], B.shape[1]), np.float32), terms, A.shape[1])


def x3_terms(A, ea, B, eb):
    a0, a1 = (p.astype(np.float64) for p in split_f16(A, ea))
    b0, b1 = (p.astype(np.float64) for p in split_f16(B, eb))
    return [(a1, b0), (a0, b1), (a0, b0)]  # small terms first


def gemm_f16_x3(A, ea, B, eb):
    acc = mfma_chain(np.zeros((A.shape[0], B.shape[1]), np.float32), x3_terms(A, ea, B, eb), A.shape[1])
    return np.ldexp(acc, -(ea + eb))


def scale_exp(bound, lo):
    """e with bound 2^e in [2^lo, 2^(lo+1)); 0 for a zero bound; clamped, and
    finite for a non-finite bound."""
    if not np.isfinite(bound):
        return E_MIN
    if bound == 0.0:
        return 0
    m, ex = np.frexp(np.float32(bound))  # bound = m 2^ex, m in [0.5, 1)
    return int(np.clip(lo + 1 - int(ex), E_MIN, E_MAX))


def x_scale(X):
    return scale_exp(np.abs(X).max(), F16_TOP - 1)  # the maximum into [2^14, 2^15)


def d_scale(bound):
    # the bound to 2^15 at most: a bound of exactly 2^k lands on 2^15, any
    # other below it
    e = scale_exp(bound, F16_TOP - 1)
    if np.isfinite(bound) and bound > 0 and np.frexp(np.float32(bound))[0] == 0.5 and e < E_MAX:
        e += 1
    return e


def gaussian(rng, K, sa=1.0, sb=1.0):
    return ((sa * rng.standard_normal((64, K))).astype(np.float32),
            (sb * rng.standard_normal((K, 32))).astype(np.float32))


def delta_like(rng, K, mag=1e-6):
    """delta1-like rows (lognormal sigma = 3 magnitudes, random signs, half of
    them zeroed by relu') against X-like windows (pixels in [0, 1))."""
    A = mag * rng.lognormal(0.0, 3.0, (64, K)) * rng.choice([-1.0, 1.0], (64, K))
    A[rng.random((64, K)) < 0.5] = 0.0
    return A.astype(np.float32), rng.random((K, 32)).astype(np.float32)


DATA = {
    "gauss": lambda rng, K: gaussian(rng, K),
    "gauss_1e-3x1e-5": lambda rng, K: gaussian(rng, K, 1e-3, 1e-5),
    "delta": lambda rng, K: delta_like(rng, K),
}


@pytest.mark.parametrize("K", [96, 640])
@pytest.mark.parametrize("short", [0, 7])
@pytest.mark.parametrize("data", sorted(DATA))
def test_f16_x3_within_fp32_error(data, K, short):
    """short: the A operand's scale is 2^short smaller than the exact one (the
    slack of a bound over the true maximum)."""
    rng = np.random.default_rng(1234)
    A, B = DATA[data](rng, K)
    ref = A.astype(np.float64) @ B.astype(np.float64)
    ea, eb = d_scale(np.abs(A).max()) - short, x_scale(B)
    parts = split_f16(A, ea) + split_f16(B, eb)
    assert all(np.isfinite(p.astype(np.float32)).all() for p in parts)
    e3 = normwise(gemm_f16_x3(A, ea, B, eb), ref)
    e6 = normwise(gemm_bf16_x6(A, B), ref)
    ef = normwise(gemm_f32_chain(A, B), ref)
    print("%s K=%d short=%d: f16 x3 %.3e  bf16 x6 %.3e  fp32 chain %.3e" % (data, K, short, e3, e6, ef))
    assert e6 <= 1.5 * ef + 2.0 ** -24
    assert e3 <= 1.5 * ef + 2.0 ** -24, (e3, ef)


@pytest.mark.parametrize("bound", [1e-30, 3e-7, 1.0, 2.0 ** -20, 2.0 ** 20, 65504.0, 1e30, 3e38])
def test_parts_finite_up_to_the_bound(bound):
    """A value at its bound (and the largest X) lands at most on 2^15, and a
    scale never makes a part non-finite."""
    rng = np.random.default_rng(5)
    b = np.float32(bound)
    x = np.concatenate([np.array([b, -b], np.float32), (b * (2 * rng.random(1000) - 1)).astype(np.float32)])
    for e in (d_scale(b), x_scale(x)):
        p0, p1 = split_f16(x, e)
        assert np.isfinite(p0.astype(np.float32)).all() and np.isfinite(p1.astype(np.float32)).all()
        assert np.abs(p0.astype(np.float64)).max() <= 2.0 ** F16_TOP
    if E_MIN < d_scale(b) < E_MAX:
        assert 2.0 ** (F16_TOP - 1) < np.ldexp(np.float64(b), d_scale(b)) <= 2.0 ** F16_TOP
        assert 2.0 ** (F16_TOP - 1) <= np.ldexp(np.float64(b), x_scale(x)) < 2.0 ** F16_TOP


def test_scale_of_odd_bounds():
    assert x_scale(np.zeros(4, np.float32)) == 0 and d_scale(np.float32(0)) == 0
    for bad in (np.inf, -np.inf, np.nan):
        assert E_MIN <= scale_exp(np.float32(bad), 14) <= E_MAX
    assert d_scale(np.float32(1e-45)) == E_MAX  # a subnormal bound


class Gw1Accumulator:
    """The kernel's bookkeeping restated: the accumulators hold 2^eacc x the
    sum.  A sample comes with its own scales e1 (delta1, from a bound) and ex
    (X, from its maximum); when e1 + ex differs from eacc the difference goes
    into the sample's X scale if the scaled maximum of X stays in [2^8, 2^15],
    else the accumulators are multiplied by the exact power of two and eacc
    moves.  A move up is capped so that the accumulators' bound stays below
    ACC_TOP (the sample then takes a smaller delta1 scale).  (d1x6.hpp moves
    to 2^3 below the sample's own exponent, the middle of the window, and
    caps a sample's scale at 2^70 above the largest sample's seen; the bias
    column has an exponent of its own, its constant 2^k taking up to 2^-14 ..
    2^15.  The arithmetic checked here is the same.)"""

    def __init__(self, M, N):
        self.acc = np.zeros((M, N), np.float32)
        self.eacc = None
        self.bound = 0.0  # >= max |acc|
        self.moves = self.folds = 0

    def add(self, D, d_bound, X):
        e1, ex = d_scale(d_bound), x_scale(X)
        xmax = float(np.abs(X).max())
        if self.eacc is None:
            self.eacc = e1 + ex
        diff = self.eacc - (e1 + ex)
        if diff != 0:
            if xmax > 0 and 2.0 ** 8 <= np.ldexp(xmax, ex + diff) <= 2.0 ** F16_TOP:
                ex += diff
                self.folds += 1
            else:
                up = -diff
                if up > 0 and self.bound > 0:
                    room = int(np.floor(np.log2(ACC_TOP / self.bound)))
                    if up > room:  # the rest comes off delta1's scale
                        e1 -= up - room
                        up = room
                self.acc = np.ldexp(self.acc, up).astype(np.float32)  # exact: a power of two
                self.bound = np.ldexp(self.bound, up)
                self.eacc += up
                self.moves += 1
        assert e1 + ex == self.eacc
        terms = x3_terms(D, e1, X, ex)
        assert all(np.isfinite(t).all() for pair in terms for t in pair)
        self.acc = mfma_chain(self.acc, terms, D.shape[1])
        self.bound += D.shape[1] * 2.0 ** (2 * F16_TOP)
        assert np.isfinite(self.acc).all() and self.bound <= ACC_TOP * 2.0 ** 40

    def result(self):
        return np.ldexp(self.acc, -self.eacc) if self.eacc is not None else self.acc


@pytest.mark.parametrize("slack", [1.0, 2.0 ** 7])
def test_scale_bookkeeping_over_samples(slack):
    """Samples whose magnitudes jump by 2^10 both ways, one of them all zero:
    the scaled accumulation gives the plain sum to the same bound.  slack: the
    delta1 bound over the true maximum."""
    rng = np.random.default_rng(99)
    K = 96
    jumps = [0, 10, 0, -10, 0, None, 10, 20, 10, 0, -10, -20, 3, 0]
    acc = Gw1Accumulator(64, 32)
    As, Bs = [], []
    for jp in jumps:
        A, B = delta_like(rng, K)
        if jp is None:
            A[:] = 0.0
        else:
            A = np.ldexp(A, jp)
        if len(As) % 3 == 2:
            B = np.ldexp(B, 4)  # X's own scale moves too
        acc.add(A, np.float32(np.abs(A).max() * slack), B)
        As.append(A)
        Bs.append(B)
    assert acc.moves >= 2 and acc.folds >= 1, (acc.moves, acc.folds)
    Acat, Bcat = np.concatenate(As, axis=1), np.concatenate(Bs, axis=0)
    ref = Acat.astype(np.float64) @ Bcat.astype(np.float64)
    e3, ef = normwise(acc.result(), ref), normwise(gemm_f32_chain(Acat, Bcat), ref)
    print("samples, slack %g: f16 x3 %.3e  fp32 chain %.3e  (%d moves, %d folds)" % (slack, e3, ef, acc.moves, acc.folds))
    assert e3 <= 1.5 * ef + 2.0 ** -24, (e3, ef)


def test_far_jump_up_cannot_overflow():
    """A sample 2^120 below its predecessor: the move up is capped."""
    rng = np.random.default_rng(3)
    acc = Gw1Accumulator(64, 32)
    A, B = gaussian(rng, 32)
    acc.add(np.ldexp(A, 40), np.float32(np.abs(A).max() * 2.0 ** 40), B)
    acc.add(np.ldexp(A, -80), np.float32(np.abs(A).max() * 2.0 ** -80), B)
    ref = (np.ldexp(A, 40).astype(np.float64) + np.ldexp(A, -80).astype(np.float64)) @ B.astype(np.float64)
    assert np.isfinite(acc.result()).all()
    assert normwise(acc.result(), ref) <= 1e-6
