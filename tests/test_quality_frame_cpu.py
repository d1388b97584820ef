"""CPU checks of srcnn_quality_frame's yardstick (tests/quality_frame_ref.py)
and of its host-side argument checks.

The GPU test's SSIM bounds are 4 x the largest error of the two float32
restatements of DESIGN.md 17.1 (a filter tap as a rounded product plus an add,
or as one fma) against float64, on the GPU test's own inputs, rounded up to two
digits.  Measured here on every run (numpy, this CPU): 9.83e-7 on the
structured pairs (bound 4.0e-6), 4.13e-5 on the flat ones (bound 1.7e-4).  The
bounds still tell the spec from its near misses: sigma = 1.4 moves every
structured case's SSIM by at least 8.9e-4, a shift off by one (x / 2k) by at
least 4.5e-4, both more than ten bounds; the reading x * 255 / peak in place of
x / k moves the cases listed in PEAK_READING_CASES by 4.4e-5 to 1.8e-4, and is
no different at 8 bits.  The mse values are integer sums: exact, no bound."""
import numpy as np
import pytest

import quality_frame_ref as F
import quality_ref as Q

CASES = {c[0]: c for c in F.cases()}
FLAT = {c[0]: c for c in F.flat_cases()}

# the structured cases (of 54 above 8 bits) that x * 255 / peak moves by more
# than ten bounds; the others it moves by 9e-7 to 4.2e-5
PEAK_READING_CASES = [
    "11x11_12b_420", "11x11_16b_420", "11x11_16b_422", "11x11_16b_444", "12x13_12b_422", "12x13_16b_444",
    "42x42_12b_420", "42x42_12b_422", "42x42_16b_422", "42x42_16b_444", "43x43_12b_422", "43x43_16b_420",
    "75x59_10b_420", "75x59_10b_444", "75x59_12b_420", "75x59_12b_422", "75x59_12b_444", "75x59_16b_420",
    "75x59_16b_444", "135x37_10b_420", "135x37_12b_420", "135x37_12b_422", "135x37_16b_420", "135x37_16b_444",
]


def restatement_error(case):
    name, A, B, bits, cx, cy, k = case
    s64 = F.ssim(A[0], B[0], bits, k)
    return max(abs(F.ssim(A[0], B[0], bits, k, np.float32, fused=f) - s64) for f in (False, True))


def test_case_set():
    assert len(CASES) == len(Q.SHAPES) * len(F.BITS) * 3 and len(FLAT) == 2 * len(F.BITS)
    odd_420 = [n for n, c in CASES.items() if n.endswith("420") and c[1][0].shape[0] % 2 and c[1][0].shape[1] % 2]
    assert len(odd_420) >= 3 * len(F.BITS)
    for name, A, B, bits, cx, cy, k in list(CASES.values()) + list(FLAT.values()):
        h, w = A[0].shape
        assert A[1].shape == A[2].shape == B[1].shape == F.chroma_shape(w, h, cx, cy)
        for p in A + B:
            assert p.min() >= 0 and p.max() <= 2 ** bits - 1
        assert all(S > 0 for S, _ in F.sq_sums(A, B, cx, cy, k)), name


def test_bounds_are_four_times_the_restatement_error():
    worst = max(restatement_error(c) for c in CASES.values())
    worst_flat = max(restatement_error(c) for c in FLAT.values())
    print("float32 restatements against float64: structured %.3e (bound %.1e), flat %.3e (bound %.1e)" % (
        worst, F.SSIM_ATOL, worst_flat, F.SSIM_ATOL_FLAT))
    assert worst <= F.SSIM_ATOL / 4 and worst_flat <= F.SSIM_ATOL_FLAT / 4
    # ... and not looser than two digits of rounding up
    assert F.SSIM_ATOL <= 4 * worst * 1.1 and F.SSIM_ATOL_FLAT <= 4 * worst_flat * 1.1


@pytest.mark.parametrize("name", list(CASES))
def test_wrong_readings_are_told_apart(name):
    _, A, B, bits, cx, cy, k = CASES[name]
    s64 = F.ssim(A[0], B[0], bits, k)
    assert abs(F.ssim(A[0], B[0], bits, k, sigma=1.4) - s64) >= 10 * F.SSIM_ATOL
    if bits > 8:
        assert abs(F.ssim(A[0], B[0], bits, k, reading="2k") - s64) >= 10 * F.SSIM_ATOL
    moved = abs(F.ssim(A[0], B[0], bits, k, reading="peak") - s64)
    if name in PEAK_READING_CASES:
        assert moved >= 10 * F.SSIM_ATOL, moved
    if bits == 8:
        assert moved == 0.0


def test_peak_reading_cases_cover_the_deep_formats():
    assert set(PEAK_READING_CASES) <= set(CASES)
    for bits in (10, 12, 16):
        assert any("_%db_" % bits in n for n in PEAK_READING_CASES)


def test_luma_input_is_exact_in_fp32():
    """x / k is exact in fp32 and below 256 at every depth"""
    for bits in F.BITS:
        x = np.arange(2 ** bits, dtype=np.int64)
        y32, y64 = F.luma8(x, bits, np.float32), F.luma8(x, bits, np.float64)
        assert y32.dtype == np.float32 and np.array_equal(y32.astype(np.float64), y64) and y64.max() < 256
        assert np.array_equal(y64 * 2 ** (bits - 8), x)


def test_integer_mse_against_a_loop():
    name, A, B, bits, cx, cy, k = CASES["12x13_10b_420"]
    sums, res = F.quality_frame(A, B, bits, cx, cy, k)
    sx, sy = -(-k // cx), -(-k // cy)
    assert (sx, sy) == (2, 2)
    for p, (dx, dy) in enumerate(((k, k), (sx, sy), (sx, sy))):
        a, b = A[p], B[p]
        S = N = 0
        for r in range(dy, a.shape[0] - dy):
            for c in range(dx, a.shape[1] - dx):
                S += (int(a[r, c]) - int(b[r, c])) ** 2
                N += 1
        assert (S, N) == sums[p]
        assert res[(0, 3, 5)[p]] == S / N
    assert res[7] == F.psnr(2 ** bits - 1, F.mse_all_of(sums))
    same, r0 = F.quality_frame(A, A, bits, cx, cy, k)
    assert r0 == [0.0, float("inf"), 1.0, 0.0, float("inf"), 0.0, float("inf"), float("inf")]


@pytest.mark.parametrize("bits,msb", [(8, 0), (10, 0), (10, 1), (12, 1), (16, 0), (16, 1)])
@pytest.mark.parametrize("layout", [F.YUV_PLANAR, F.YUV_SEMIPLANAR])
@pytest.mark.parametrize("sub", ["420", "422", "444"])
def test_packers_round_trip(bits, msb, layout, sub):
    cx, cy = F.SUBSAMPLINGS[sub]
    rng = np.random.default_rng(bits + msb + layout)
    A = F.make_frame(rng, 19, 13, cx, cy, bits)
    for extra in ((0, 0), (5, 3)):
        p = F.pack(A, bits, msb, layout, cx, cy, extra[0], extra[1], rng)
        B = 1 if bits == 8 else 2
        nch = 2 if layout == F.YUV_SEMIPLANAR else 1
        assert p.pitch_y == (19 + extra[0]) * B and p.pitch_c == (A[1].shape[1] * nch + extra[1]) * B
        assert p.y.size == p.pitch_y * 13 and p.u.size == p.pitch_c * A[1].shape[0]
        assert (p.v is None) == (layout == F.YUV_SEMIPLANAR)
        for got, want in zip(F.unpack(p), A):
            assert np.array_equal(got, want)
    if bits > 8:  # the code sits where msb says
        word = int(np.ascontiguousarray(p.y[:2]).view("<u2")[0])
        assert word == int(A[0][0, 0]) << ((16 - bits) if msb else 0)


@pytest.fixture(scope="module")
def S():
    import srcnn_amd
    return srcnn_amd


def test_a_valid_call_passes_the_checks(S):
    """base_args() itself is valid: one byte less of workspace is the only
    complaint, so every INVALID mutation fails for its own reason"""
    g = F.base_args(S)
    assert g["ws_bytes"] > 0 and g["ws_bytes"] % 256 == 0
    g["ws_bytes"] -= 1
    with pytest.raises(S.SrcnnError) as e:
        F.call(S, g)
    assert e.value.code == S.ERR_WORKSPACE
    g = F.base_args(S)
    F._semi(g)
    g["ws_bytes"] -= 1
    with pytest.raises(S.SrcnnError) as e:
        F.call(S, g)
    assert e.value.code == S.ERR_WORKSPACE


@pytest.mark.parametrize("name", list(F.INVALID))
def test_validation_errors_without_gpu(S, name):
    g = F.base_args(S)
    F.INVALID[name](g)
    with pytest.raises(S.SrcnnError) as e:
        F.call(S, g)
    assert e.value.code == S.ERR_INVALID, S.last_error()
    assert S.last_error().startswith("quality_frame: ")


def test_workspace_query(S):
    q = S.quality_frame_workspace_bytes
    # 3840 x 2160 4:2:0: 120 x 68 luma tiles of two words, 8 x 68 chroma tiles of one word and two planes
    assert q(3840, 2160, 2, 2, 0) == 256 * -(-(16 * (120 * 68 + 8 * 68)) // 256)
    assert q(11, 11, 1, 1, 0) == 256 and q(17, 17, 2, 2, 3) == 256
    for bad in ((10, 11, 2, 2, 0), (11, 10, 2, 2, 0), (16, 17, 2, 2, 3), (17, 17, 2, 2, 0x80000003),
                (17, 17, 3, 1, 0), (17, 17, 1, 2, 0), (17, 17, 0, 0, 0), (46341, 46341, 2, 2, 0), (0, 0, 2, 2, 0)):
        assert q(*bad) == 0, bad
