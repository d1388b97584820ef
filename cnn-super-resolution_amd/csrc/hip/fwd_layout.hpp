// fwd_layout.hpp -- the geometry, limits and LDS layouts of the fused forward
// (forward_fused.hip), included inside namespace srcnn::fused.
//
// Host-and-device code without any device intrinsic: the plan (fwd_plan.hpp)
// takes the region heights and the dynamic-LDS byte count from here, the
// kernels size and carve their LDS by the same structs, so no extent is
// written twice.  tests/fwd_plan_check.cpp compiles this header and the plan
// for the host with the qualifiers defined away.  What schedules a kernel's
// instruction stream (kFwdPD, the window-sum steps) stays with that kernel.

// ---- the region (every kernel) ------------------------------------------------
constexpr int kFwdRW = 32;        // region width (one chunk per region row)
constexpr int kFwdGrid = 2048;  // grid cap (blocks)

constexpr int kFwdRhMax = 28;  // region rows (LDS partial-sum accumulator bound)
constexpr int kFwdXs = (kFwdRhMax + 12) * 40;  // input tile floats staged in LDS (f1 <= 9)

struct FwdGeom {
  int W, H;      // input frame
  int ow, oh;    // L1 / L2 output
  int rh;        // region rows
  int nrx, nry;  // regions per frame
  int batch;
};

// ---- fwd_l123 (fwd_l123.hpp): four static arrays -------------------------------
// Extents in floats.  (The kernel declares them as static __shared__ arrays of
// these extents, 16-B aligned where read as vectors; `bytes` is the code
// object's group segment.)
template <int F3>
struct FwdLds {
  static constexpr int kWaves = 4;
  static constexpr int EW = kFwdRW + F3 - 1;      // partial-sum window width
  static constexpr int EHM = kFwdRhMax + F3 - 1;  // ... and its rows at the tallest region
  // per-wave Q^T[tap][pixel + F3-1]: F3-1 zero columns either side, so a
  // window sum reads its F3 taps without bounds tests.  Row stride 52 floats
  // (5 x 52 = 4 mod 32): the window-sum items (dy, e) of one ds_read_b32 fall
  // in consecutive banks.  (Round 3 held Q as [pixel][tap] at stride 36 with
  // float4 stores; its window-sum reads were 4-way bank conflicted: same-box
  // A/B, 4 pairs, the frame 0.4-1.0% faster this way, profiles/r04_ab_fwdq.)
  static constexpr int QR = kFwdRW + 2 * (F3 - 1);
  static constexpr int QTS = 52;
  static_assert(QR <= QTS, "Q^T row");
  static constexpr int xs = kFwdXs;               // the region's input tile
  static constexpr int b2i = 2 * 16;              // L2 bias image [half][register]
  static constexpr int qs = kWaves * 32 * QTS;    // [wave][tap][QTS]
  static constexpr int accs = F3 * EHM * EW;      // [dy][partial row][partial col]
  static constexpr int bytes = (xs + b2i + qs + accs) * 4;
};

// fp32 region rows: the input tile (32 + f1 - 1) x (rh + f1 - 1) fits the LDS
// tile, a multiple of the 4 waves
constexpr int fwd_rh_f32(int f1) {
  const int fit = (kFwdXs / (kFwdRW + f1 - 1) - (f1 - 1)) / 4 * 4, cap = kFwdRhMax / 4 * 4;
  return fit < cap ? fit : cap;
}

// ---- fwd_l123x6 (fwd_l123x6.hpp): dynamic LDS -----------------------------------
// Eight waves share one block (and the 48 KB of split weight images) per
// CU, two per SIMD; a region is 24 rows (3 chunks per wave).
constexpr int kF6Waves = 8;
constexpr int kF6Rh = 24;              // region rows
constexpr int kF6TW = kFwdRW + 8;      // input tile row stride (f1 = 9)
constexpr int kF6XR = kF6Rh + 8;       // input tile rows
constexpr int kF6QS = 41;              // Q^T row stride (32 + 2 (f3 - 1) columns)
constexpr int kF6W1 = 5 * 2 * 3 * 512; // bf16: [s][t][part][lane][8]
constexpr int kF6W2 = 4 * 3 * 512;     // bf16: [m][part][lane][8]
constexpr int kF6W3 = 2 * 3 * 512;     // bf16: [m][part][lane][8]
struct F6Lds {
  static constexpr int w1 = 0, w2 = w1 + kF6W1 * 2, w3 = w2 + kF6W2 * 2, a88 = w3 + kF6W3 * 2,
                       b2 = a88 + 128 * 4, r = b2 + 32 * 4,
                       rn = kF6TW * kF6XR + 1,  // pair-image dwords per part
                       xs = r + 3 * rn * 4, qs = (xs + kF6TW * kF6XR * 4 + 15) & ~15,
                       accs = qs + kF6Waves * 25 * kF6QS * 4, bytes = accs + 5 * (kF6Rh + 4) * (kFwdRW + 4) * 4;
};

// x6 region rows: fixed; the input tile of the default net's f1 = 9 fills the
// pair images' kF6XR rows, and every wave takes the same number of chunks
constexpr int fwd_rh_x6() {
  static_assert(kF6Rh + 9 - 1 <= kF6XR && kF6Rh % kF6Waves == 0, "x6 region");
  return kF6Rh;
}
