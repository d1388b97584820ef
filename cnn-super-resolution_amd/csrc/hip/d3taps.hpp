// d3taps.hpp -- the tap slots of d1x6's delta2 GEMM (d1x6.hpp, kD3), included
// by train_fused.hip inside namespace srcnn::fused.  No device intrinsic: it
// compiles for the host with the qualifiers defined away
// (tests/d3_tap_slots_check.cpp).
//
// The GEMM's K dimension is 2 k-steps of 16 tap slots.  A lane's 8 elements of
// a k-step are four PAIRS, each read from the delta3 pair image as one
// separately addressed dword, so only the two elements of a pair have to be
// neighbours in an image row.  Pair slot p = 8 s + 4 h + e (k-step s, lane
// half h, pair e of the fragment; element j = 2 e + i); a tap row takes
// ceil(f3 / 2) pairs:
//   - pairs e = 0 .. 2 of group g = 2 s + h are tap row g, image columns 2 e +
//     2, + 3 of the slot's window (one base address and immediates: e = 0, 1
//     are one ds_read2_b32);
//   - pair e = 3 is tap row 4, columns 6 - 2 g, + 1 (groups 0 .. 2).
// That is 15 of the 16 pair slots at f3 = 5.  (Eight consecutive positions
// per lane took a k-step per two tap rows: 3 k-steps, 48 slots for 25 taps.)
struct D3Pair {
  int dy;     // tap row (0 .. 4); an unused pair names a row too: it is read, with zero weights
  int col;    // image column of element 0 relative to the slot's (element 1: col + 1), 0 .. 6
  bool used;  // false: both weights zero
};

// pair slot p (0 .. 15) of an f3 x f3 filter, f3 <= 5.  Window column c holds
// tap column dx = 7 - c (delta3 column px - dx sits at image column px + 7 -
// dx), so pair k of a row (taps dx = 2k + 1, 2k) is at columns 6 - 2k, 7 - 2k
__host__ __device__ constexpr D3Pair d3_pair_slot(int p, int f3) {
  const int npr = (f3 + 1) / 2, g = p >> 2, e = p & 3;
  return e < 3 ? D3Pair{g, 2 + 2 * e, g < f3 && 2 - e < npr} : D3Pair{4, 6 - 2 * g, 4 < f3 && g < npr};
}

// the tap column dx of element i (0, 1) of a pair, or -1 for a zero weight
// (an unused pair, or the sixth column of an odd filter row)
__host__ __device__ constexpr int d3_pair_dx(D3Pair t, int i, int f3) {
  const int dx = 7 - (t.col + i);
  return t.used && dx >= 0 && dx < f3 ? dx : -1;
}

// what d1x6's reads rely on: pairs 0 .. 2 of every group lie in one row at
// columns c, c + 2, c + 4, and every pair inside the window's rows and columns
__host__ __device__ constexpr bool d3_pairs_addressable(int f3) {
  for (int g = 0; g < 4; g++) {
    const D3Pair a = d3_pair_slot(4 * g, f3);
    for (int e = 0; e < 4; e++) {
      const D3Pair t = d3_pair_slot(4 * g + e, f3);
      if (t.dy < 0 || t.dy > 4 || t.col < 0 || t.col > 6) return false;
      if (e < 3 && (t.dy != a.dy || t.col != a.col + 2 * e)) return false;
    }
  }
  return true;
}
static_assert(d3_pairs_addressable(1) && d3_pairs_addressable(2) && d3_pairs_addressable(3) &&
                  d3_pairs_addressable(4) && d3_pairs_addressable(5),
              "d1x6's delta3 reads: one base per row group");
