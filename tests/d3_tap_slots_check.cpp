// d3_tap_slots_check.cpp -- host check of the pair-slot <-> tap map of d1x6's
// delta2 GEMM (csrc/hip/d3taps.hpp), compiled and run by
// tests/test_d3_tap_slots_cpu.py.  d3taps.hpp is device code without any
// device intrinsic, so it compiles for the host with its qualifiers defined
// away.
//
// For f3 = 1 .. 5, over the 16 pair slots (2 k-steps x 2 lane halves x 4
// pairs) and their 32 elements:
//   - every tap (dy, dx) of the f3 x f3 filter occurs exactly once, so no tap
//     needs a slot index >= 16;
//   - every other element is marked zero-weight (dx = -1);
//   - the two elements of a pair are image columns c, c + 1 of one row; the
//     row is one of the five tap rows and the columns lie in the slot's
//     eight-column window (0 .. 7), whose column c holds tap column dx = 7 - c
//     (unused pairs are read too, so this holds for them as well);
//   - a pair is marked unused exactly when both its elements are zero-weight;
//   - pairs 0 .. 2 of a group of four lie in one row, columns 2 apart (the
//     kernel addresses them from one base).
// Prints one line per failure and returns 1.
#include <cstdio>

#define __host__
#define __device__
#include "d3taps.hpp"

static int g_fail = 0;

#define FAIL(...)                     \
  do {                                \
    g_fail++;                         \
    std::printf("FAIL " __VA_ARGS__); \
    std::printf("\n");                \
  } while (0)

// the map is usable in constant expressions (the kernel's static checks)
static_assert(d3_pair_slot(0, 5).dy == 0 && d3_pair_slot(11, 5).dy == 4 && !d3_pair_slot(15, 5).used, "f3 = 5 rows");
static_assert(d3_pair_dx(d3_pair_slot(0, 5), 0, 5) == -1 && d3_pair_dx(d3_pair_slot(0, 5), 1, 5) == 4, "odd row's zero");

int main() {
  int taps_total = 0;
  for (int f3 = 1; f3 <= 5; f3++) {
    int hits[5][5] = {};
    int zero = 0;
    for (int p = 0; p < 16; p++) {
      const D3Pair t = d3_pair_slot(p, f3);
      if (t.dy < 0 || t.dy > 4) FAIL("f3=%d slot %d: row %d", f3, p, t.dy);
      if (t.col < 0 || t.col + 1 > 7) FAIL("f3=%d slot %d: columns %d, %d outside the window", f3, p, t.col, t.col + 1);
      if ((p & 3) < 3) {
        const D3Pair a = d3_pair_slot(p & ~3, f3);
        if (t.dy != a.dy || t.col != a.col + 2 * (p & 3))
          FAIL("f3=%d slot %d: (%d, %d) not 2 apart from the group's (%d, %d)", f3, p, t.dy, t.col, a.dy, a.col);
      }
      int used = 0;
      for (int i = 0; i < 2; i++) {
        const int dx = d3_pair_dx(t, i, f3);
        if (dx < 0) {
          zero++;
          continue;
        }
        used++;
        if (t.dy >= f3 || dx >= f3) {
          FAIL("f3=%d slot %d element %d: tap (%d, %d)", f3, p, i, t.dy, dx);
          continue;
        }
        // element i reads image column col + i of row 5 - dy: tap column 7 - (col + i)
        if (dx != 7 - (t.col + i)) FAIL("f3=%d slot %d element %d: dx %d at column %d", f3, p, i, dx, t.col + i);
        hits[t.dy][dx]++;
      }
      if (t.used != (used > 0)) FAIL("f3=%d slot %d: used %d with %d used elements", f3, p, (int)t.used, used);
    }
    for (int dy = 0; dy < 5; dy++)
      for (int dx = 0; dx < 5; dx++) {
        const int want = dy < f3 && dx < f3 ? 1 : 0;
        if (hits[dy][dx] != want) FAIL("f3=%d: tap (%d, %d) occurs %d times", f3, dy, dx, hits[dy][dx]);
        taps_total += hits[dy][dx];
      }
    if (zero != 32 - f3 * f3) FAIL("f3=%d: %d zero-weight elements, expected %d", f3, zero, 32 - f3 * f3);
  }
  std::printf("filters=5 taps=%d failures=%d\n", taps_total, g_fail);
  return g_fail ? 1 : 0;
}
