// run_geometry_check.cpp -- host check of the slot <-> pixel maps of the
// split-bf16 fused step (csrc/hip/runs.hpp), compiled and run by
// tests/test_run_geometry_cpu.py.  runs.hpp is device code without any device
// intrinsic, so it compiles for the host with its qualifiers defined away.
//
// For every output tile (ow, oh) in [1, 49]^2 (the kernels take w <= 57 at
// f1 = 9):
//   - slot_pixel over the nch x 32 slots hits each of the ow * oh pixels
//     exactly once and is -1 elsewhere; the dummies number 32 nch - ow oh
//   - slot_coord agrees with it, and gives (0, 0) / false on dummies
//   - the four slots of a run are consecutive pixels of one row (all four
//     valid) or of one column (cut at the tile's last row)
//   - run_div(k, 1 / d) == k / d for every k and d run_origin divides
// and, exhaustively, run_div(k, 1 / d) == k / d for k < 2^20 and d <= 128
// (its comment's range; d <= 128 covers every nch, the divisor of d1x6's item
// stream, up to 76 chunks at 49 x 49).
// Prints one line per failure (at most kMaxPrint, then a count) and returns 1.
#include <cstdio>
#include <vector>

#define __device__
#define __forceinline__ inline
#include "runs.hpp"

static int g_fail = 0;
constexpr int kMaxPrint = 50;

#define FAIL(...)                   \
  do {                              \
    if (g_fail++ < kMaxPrint) {     \
      std::printf("FAIL " __VA_ARGS__); \
      std::printf("\n");            \
    }                               \
  } while (0)

static void check_tile(int ow, int oh) {
  const RunGeom r = run_geom(ow, oh);
  const int npx = ow * oh;
  if (r.nrun != r.a * oh + r.b * ((oh + 3) / 4) || r.nch != (r.nrun + 7) / 8 || 4 * r.a + r.b != ow)
    FAIL("%dx%d: run_geom a=%d b=%d cr=%d nrun=%d nch=%d", ow, oh, r.a, r.b, r.cr, r.nrun, r.nch);
  // the divisions run_origin makes
  for (int k = 0; k < r.nrow; k++)
    if (run_div(k, r.inv_a) != k / r.a) FAIL("%dx%d: run_div(%d, 1/%d) = %d", ow, oh, k, r.a, run_div(k, r.inv_a));
  for (int k = 0; k < r.b * r.cr; k++)
    if (run_div(k, r.inv_cr) != k / r.cr) FAIL("%dx%d: run_div(%d, 1/%d) = %d", ow, oh, k, r.cr, run_div(k, r.inv_cr));

  std::vector<int> hits(npx, 0);
  int dummies = 0;
  for (int c = 0; c < r.nch; c++) {
    for (int s = 0; s < 32; s++) {
      const int p = slot_pixel(r, c, s);
      if (p < -1 || p >= npx) {
        FAIL("%dx%d: slot_pixel(%d, %d) = %d out of range", ow, oh, c, s, p);
        continue;
      }
      if (p < 0)
        dummies++;
      else
        hits[p]++;
      int iy = -7, ix = -7;
      const bool ok = slot_coord(r, c, s, iy, ix);
      if (ok != (p >= 0) || (ok && iy * ow + ix != p) || (!ok && (iy != 0 || ix != 0)) ||
          iy < 0 || iy >= oh || ix < 0 || ix >= ow)
        FAIL("%dx%d: slot_coord(%d, %d) = (%d, %d, %d) against slot_pixel %d", ow, oh, c, s, iy, ix, (int)ok, p);
    }
    // the runs of this chunk
    for (int q = 0; q < 8; q++) {
      const int k = 8 * c + q;
      int p[4];
      for (int i = 0; i < 4; i++) p[i] = slot_pixel(r, c, 4 * q + i);
      if (k >= r.nrun) {
        if (p[0] != -1 || p[1] != -1 || p[2] != -1 || p[3] != -1) FAIL("%dx%d: run %d past nrun has pixels", ow, oh, k);
        continue;
      }
      int iy, ix;
      bool col;
      run_origin(r, k, iy, ix, col);
      if (col != (k >= r.nrow)) FAIL("%dx%d: run %d orientation %d", ow, oh, k, (int)col);
      if (p[0] != iy * ow + ix) FAIL("%dx%d: run %d starts at %d, origin (%d, %d)", ow, oh, k, p[0], iy, ix);
      for (int i = 1; i < 4; i++) {
        if (!col) {  // one row: four valid pixels, x consecutive
          if (p[i] != p[0] + i || p[i] / ow != p[0] / ow)
            FAIL("%dx%d: row run %d slot %d = %d after %d", ow, oh, k, i, p[i], p[0]);
        } else {  // one column: y consecutive, dummies only past the last row
          const bool in = iy + i < oh;
          if (p[i] != (in ? p[0] + i * ow : -1))
            FAIL("%dx%d: column run %d slot %d = %d after %d", ow, oh, k, i, p[i], p[0]);
        }
      }
    }
  }
  for (int p = 0; p < npx; p++)
    if (hits[p] != 1) FAIL("%dx%d: pixel %d hit %d times", ow, oh, p, hits[p]);
  if (dummies != 32 * r.nch - npx) FAIL("%dx%d: %d dummy slots, expected %d", ow, oh, dummies, 32 * r.nch - npx);
}

int main() {
  int tiles = 0, max_nch = 0;
  for (int oh = 1; oh <= 49; oh++)
    for (int ow = 1; ow <= 49; ow++) {
      check_tile(ow, oh);
      tiles++;
      const int nch = run_geom(ow, oh).nch;
      if (nch > max_nch) max_nch = nch;
    }
  constexpr int kMaxD = 128;
  if (max_nch > kMaxD) FAIL("nch %d exceeds the exhaustive run_div range %d", max_nch, kMaxD);
  long divs = 0;
  for (int d = 1; d <= kMaxD; d++) {
    const float inv = 1.0f / (float)d;
    for (int k = 0; k < (1 << 20); k++, divs++)
      if (run_div(k, inv) != k / d) FAIL("run_div(%d, 1/%d) = %d", k, d, run_div(k, inv));
  }
  std::printf("tiles=%d max_nch=%d divisions=%ld failures=%d\n", tiles, max_nch, divs, g_fail);
  return g_fail ? 1 : 0;
}
