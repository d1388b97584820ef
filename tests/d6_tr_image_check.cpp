// d6_tr_image_check.cpp -- host check of the per-wave delta2 part image of
// d1x6 (csrc/hip/d6tr.hpp), compiled and run by tests/test_d6_tr_image_cpu.py.
// d6tr.hpp is device code without any device intrinsic, so it compiles for the
// host with its qualifiers defined away.
//
// For each of the four waves the image is filled through the write map, as the
// kernel does it: lane (slot, h) stores, for k-step k, part q and quad w, the
// four values of channels n = 16 k + 8 w + 4 h + 0 .. 3, each tagged (wave,
// slot, n, part).  Then ds_read_b64_tr_b16 is modelled as the hardware does it:
// in each group of 16 consecutive lanes, lane 4 i + p addresses row i, columns
// 4 p .. 4 p + 3 of a block of 4 rows x 16 columns of 16-bit elements, and lane
// c of the group receives column c of the four rows, row i in its element i.
// Checked for all 64 lanes, both k-steps m, all three parts and both reads w:
//   - element j = 4 w + i of gW2's B fragment is delta2[slot crow(8 m + j,
//     h)][n = lane & 31] of that part, the order of the A1 fragment aa[t][m];
//   - every address is 8-B aligned and inside its wave's region, and the four
//     waves' regions are disjoint;
//   - every element of the image is written exactly once;
//   - the modelled bank-conflict degree (distinct 8-B addresses on one bank
//     within a lane group: writes per 16 consecutive lanes on dword mod 32,
//     transposed reads per 32-lane half on dword mod 64) is at most 2.
// Prints one line per failure, the two degrees and a summary, and returns 1 on
// any failure.
#include <cstdio>
#include <cstring>
#include <set>

#define __host__
#define __device__
#include "d6tr.hpp"

static int g_fail = 0;

#define FAIL(...)                     \
  do {                                \
    g_fail++;                         \
    std::printf("FAIL " __VA_ARGS__); \
    std::printf("\n");                \
  } while (0)

static int crow(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }
static unsigned tag(int wave, int slot, int n, int q) { return 1u + (unsigned)(((wave * 32 + slot) * 32 + n) * 3 + q); }

constexpr int kWaves = 4;
static unsigned g_img[kWaves * kD6TrWave / 2];  // 16-bit elements, holding tags
static int g_written[kWaves * kD6TrWave / 2];

// distinct 8-B addresses per bank (each covers two dwords) among lanes lo .. hi - 1
static int degree(const int* addr, int lo, int hi, int banks) {
  int worst = 0;
  for (int b = 0; b < banks; b++) {
    std::set<int> a;
    for (int l = lo; l < hi; l++)
      for (int d = 0; d < 2; d++)
        if ((addr[l] / 4 + d) % banks == b) a.insert(addr[l]);
    if ((int)a.size() > worst) worst = (int)a.size();
  }
  return worst;
}

static bool check_addr(const char* what, int wave, int lane, int a) {
  if (a % 8) {
    FAIL("%s wave %d lane %d: address %d not 8-B aligned", what, wave, lane, a);
    return false;
  }
  if (a < d6tr_wave_off(wave) || a + 8 > d6tr_wave_off(wave) + kD6TrWave) {
    FAIL("%s wave %d lane %d: address %d outside the wave's region", what, wave, lane, a);
    return false;
  }
  return true;
}

int main() {
  for (int w = 0; w + 1 < kWaves; w++)
    if (d6tr_wave_off(w) + kD6TrWave > d6tr_wave_off(w + 1)) FAIL("waves %d and %d overlap", w, w + 1);
  int wdeg = 0, rdeg = 0, checked = 0;
  // ---- the writes ----
  for (int wave = 0; wave < kWaves; wave++)
    for (int k = 0; k < 2; k++)
      for (int q = 0; q < 3; q++)
        for (int w = 0; w < 2; w++) {
          int addr[64];
          for (int lane = 0; lane < 64; lane++) {
            const int slot = lane & 31, h = lane >> 5;
            addr[lane] = d6tr_wave_off(wave) + d6tr_write_off(slot, h, k, q, w);
            if (!check_addr("write", wave, lane, addr[lane])) continue;
            for (int e = 0; e < 4; e++) {
              g_img[addr[lane] / 2 + e] = tag(wave, slot, 16 * k + 8 * w + 4 * h + e, q);
              g_written[addr[lane] / 2 + e]++;
            }
          }
          for (int g = 0; g < 4; g++) {
            const int d = degree(addr, 16 * g, 16 * g + 16, 32);
            if (d > wdeg) wdeg = d;
          }
        }
  for (int i = 0; i < kWaves * kD6TrWave / 2; i++)
    if (g_written[i] != 1) {
      FAIL("element %d of the images written %d times", i, g_written[i]);
      break;
    }
  // ---- the transposed reads ----
  for (int wave = 0; wave < kWaves; wave++)
    for (int m = 0; m < 2; m++)
      for (int q = 0; q < 3; q++)
        for (int w = 0; w < 2; w++) {
          int addr[64];
          bool ok = true;
          for (int lane = 0; lane < 64; lane++) {
            addr[lane] = d6tr_wave_off(wave) + d6tr_read_off(lane, m, q, w);
            ok = check_addr("read", wave, lane, addr[lane]) && ok;
          }
          if (!ok) continue;
          for (int hf = 0; hf < 2; hf++) {
            const int d = degree(addr, 32 * hf, 32 * hf + 32, 64);
            if (d > rdeg) rdeg = d;
          }
          for (int lane = 0; lane < 64; lane++) {
            const int grp = lane >> 4, c = lane & 15, h = lane >> 5;
            for (int i = 0; i < 4; i++) {
              // row i of the group's block: lanes 4 i + p, p = 0 .. 3, hold its
              // columns 4 p .. 4 p + 3; column c is element c & 3 of lane 4 i + (c >> 2)
              const unsigned got = g_img[addr[16 * grp + 4 * i + (c >> 2)] / 2 + (c & 3)];
              const unsigned want = tag(wave, crow(8 * m + 4 * w + i, h), lane & 31, q);
              checked++;
              if (got != want)
                FAIL("wave %d k-step %d part %d read %d lane %d element %d: tag %u, expected %u", wave, m, q, w, lane,
                     4 * w + i, got, want);
            }
          }
        }
  std::printf("write conflict degree %d (dword mod 32, 16 lanes)\n", wdeg);
  std::printf("read conflict degree %d (dword mod 64, 32 lanes)\n", rdeg);
  if (wdeg > 2) FAIL("writes %d-way", wdeg);
  if (rdeg > 2) FAIL("transposed reads %d-way", rdeg);
  std::printf("elements=%d write_degree=%d read_degree=%d failures=%d\n", checked, wdeg, rdeg, g_fail);
  return g_fail ? 1 : 0;
}
