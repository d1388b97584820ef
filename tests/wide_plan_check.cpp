// wide_plan_check.cpp -- host print-out and check of the wide step's plan
// (csrc/hip/wide_layout.hpp, wide_plan.hpp), compiled and run by
// tests/test_wide_plan_cpu.py.  Both headers are free of device intrinsics, so
// they compile for the host with the qualifiers defined away.
//
// Prints the whole WidePlan for every tile w, h in 17..34 (the step serves up
// to 33; 34 is the first refusal), batches 1, 8 and 4096 (8: the smallest grid
// that takes the XCD mapping) and both arithmetics; the Python side compares
// the text with tests/golden/wide_plan_table.txt.  A `T` line is one (arith,
// tile); what depends on the batch (grids, slab counts, workspace regions) is a
// `B` block of three rows, printed once and referred to by its number.
// Checks, one FAIL line each:
//   - every served plan's dynamic LDS counts are <= 160 KiB (wl3l's with its
//     static 64 B), wl1x6's <= 36 KiB and wg1x6's <= 80 KiB where planned
//   - the op-level geometry builders return the step's geometry wherever the
//     step serves the tile
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>

#define __device__
#define __host__
#define __forceinline__ inline
namespace srcnn {
namespace wide {
#include "wide_layout.hpp"
#include "wide_plan.hpp"
}  // namespace wide
}  // namespace srcnn
using namespace srcnn::wide;

static int g_fail = 0;
#define FAIL(...)                     \
  do {                                \
    g_fail++;                         \
    std::printf("FAIL " __VA_ARGS__); \
    std::printf("\n");                \
  } while (0)

static const uint32_t kBatches[3] = {1, 8, 4096};

static std::string batch_row(const WidePlan& p) {
  char s[512];
  std::snprintf(s, sizeof s, "%d %d %d %d %d %d %d %d %d | %zu %zu %zu %zu %zu %zu %zu %zu", p.GL1, p.GL2, p.G3, p.GD,
                p.GW1, p.GG1, p.GG2, p.nslab1, p.g2.groups, p.nWf, p.nWd, p.nWx, p.n1, p.n2, p.n3, p.nsq, p.bytes);
  return s;
}

template <class T>
static bool same(const T& a, const T& b) {
  return std::memcmp(&a, &b, sizeof(T)) == 0;
}

static void check(int arith, int w, int h, const WidePlan& p) {
  const size_t lds[6] = {p.lds1, p.lds2, p.lds3 + (p.wl3l ? Wl3lLds::kStatic : 0), p.ldsd, p.ldsg1, p.ldsg2};
  for (int i = 0; i < 6; i++)
    if (lds[i] > 160 * 1024) FAIL("arith %d %dx%d: LDS count %d is %zu B", arith, w, h, i, lds[i]);
  if (p.x6f && p.lds1 > 36 * 1024) FAIL("arith %d %dx%d: wl1x6 LDS %zu B", arith, w, h, p.lds1);
  if (p.x6g1 && p.ldsg1 > 80 * 1024) FAIL("arith %d %dx%d: wg1x6 LDS %zu B", arith, w, h, p.ldsg1);
  // the op-level builders on the step's images (delta1's carries no X tile there)
  const CGeom cf = conv_fwd_geom(p.g.w1, p.g.h1, p.g.batch);
  CGeom cd = conv_delta_geom(p.g.w1, p.g.h1, p.g.batch);
  cd.xw = p.g.w;
  cd.xh = p.g.h;
  G2Geom g2;
  const bool full = g2_geom(p.g.w2, p.g.h2, p.g.batch, &g2);
  g2.groups = p.g2.groups;  // (the step's wgrad2x6 takes fewer)
  if (!same(cf, p.cf)) FAIL("arith %d %dx%d: op-level L2 forward geometry differs", arith, w, h);
  if (!same(cd, p.cd)) FAIL("arith %d %dx%d: op-level delta1 geometry differs", arith, w, h);
  if (!full || !same(g2, p.g2)) FAIL("arith %d %dx%d: op-level gW2 band geometry differs", arith, w, h);
}

int main() {
  std::printf("# B id / batch: GL1 GL2 G3 GD GW1 GG1 GG2 nslab1 g2.groups | nWf nWd nWx n1 n2 n3 nsq bytes\n");
  std::printf("# T arith w h served: x6 x6d x6f x6g1 x6g wl3l | lds1 lds2 lds3 ldsd ldsg1 ldsg2 qfloats nch1 |"
              " g2 w1 h1 w2 h2 rows nbands cols nbx aw | B\n");
  std::map<std::string, int> blocks;
  int tiles = 0, served = 0;
  for (int arith = 0; arith < 2; arith++)
    for (int h = 17; h <= 34; h++)
      for (int w = 17; w <= 34; w++) {
        WidePlan p[3];
        bool ok[3];
        for (int b = 0; b < 3; b++) ok[b] = plan_step((uint32_t)w, (uint32_t)h, kBatches[b], arith, &p[b]);
        tiles++;
        if (ok[0] != ok[1] || ok[0] != ok[2]) FAIL("arith %d %dx%d: served depends on the batch", arith, w, h);
        if (!ok[0]) {
          std::printf("T %d %d %d 0\n", arith, w, h);
          continue;
        }
        served++;
        std::string blk;
        for (int b = 0; b < 3; b++) {
          blk += batch_row(p[b]) + "\n";
          check(arith, w, h, p[b]);
          // everything on the T line is the same for every batch
          const WidePlan &a = p[0], &c = p[b];
          if (a.x6 != c.x6 || a.x6d != c.x6d || a.x6f != c.x6f || a.x6g1 != c.x6g1 || a.x6g != c.x6g || a.wl3l != c.wl3l ||
              a.lds1 != c.lds1 || a.lds2 != c.lds2 || a.lds3 != c.lds3 || a.ldsd != c.ldsd || a.ldsg1 != c.ldsg1 ||
              a.ldsg2 != c.ldsg2 || a.qfloats != c.qfloats || a.g2.rows != c.g2.rows || a.g2.nbands != c.g2.nbands ||
              a.g2.cols != c.g2.cols || a.g2.nbx != c.g2.nbx || a.g2.aw != c.g2.aw || c.g2.batch != (int)kBatches[b] ||
              c.g.batch != (int)kBatches[b] || c.cf.batch != (int)kBatches[b] || c.cd.batch != (int)kBatches[b])
            FAIL("arith %d %dx%d: a tile field depends on the batch", arith, w, h);
        }
        auto it = blocks.find(blk);
        if (it == blocks.end()) {
          it = blocks.emplace(blk, (int)blocks.size()).first;
          for (int b = 0; b < 3; b++) std::printf("B %d / %u: %s\n", it->second, kBatches[b], batch_row(p[b]).c_str());
        }
        const WidePlan& a = p[0];
        std::printf("T %d %d %d 1: %d %d %d %d %d %d | %zu %zu %zu %zu %zu %zu %d %d | %d %d %d %d %d %d %d %d %d | %d\n",
                    arith, w, h, (int)a.x6, (int)a.x6d, (int)a.x6f, (int)a.x6g1, (int)a.x6g, (int)a.wl3l, a.lds1, a.lds2,
                    a.lds3, a.ldsd, a.ldsg1, a.ldsg2, a.qfloats, a.rg1.nch, a.g2.w1, a.g2.h1, a.g2.w2, a.g2.h2, a.g2.rows,
                    a.g2.nbands, a.g2.cols, a.g2.nbx, a.g2.aw, it->second);
      }
  std::printf("tiles=%d served=%d failures=%d\n", tiles, served, g_fail);
  return g_fail ? 1 : 0;
}
