// fused_plan_check.cpp -- host print-out and check of the fused step's plan
// (csrc/hip/fused_layout.hpp, fused_plan.hpp), compiled and run by
// tests/test_fused_plan_cpu.py.  Both headers are free of device intrinsics, so
// they compile for the host with the qualifiers defined away.
//
// Without arguments: prints the whole StepPlan of
//   - Net<64,32,9,5>: every tile w, h in 13..41 under both arithmetics, and
//     w in 42..58 at h = 13 and 14 (41 rows and 58 columns are the first
//     refusals of kL12Rows and kL12S, 40 x 40 the first of kXsMax)
//   - the other three nets of with_net: the squares 11..41 and the rows and
//     columns through 33, arithmetic 0
// at batches 1, 300, 700 and 4096 (300 and 700 take the two middle branches of
// g3 and change d1c_parts); the Python side compares the text with
// tests/golden/fused_plan_table.txt.  A section (`#` line) is one (net,
// arithmetic); a line that starts with a number is one tile, `-` where the
// plan refuses it.  What many tiles share is printed once as a numbered block
// and referred to by its number: `K` the kernel variants (flags, the A1 layout,
// the three kernel names), `B` what depends on the batch (four rows: grids,
// d1c_parts, slab regions), `M` m2_off at the four batches.
// The two quantities the plan takes from other units are stand-ins here that
// return fixed sentinels, so a plan whose layer 3 runs on the op-level kernels
// (!l3_fused) prints s3 and bytes as `op`; tests/test_workspace_table_cpu.py
// pins the true totals.
// Checks, one FAIL line each:
//   - lds12 <= 80 KiB where x6; ldsd <= 160 KiB; lds3 <= 80 KiB where l3r, else
//     <= 160 KiB where l3_fused
//   - d3mode implies x6 && l3r; d1tr implies d3mode; with d3mode the mask fits
//     the D2 region: m2_off + batch ow oh <= batch ow oh N2
//   - d1c_parts >= 1 and every part holds a chunk
//   - whether a tile is served, and everything on its line but B and M, does
//     not depend on the batch
//
// `names N1 N2 F1 F3 arith w h batch`: prints the plan's three kernel names
// for that case (`-` if refused), for the comparison with
// tests/golden/dispatch_table.json.
#include <algorithm>
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

#include "srcnn.h"

#define __device__
#define __host__
#define __forceinline__ inline
namespace srcnn {
// stand-ins for the two calls into other units (ops.hpp)
constexpr size_t kOpFloats = 1000003, kOpBlocks = 7;
namespace fast {
static size_t grad_workspace_bytes(uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t) {
  return kOpFloats * sizeof(float);
}
}  // namespace fast
static uint32_t reduce_blocks(size_t) { return kOpBlocks; }
namespace fused {
enum { kA1Blocked = 0, kA1Runs = 1, kA1Hwc = 2 };  // (ops.hpp)
#include "fused_layout.hpp"
#include "fused_plan.hpp"
}  // namespace fused
}  // namespace srcnn
using namespace srcnn::fused;

static int g_fail = 0;
#define FAIL(...)                     \
  do {                                \
    g_fail++;                         \
    std::printf("FAIL " __VA_ARGS__); \
    std::printf("\n");                \
  } while (0)

static const uint32_t kBatches[4] = {1, 300, 700, 4096};
static int g_tiles = 0, g_served = 0;
static std::map<std::string, int> g_k, g_b, g_m;

// the block's number, printed at its first use
static int block(std::map<std::string, int>& m, const char* tag, const std::string& text) {
  auto it = m.find(text);
  if (it == m.end()) {
    it = m.emplace(text, (int)m.size()).first;
    std::printf("%s %d:%s%s", tag, it->second, text.find('\n') == std::string::npos ? " " : "\n", text.c_str());
    if (text.back() != '\n') std::printf("\n");
  }
  return it->second;
}

static std::string fmt(const char* f, ...) __attribute__((format(printf, 1, 2)));
static std::string fmt(const char* f, ...) {
  char s[512];
  va_list ap;
  va_start(ap, f);
  std::vsnprintf(s, sizeof s, f, ap);
  va_end(ap);
  return s;
}

static std::string variant_row(const StepPlan& p) {
  return fmt("%d %d %d %d %d %d %d | %s %s %s", (int)p.x6, (int)p.l3r, (int)p.l3_fused, (int)p.d3mode, (int)p.kD1c,
             (int)p.d1tr, p.a1_layout, p.k12, p.k3, p.kd1);
}
static std::string tile_row(const StepPlan& p) {
  return fmt("%d %d %d %d %d %zu %zu %zu", p.ow, p.oh, p.w3, p.h3, p.rg.nch, p.lds12, p.lds3, p.ldsd);
}
static std::string batch_row(const StepPlan& p) {
  if (!p.l3_fused) return fmt("%d %d %d %d | %zu op %zu op", p.g12, p.g3, p.gd, p.d1c_parts, p.s12, p.ssq);
  return fmt("%d %d %d %d | %zu %zu %zu %zu", p.g12, p.g3, p.gd, p.d1c_parts, p.s12, p.s3, p.ssq, p.bytes);
}

template <typename NetT>
static void check(int arith, int w, int h, uint32_t batch, const StepPlan& p) {
#define WHERE "net %d %d %d %d arith %d %dx%d batch %u: "
#define HERE NetT::N1, NetT::N2, NetT::F1, NetT::F3, arith, w, h, batch
  if (p.x6 && p.lds12 > (size_t)kLdsHalf) FAIL(WHERE "l12x6 LDS %zu B", HERE, p.lds12);
  if (p.ldsd > (size_t)kLdsMax) FAIL(WHERE "delta1 LDS %zu B", HERE, p.ldsd);
  if (p.l3r ? p.lds3 > (size_t)kLdsHalf : p.l3_fused && p.lds3 > (size_t)kLdsMax) FAIL(WHERE "layer-3 LDS %zu B", HERE, p.lds3);
  if (p.d3mode && !(p.x6 && p.l3r)) FAIL(WHERE "d3mode without x6 and l3r", HERE);
  if (p.d1tr && !p.d3mode) FAIL(WHERE "d1tr without d3mode", HERE);
  const size_t px = (size_t)batch * p.ow * p.oh;
  if (p.d3mode && p.m2_off + px > px * NetT::N2) FAIL(WHERE "the mask at %zu passes the D2 region", HERE, p.m2_off);
  const int nch1 = (p.ow * p.oh + 31) / 32;
  if (p.d1c_parts < 1 || (p.d1c_parts - 1) * ((nch1 + p.d1c_parts - 1) / p.d1c_parts) >= nch1)
    FAIL(WHERE "%d d1c parts over %d chunks", HERE, p.d1c_parts, nch1);
  if (p.bytes != (p.s12 + p.s3 + p.ssq) * sizeof(float)) FAIL(WHERE "bytes is not the three regions", HERE);
#undef WHERE
#undef HERE
}

template <typename NetT>
static void tile(int arith, int w, int h) {
  StepPlan p[4];
  bool ok[4];
  for (int b = 0; b < 4; b++) ok[b] = plan_step<NetT>((uint32_t)w, (uint32_t)h, kBatches[b], arith, &p[b]);
  g_tiles++;
  if (ok[0] != ok[1] || ok[0] != ok[2] || ok[0] != ok[3]) FAIL("arith %d %dx%d: served depends on the batch", arith, w, h);
  if (!ok[0]) {
    std::printf("%d %d -\n", w, h);
    return;
  }
  g_served++;
  std::string brows, mrow;
  for (int b = 0; b < 4; b++) {
    check<NetT>(arith, w, h, kBatches[b], p[b]);
    if (variant_row(p[b]) != variant_row(p[0]) || tile_row(p[b]) != tile_row(p[0]))
      FAIL("arith %d %dx%d: a tile field depends on the batch", arith, w, h);
    brows += fmt("%u: ", kBatches[b]) + batch_row(p[b]) + "\n";
    mrow += fmt(b ? " %zu" : "%zu", p[b].m2_off);
  }
  const int k = block(g_k, "K", variant_row(p[0]));
  const int bi = block(g_b, "B", brows);
  const int m = block(g_m, "M", mrow);
  std::printf("%d %d: %s %d %d %d\n", w, h, tile_row(p[0]).c_str(), k, bi, m);
}

template <typename NetT>
static void section(int arith) {
  std::printf("# net %d %d %d %d arith %d\n", NetT::N1, NetT::N2, NetT::F1, NetT::F3, arith);
}

// names N1 N2 F1 F3 arith w h batch
static int names(char** a) {
  const srcnn_net net{(uint32_t)std::atoi(a[0]), (uint32_t)std::atoi(a[1]), (uint32_t)std::atoi(a[2]), 1,
                      (uint32_t)std::atoi(a[3])};
  const int served = with_net(&net, [&](auto n) {
    StepPlan p;
    if (!plan_step<decltype(n)>(std::atoi(a[5]), std::atoi(a[6]), std::atoi(a[7]), std::atoi(a[4]), &p)) return 0;
    std::printf("%s %s %s\n", p.k12, p.k3, p.kd1);
    return 1;
  });
  if (!served) std::printf("-\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 10 && !std::strcmp(argv[1], "names")) return names(argv + 2);
  std::printf("# K id: x6 l3r l3_fused d3mode kD1c d1tr a1_layout | l12 layer-3 delta1 names\n");
  std::printf("# B id: (batch: g12 g3 gd d1c_parts | s12 s3 ssq bytes) x 4\n");
  std::printf("# M id: m2_off at batch 1, 300, 700, 4096\n");
  std::printf("# w h: ow oh w3 h3 nch lds12 lds3 ldsd K B M\n");
  using Default = Net<64, 32, 9, 5>;
  for (int arith = 0; arith < 2; arith++) {
    section<Default>(arith);
    for (int h = 13; h <= 41; h++)
      for (int w = 13; w <= 41; w++) tile<Default>(arith, w, h);
    for (int h = 13; h <= 14; h++)
      for (int w = 42; w <= 58; w++) tile<Default>(arith, w, h);
  }
  auto minor = [](auto n) {
    using N = decltype(n);
    section<N>(0);
    for (int s = 11; s <= 41; s++) tile<N>(0, s, s);
    for (int s = 11; s <= 41; s++)
      if (s != 33) tile<N>(0, s, 33);
    for (int s = 11; s <= 41; s++)
      if (s != 33) tile<N>(0, 33, s);
  };
  minor(Net<32, 16, 9, 5>{});
  minor(Net<64, 32, 9, 3>{});
  minor(Net<32, 16, 9, 3>{});
  std::printf("tiles=%d served=%d failures=%d\n", g_tiles, g_served, g_fail);
  return g_fail ? 1 : 0;
}
