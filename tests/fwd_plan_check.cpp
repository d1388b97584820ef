// fwd_plan_check.cpp -- host print-out and check of the fused forward's plan
// (csrc/hip/fwd_layout.hpp, fwd_plan.hpp), compiled and run by
// tests/test_fwd_plan_cpu.py.  Both headers are free of device intrinsics and
// of HIP types, so they compile for the host with the qualifiers defined away.
//
// Prints the FwdPlan of Net<64,32,9,5> under both arithmetics and of
// Net<32,16,9,5> under arithmetic 0, a section (`#` line) each:
//   - 12x12 and 13x12 (refused: `-`)
//   - every w in 13..110 at h in {13, 32, 33, 36, 37, 80} and every h in
//     13..110 at w in {13, 40, 41, 105}, at batches 1, 3 and 64: 1 -> 4 region
//     columns (at 32, 64 and 96 L1 outputs), the 24- and 28-row region heights,
//     1 -> 4 region rows
//   - the named frames 256x256, 640x365, 1280x720, 1920x1080, 3840x2160 and
//     7680x4320 at batch 1, and 3840x2160 at batch 8 (`w h @batch:` lines with
//     grid, seam_rb and the seam grid's y and z in place of G and S)
// The Python side compares the text with tests/golden/fwd_plan_table.txt.
// What many frames share is printed once as a numbered block and referred to
// by its number: `R` the kernel and its region (x6, rh, lds), `G` the grid at
// the three batches, `S` the seam's rows per block and grid y, z at the three
// batches.  part_bytes is printed at batch 1; that it is linear in the batch
// is a check.
// Checks, one FAIL line each:
//   - nrx == ceil(ow / 32), nry == ceil(oh / rh); F3 <= rh <= oh and
//     rh <= kF6Rh where x6, else kFwdRhMax
//   - the input tile fits its LDS image: (rh + F1-1) (32 + F1-1) <= kFwdXs for
//     fwd_l123, rh + F1-1 <= kF6XR for fwd_l123x6
//   - x6 only for the default net under arithmetic 0; lds == F6Lds::bytes
//     <= 160 KiB where x6, else 0
//   - FwdLds<5>::bytes == 56192 (the code object's group segment of
//     fwd_l123_kernel<., ., 9, 5>) and 2 FwdLds<F3>::bytes <= 160 KiB (two
//     blocks per CU)
//   - 1 <= grid <= min(batch nrx nry, cap), cap 256 where x6 (one block per
//     CU), else kFwdGrid
//   - part_bytes >= batch nrx nry (rh + F3-1) (32 + F3-1) 4, what the chosen
//     kernel writes; equal under both arithmetics for the default net; linear
//     in the batch
//   - seam: seam_bx in {64, 128, 192, 256}, gx seam_bx >= w3, 1 <= seam_rb <= 8,
//     1 <= gy, gz <= 65535
//   - whether a frame is served, and everything on its line but G and S, does
//     not depend on the batch
#include <algorithm>
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <map>
#include <string>

#include "srcnn.h"

#define __device__
#define __host__
#define __forceinline__ inline
namespace srcnn {
namespace fused {
#include "fwd_layout.hpp"
#include "fwd_plan.hpp"
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

constexpr size_t kLds = 160 * 1024;  // LDS bytes of a CU
static_assert(FwdLds<5>::bytes == 56192, "fwd_l123's group segment");

static const uint32_t kBatches[3] = {1, 3, 64};
static int g_frames = 0, g_served = 0;
static std::map<std::string, int> g_r, g_g, g_s;

// the block's number, printed at its first use
static int block(std::map<std::string, int>& m, const char* tag, const std::string& text) {
  auto it = m.find(text);
  if (it == m.end()) {
    it = m.emplace(text, (int)m.size()).first;
    std::printf("%s %d: %s\n", tag, it->second, text.c_str());
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

static std::string region_row(const FwdPlan& p) { return fmt("%d %d %zu", (int)p.x6, p.g.rh, p.lds); }
static std::string frame_row(const FwdPlan& p, uint32_t batch) {
  return fmt("%d %d %zu %d %u", p.g.nrx, p.g.nry, p.part_bytes / batch, p.seam_bx, p.seam_gx);
}
static std::string seam_row(const FwdPlan& p) { return fmt("%d %u %u", p.seam_rb, p.seam_gy, p.seam_gz); }

template <typename NetT>
static void check(int arith, int w, int h, uint32_t batch, const FwdPlan& p) {
#define WHERE "net %d %d %d %d arith %d %dx%d batch %u: "
#define HERE NetT::N1, NetT::N2, NetT::F1, NetT::F3, arith, w, h, batch
  constexpr int F1 = NetT::F1, F3 = NetT::F3;
  static_assert(2 * (size_t)FwdLds<F3>::bytes <= kLds, "two fwd_l123 blocks per CU");
  const FwdGeom& g = p.g;
  const int ow = w - F1 + 1, oh = h - F1 + 1, w3 = ow - F3 + 1;
  if (g.W != w || g.H != h || g.ow != ow || g.oh != oh || g.batch != (int)batch) FAIL(WHERE "geometry", HERE);
  if (g.nrx != (ow + 31) / 32 || g.nry != (oh + g.rh - 1) / g.rh) FAIL(WHERE "%d x %d regions", HERE, g.nrx, g.nry);
  if (g.rh < F3 || g.rh > (p.x6 ? kF6Rh : kFwdRhMax) || g.rh > oh) FAIL(WHERE "region height %d", HERE, g.rh);
  if (p.x6 ? g.rh + F1 - 1 > kF6XR : (g.rh + F1 - 1) * (32 + F1 - 1) > kFwdXs)
    FAIL(WHERE "a %d-row input tile passes its LDS image", HERE, g.rh + F1 - 1);
  if (p.x6 != (NetT::kDefault && arith == 0)) FAIL(WHERE "x6 = %d", HERE, (int)p.x6);
  if (p.x6 ? p.lds != (size_t)F6Lds::bytes || p.lds > kLds : p.lds != 0) FAIL(WHERE "dynamic LDS %zu B", HERE, p.lds);
  const long items = (long)batch * g.nrx * g.nry;
  if (p.grid < 1 || (long)p.grid > std::min<long>(items, p.x6 ? 256 : kFwdGrid)) FAIL(WHERE "grid %u", HERE, p.grid);
  if (p.part_bytes < (size_t)items * (g.rh + F3 - 1) * (32 + F3 - 1) * 4) FAIL(WHERE "part_bytes %zu", HERE, p.part_bytes);
  if (NetT::kDefault) {
    FwdPlan o;
    if (!plan_forward<NetT>((uint32_t)w, (uint32_t)h, batch, 1 - arith, &o) || o.part_bytes != p.part_bytes)
      FAIL(WHERE "part_bytes differs under the other arithmetic", HERE);
  }
  if (p.seam_bx % 64 || p.seam_bx < 64 || p.seam_bx > 256 || (long)p.seam_gx * p.seam_bx < w3)
    FAIL(WHERE "seam columns: %u blocks of %d", HERE, p.seam_gx, p.seam_bx);
  if (p.seam_rb < 1 || p.seam_rb > 8) FAIL(WHERE "seam_rb %d", HERE, p.seam_rb);
  if (p.seam_gy < 1 || p.seam_gy > 65535 || p.seam_gz < 1 || p.seam_gz > 65535)
    FAIL(WHERE "seam grid y %u z %u", HERE, p.seam_gy, p.seam_gz);
#undef WHERE
#undef HERE
}

template <typename NetT>
static void frame(int arith, int w, int h) {
  FwdPlan p[3];
  bool ok[3];
  for (int b = 0; b < 3; b++) ok[b] = plan_forward<NetT>((uint32_t)w, (uint32_t)h, kBatches[b], arith, &p[b]);
  g_frames++;
  if (ok[0] != ok[1] || ok[0] != ok[2]) FAIL("arith %d %dx%d: served depends on the batch", arith, w, h);
  if (!ok[0]) {
    std::printf("%d %d -\n", w, h);
    return;
  }
  g_served++;
  std::string grow, srow;
  for (int b = 0; b < 3; b++) {
    check<NetT>(arith, w, h, kBatches[b], p[b]);
    if (region_row(p[b]) != region_row(p[0]) || frame_row(p[b], kBatches[b]) != frame_row(p[0], 1) ||
        p[b].part_bytes % kBatches[b])
      FAIL("arith %d %dx%d: a frame field depends on the batch", arith, w, h);
    grow += fmt(b ? " %u" : "%u", p[b].grid);
    srow += (b ? ", " : "") + seam_row(p[b]);
  }
  const int r = block(g_r, "R", region_row(p[0]));
  const int gi = block(g_g, "G", grow);
  const int s = block(g_s, "S", srow);
  std::printf("%d %d: %d %s %d %d\n", w, h, r, frame_row(p[0], 1).c_str(), gi, s);
}

template <typename NetT>
static void named(int arith, int w, int h, uint32_t batch) {
  FwdPlan p;
  g_frames++;
  if (!plan_forward<NetT>((uint32_t)w, (uint32_t)h, batch, arith, &p)) {
    std::printf("%d %d @%u -\n", w, h, batch);
    return;
  }
  g_served++;
  check<NetT>(arith, w, h, batch, p);
  if (p.part_bytes % batch) FAIL("arith %d %dx%d: part_bytes is not linear in the batch", arith, w, h);
  const int r = block(g_r, "R", region_row(p));
  std::printf("%d %d @%u: %d %s | %u %s\n", w, h, batch, r, frame_row(p, batch).c_str(), p.grid, seam_row(p).c_str());
}

template <typename NetT>
static void section(int arith) {
  std::printf("# net %d %d %d %d arith %d\n", NetT::N1, NetT::N2, NetT::F1, NetT::F3, arith);
  frame<NetT>(arith, 12, 12);
  frame<NetT>(arith, 13, 12);
  const int hs[6] = {13, 32, 33, 36, 37, 80}, ws[4] = {13, 40, 41, 105};
  for (int h : hs)
    for (int w = 13; w <= 110; w++) frame<NetT>(arith, w, h);
  for (int w : ws)
    for (int h = 13; h <= 110; h++)
      if (std::find(hs, hs + 6, h) == hs + 6) frame<NetT>(arith, w, h);  // (the others stand above)
  const int fr[6][2] = {{256, 256}, {640, 365}, {1280, 720}, {1920, 1080}, {3840, 2160}, {7680, 4320}};
  for (auto& f : fr) named<NetT>(arith, f[0], f[1], 1);
  named<NetT>(arith, 3840, 2160, 8);
}

int main() {
  std::printf("# R id: x6 rh lds\n");
  std::printf("# G id: grid at batch 1, 3, 64\n");
  std::printf("# S id: (seam_rb seam_gy seam_gz) at batch 1, 3, 64\n");
  std::printf("# w h: R nrx nry part_bytes/batch seam_bx seam_gx G S\n");
  std::printf("# w h @batch: R nrx nry part_bytes/batch seam_bx seam_gx | grid seam_rb seam_gy seam_gz\n");
  section<Net<64, 32, 9, 5>>(0);
  section<Net<64, 32, 9, 5>>(1);
  section<Net<32, 16, 9, 5>>(0);
  std::printf("frames=%d served=%d failures=%d\n", g_frames, g_served, g_fail);
  return g_fail ? 1 : 0;
}
