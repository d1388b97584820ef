// fused_plan.hpp -- what the fused family decides on the host before a
// launch: the nets it serves and the step's plan.  Included inside namespace
// srcnn::fused after fused_layout.hpp; includes net.hpp (Net, first_net) itself,
// as fused_layout.hpp includes runs.hpp, so whoever includes the plan needs no
// further header.  Host code without any HIP call
// (tests/fused_plan_check.cpp prints and checks every plan on the CPU).  Two
// quantities come from other units, as declared calls (ops.hpp): the op-level
// layer-3 gradient workspace (fast::grad_workspace_bytes) and the squared-error
// reduction's blocks (reduce_blocks), for tiles whose layer 3 runs on the
// op-level kernels.
#include "net.hpp"

// The instantiated nets, once.
template <typename F>
static int with_net(const srcnn_net* net, F&& f) {
  return first_net(net, f, Net<64, 32, 9, 5>{},  // reference default (BASELINE.json configs[1])
                   Net<32, 16, 9, 5>{},          // example_config.json
                   Net<64, 32, 9, 3>{}, Net<32, 16, 9, 3>{});  // the same with a 3x3 last layer
}

static int grid_for_batch(uint32_t batch, int cap) { return (int)std::min<uint32_t>(batch, cap); }

// Everything the step decides before its first launch.  plan_step fills it
// from the shape and the arithmetic alone: no buffer, no HIP call.
struct StepPlan {
  int ow, oh, w3, h3;
  // x6: split-bf16 l12x6 + d1x6.  l3r / l3_fused: layer 3 by l3r_delta, else
  // by l3_delta, else (not l3_fused) by the op-level kernels.  d3mode: l3r
  // leaves delta3 and layer 2's relu' mask in the D2 region and d1x6 forms
  // delta2 (d1x6.hpp kD3).  kD1c: the fp32 delta1 kernel is d1c, split over
  // d1c_parts ranges of chunks per sample.
  bool x6, l3r, l3_fused, d3mode, kD1c;
  bool d1tr;                 // d3mode: d1x6 with the delta2 part images (D6Lds::tr)
  int d1c_parts;
  RunGeom rg;
  int g12, g3, gd;           // grids of l12, layer 3 and delta1 (one slab per block of the last two)
  size_t lds12, lds3, ldsd;  // their dynamic LDS bytes
  size_t s12, s3, ssq;       // slab regions in floats: layers 1-2 | layer 3 | squared error
  size_t bytes;              // the three in bytes
  size_t m2_off;             // d3mode: dwords from D2 to the mask (delta3 first, 256-B aligned)
  // d3mode: dwords from D2 to the launch maxima behind the mask (256-B aligned
  // each): one max |X| per l12x6 block at mx_off, one max |delta3| per l3r
  // block at d3mx_off (d1x6.hpp: its launch scale)
  size_t mx_off, d3mx_off;
  int a1_layout;             // what l12 writes: kA1Runs or kA1Blocked
  // the names the step notes (srcnn_last_kernels): l12's without the lazy
  // suffix, layer 3's, delta1's
  const char *k12, *k3, *kd1;
};

template <typename NetT>
static bool plan_step(uint32_t w, uint32_t h, uint32_t batch, int arith, StepPlan* out) {
  constexpr int N2 = NetT::N2, F1 = NetT::F1, F3 = NetT::F3;
  StepPlan& p = *out = {};
  const int ow = p.ow = w - F1 + 1, oh = p.oh = h - F1 + 1;
  const int w3 = p.w3 = ow - F3 + 1, h3 = p.h3 = oh - F3 + 1;
  if ((int)(w * h) > kXsMax || (int)w > kL12S || (int)h > kL12Rows || w3 <= 0 || h3 <= 0) return false;
  // l3_delta holds two A2 tiles in LDS: up to 640 A2 pixels (33x33 tiles at
  // f1 = 9).  Larger tiles (e.g. the reference's 36x36 samples, profile.py:7)
  // keep l12 and d1 and run layer 3 through the op-level kernels instead
  // (ops_fast.hip: L3 forward, last delta, delta2, gW3 over HWC A2 / A3 / D3).
  // n2 = 32: l3r (A2 in registers, two blocks per CU) where the tile fits it
  p.l3r = N2 == 32 && l3r_fits<F3>(ow, oh, w3, h3);
  p.lds3 = p.l3r ? L3RLds<F3>(ow, oh).bytes() : l3_lds_bytes<N2, F3>(ow, oh);
  // (n2 = 32 tiles past l3r's 512 outputs, e.g. f3 = 3 on 33x33: l3_delta)
  p.l3_fused =
      p.l3r || (p.lds3 <= (size_t)kLdsMax && w3 * h3 <= kL3MaxOut &&
                ((ow * oh + 15) / 16 + kL3Threads / 64 - 1) / (kL3Threads / 64) <= L3Lds<N2, F3>::kUnitsPerWave);
  p.g12 = grid_for_batch(batch, kL12Grid);
  // split-bf16 products (l12x6.hpp, d1x6.hpp) serve the default net where both fit
  p.x6 = NetT::kDefault12 && arith == 0 && l12x6_fits(w, h) && d1x6_fits(w, h);
  p.a1_layout = p.x6 ? kA1Runs : kA1Blocked;
  p.rg = run_geom(ow, oh);
  // l3r: up to 2 resident blocks per CU; between 256 and 1024 samples keep
  // two samples per block, so the second sample's A2 loads run under the first
  // one's delta2 phase (512 tiles: l3 0.0306 -> 0.0295 ms; at batch 4096 a
  // 256-block grid is slower, 0.155 -> 0.167 ms; profiles/r04_ab_l3rgrid)
  const int b3 = (int)batch;
  p.g3 = p.l3r ? std::min(kL3RGrid, std::max(std::min(b3, 256), (b3 + 1) / 2)) : grid_for_batch(batch, 256);
  p.kD1c = NetT::kDefault12 && d1c_fits(w, h);
  // d1c below kD1cGrid samples: each sample's chunks split into `parts`
  // ranges (work items), so the grid still fills every CU's 4 block slots
  const int nch1 = (ow * oh + 31) / 32;
  p.d1c_parts = p.kD1c ? std::max(1, std::min({4, nch1, kD1cGrid / (int)std::max<uint32_t>(batch, 1)})) : 1;
  while (p.d1c_parts > 1 && (p.d1c_parts - 1) * ((nch1 + p.d1c_parts - 1) / p.d1c_parts) >= nch1)
    p.d1c_parts--;  // every part holds at least one chunk (the kernel's DMA pipeline assumes it)
  // split-bf16 with l3r: delta2 is formed in d1x6 from l3r's delta3, where
  // delta3 and the mask (one dword per A2 pixel) fit the region sized for
  // delta2 (ow * oh * N2 floats per sample)
  p.m2_off = ((size_t)batch * w3 * h3 + 63) & ~(size_t)63;
  // (the maxima always fit where the mask does: they end within (2 ow oh + 1)
  // batch + 3 x 63 + kL3RGrid dwords, and a d3mode tile has nch >= 4, ow oh > 96;
  // no served tile changes its mode by the last condition)
  p.mx_off = (p.m2_off + (size_t)batch * ow * oh + 63) & ~(size_t)63;
  p.d3mx_off = (p.mx_off + p.g12 + 63) & ~(size_t)63;
  p.d3mode = p.x6 && p.l3r && F3 <= 5 && d1x6_fits(w, h, true) && l3r_d3_fits<F3>(ow, oh) &&
             p.m2_off + (size_t)batch * ow * oh <= (size_t)batch * ow * oh * N2 &&
             p.d3mx_off + kL3RGrid <= (size_t)batch * ow * oh * N2;
  const int gd6 = grid_for_batch(batch, 256);  // d1x6
  const int gdf = p.kD1c ? (int)std::min<size_t>((size_t)batch * p.d1c_parts, kD1cGrid) : grid_for_batch(batch, 512);
  p.gd = p.x6 ? gd6 : gdf;
  p.lds12 = p.x6 ? H6Lds(w, h).bytes : 0;
  const D6Lds ld6(w, h, p.rg, p.d3mode);
  p.ldsd = p.x6 ? ld6.bytes : p.kD1c ? d1c_lds_bytes(w, h) : 0;
  // d1x6 in delta3 mode: its form with the delta2 part images (d6tr.hpp) where
  // D6Lds has room for them
  p.d1tr = p.x6 && p.d3mode && ld6.tr;
  p.k12 = p.x6 ? "l12x6_fwd" : "l12_fwd";
  p.k3 = !p.l3_fused ? "l3_op_level" : !p.l3r ? "l3_delta" : p.d3mode ? "l3r_d3" : "l3r_delta";
  // (d1x6_d3: the form with the part images; d1x6_d3_sc: the fp32 scratch form)
  p.kd1 = p.x6 ? (p.d1tr ? "d1x6_d3" : p.d3mode ? "d1x6_d3_sc" : "d1x6_grad12") : p.kD1c ? "d1c_grad12" : "d1_grad12";
  // (the workspace holds either arithmetic's slabs: srcnn_set_arith between
  // the size query and the step needs no new query)
  p.s12 = (size_t)std::max(gd6, gdf) * NetT::P12;
  p.s3 = (size_t)p.g3 * NetT::P3;  // gW3 slabs
  p.ssq = p.g3;
  if (!p.l3_fused) {  // the op-level gW3 slabs; the same space serves the squared-error reduction
    p.s3 = fast::grad_workspace_bytes(N2, 1, F3, w3, h3, batch) / sizeof(float);
    if (p.s3 == 0) return false;  // the op-level layer-3 kernels do not take this tile either
    p.s3 = std::max<size_t>(p.s3, reduce_blocks((size_t)batch * w3 * h3) + 1);
    p.ssq = 0;
  }
  p.bytes = (p.s12 + p.s3 + p.ssq) * sizeof(float);
  return true;
}
