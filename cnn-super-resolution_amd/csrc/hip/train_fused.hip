// train_fused.hip -- gfx950 fused training step for SRCNN nets with a 1x1
// middle layer (f2 == 1), e.g. the reference default n1=64, n2=32, f1=9, f3=5.
//
// The reference runs one OpenCL kernel per op (ConfigBasedDataPipeline.cpp:
// 200-323): 3 forward, last delta, 2 deltas, 3 gradient kernels, every tensor
// round-tripping through global memory and the gradients summed serially per
// weight (backpropagate.cl:89-106).  Here the same mathematics runs as three
// kernels plus a deterministic reduction; each stage has one kernel per
// arithmetic and tile range, one header each, and the plan (fused_plan.hpp,
// StepPlan) picks among them by the flag named last:
//
//   layers 1-2 forward: A1 to HBM (backward needs it) and on into L2, A2 to HBM
//     l12.hpp        l12_fwd_kernel<N1, N2, F1, lazy>: fp32 MFMA implicit GEMMs
//                    per 32-pixel chunk, both layers transposed; blocked A1.
//                    Every net.  !x6
//     l12x6.hpp      l12x6_fwd_kernel<lazy>: layer 1 on two-part fp16 split
//                    products, layer 2 on three-part bf16 ones (split.hpp); A1
//                    in run order (runs.hpp).  The default layers 1-2 under
//                    arithmetic 0 where l12x6 and d1x6 both fit.  x6
//   layer 3 forward, last delta (reference quirk), squared error, gW3 / gB3,
//   and delta2 (or, for d1x6, delta3 and layer 2's relu' mask):
//     l3_delta.hpp   l3_delta_kernel<N2, F3>: fp32 MFMA, Q trick, two A2 tiles
//                    in LDS, one block per CU.  l3_fused && !l3r
//     l3r.hpp        l3r_delta_kernel<F3, d3>: fp32 MFMA with the A2 tile in
//                    registers, two blocks per CU; n2 = 32, tiles of up to 640
//                    A2 pixels.  l3r; its <F3, true> form, which leaves delta3
//                    and the mask for d1x6: d3mode
//     (larger tiles: the op-level kernels of ops_fast.hip.  !l3_fused)
//   delta1 = relu'(A1) * (delta2 . W2^T), gW2 / gB2, gW1 / gB1, one slab a block:
//     d1.hpp         d1_grad12_kernel<N1, N2, F1>: fp32 MFMA, one wave per
//                    chunk, operands by LDS-DMA.  Every net.  !x6 && !kD1c
//     d1c.hpp        d1c_grad12_kernel<9>: fp32 MFMA, a block's four waves on
//                    one chunk, 16 channels each, four blocks per CU; each
//                    sample's chunks in d1c_parts ranges.  The default layers
//                    1-2, tiles up to 40 wide.  !x6 && kD1c
//     d1x6.hpp       d1x6_grad12_kernel<d3, tr>: bf16 split products (gW1 on
//                    two-part fp16 ones in the d3 form, scaled once per launch
//                    from the maxima l12x6 and l3r leave); <true, .> forms delta2
//                    itself from l3r's delta3 (d3taps.hpp), <true, true> passes
//                    delta2's parts through a bf16 image (d6tr.hpp).  x6; d3mode;
//                    d1tr
//   slab_reduce.hpp  slab_reduce_kernel: per-block partial gradients summed in
//                    block order -> grads, with the SGD update where asked
//   a1_unlayout.hpp  unblock_a1_kernel, unrun_a1_kernel: either A1 layout ->
//                    HWC (srcnn_train_activations; not part of the step)
//
// fused_layout.hpp holds what the kernels and the plan share: the geometry
// structs, the tile limits and every LDS layout with its "fits" rule.
//
// HBM traffic per 33x33 tile on the fp32 trio: X 4.4 KB + A1 160 KB (write +
// read) + A2 80 KB (write + read) + delta2 80 KB (write + read) ~ 650 KB vs
// 1.54 MB for the layer-by-layer dataflow; d3mode drops
// delta2's round trip.  Results are deterministic: the sample -> block -> wave
// assignment is static and every sum has a fixed order; no float atomics
// anywhere.
//
// This file is the host side: the slab reduction's launcher, the step's
// launcher (run: every decision comes from the plan), the plan query, preload,
// the A1 layout helpers and the clock read-out.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>

#include "common.hpp"
#include "lds_dma.hpp"
#include "mfma.hpp"
#include "ops.hpp"
#include "split.hpp"

namespace srcnn {
namespace fused {

using mfma::crow;
using mfma::f32x16;
using mfma::f32x4;
using mfma::mma;
using mfma::zero16;

// held-clock probe slots (common.hpp): 0 l12_fwd, 1 l3_delta, 2 d1_grad12
__device__ unsigned long long g_clk[3][kClockBlocks][2];

// streaming-cache hints (bits): 1 l3 A2 DMA nt, 2 l3 D2 stores nt, 4 d1
// operand DMA nt, 8 l12 A1 stores nt.  Default 1 | 8 (same-box A/B, steady
// state, 2 reps: step 0.938 -> 0.931 ms): A1 (655 MB per step, read back only
// by d1) streams past the caches, so more of the A2 that l12 writes just
// before l3 reads it stays in the 256 MB MALL (l3 -4.5%); nt on the D2
// stores or the d1 DMA was slower.
constexpr int kNtMask = 9;

// the family: layouts and limits (host and device), one header per kernel, the
// plan (host)
#include "d3taps.hpp"
#include "fused_layout.hpp"
#include "l12.hpp"
#include "l12x6.hpp"
#include "l3_delta.hpp"
#include "l3r.hpp"
#include "d1.hpp"
#include "d1c.hpp"
#include "d1x6.hpp"
#include "slab_reduce.hpp"
#include "a1_unlayout.hpp"
#include "fused_plan.hpp"

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
int reduce_slabs(const SlabSeg* segs, int nseg, hipStream_t s, const SlabUpdate* up, int assign) {
  SlabSegs ss{};
  if (up) ss.up = *up;
  ss.assign = assign;
  int blocks = 0;
  for (int k = 0; k < kMaxSlabSegs; k++) {
    ss.first[k] = blocks;
    if (k < nseg) {
      ss.seg[k] = segs[k];
      blocks += (segs[k].P + kSlabCols - 1) / kSlabCols;
    } else {
      ss.seg[k] = SlabSeg{nullptr, nullptr, 0, 0, 0};
    }
  }
  ss.first[kMaxSlabSegs] = blocks;
  hipLaunchKernelGGL(slab_reduce_kernel, dim3(blocks), dim3(1024), 0, s, ss);
  SRCNN_LAUNCH_TRY();
  return SRCNN_OK;
}

// the A1 region and layout this thread's last step wrote (a1_layout_written:
// srcnn_train_activations)
static thread_local const float* t_a1_region = nullptr;
static thread_local int t_a1_layout = -1;

// Carves the slab and launches in order; every decision comes from the plan.
template <typename NetT>
static int run(const StepPlan& p, const srcnn_net* net, uint32_t w, uint32_t h, uint32_t batch,
               const StepBuffers& b, hipStream_t s, const SlabUpdate* up, const LazyUpdate* lz) {
  constexpr int N1 = NetT::N1, N2 = NetT::N2, F1 = NetT::F1, F3 = NetT::F3;
  if (b.slab_bytes < p.bytes)
    return fail(SRCNN_ERR_WORKSPACE, "fused train step: slab workspace %zu B < %zu B", b.slab_bytes, p.bytes);
  float* slab12 = b.slab;
  float* slab3 = slab12 + p.s12;
  float* sqs = slab3 + p.s3;
  const float *X = b.X, *T = b.T;
  float *grads = b.grads, *A1 = b.A1, *A2 = b.A2, *D2 = b.D2, *A3 = b.A3;
  // lazy: l12 applies the pending update and the step runs on lz->Po
  const bool lazy = lz && lz->batch > 0.0f;
  const LazyUpdate lu = lazy ? *lz : LazyUpdate{};
  const auto P = split_params(lazy ? lz->Po : b.params, net);
  const int ow = p.ow, oh = p.oh, w3 = p.w3, h3 = p.h3;
  const Geom g{(int)w, (int)h, ow, oh, (int)batch};
  // d3mode: the launch maxima behind the mask in the D2 region, one slot per
  // block of l12x6 (max |X|) and of l3r (max |delta3|), read by d1x6
  float* const xmax = p.d3mode ? D2 + p.mx_off : nullptr;
  float* const d3max = p.d3mode ? D2 + p.d3mx_off : nullptr;
  {
    SRCNN_PROFILE("l12_fwd_mfma", s);
    kernels_note(lazy ? (std::string(p.k12) + "_lazy").c_str() : p.k12);
    note_a1_layout(A1, p.a1_layout);
    const dim3 grid(p.g12), blk(256);
    const auto k6 = lazy ? l12x6_fwd_kernel<true> : l12x6_fwd_kernel<false>;
    const auto k = lazy ? l12_fwd_kernel<N1, N2, F1, true> : l12_fwd_kernel<N1, N2, F1>;
    // l12x6: 78 KB of LDS for 33x33 tiles, two blocks per CU
    if (int rc = p.x6 ? launch(k6, grid, blk, p.lds12, s, X, P.W1, P.B1, P.W2, P.B2, A1, A2, g, p.rg, lu, xmax)
                      : launch(k, grid, blk, 0, s, X, P.W1, P.B1, P.W2, P.B2, A1, A2, g, lu))
      return rc;
  }
  // lazy, layer 3 on the op-level kernels: they accumulate, so their
  // gradient segment starts from zero (after l12 has read the pending one)
  if (lz && !p.l3_fused)
    SRCNN_HIP_TRY(hipMemsetAsync(grads + NetT::P12, 0, NetT::P3 * sizeof(float), s));
  const L3Geom lg{(int)w, (int)h, ow, oh, w3, h3, (int)batch};
  uint32_t* M2 = p.d3mode ? reinterpret_cast<uint32_t*>(D2) + p.m2_off : nullptr;
  kernels_note(p.k3);
  if (p.l3_fused) {
    SRCNN_PROFILE("l3_delta_fused", s);
    const dim3 grid(p.g3);
    const auto kr = p.d3mode ? l3r_delta_kernel<F3, true> : l3r_delta_kernel<F3, false>;
    if (int rc = p.l3r ? launch(kr, grid, dim3(kL3RThreads), p.lds3, s, A2, T, P.W3, P.B3, D2, slab3, sqs, A3, M2, d3max, lg)
                       : launch(l3_delta_kernel<N2, F3>, grid, dim3(kL3Threads), p.lds3, s, A2, T, P.W3, P.B3, D2, slab3, sqs, A3, lg))
      return rc;
  } else {
    // ConfigBasedDataPipeline.cpp:200-323 for layer 3 on the op-level kernels
    const int rf = fast::try_conv_fwd(A2, A3, P.W3, P.B3, ow, oh, N2, 1, F3, 0, batch, s);
    if (rf != 1) return rf < 0 ? rf : fail(SRCNN_ERR_INVALID, "fused step: no layer-3 kernel for %dx%d", ow, oh);
    if (b.sq_err)
      if (int rc = reduce(2, A3, T, (size_t)batch * w3 * h3, w, h, w3, h3, b.sq_err, 1, slab3,
                          p.s3 * sizeof(float), s))
        return rc;
    if (int rc = generic::last_delta(T, A3, b.D3, w, h, w3, h3, batch, s)) return rc;
    const int rd = fast::try_conv_delta(b.D3, A2, D2, P.W3, F3, N2, 1, ow, oh, batch, s);
    if (rd != 1) return rd < 0 ? rd : fail(SRCNN_ERR_INVALID, "fused step: no delta2 kernel for %dx%d", ow, oh);
    const int rg = fast::try_conv_grad_acc(A2, b.D3, grads + NetT::P12, grads + NetT::P12 + NetT::P3 - 1, N2, 1,
                                           F3, w3, h3, batch, slab3, p.s3 * sizeof(float), s);
    if (rg != 1) return rg < 0 ? rg : fail(SRCNN_ERR_INVALID, "fused step: no gW3 kernel for %dx%d", ow, oh);
  }
  {
    SRCNN_PROFILE("delta1_grad12_fused", s);
    kernels_note(p.kd1);
    const dim3 grid(p.gd), blk(256);
    const D3Geom dg{w3, h3, F3};
    const D6MaxGeom mg{p.g12, p.g3};  // the blocks of l12x6 and l3r, each with a sample
    // d1x6<true>: D2 holds delta3 and M2 the mask; A2 is not read then
    const auto k6 = p.d1tr ? d1x6_grad12_kernel<true, true> : p.d3mode ? d1x6_grad12_kernel<true> : d1x6_grad12_kernel<false>;
    if (int rc = p.x6 ? launch(k6, grid, blk, p.ldsd, s, X, A1, D2, A2, M2, xmax, d3max, mg, P.W2, P.W3, slab12, g, p.rg, dg)
                 : p.kD1c ? launch(d1c_grad12_kernel<9>, grid, dim3(256 * kD1cTeams), p.ldsd, s, X, A1, D2, P.W2, slab12, g,
                                   d1c_xs_floats(h), p.d1c_parts)
                          : launch(d1_grad12_kernel<N1, N2, F1>, grid, blk, 0, s, X, A1, D2, P.W2, slab12, g))
      return rc;
  }
  SRCNN_PROFILE("slab_reduce", s);
  const bool update = up && p.l3_fused;
  kernels_note(update ? "slab_reduce_update" : "slab_reduce");
  const SlabSeg segs[3] = {{slab12, grads, p.gd, NetT::P12, 0},
                           {slab3, grads + NetT::P12, p.g3, NetT::P3, 0},
                           {sqs, b.sq_err, p.g3, 1, 0}};
  // with `up`, segments 0 and 1 are every parameter: the update rides along
  SlabUpdate u{};
  if (update) {
    u = *up;
    u.nseg = 2;
  }
  // lazy: the slabs are this step's whole gradient (assigned, not added)
  const int assign = lz ? (p.l3_fused ? 2 : 1) : 0;
  if (int rc = p.l3_fused ? reduce_slabs(segs, b.sq_err ? 3 : 2, s, &u, assign) : reduce_slabs(segs, 1, s, nullptr, assign))
    return rc;
  return update ? 2 : 1;
}

bool train_plan(const srcnn_net* net, uint32_t w, uint32_t h, uint32_t batch, StepNeed* need) {
  return with_net(net, [&](auto n) {
    StepPlan p;
    if (!plan_step<decltype(n)>(w, h, batch, g_arith, &p)) return 0;
    *need = {p.bytes, p.a1_layout};
    return 1;
  });
}

int train_fwd_bwd(const srcnn_net* net, uint32_t w, uint32_t h, uint32_t batch, const StepBuffers& b,
                  hipStream_t s, const SlabUpdate* up, const LazyUpdate* lz) {
  return with_net(net, [&](auto n) {
    StepPlan p;
    if (!plan_step<decltype(n)>(w, h, batch, g_arith, &p)) return 0;
    return run<decltype(n)>(p, net, w, h, batch, b, s, up, lz);
  });
}

int preload(const srcnn_net* net) {
  return with_net(net, [&](auto n) {
    using N = decltype(n);
    // the kernels of every net, and those built for layers 1-2 of the default net
    const void* every[] = {(const void*)l12_fwd_kernel<N::N1, N::N2, N::F1>, (const void*)l12_fwd_kernel<N::N1, N::N2, N::F1, true>,
                           (const void*)l3_delta_kernel<N::N2, N::F3>, (const void*)d1_grad12_kernel<N::N1, N::N2, N::F1>,
                           (const void*)slab_reduce_kernel, (const void*)l3r_delta_kernel<N::F3, false>,
                           (const void*)l3r_delta_kernel<N::F3, true>};
    const void* default12[] = {(const void*)d1c_grad12_kernel<9>, (const void*)l12x6_fwd_kernel<false>,
                               (const void*)l12x6_fwd_kernel<true>, (const void*)d1x6_grad12_kernel<false>,
                               (const void*)d1x6_grad12_kernel<true>, (const void*)d1x6_grad12_kernel<true, true>};
    int rc = resolve_kernels(every, sizeof(every) / sizeof(*every));
    if (!rc && N::kDefault12) rc = resolve_kernels(default12, sizeof(default12) / sizeof(*default12));
    return rc ? rc : 1;
  });
}

void note_a1_layout(const float* A1, int layout) {
  t_a1_region = A1;
  t_a1_layout = layout;
}

int a1_layout_written(const float* A1) { return A1 && A1 == t_a1_region ? t_a1_layout : -1; }

size_t a1_chunks(uint32_t ow, uint32_t oh) {
  return std::max<size_t>((ow * oh + 31) / 32, run_geom((int)ow, (int)oh).nch);
}

int unrun_a1(const float* A1t, float* A1, uint32_t ow, uint32_t oh, uint32_t batch, hipStream_t s) {
  const size_t total = (size_t)batch * ow * oh * 64;
  if (total == 0) return SRCNN_OK;
  const int blocks = (int)std::min<size_t>((total + 255) / 256, 4096);
  hipLaunchKernelGGL(unrun_a1_kernel, dim3(blocks), dim3(256), 0, s, A1t, A1, run_geom((int)ow, (int)oh), total);
  SRCNN_LAUNCH_TRY();
  return SRCNN_OK;
}

int unblock_a1(const float* A1b, float* A1, uint32_t n1, uint32_t npx, uint32_t batch, hipStream_t s) {
  const size_t total = (size_t)batch * npx * n1;
  if (total == 0) return SRCNN_OK;
  const int blocks = (int)std::min<size_t>((total + 255) / 256, 4096);
  hipLaunchKernelGGL(unblock_a1_kernel, dim3(blocks), dim3(256), 0, s, A1b, A1, (int)n1, (int)npx,
                     total);
  SRCNN_LAUNCH_TRY();
  return SRCNN_OK;
}

int train_clock(int slot, double* ghz) {
  unsigned long long a[3][kClockBlocks][2];
  SRCNN_HIP_TRY(hipMemcpyFromSymbol(a, HIP_SYMBOL(g_clk), sizeof(a)));
  *ghz = clock_ghz(a[slot]);
  return SRCNN_OK;
}

}  // namespace fused
}  // namespace srcnn

