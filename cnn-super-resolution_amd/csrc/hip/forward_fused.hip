// forward_fused.hip -- gfx950 inference (forward only) for SRCNN nets with a
// 1x1 middle layer (f2 == 1), for frames of any size (4K and up).
//
// The reference runs three layer launches with A1 and A2 round-tripping
// through global memory (ConfigBasedDataPipeline.cpp:200-241, kernel
// layer_uber_kernel.cl:36-96).  Here two kernels run, one header each; the
// plan (fwd_plan.hpp, FwdPlan) picks the region kernel by the flag named last:
//
//   per 32 x RH region of L1/L2 outputs: L1 (f1 x f1 x 1 -> n1) and L2 (1x1,
//   n1 -> n2) as implicit GEMMs, then the L3 "Q trick" GEMM
//   Q[p][tap] = sum_c A2[p][c] * W3[tap][c], and the L3 window sums
//   sum_tap Q[p + off(tap)][tap]  of every output the region's A2 pixels
//   reach, accumulated in LDS.  Only those partial output sums ((32 + f3 - 1) x
//   (RH + f3 - 1) floats per region) leave the CU -- A1, A2 and Q never reach
//   HBM.
//     fwd_l123.hpp    fwd_l123_kernel<N1, N2, F1, F3>: fp32 MFMAs, 256 threads,
//                     two blocks per CU, regions of up to 28 rows, static LDS
//                     (FwdLds).  Every net of the forward.  !x6
//     fwd_l123x6.hpp  fwd_l123x6_kernel: split-bf16 products (split.hpp), 512
//                     threads, one block per CU, 24-row regions, dynamic LDS
//                     (F6Lds).  The default net under arithmetic 0.  x6
//     fwd_region.hpp  what the two share: a work item's rows and its
//                     register-staged input tile, the window sums' read and
//                     store, an element of the partial-sum epilogue
//   per output pixel: A3 = B3 + the partial sums of the (at most 2 x 2) regions
//   whose A2 it reads, in a fixed order (no ReLU: SKIP_RELU), so the result is
//   deterministic.
//     fwd_seam.hpp    fwd_seam_kernel<F3>: fp32 adds.  Always; the plan sets its
//                     block width, rows per block and grid
//
// fwd_layout.hpp holds what the kernels and the plan share: the geometry, the
// region limits and both LDS layouts with their region-height rules.
//
// A region chunk is one region row of 32 pixels.  Rows / columns past the
// frame are computed on zero-padded inputs; they only reach outputs past the
// frame, which are never stored.  Each (tap row dy, partial row) pair of the
// LDS accumulator is written by exactly one chunk, so no atomics are needed.
//
// This file is the host side: the launcher (run_forward: every decision comes
// from the plan), the plan query, preload and the clock read-out.
#include <algorithm>

#include "common.hpp"
#include "mfma.hpp"
#include "ops.hpp"
#include "split.hpp"

namespace srcnn {
namespace fused {

using mfma::crow;
using mfma::f32x16;
using mfma::mma;
using mfma::zero16;

// held-clock probe slot (common.hpp) of fwd_l123
__device__ unsigned long long g_clk_fwd[1][kClockBlocks][2];

namespace {

// the family: layouts and limits (host and device), the shared region code, one
// header per kernel, the plan (host)
#include "fwd_layout.hpp"
#include "fwd_region.hpp"
#include "fwd_l123.hpp"
#include "fwd_l123x6.hpp"
#include "fwd_seam.hpp"
#include "fwd_plan.hpp"

template <typename NetT>
int run_forward(const FwdPlan& p, const srcnn_net* net, const float* X, const float* params, float* out, void* ws,
                size_t ws_bytes, hipStream_t s) {
  if (ws_bytes < p.part_bytes)
    return fail(SRCNN_ERR_WORKSPACE, "fused forward: workspace %zu B < %zu B", ws_bytes, p.part_bytes);
  float* part = static_cast<float*>(ws);
  const auto P = split_params(params, net);
  {
    SRCNN_PROFILE("fwd_l123_mfma", s);
    if (int rc = p.x6 ? launch(fwd_l123x6_kernel, dim3(p.grid), dim3(512), p.lds, s, X, P.W1, P.B1, P.W2, P.B2, P.W3, part, p.g)
                      : launch(fwd_l123_kernel<NetT::N1, NetT::N2, NetT::F1, NetT::F3>, dim3(p.grid), dim3(256), p.lds, s, X,
                               P.W1, P.B1, P.W2, P.B2, P.W3, part, p.g))
      return rc;
  }
  SRCNN_PROFILE("fwd_l3_seam", s);
  if (int rc = launch(fwd_seam_kernel<NetT::F3>, dim3(p.seam_gx, p.seam_gy, p.seam_gz), dim3(p.seam_bx), 0, s, part, P.B3,
                      out, p.g, p.seam_rb))
    return rc;
  return 1;
}

}  // namespace

bool forward_plan(const srcnn_net* net, uint32_t w, uint32_t h, uint32_t batch, size_t* ws_bytes) {
  return with_fwd_net(net, [&](auto n) {
    FwdPlan p;
    if (!plan_forward<decltype(n)>(w, h, batch, g_arith, &p)) return 0;
    *ws_bytes = p.part_bytes;
    return 1;
  });
}

int forward(const srcnn_net* net, const float* X, uint32_t w, uint32_t h, uint32_t batch,
            const float* params, float* out, void* ws, size_t ws_bytes, hipStream_t s) {
  return with_fwd_net(net, [&](auto n) {
    FwdPlan p;
    if (!plan_forward<decltype(n)>(w, h, batch, g_arith, &p)) return 0;
    return run_forward<decltype(n)>(p, net, X, params, out, ws, ws_bytes, s);
  });
}

int preload_forward(const srcnn_net* net) {
  return with_fwd_net(net, [&](auto n) {
    using N = decltype(n);
    // the kernels of every net, and the one built for the default net
    const void* every[] = {(const void*)fwd_l123_kernel<N::N1, N::N2, N::F1, N::F3>, (const void*)fwd_seam_kernel<N::F3>};
    const void* dflt[] = {(const void*)fwd_l123x6_kernel};
    int rc = resolve_kernels(every, sizeof(every) / sizeof(*every));
    if (!rc && N::kDefault) rc = resolve_kernels(dflt, sizeof(dflt) / sizeof(*dflt));
    return rc ? rc : 1;
  });
}

int forward_clock(double* ghz) {
  unsigned long long a[1][kClockBlocks][2];
  SRCNN_HIP_TRY(hipMemcpyFromSymbol(a, HIP_SYMBOL(g_clk_fwd), sizeof(a)));
  *ghz = clock_ghz(a[0]);
  return SRCNN_OK;
}

}  // namespace fused
}  // namespace srcnn
