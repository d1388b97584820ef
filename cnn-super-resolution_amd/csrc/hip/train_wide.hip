// train_wide.hip -- gfx950 training step for SRCNN nets whose middle layer is
// spatial (f2 > 1): BASELINE.json configs[3], n1=128, n2=64, f1=9, f2=5, f3=5.
//
// The reference runs the same nine OpenCL kernels as for the default net
// (ConfigBasedDataPipeline.cpp:200-323); for this net 95% of the step's FLOPs
// are the three f2 x f2 x n1 x n2 contractions of layer 2 (forward, delta1 and
// gW2: 180.6 MFLOP each per 33x33 tile).  Here every stage is
// an fp32 MFMA implicit GEMM over the reference-layout (HWC) buffers (the
// kernels live in one header per family: wl1.hpp, wconv_mfma.hpp, wd1g16.hpp,
// wl3.hpp, wgrad2.hpp; their split-bf16 forms, the default arithmetic, in
// wl1x6.hpp, wg1x6.hpp, wl2x6.hpp, wgrad2x6.hpp):
//
//   prepack_w2   W2 -> two operand-ordered images (forward / flipped-transposed
//                for delta1), one 1 KB coalesced load per wave per k-step
//   wl1_fwd      L1 9x9x1 -> n1 + bias + ReLU (K = 81 taps, X tile in LDS)
//   conv_mfma    L2 forward (+bias, ReLU) and delta1 = relu'(A1) * full-conv
//                (delta2, W2^T): input channel chunks staged HBM -> LDS by
//                LDS-DMA (double-buffered, 80-B pixel rows: conflict-free
//                ds_read_b128), accumulators for the whole sample in registers;
//                the delta1 variant feeds its masked tiles straight into
//                gW1 / gB1 (ones row) MFMAs, so delta1 never reaches HBM
//   wl3          L3 (Q trick) + last delta (reference relu' quirk) + squared
//                error + delta2 (MFMA over taps) + gW3 / gB3 (MFMA over pixels)
//   wgrad2       gW2 / gB2: 16x16x4 MFMA, K = pixels, per row band of a sample
//                (A1 rows + delta2 rows in LDS), per-block slabs
//   slab_reduce  fixed-order sum of the slabs into the gradient buffer
//
// Deterministic: static work assignment, fixed summation order, no atomics.
//
// This file is the host side: the step's launcher (the plan: wide_plan.hpp,
// over the LDS layouts and limits of wide_layout.hpp), the op-level entry
// points with their per-device W2 image, preload.
#include <algorithm>
#include <iterator>
#include <map>
#include <mutex>
#include <utility>

#include "common.hpp"
#include "lds_dma.hpp"
#include "mfma.hpp"
#include "ops.hpp"
#include "split.hpp"

namespace srcnn {
namespace wide {

using lds_dma::dma16;
using lds_dma::dma4;
using mfma::crow;
using mfma::f32x16;
using mfma::f32x4;
using mfma::lane_id;
using mfma::mma;
using mfma::mma16;
using mfma::wave_id;
using mfma::zero16;
using mfma::zero4;

// 16-B zero source for the LDS-DMA of padding / out-of-image slots
__device__ float g_zero_src[64] = {0.0f};

// Blocks go round-robin over the 8 XCDs, so blocks x, x + 8, ... share an XCD
// and its L2.  The item index that puts the NP consecutive items NP k ..
// NP k + NP - 1 (the 64-channel parts of one sample in wd1x6 and d1g16:
// readers of the same delta2 image) on one XCD, where the grid allows it.
// (wgrad2 and wgrad2x6 write the same mapping out for their channel slices:
// through this helper they compile to other code.)
template <int NP>
__device__ __forceinline__ int xcd_item() {
  int vb = blockIdx.x;
  if (gridDim.x % (8 * NP) == 0) {
    const int j = blockIdx.x / 8;
    vb = (blockIdx.x % 8 + 8 * (j / NP)) * NP + j % NP;
  }
  return vb;
}

// the family: layouts and limits (host and device), one header per kernel
// family, the plan (host)
#include "wide_layout.hpp"
#include "wl1.hpp"
#include "wl1x6.hpp"
#include "wg1x6.hpp"
#include "wconv_mfma.hpp"
#include "wl2x6.hpp"
#include "wd1g16.hpp"
#include "wl3.hpp"
#include "wgrad2.hpp"
#include "wgrad2x6.hpp"
#include "wide_plan.hpp"

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// The family's kernels at the one net (WideNet, wide_plan.hpp): the step, the
// op-level calls and preload all launch these.
namespace {
using NetT = WideNet;
constexpr int N1 = NetT::N1, N2 = NetT::N2, F1 = NetT::F1, F2 = NetT::F2, F3 = NetT::F3;
constexpr auto k_prepack_step = prepack_w2_kernel<N1, N2, F2, true>;  // forward image + d1g16's delta1 image
constexpr auto k_prepack_op = prepack_w2_kernel<N1, N2, F2>;          // forward image + conv_mfma's delta1 image
constexpr auto k_wprep_w2x6 = wprep_w2x6_kernel<N1, N2, F2>;
constexpr auto k_wprep_d1x6 = wprep_d1x6_kernel<N1, N2, F2>;
constexpr auto k_wl1 = wl1_fwd_kernel<N1, F1>;
constexpr auto k_wl1x6 = wl1x6_fwd_kernel;
constexpr auto k_conv_fwd = conv_mfma_kernel<N1, N2, F2, NetT::MT2, false>;
constexpr auto k_conv_delta = conv_mfma_kernel<N2, N1, F2, NetT::MT4, true>;
constexpr auto k_wl2x6 = wl2x6_fwd_kernel<N1, N2, F2, NetT::MT2>;
constexpr auto k_wl3 = wl3_kernel<N2, F3>;
constexpr auto k_wl3l = wl3l_kernel<N2, F3>;
constexpr auto k_wd1x6 = wd1x6_kernel<N2, N1, F2, NetT::MT4>;
constexpr auto k_d1g16 = d1g16_kernel<N2, N1, F2, F1>;
constexpr auto k_wg1x6 = wg1x6_kernel;
constexpr auto k_wgrad2 = wgrad2_kernel<N1, N2, F2>;
constexpr auto k_wgrad2x6 = wgrad2x6_kernel<N1, N2, F2>;

dim3 blocks_for(int threads) { return dim3((threads + 255) / 256); }
}  // namespace

// Carves the workspace and launches in order; every decision comes from the
// plan.  Each kernel has one profile scope, under either arithmetic.
static int run(const WidePlan& p, const srcnn_net* net, const StepBuffers& b, hipStream_t s,
               const fused::SlabUpdate* up) {
  if (b.slab_bytes < p.bytes)
    return fail(SRCNN_ERR_WORKSPACE, "wide train step: workspace %zu B < %zu B", b.slab_bytes, p.bytes);
  float* Wf = b.slab;
  float* Wd = Wf + p.nWf;
  uint16_t* Wx = reinterpret_cast<uint16_t*>(Wd + p.nWd);
  uint16_t* Wx1 = reinterpret_cast<uint16_t*>(Wd + p.nWd + p.nWx);
  float* slab1 = Wd + p.nWd + 2 * p.nWx;
  float* slab2 = slab1 + p.n1;
  float* slab3 = slab2 + p.n2;
  float* sqs = slab3 + p.n3;
  const auto P = split_params(b.params, net);
  const float *X = b.X, *T = b.T;
  float *A1 = b.A1, *D1 = b.D1, *A2 = b.A2, *D2 = b.D2, *A3 = b.A3;
  const WGeom& g = p.g;
  const dim3 blk(256);
  {
    SRCNN_PROFILE("wide_prepack_w2", s);
    // (every W2 image has one element per weight)
    if (int rc = launch(k_prepack_step, blocks_for(2 * NetT::W2), blk, 0, s, P.W2, Wf, Wd)) return rc;
    if (p.x6)
      if (int rc = launch(k_wprep_w2x6, blocks_for(NetT::W2), blk, 0, s, P.W2, Wx)) return rc;
    if (p.x6d)
      if (int rc = launch(k_wprep_d1x6, blocks_for(NetT::W2), blk, 0, s, P.W2, Wx1)) return rc;
  }
  {
    SRCNN_PROFILE("wide_l1_fwd", s);
    kernels_note(p.x6f ? "wl1x6_fwd" : "wide_l1_fwd");
    if (int rc = p.x6f ? launch(k_wl1x6, dim3(p.GL1), blk, p.lds1, s, X, P.W1, P.B1, A1, g, p.rg1)
                       : launch(k_wl1, dim3(p.GL1), blk, 0, s, X, P.W1, P.B1, A1, g))
      return rc;
  }
  {
    SRCNN_PROFILE("wide_l2_fwd", s);
    kernels_note(p.x6 ? "wl2x6_fwd" : "wide_l2_fwd");
    if (int rc = p.x6 ? launch(k_wl2x6, dim3(p.GL2), blk, p.lds2, s, A1, Wx, P.B2, A2, p.cf)
                      : launch(k_conv_fwd, dim3(p.GL2), blk, p.lds2, s, A1, Wf, P.B2, (const float*)nullptr, A2, p.cf))
      return rc;
  }
  {
    SRCNN_PROFILE("wide_l3_delta", s);
    if (int rc = p.wl3l ? launch(k_wl3l, dim3(p.G3), dim3(512), p.lds3, s, A2, T, P.W3, P.B3, D2, slab3, sqs, A3, g)
                        : launch(k_wl3, dim3(p.G3), blk, p.lds3, s, A2, T, P.W3, P.B3, D2, slab3, sqs, A3, g, p.qfloats))
      return rc;
  }
  {
    SRCNN_PROFILE(p.x6d ? "wide_delta1" : "wide_delta1_grad1", s);
    kernels_note(p.x6d ? "wd1x6" : "d1g16");
    if (int rc = p.x6d ? launch(k_wd1x6, dim3(p.GD), blk, p.ldsd, s, D2, Wx1, D1, p.cd)
                       : launch(k_d1g16, dim3(p.GD), blk, p.ldsd, s, D2, Wd, A1, X, slab1, p.cd))
      return rc;
  }
  if (p.x6d) {
    SRCNN_PROFILE("wide_grad1", s);
    if (p.x6g1) {
      kernels_note("wg1x6");
      if (int rc = launch(k_wg1x6, dim3(p.GG1), blk, p.ldsg1, s, X, D1, A1, slab1, g, p.rg1)) return rc;
    } else if (int rc = fast::l1_grad_slabs(X, D1, A1, slab1, N1, F1, g.w, g.h, g.batch, p.GW1, s); rc != 1) {
      return rc ? rc : fail(SRCNN_ERR_INVALID, "wide step: no layer-1 gradient kernel for n1 %d f1 %d", N1, F1);
    }
  }
  {
    SRCNN_PROFILE("wide_grad2", s);
    kernels_note(p.x6g ? "wgrad2x6" : "wgrad2");
    if (int rc = launch(p.x6g ? k_wgrad2x6 : k_wgrad2, dim3(p.GG2), dim3(512), p.ldsg2, s, A1, D2, slab2, p.g2)) return rc;
  }
  SRCNN_PROFILE("slab_reduce", s);
  const fused::SlabSeg segs[4] = {{slab1, b.grads, p.nslab1, NetT::P1},
                                  {slab2, b.grads + NetT::P1, p.g2.groups, NetT::P2},
                                  {slab3, b.grads + NetT::P1 + NetT::P2, p.G3, NetT::P3},
                                  {sqs, b.sq_err, p.G3, 1}};
  // with `up` (srcnn_train_step), segments 0-2 are every parameter
  fused::SlabUpdate u{};
  if (up) {
    u = *up;
    u.nseg = 3;
  }
  if (int rc = fused::reduce_slabs(segs, b.sq_err ? 4 : 3, s, &u)) return rc;
  return up ? 2 : 1;
}

static bool is_wide_net(const srcnn_net* net) {
  return net->n1 == N1 && net->n2 == N2 && net->f1 == F1 && net->f2 == F2 && net->f3 == F3;
}

bool train_plan(const srcnn_net* net, uint32_t w, uint32_t h, uint32_t batch, StepNeed* need) {
  WidePlan p;
  if (!is_wide_net(net) || !plan_step(w, h, batch, g_arith, &p)) return false;
  *need = {p.bytes, fused::kA1Hwc};
  return true;
}

int train_fwd_bwd(const srcnn_net* net, uint32_t w, uint32_t h, uint32_t batch, const StepBuffers& b,
                  hipStream_t s, const fused::SlabUpdate* up) {
  WidePlan p;
  if (!is_wide_net(net) || !plan_step(w, h, batch, g_arith, &p)) return 0;
  return run(p, net, b, s, up);
}

// ---------------------------------------------------------------------------
// op-level entry points (srcnn_conv_fwd / _delta / _grad_acc through
// ops_fast.hip) for the wide middle layer: 5x5, n1 = 128 <-> n2 = 64, the
// same kernels as the net-level step, over the caller's reference-layout
// buffers.  The operand images of W2 live in a per-(device, stream) buffer
// of the library.  1 = handled,
// 0 = shape not served here, < 0 = error.
// ---------------------------------------------------------------------------
namespace {
// the middle layer these calls serve
bool is_wide_l2(uint32_t n_prev, uint32_t n_cur, uint32_t f) { return n_prev == N1 && n_cur == N2 && f == F2; }

// W2 operand images of the op-level calls: ONE device buffer per device
// (2 x 819 KB), reused in stream order.  A W2Image lease holds the device's
// lock from the prepack launch to the consumer launch; a call on another
// stream than the previous user first waits (hipStreamWaitEvent) for the
// event recorded after that user's consumer kernel, so no two streams ever
// share the image at once and nothing grows with the number of streams.
struct ImgSlot {
  float* buf = nullptr;
  hipEvent_t done = nullptr;  // recorded after the last consumer kernel
  hipStream_t last = nullptr;
  bool used = false;
  std::mutex mu;
};
std::mutex g_img_mu;
std::map<int, ImgSlot> g_img;

class W2Image {
 public:
  // prepacks W2 into the device's image on stream s; rc() < 0 on error
  W2Image(const float* W2, hipStream_t s) : s_(s) { rc_ = acquire(W2); }
  ~W2Image() {
    if (slot_) {
      if (rc_ == SRCNN_OK) {
        (void)hipEventRecord(slot_->done, s_);
        slot_->last = s_;
        slot_->used = true;
      }
      slot_->mu.unlock();
    }
  }
  int rc() const { return rc_; }
  float* img() const { return slot_ ? slot_->buf : nullptr; }

 private:
  int acquire(const float* W2) {
    int dev = 0;
    SRCNN_HIP_TRY(hipGetDevice(&dev));
    {
      std::lock_guard<std::mutex> lk(g_img_mu);
      slot_ = &g_img[dev];  // std::map nodes never move
    }
    slot_->mu.lock();
    if (!slot_->buf) {
      SRCNN_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&slot_->buf),
                              2 * align_f(WideNet::W2) * sizeof(float)));
      SRCNN_HIP_TRY(hipEventCreateWithFlags(&slot_->done, hipEventDisableTiming));
    }
    if (slot_->used && slot_->last != s_) SRCNN_HIP_TRY(hipStreamWaitEvent(s_, slot_->done, 0));
    SRCNN_PROFILE("wide_prepack_w2", s_);
    return launch(k_prepack_op, blocks_for(2 * WideNet::W2), dim3(256), 0, s_, W2, slot_->buf,
                  slot_->buf + align_f(WideNet::W2));
  }
  hipStream_t s_;
  ImgSlot* slot_ = nullptr;
  int rc_ = SRCNN_OK;
};
}  // namespace

int op_conv_fwd(const float* in, float* out, const float* W, const float* B, uint32_t in_w,
                uint32_t in_h, uint32_t n_prev, uint32_t n_cur, uint32_t f, int relu,
                uint32_t batch, hipStream_t s) {
  if (!is_wide_l2(n_prev, n_cur, f) || !relu) return 0;
  const CGeom cf = conv_fwd_geom((int)in_w, (int)in_h, (int)batch);
  W2Image w2i(W, s);
  if (w2i.rc()) return w2i.rc();
  float* img = w2i.img();
  SRCNN_PROFILE("conv_fwd_wide_mfma", s);
  const int items = (int)batch * (N2 / 64) * conv_windows(cf);
  if (int rc = launch(k_conv_fwd, dim3(std::min(items, 256)), dim3(256), DmaImgLds(cf).bytes, s, in, img, B,
                      (const float*)nullptr, out, cf))
    return rc;
  return 1;
}

int op_conv_delta(const float* d_next, const float* y_curr, float* d_curr, const float* W_next,
                  uint32_t f_next, uint32_t n_curr, uint32_t n_next, uint32_t curr_w,
                  uint32_t curr_h, uint32_t batch, hipStream_t s) {
  if (!is_wide_l2(n_curr, n_next, f_next)) return 0;
  const CGeom cd = conv_delta_geom((int)curr_w, (int)curr_h, (int)batch);
  W2Image w2i(W_next, s);
  if (w2i.rc()) return w2i.rc();
  float* img = w2i.img();
  SRCNN_PROFILE("conv_delta_wide_mfma", s);
  const int items = (int)batch * (N1 / 64) * conv_windows(cd);
  if (int rc = launch(k_conv_delta, dim3(std::min(items, 256)), dim3(256), DmaImgLds(cd).bytes, s, d_next,
                      img + align_f(WideNet::W2), (const float*)nullptr, y_curr, d_curr, cd))
    return rc;
  return 1;
}

size_t op_grad_workspace_bytes(uint32_t n_prev, uint32_t n_cur, uint32_t f, uint32_t out_w,
                               uint32_t out_h, uint32_t batch) {
  if (!is_wide_l2(n_prev, n_cur, f)) return 0;
  G2Geom g2;
  g2_geom((int)out_w, (int)out_h, batch, &g2);  // (full-width bands or windows: either is served)
  return (size_t)g2.groups * WideNet::P2 * sizeof(float);
}

int op_conv_grad_acc(const float* in, const float* d, float* gW, float* gB, uint32_t n_prev,
                     uint32_t n_cur, uint32_t f, uint32_t out_w, uint32_t out_h, uint32_t batch,
                     void* ws, size_t ws_bytes, hipStream_t s) {
  if (!is_wide_l2(n_prev, n_cur, f)) return 0;
  G2Geom g2;
  g2_geom((int)out_w, (int)out_h, batch, &g2);
  const size_t need = (size_t)g2.groups * WideNet::P2 * sizeof(float);
  if (ws_bytes < need)
    return fail(SRCNN_ERR_WORKSPACE, "backpropagate: workspace %zu B < %zu B", ws_bytes, need);
  float* slab2 = static_cast<float*>(ws);
  {
    SRCNN_PROFILE("grad_wide_mfma", s);
    if (int rc = launch(k_wgrad2, dim3(g2.groups * (N1 / 32)), dim3(512), kG2Lds, s, in, d, slab2, g2)) return rc;
  }
  {
    SRCNN_PROFILE("slab_reduce", s);
    const int nW = WideNet::W2;
    const fused::SlabSeg segs[2] = {{slab2, gW, g2.groups, nW, WideNet::P2},
                                    {slab2 + nW, gB, g2.groups, N2, WideNet::P2}};
    if (int rc = fused::reduce_slabs(segs, 2, s)) return rc;
  }
  return 1;
}

int preload(const srcnn_net* net) {
  if (!is_wide_net(net)) return 0;
  // the training step's kernels (and the op-level delta1 / forward ones)
  const void* k[] = {(const void*)k_prepack_step, (const void*)k_wl1,       (const void*)k_conv_fwd,
                     (const void*)k_wl3l,         (const void*)k_wl3,       (const void*)k_d1g16,
                     (const void*)k_conv_delta,   (const void*)k_prepack_op, (const void*)k_wgrad2,
                     (const void*)k_wprep_w2x6,   (const void*)k_wl2x6,     (const void*)k_wgrad2x6,
                     (const void*)k_wprep_d1x6,   (const void*)k_wd1x6,     (const void*)k_wl1x6,
                     (const void*)k_wg1x6};
  int rc = resolve_kernels(k, (int)std::size(k));
  return rc ? rc : 1;
}

}  // namespace wide
}  // namespace srcnn
