// ops.hpp -- internal launchers behind srcnn.h (no validation here; abi.cpp
// validates shapes exactly once, then dispatches generic vs gfx950 paths, and
// abi_upscale.cpp validates and launches the image-level operators).
// The net-level families answer "is this shape served, and what does it
// need" through their *_plan queries, which take no buffer.
#pragma once

#include "common.hpp"

namespace srcnn {

namespace generic {
int conv_fwd(const float* in, float* out, const float* W, const float* B, uint32_t in_w,
             uint32_t in_h, uint32_t n_prev, uint32_t n_cur, uint32_t f, int relu,
             uint32_t batch, hipStream_t s);
int last_delta(const float* gt, const float* y, float* d, uint32_t gt_w, uint32_t gt_h,
               uint32_t out_w, uint32_t out_h, uint32_t batch, hipStream_t s);
int conv_delta(const float* d_next, const float* y_curr, float* d_curr, const float* W_next,
               uint32_t f_next, uint32_t n_curr, uint32_t n_next, uint32_t curr_w,
               uint32_t curr_h, uint32_t batch, hipStream_t s);
size_t grad_workspace_bytes(uint32_t n_prev, uint32_t n_cur, uint32_t f, uint32_t batch);
int conv_grad_acc(const float* in, const float* d, float* gW, float* gB, uint32_t n_prev,
                  uint32_t n_cur, uint32_t f, uint32_t out_w, uint32_t out_h, uint32_t batch,
                  void* ws, size_t ws_bytes, hipStream_t s);
}  // namespace generic

// gfx950 specialisations (ops_fast.hip).  Each `try_*` returns 1 when it
// handled the call, 0 when the shape is not specialised, <0 on error.
namespace fast {
int try_conv_fwd(const float* in, float* out, const float* W, const float* B, uint32_t in_w,
                 uint32_t in_h, uint32_t n_prev, uint32_t n_cur, uint32_t f, int relu,
                 uint32_t batch, hipStream_t s);
int try_conv_delta(const float* d_next, const float* y_curr, float* d_curr, const float* W_next,
                   uint32_t f_next, uint32_t n_curr, uint32_t n_next, uint32_t curr_w,
                   uint32_t curr_h, uint32_t batch, hipStream_t s);
// workspace the fast gradient path needs for this shape (0 = not specialised)
size_t grad_workspace_bytes(uint32_t n_prev, uint32_t n_cur, uint32_t f, uint32_t out_w,
                            uint32_t out_h, uint32_t batch);
int try_conv_grad_acc(const float* in, const float* d, float* gW, float* gB, uint32_t n_prev,
                      uint32_t n_cur, uint32_t f, uint32_t out_w, uint32_t out_h,
                      uint32_t batch, void* ws, size_t ws_bytes, hipStream_t s);
// layer-1 gradient slabs of a whole batch (l1_grad_kernel: slab b = the sum over
// blocks b's samples, P = f1^2 n1 + n1 floats) from delta1 before its ReLU'
// factor (taken from A1), for the wide step's split delta1
int l1_grad_slabs(const float* X, const float* D1, const float* A1, float* slab, uint32_t n1, uint32_t f1,
                  int w, int h, int batch, int grid, hipStream_t s);
}  // namespace fast

// The buffers of one net-level training step: the caller's tensors, the regions
// of the training workspace (abi.cpp: train_ws) and the scratch behind them.
struct StepBuffers {
  const float *X, *T, *params;
  float *grads, *sq_err;
  float *A1, *D1, *A2, *D2, *A3, *D3;
  float* slab;
  size_t slab_bytes;
};
// What a family's step needs: slab bytes, and the layout it writes A1 in (fused::kA1*).
struct StepNeed {
  size_t slab_bytes;
  int a1_layout;
};
// The flat parameter (or gradient) buffer [W1|B1|W2|B2|W3|B3] by layer.
template <typename T>
struct LayerPtrs {
  T *W1, *B1, *W2, *B2, *W3, *B3;
};
template <typename T>
inline LayerPtrs<T> split_params(T* p, const srcnn_net* net) {
  size_t off[6];
  srcnn_net_offsets(net, off);
  return {p + off[0], p + off[1], p + off[2], p + off[3], p + off[4], p + off[5]};
}

// Fused training step for nets with a 1x1 middle layer (train_fused.hip).
namespace fused {
struct SlabUpdate;
struct LazyUpdate;
// Whether the family serves this net / tile under the current arithmetic, and
// if so what its step needs (else *need is left alone): the step's StepPlan.
bool train_plan(const srcnn_net* net, uint32_t w, uint32_t h, uint32_t batch, StepNeed* need);
// The step: 1 when enqueued, 0 when the family does not serve the shape,
// < 0 on error.  With `up` (srcnn_train_step, else null) the
// slab reduction also applies the SGD update to every parameter it completes
// and returns 2 instead of 1 when it did (layer 3 on l3_delta, so the slabs
// cover all parameters).  With `lz` (srcnn_train_fwd_bwd_lazy, else null) the
// step first applies lz's pending update inside l12 (lz->batch > 0; b.params
// is then ignored and the step runs on lz->Po) and OVERWRITES grads instead
// of accumulating.  b.D1 is not used.
int train_fwd_bwd(const srcnn_net* net, uint32_t w, uint32_t h, uint32_t batch, const StepBuffers& b,
                  hipStream_t s, const SlabUpdate* up, const LazyUpdate* lz);
// Fused inference (forward_fused.hip; the plan is FwdPlan of fwd_plan.hpp):
// forward_plan tells whether the net and frame are served under the current
// arithmetic and the workspace bytes (the plan's part_bytes); forward returns
// 1 when it ran, 0 when they are not served, < 0 on error.
bool forward_plan(const srcnn_net* net, uint32_t w, uint32_t h, uint32_t batch, size_t* ws_bytes);
int forward(const srcnn_net* net, const float* X, uint32_t w, uint32_t h, uint32_t batch,
            const float* params, float* out, void* ws, size_t ws_bytes, hipStream_t s);
// Deterministic slab reduction shared by the fused families and the op-level
// gradient kernels: for every segment, dst[i] += sum_{b < nslab}
// slab[b * stride + i] (i < P), summed in block order.
constexpr int kMaxSlabSegs = 4;
struct SlabSeg {
  const float* slab;
  float* dst;
  int nslab, P;
  int stride;  // floats between consecutive slabs (0 = P)
};
// Optional SGD update fused into the reduction (srcnn_train_step): segments
// k < nseg of `up` are parameter gradients inside the flat buffer G; element
// i = dst - G + col gets g = G[i] + sum, then sgd_step (same arithmetic as
// update_all) on P[i] / M[i], and G[i] = 0.
struct SlabUpdate {
  float *P, *G, *M;
  uint32_t off[7];  // [W1|B1|W2|B2|W3|B3] offsets, off[6] = total
  float lr[3];
  float mu, wd, batch;
  int nseg;
};
// assign: segments k < assign are written (dst = sum) instead of accumulated
int reduce_slabs(const SlabSeg* segs, int nseg, hipStream_t s, const SlabUpdate* up = nullptr,
                 int assign = 0);
// SGD-momentum step of one parameter (update_parameters.cl:14-32): segment
// seg of [W1|B1|W2|B2|W3|B3], weights with weight decay, biases without;
// w, m = parameter and momentum in, out.  Shared by update_all_kernel and the
// fused reduction so both round alike.
__device__ __forceinline__ void sgd_step(float& w, float& m, int seg, float g, float lr, float mu,
                                         float wd, float batch) {
  // no FMA contraction: both call sites must round identically
#pragma clang fp contract(off)
  if ((seg & 1) == 0) {
    const float dw = mu * m + lr * g + wd * w;
    w = w - dw / batch;
    m = dw;
  } else {
    const float db = mu * m + lr * g;
    w -= db / batch;
    m = db;
  }
}
// The previous data-parallel step's update, applied out of place by the next
// step's first kernel (srcnn_train_fwd_bwd_lazy): Po = sgd(P, M, G),
// Mo likewise, with sgd_step's arithmetic.  batch == 0: no pending update.
struct LazyUpdate {
  const float *P, *M, *G;
  float *Po, *Mo;
  uint32_t off[7];  // [W1|B1|W2|B2|W3|B3] offsets, off[6] = total
  float lr[3];
  float mu, wd, batch;
};
// segment of flat parameter index i
__device__ __forceinline__ int param_seg(const uint32_t* off, uint32_t i) {
  int seg = 0;
#pragma unroll
  for (int k = 1; k < 6; k++) seg += i >= off[k];
  return seg;
}
// updated value of parameter off[seg] + i
__device__ __forceinline__ float lazy_param(const LazyUpdate& u, int seg, uint32_t i) {
  const uint32_t gi = u.off[seg] + i;
  float w = u.P[gi], m = u.M[gi];
  sgd_step(w, m, seg, u.G[gi], u.lr[seg >> 1], u.mu, u.wd, u.batch);
  return w;
}
// this block's slice of Po / Mo (the slices of a grid cover every parameter)
__device__ __forceinline__ void lazy_write_slice(const LazyUpdate& u) {
  const uint32_t n = u.off[6], per = (n + gridDim.x - 1) / gridDim.x;
  const uint32_t b0 = blockIdx.x * per, e = min(n, b0 + per);
  for (uint32_t i = b0 + threadIdx.x; i < e; i += blockDim.x) {
    const int seg = param_seg(u.off, i);
    float w = u.P[i], m = u.M[i];
    sgd_step(w, m, seg, u.G[i], u.lr[seg >> 1], u.mu, u.wd, u.batch);
    u.Po[i] = w;
    u.Mo[i] = m;
  }
}
// held-clock probes (common.hpp): slot 0 l12_fwd, 1 l3_delta, 2 d1_grad12
int train_clock(int slot, double* ghz);
// the layout the last training step of this thread wrote into the A1 region
// at `A1` (kA1Runs, kA1Blocked, kA1Hwc), or -1 if it wrote none there; so
// srcnn_train_activations follows the arithmetic the step ran with, whatever
// srcnn_set_arith says since (note_a1_layout records it)
enum { kA1Blocked = 0, kA1Runs = 1, kA1Hwc = 2 };
void note_a1_layout(const float* A1, int layout);
int a1_layout_written(const float* A1);
// the split-bf16 step (l12x6) stores A1 in run order, transposed per chunk
// (kA1Runs): a1_chunks is the A1 chunks per sample either layout needs,
// unrun_a1 converts to HWC
size_t a1_chunks(uint32_t ow, uint32_t oh);
int unrun_a1(const float* A1t, float* A1, uint32_t ow, uint32_t oh, uint32_t batch, hipStream_t s);
// the fused step's blocked A1 (l12_fwd_kernel) -> reference HWC [batch][npx][n1]
int unblock_a1(const float* A1b, float* A1, uint32_t n1, uint32_t npx, uint32_t batch, hipStream_t s);
// srcnn_preload: resolve the family's kernels for this net (1 = this family's
// net, 0 = not, < 0 error)
int preload(const srcnn_net* net);
int preload_forward(const srcnn_net* net);
int forward_clock(double* ghz);
}  // namespace fused

// Training step for nets with a spatial middle layer (train_wide.hip; one
// header per kernel family, wl1.hpp .. wgrad2x6.hpp), e.g. the wide config
// n1=128, n2=64, f1=9, f2=5, f3=5: per-stage MFMA kernels over the
// reference-layout A1 / D1 / A2 / D2 buffers (A1 in kA1Hwc; b.D3 is not used).
// Same contracts as fused::train_plan (WidePlan, wide_plan.hpp) and
// fused::train_fwd_bwd; with `up` the update always rides along (returns 2).
namespace wide {
bool train_plan(const srcnn_net* net, uint32_t w, uint32_t h, uint32_t batch, StepNeed* need);
int train_fwd_bwd(const srcnn_net* net, uint32_t w, uint32_t h, uint32_t batch, const StepBuffers& b,
                  hipStream_t s, const fused::SlabUpdate* up);
int preload(const srcnn_net* net);
// op-level launchers of the 5x5 128 <-> 64 middle layer (same contract as
// the fast::try_* functions: 1 handled, 0 not this shape, < 0 error)
int op_conv_fwd(const float* in, float* out, const float* W, const float* B, uint32_t in_w,
                uint32_t in_h, uint32_t n_prev, uint32_t n_cur, uint32_t f, int relu,
                uint32_t batch, hipStream_t s);
int op_conv_delta(const float* d_next, const float* y_curr, float* d_curr, const float* W_next,
                  uint32_t f_next, uint32_t n_curr, uint32_t n_next, uint32_t curr_w,
                  uint32_t curr_h, uint32_t batch, hipStream_t s);
size_t op_grad_workspace_bytes(uint32_t n_prev, uint32_t n_cur, uint32_t f, uint32_t out_w,
                               uint32_t out_h, uint32_t batch);
int op_conv_grad_acc(const float* in, const float* d, float* gW, float* gB, uint32_t n_prev,
                     uint32_t n_cur, uint32_t f, uint32_t out_w, uint32_t out_h, uint32_t batch,
                     void* ws, size_t ws_bytes, hipStream_t s);
}  // namespace wide

int sgd_update(float* W, float* B, const float* gW, const float* gB, float* dW, float* dB,
               float mu, float wd, float lr, uint32_t batch, uint32_t nW, uint32_t nB,
               hipStream_t s);
uint32_t reduce_blocks(size_t len);
// mode 0 sum, 1 sum of squares, 2 squared error (gt/out dims used only by mode 2)
int reduce(int mode, const float* a, const float* gt, size_t len, uint32_t gt_w, uint32_t gt_h,
           uint32_t out_w, uint32_t out_h, float* result, int accumulate, void* ws,
           size_t ws_bytes, hipStream_t s);
int sub_scalar(float* d, float v, size_t len, hipStream_t s);
int sub_mean(float* d, size_t len, float* mean_out, void* ws, size_t ws_bytes, hipStream_t s);
int fill(float* d, float v, size_t n, hipStream_t s);
// update_all: the three layers' sgd_update + zero-fill of grads, one launch;
// off = srcnn_net_offsets(), total = P
int preload_update();
int update_all(float* params, float* grads, float* mom, const size_t* off, size_t total,
               const float* lr, float mu, float wd, uint32_t batch, hipStream_t s);
// srcnn_train_fwd_bwd_lazy off the fused path: u.Po / u.Mo = the pending
// update of u.P / u.M by u.G (update_all's arithmetic), then G = 0
int lazy_update(const fused::LazyUpdate& u, hipStream_t s);
int extract_luma(const uint8_t* rgba, float* luma, uint32_t w, uint32_t h, int normalize,
                 hipStream_t s);
int swap_luma(const uint8_t* rgba, const float* nl, uint8_t* rgb, uint32_t w, uint32_t h,
              uint32_t lw, uint32_t lh, hipStream_t s);
// upscale.hip: bicubic x scale (1..4) luma into the edge-replicated padded
// plane [(scale*h+pad)][(scale*w+pad)], and the composition of the bicubic
// r, g, b with the net's luma [scale*h][scale*w] into rgb
int upscale_luma(const uint8_t* rgba, float* plane, uint32_t w, uint32_t h, uint32_t scale,
                 uint32_t pad, hipStream_t s);
int upscale_compose(const uint8_t* rgba, const float* nl, uint8_t* rgb, uint32_t w, uint32_t h,
                    uint32_t scale, hipStream_t s);
int preload_upscale();
// yuv.hip: the same resampling for Y'CbCr frames: the Y
// plane [h][w] into the padded plane as upscale_luma does, normalised by the
// range; a frame's chroma [ph][pw] bicubic x scale, rounded and clamped, the
// top-left ow x oh of it in the same layout; the net's luma [H][W] back into
// a Y plane.  A sample has `bits` bits, 8..16: one byte at 8 bits, else a
// 16-bit word with the value in its low (msb false) or high bits; pitches in
// bytes; semiplanar: src0 / dst0 hold (U, V) pairs [ph][pw][2], src1 / dst1
// unused, else two planes each way
int yuv_upscale_luma(const void* y, uint32_t pitch_y, float* plane, uint32_t w, uint32_t h,
                     uint32_t scale, uint32_t pad, uint32_t bits, bool msb, bool full_range,
                     hipStream_t s);
int upscale_planes(const void* src0, const void* src1, uint32_t src_pitch, uint32_t pw, uint32_t ph,
                   void* dst0, void* dst1, uint32_t dst_pitch, uint32_t ow, uint32_t oh,
                   uint32_t scale, uint32_t bits, bool msb, bool semiplanar, hipStream_t s);
int yuv_compose_luma(const float* luma, void* y, uint32_t pitch_y, uint32_t W, uint32_t H,
                     uint32_t bits, bool msb, bool full_range, hipStream_t s);
int preload_yuv();
// yuv_down.hip: the antialiased bicubic / scale (1..4) of a frame's planes of
// code values: [ph][pw] -> [oh][ow], ow <= ceil(pw / scale), oh
// likewise, rounded to nearest even and clamped; samples, pitches and
// semiplanar as in upscale_planes; planar with src1 == dst1 == nullptr: one
// plane
int downscale_planes(const void* src0, const void* src1, uint32_t src_pitch, uint32_t pw, uint32_t ph,
                     void* dst0, void* dst1, uint32_t dst_pitch, uint32_t ow, uint32_t oh,
                     uint32_t scale, uint32_t bits, bool msb, bool semiplanar, hipStream_t s);
int preload_yuv_down();
// resize.hip: the same front and back end for any output size W x H with
// w <= W <= 4w, h <= H <= 4h: the ratio of an axis is the
// fraction w / W; resize_planes takes it explicitly (source step per output
// sample rx_num / rx_den, ry_num / ry_den), because a frame's chroma is
// resampled at the luma's ratio
int resize_luma(const uint8_t* rgba, float* plane, uint32_t w, uint32_t h, uint32_t W, uint32_t H,
                uint32_t pad, hipStream_t s);
int resize_compose(const uint8_t* rgba, const float* nl, uint8_t* rgb, uint32_t w, uint32_t h,
                   uint32_t W, uint32_t H, hipStream_t s);
int yuv_resize_luma(const void* y, uint32_t pitch_y, float* plane, uint32_t w, uint32_t h, uint32_t W,
                    uint32_t H, uint32_t pad, uint32_t bits, bool msb, bool full_range, hipStream_t s);
int resize_planes(const void* src0, const void* src1, uint32_t src_pitch, uint32_t pw, uint32_t ph,
                  void* dst0, void* dst1, uint32_t dst_pitch, uint32_t ow, uint32_t oh, uint32_t rx_num,
                  uint32_t rx_den, uint32_t ry_num, uint32_t ry_den, uint32_t bits, bool msb,
                  bool semiplanar, hipStream_t s);
int preload_resize();
// pairs.hip: antialiased bicubic / scale (1..4) of rgba [H][W][4] into small
// [H/scale][W/scale][4], and the cut of a grid of nx x ny tiles (tw x th,
// origin (x0, y0), step `stride`) out of a float plane of pitch pw into
// tiles [nx*ny][th][tw], each minus its own mean when sub_mean
int downscale_rgba(const uint8_t* rgba, uint8_t* small, uint32_t W, uint32_t H, uint32_t scale,
                   hipStream_t s);
int gather_tiles(const float* plane, uint32_t pw, uint32_t x0, uint32_t y0, uint32_t stride,
                 uint32_t nx, uint32_t ny, uint32_t tw, uint32_t th, int sub_mean, float* tiles,
                 float* means, hipStream_t s);
// one workgroup per record of refs [n] (device): the record's footprint of
// planes[ref.plane] (device table) through orientation ref.op into X, T
// [n][th][tw], X minus the footprint's mean; an invalid record gives NaN tiles
// 
int gather_batch(const srcnn_plane_pair* planes, uint32_t n_planes, const srcnn_tile_ref* refs,
                 uint32_t n, uint32_t tw, uint32_t th, float* X, float* T, float* means,
                 hipStream_t s);
int preload_pairs();
// quality.hip: {mse, psnr, ssim} of the luma of two Ws x Hs windows (a, b: the
// window's first pixel; SRCNN_PIX_* formats; pitches in pixels) into result
// [3]; partial: 2 * quality_tile_count(Ws, Hs) doubles of scratch
// (DESIGN.md 12).  Ws, Hs >= 11.
uint64_t quality_tile_count(uint32_t Ws, uint32_t Hs);
int quality(const void* a, int fmt_a, uint32_t pitch_a, const void* b, int fmt_b, uint32_t pitch_b,
            uint32_t Ws, uint32_t Hs, double* result, double* partial, hipStream_t s);
// the same of two Y'CbCr frames: PSNR per plane, SSIM on luma
// into result [8].  A side's pointers are the first samples of its shaved
// windows, Ws x Hs of luma and CWs x CHs of each chroma plane; pitches in
// bytes; semiplanar: c0 holds the (U, V) pairs, c1 unused.  ws: two 8-byte
// words per luma tile, then one per chroma tile (quality_chroma_tile_count)
// and plane.  Three launches.
struct QualityFrameSide {
  const void *y, *c0, *c1;
  uint32_t pitch_y, pitch_c;
  bool msb, semiplanar;
};
uint64_t quality_chroma_tile_count(uint32_t CWs, uint32_t CHs);
int quality_frame(const QualityFrameSide& a, const QualityFrameSide& b, uint32_t bits, uint32_t Ws,
                  uint32_t Hs, uint32_t CWs, uint32_t CHs, double* result, void* ws, hipStream_t s);
int preload_quality();

}  // namespace srcnn
