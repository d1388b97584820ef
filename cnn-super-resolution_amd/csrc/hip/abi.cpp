// abi.cpp -- extern "C" operator + network entry points of srcnn.h: the
// layer operators, the reductions, the training step and the forward pass.
// The image-level calls (resampling, upscale, pairs, quality) are in
// abi_upscale.cpp, which comes here only through the public ABI.
//
// Each operator validates its arguments the way the reference launcher does
// (src/DataPipeline.cpp, src/LayerData.cpp:20-42), then dispatches: a gfx950
// specialisation from ops_fast.hip when the shape matches and the path is
// "auto", otherwise the shape-generic kernels of ops_generic.hip.  There is
// no CPU fallback: every path launches HIP kernels.
#include <algorithm>
#include <cstdio>

#include "common.hpp"
#include "ops.hpp"

using srcnn::align_up;
using srcnn::as_stream;
using srcnn::fail;

namespace {

bool fast_enabled() { return srcnn::g_path == 0; }

// kernel family of the most recent conv operator / network call (srcnn_last_path)
thread_local const char* t_path = "";
thread_local unsigned t_generic_ops = 0;  // op-level calls served by ops_generic.hip
int tag(const char* path, int rc) {
  if (rc == SRCNN_OK) {
    t_path = path;
    if (path[0] == 'g') ++t_generic_ops;
  }
  return rc;
}
// a network call composed of op-level calls: "generic" if any op was
struct OpSequence {
  unsigned g0 = t_generic_ops;
  int done(int rc) { return tag(t_generic_ops != g0 ? "generic" : "fast", rc); }
};

int check_layer(const char* who, uint32_t n_prev, uint32_t n_cur, uint32_t f) {
  SRCNN_REQUIRE(f > 0 && n_prev > 0 && n_cur > 0,
                "%s: f(%u), n_prev_filter_cnt(%u) and current_filter_count(%u) must be > 0", who,
                f, n_prev, n_cur);
  return SRCNN_OK;
}

struct NetDims {
  uint32_t w1, h1, w2, h2, w3, h3;
  size_t s1, s2, s3;  // per-sample floats of A1, A2, A3
  size_t s1p;         // A1 region per sample: whole 32-pixel chunks (the fused
                      // step stores A1 blocked per chunk, train_fused.hip)
};

int net_dims(const srcnn_net* net, uint32_t w, uint32_t h, NetDims* d) {
  SRCNN_REQUIRE(net, "null srcnn_net");
  SRCNN_REQUIRE(net->n1 > 0 && net->n2 > 0, "n1(%u) and n2(%u) should be >0", net->n1, net->n2);
  SRCNN_REQUIRE(net->f1 > 0 && net->f2 > 0 && net->f3 > 0 && (net->f1 & 1) && (net->f2 & 1) &&
                    (net->f3 & 1),
                "f1(%u), f2(%u), f3(%u) should be odd and >0 (Config.cpp:64-74)", net->f1,
                net->f2, net->f3);
  const uint32_t pad = net->f1 + net->f2 + net->f3 - 3;  // Config::total_padding
  SRCNN_REQUIRE(w > pad && h > pad, "sample %ux%u is not larger than total padding %u", w, h, pad);
  d->w1 = w - net->f1 + 1;
  d->h1 = h - net->f1 + 1;
  d->w2 = d->w1 - net->f2 + 1;
  d->h2 = d->h1 - net->f2 + 1;
  d->w3 = d->w2 - net->f3 + 1;
  d->h3 = d->h2 - net->f3 + 1;
  d->s1 = (size_t)d->w1 * d->h1 * net->n1;
  d->s1p = srcnn::fused::a1_chunks(d->w1, d->h1) * 32 * net->n1;
  d->s2 = (size_t)d->w2 * d->h2 * net->n2;
  d->s3 = (size_t)d->w3 * d->h3;
  return SRCNN_OK;
}

size_t grad_ws_bytes(uint32_t n_prev, uint32_t n_cur, uint32_t f, uint32_t ow, uint32_t oh,
                     uint32_t batch) {
  size_t b = 0;
  if (fast_enabled()) b = srcnn::fast::grad_workspace_bytes(n_prev, n_cur, f, ow, oh, batch);
  if (b == 0) b = srcnn::generic::grad_workspace_bytes(n_prev, n_cur, f, batch);
  return b;
}

// what the family that train_impl will dispatch this shape to needs, under
// the current path and arithmetic: the fused step, else the wide one, else
// (the op-level kernels) no slab and A1 in HWC
srcnn::StepNeed step_need(const srcnn_net* net, uint32_t w, uint32_t h, uint32_t batch) {
  srcnn::StepNeed n{0, srcnn::fused::kA1Hwc};
  if (fast_enabled() && !srcnn::fused::train_plan(net, w, h, batch, &n))
    srcnn::wide::train_plan(net, w, h, batch, &n);
  return n;
}

}  // namespace

extern "C" {

const char* srcnn_last_path(void) { return t_path; }

const char* srcnn_last_kernels(void) { return srcnn::kernels_last(); }

int srcnn_fill_f32(float* dst, float value, size_t count, srcnn_stream_t stream) {
  if (count == 0) return SRCNN_OK;
  SRCNN_REQUIRE(dst, "srcnn_fill_f32: null pointer");
  return srcnn::fill(dst, value, count, as_stream(stream));
}

int srcnn_conv_fwd(const float* in, float* out, const float* W, const float* B, uint32_t in_w,
                   uint32_t in_h, uint32_t n_prev, uint32_t n_cur, uint32_t f, int relu,
                   uint32_t batch, srcnn_stream_t stream) {
  if (int rc = check_layer("execute_layer", n_prev, n_cur, f)) return rc;
  SRCNN_REQUIRE(in_w >= f && in_h >= f,
                "execute_layer: input %ux%u smaller than filter f=%u", in_w, in_h, f);
  if (batch == 0) return SRCNN_OK;
  SRCNN_REQUIRE(in && out && W && B, "execute_layer: null buffer");
  hipStream_t s = as_stream(stream);
  if (fast_enabled()) {
    int rc = srcnn::fast::try_conv_fwd(in, out, W, B, in_w, in_h, n_prev, n_cur, f, relu, batch, s);
    if (rc != 0) return rc < 0 ? rc : tag("fast", SRCNN_OK);
  }
  return tag("generic",
             srcnn::generic::conv_fwd(in, out, W, B, in_w, in_h, n_prev, n_cur, f, relu, batch, s));
}

int srcnn_last_delta(const float* gt, const float* y, float* d, uint32_t gt_w, uint32_t gt_h,
                     uint32_t out_w, uint32_t out_h, uint32_t batch, srcnn_stream_t stream) {
  SRCNN_REQUIRE(out_w > 0 && out_h > 0 && gt_w >= out_w && gt_h >= out_h,
                "last_layer_delta: ground truth %ux%u smaller than result %ux%u", gt_w, gt_h,
                out_w, out_h);
  if (batch == 0) return SRCNN_OK;
  SRCNN_REQUIRE(gt && y && d, "last_layer_delta: null buffer");
  return srcnn::generic::last_delta(gt, y, d, gt_w, gt_h, out_w, out_h, batch, as_stream(stream));
}

int srcnn_conv_delta(const float* d_next, const float* y_curr, float* d_curr,
                     const float* W_next, uint32_t f_next, uint32_t n_curr, uint32_t n_next,
                     uint32_t curr_w, uint32_t curr_h, uint32_t batch, srcnn_stream_t stream) {
  if (int rc = check_layer("calculate_deltas", n_curr, n_next, f_next)) return rc;
  SRCNN_REQUIRE(curr_w >= f_next && curr_h >= f_next,
                "calculate_deltas: layer output %ux%u smaller than next filter f=%u", curr_w,
                curr_h, f_next);
  if (batch == 0) return SRCNN_OK;
  SRCNN_REQUIRE(d_next && y_curr && d_curr && W_next, "calculate_deltas: null buffer");
  hipStream_t s = as_stream(stream);
  if (fast_enabled()) {
    int rc = srcnn::fast::try_conv_delta(d_next, y_curr, d_curr, W_next, f_next, n_curr, n_next,
                                         curr_w, curr_h, batch, s);
    if (rc != 0) return rc < 0 ? rc : tag("fast", SRCNN_OK);
  }
  return tag("generic", srcnn::generic::conv_delta(d_next, y_curr, d_curr, W_next, f_next, n_curr,
                                                   n_next, curr_w, curr_h, batch, s));
}

size_t srcnn_conv_grad_workspace_bytes(uint32_t n_prev, uint32_t n_cur, uint32_t f,
                                       uint32_t out_w, uint32_t out_h, uint32_t batch) {
  if (!f || !n_prev || !n_cur || !batch) return 0;
  return grad_ws_bytes(n_prev, n_cur, f, out_w, out_h, batch);
}

int srcnn_conv_grad_acc(const float* in, const float* delta, float* gW, float* gB,
                        uint32_t n_prev, uint32_t n_cur, uint32_t f, uint32_t out_w,
                        uint32_t out_h, uint32_t batch, void* ws, size_t ws_bytes,
                        srcnn_stream_t stream) {
  if (int rc = check_layer("backpropagate", n_prev, n_cur, f)) return rc;
  SRCNN_REQUIRE(out_w > 0 && out_h > 0, "backpropagate: empty layer output %ux%u", out_w, out_h);
  if (batch == 0) return SRCNN_OK;
  SRCNN_REQUIRE(in && delta && gW && gB, "backpropagate: null buffer");
  SRCNN_REQUIRE(ws, "backpropagate: null workspace (see srcnn_conv_grad_workspace_bytes)");
  hipStream_t s = as_stream(stream);
  if (fast_enabled()) {
    int rc = srcnn::fast::try_conv_grad_acc(in, delta, gW, gB, n_prev, n_cur, f, out_w, out_h,
                                            batch, ws, ws_bytes, s);
    if (rc != 0) return rc < 0 ? rc : tag("fast", SRCNN_OK);
  }
  return tag("generic", srcnn::generic::conv_grad_acc(in, delta, gW, gB, n_prev, n_cur, f, out_w,
                                                      out_h, batch, ws, ws_bytes, s));
}

int srcnn_sgd_update(float* W, float* B, const float* gW, const float* gB, float* dW_prev,
                     float* dB_prev, float momentum, float wd, float lr, uint32_t batch,
                     uint32_t nW, uint32_t nB, srcnn_stream_t stream) {
  SRCNN_REQUIRE(batch > 0, "update_parameters: batch size must be > 0");
  SRCNN_REQUIRE(nB <= nW, "update_parameters: bias_size(%u) > weights_size(%u)", nB, nW);
  if (nW == 0) return SRCNN_OK;
  SRCNN_REQUIRE(W && gW && dW_prev && (nB == 0 || (B && gB && dB_prev)),
                "update_parameters: null buffer");
  return srcnn::sgd_update(W, B, gW, gB, dW_prev, dB_prev, momentum, wd, lr, batch, nW, nB,
                           as_stream(stream));
}

size_t srcnn_reduce_workspace_bytes(size_t len) {
  return (srcnn::reduce_blocks(len) + 1) * sizeof(float);
}

int srcnn_sq_err(const float* gt, const float* y, float* result, uint32_t gt_w, uint32_t gt_h,
                 uint32_t out_w, uint32_t out_h, uint32_t batch, void* ws, size_t ws_bytes,
                 srcnn_stream_t stream) {
  SRCNN_REQUIRE(out_w > 0 && out_h > 0 && gt_w >= out_w && gt_h >= out_h,
                "squared_error: ground truth %ux%u smaller than result %ux%u", gt_w, gt_h, out_w,
                out_h);
  SRCNN_REQUIRE(gt && y && result && ws, "squared_error: null buffer");
  const size_t len = (size_t)batch * out_w * out_h;
  if (len == 0) return srcnn::fill(result, 0.0f, 1, as_stream(stream));
  return srcnn::reduce(2, y, gt, len, gt_w, gt_h, out_w, out_h, result, 0, ws, ws_bytes,
                       as_stream(stream));
}

int srcnn_sum(const float* data, size_t len, int squared, float* result, void* ws,
              size_t ws_bytes, srcnn_stream_t stream) {
  SRCNN_REQUIRE(result && ws, "sum: null buffer");
  if (len == 0) return srcnn::fill(result, 0.0f, 1, as_stream(stream));
  SRCNN_REQUIRE(data, "sum: null data");
  return srcnn::reduce(squared ? 1 : 0, data, nullptr, len, 0, 0, 0, 0, result, 0, ws, ws_bytes,
                       as_stream(stream));
}

int srcnn_sub_scalar(float* data, float value, size_t len, srcnn_stream_t stream) {
  if (len == 0) return SRCNN_OK;
  SRCNN_REQUIRE(data, "subtract_from_all: null data");
  return srcnn::sub_scalar(data, value, len, as_stream(stream));
}

int srcnn_sub_mean(float* data, size_t len, float* mean, void* ws, size_t ws_bytes,
                   srcnn_stream_t stream) {
  SRCNN_REQUIRE(len > 0 && data && ws, "subtract_mean: empty or null buffer");
  return srcnn::sub_mean(data, len, mean, ws, ws_bytes, as_stream(stream));
}

int srcnn_extract_luma(const uint8_t* rgba, float* luma, uint32_t w, uint32_t h, int normalize,
                       srcnn_stream_t stream) {
  if ((size_t)w * h == 0) return SRCNN_OK;
  SRCNN_REQUIRE(rgba && luma, "extract_luma: null buffer");
  return srcnn::extract_luma(rgba, luma, w, h, normalize, as_stream(stream));
}

int srcnn_swap_luma(const uint8_t* rgba, const float* new_luma, uint8_t* rgb, uint32_t w,
                    uint32_t h, uint32_t luma_w, uint32_t luma_h, srcnn_stream_t stream) {
  SRCNN_REQUIRE(luma_w <= w && luma_h <= h, "swap_luma: luma %ux%u larger than image %ux%u",
                luma_w, luma_h, w, h);
  if ((size_t)w * h == 0) return SRCNN_OK;
  SRCNN_REQUIRE(rgba && rgb && (new_luma || luma_w * luma_h == 0), "swap_luma: null buffer");
  return srcnn::swap_luma(rgba, new_luma, rgb, w, h, luma_w, luma_h, as_stream(stream));
}

// ---------------------------------------------------------------------------
// network level
// ---------------------------------------------------------------------------
int srcnn_net_offsets(const srcnn_net* net, size_t off[6]) {
  SRCNN_REQUIRE(net && off, "srcnn_net_offsets: null argument");
  off[0] = 0;
  off[1] = off[0] + (size_t)net->f1 * net->f1 * net->n1;
  off[2] = off[1] + net->n1;
  off[3] = off[2] + (size_t)net->f2 * net->f2 * net->n1 * net->n2;
  off[4] = off[3] + net->n2;
  off[5] = off[4] + (size_t)net->f3 * net->f3 * net->n2;
  return SRCNN_OK;
}

size_t srcnn_net_param_count(const srcnn_net* net) {
  size_t off[6];
  if (srcnn_net_offsets(net, off)) return 0;
  return off[5] + 1;
}

int srcnn_preload(const srcnn_net* net) {
  size_t off[6];
  if (int rc = srcnn_net_offsets(net, off)) return rc;
  int rc;
  if ((rc = srcnn::fused::preload(net)) < 0 || (rc = srcnn::fused::preload_forward(net)) < 0 ||
      (rc = srcnn::wide::preload(net)) < 0 || (rc = srcnn::preload_upscale()) < 0 ||
      (rc = srcnn::preload_pairs()) < 0 || (rc = srcnn::preload_quality()) < 0 ||
      (rc = srcnn::preload_yuv()) < 0 || (rc = srcnn::preload_yuv_down()) < 0 ||
      (rc = srcnn::preload_resize()) < 0)
    return rc;
  return srcnn::preload_update();
}

size_t srcnn_train_workspace_bytes(const srcnn_net* net, uint32_t w, uint32_t h, uint32_t batch) {
  NetDims d;
  if (net_dims(net, w, h, &d) || batch == 0) return 0;
  size_t b = 0;
  b += align_up(d.s1p * batch * sizeof(float));  // A1
  b += align_up(d.s1 * batch * sizeof(float));   // D1
  b += 2 * align_up(d.s2 * batch * sizeof(float));  // A2, D2
  b += 2 * align_up(d.s3 * batch * sizeof(float));  // A3, D3
  size_t g = std::max({grad_ws_bytes(1, net->n1, net->f1, d.w1, d.h1, batch),
                       grad_ws_bytes(net->n1, net->n2, net->f2, d.w2, d.h2, batch),
                       grad_ws_bytes(net->n2, 1, net->f3, d.w3, d.h3, batch),
                       srcnn_reduce_workspace_bytes(d.s3 * batch)});
  return b + align_up(std::max(g, step_need(net, w, h, batch).slab_bytes));
}

// regions of the training workspace (srcnn_train_workspace_bytes): A1 (whole
// 32-pixel chunks per sample) | D1 | A2 | D2 | A3 | D3 | gradient scratch
// (L.slab), as the buffers of a step; the caller's tensors are left null
static srcnn::StepBuffers train_ws(const NetDims& d, uint32_t batch, void* ws, size_t ws_bytes) {
  srcnn::StepBuffers L{};
  char* p = static_cast<char*>(ws);
  auto take = [&](size_t floats) {
    float* r = reinterpret_cast<float*>(p);
    p += align_up(floats * batch * sizeof(float));
    return r;
  };
  L.A1 = take(d.s1p);
  L.D1 = take(d.s1);
  L.A2 = take(d.s2);
  L.D2 = take(d.s2);
  L.A3 = take(d.s3);
  L.D3 = take(d.s3);
  L.slab = reinterpret_cast<float*>(p);
  L.slab_bytes = ws_bytes - (size_t)(p - static_cast<char*>(ws));
  return L;
}

// srcnn_train_fwd_bwd, and with `up` srcnn_train_step's fused variant:
// *updated = true when the fused slab reduction also applied the update
static int train_impl(const srcnn_net* net, const float* X, const float* T, uint32_t w,
                      uint32_t h, uint32_t batch, const float* params, float* grads,
                      float* sq_err, void* ws, size_t ws_bytes, srcnn_stream_t stream,
                      const srcnn::fused::SlabUpdate* up, bool* updated,
                      const srcnn::fused::LazyUpdate* lz = nullptr) {
  NetDims d;
  if (int rc = net_dims(net, w, h, &d)) return rc;
  if (!lz) srcnn::kernels_reset();  // (the lazy entry resets before its update)
  if (batch == 0) return SRCNN_OK;
  SRCNN_REQUIRE(X && T && grads && ws && (params || (lz && lz->batch > 0.0f)), "train_fwd_bwd: null buffer");
  const size_t need = srcnn_train_workspace_bytes(net, w, h, batch);
  if (ws_bytes < need)
    return fail(SRCNN_ERR_WORKSPACE, "train_fwd_bwd: workspace %zu B < %zu B", ws_bytes, need);
  srcnn::StepBuffers L = train_ws(d, batch, ws, ws_bytes);
  L.X = X;
  L.T = T;
  L.params = params;
  L.grads = grads;
  L.sq_err = sq_err;
  hipStream_t s = as_stream(stream);
  int rc;
  if (fast_enabled()) {
    rc = srcnn::fused::train_fwd_bwd(net, w, h, batch, L, s, up, lz);
    if (rc == 2 && updated) *updated = true;
    if (rc != 0) return rc < 0 ? rc : tag("fused", SRCNN_OK);
  }
  if (lz) {
    // srcnn_train_fwd_bwd_lazy off the fused path: the pending update out of
    // place and the gradients zeroed in one launch, then the accumulating step
    if (lz->batch > 0.0f) {
      if ((rc = srcnn::lazy_update(*lz, s))) return rc;
      L.params = lz->Po;
    } else if ((rc = srcnn::fill(grads, 0.0f, srcnn_net_param_count(net), s))) {
      return rc;
    }
  }
  // the wide step and the op-level kernels write A1 in HWC
  srcnn::fused::note_a1_layout(L.A1, srcnn::fused::kA1Hwc);
  if (fast_enabled()) {
    rc = srcnn::wide::train_fwd_bwd(net, w, h, batch, L, s, up);
    if (rc == 2 && updated) *updated = true;
    if (rc != 0) return rc < 0 ? rc : tag("wide", SRCNN_OK);
  }
  const auto P = srcnn::split_params(L.params, net);
  const auto G = srcnn::split_params(grads, net);
  // the op-level launchers (srcnn_last_kernels: one entry per reference
  // launcher, with the kernel family that served it)
  auto op = [](const char* name, int rc) {
    if (rc == SRCNN_OK) {
      char buf[64];
      snprintf(buf, sizeof buf, "%s:%s", name, t_path);
      srcnn::kernels_note(buf);
    }
    return rc;
  };
  OpSequence seq;
  // forward: ConfigBasedDataPipeline.cpp:200-241
  if ((rc = op("conv_fwd_l1", srcnn_conv_fwd(X, L.A1, P.W1, P.B1, w, h, 1, net->n1, net->f1, 1, batch, stream))))
    return rc;
  if ((rc = op("conv_fwd_l2",
               srcnn_conv_fwd(L.A1, L.A2, P.W2, P.B2, d.w1, d.h1, net->n1, net->n2, net->f2, 1, batch, stream))))
    return rc;
  if ((rc = op("conv_fwd_l3", srcnn_conv_fwd(L.A2, L.A3, P.W3, P.B3, d.w2, d.h2, net->n2, 1, net->f3, 0, batch, stream))))
    return rc;
  if (sq_err &&
      (rc = srcnn::reduce(2, L.A3, T, d.s3 * batch, w, h, d.w3, d.h3, sq_err, 1, L.slab, L.slab_bytes, s)))
    return rc;
  // backward: ConfigBasedDataPipeline.cpp:243-323
  if ((rc = srcnn_last_delta(T, L.A3, L.D3, w, h, d.w3, d.h3, batch, stream))) return rc;
  if ((rc = op("conv_delta_l2",
               srcnn_conv_delta(L.D3, L.A2, L.D2, P.W3, net->f3, net->n2, 1, d.w2, d.h2, batch, stream))))
    return rc;
  if ((rc = op("conv_delta_l1",
               srcnn_conv_delta(L.D2, L.A1, L.D1, P.W2, net->f2, net->n1, net->n2, d.w1, d.h1, batch, stream))))
    return rc;
  if ((rc = op("conv_grad_l3", srcnn_conv_grad_acc(L.A2, L.D3, G.W3, G.B3, net->n2, 1, net->f3, d.w3, d.h3, batch,
                                                   L.slab, L.slab_bytes, stream))))
    return rc;
  if ((rc = op("conv_grad_l2", srcnn_conv_grad_acc(L.A1, L.D2, G.W2, G.B2, net->n1, net->n2, net->f2, d.w2, d.h2,
                                                   batch, L.slab, L.slab_bytes, stream))))
    return rc;
  return seq.done(op("conv_grad_l1", srcnn_conv_grad_acc(X, L.D1, G.W1, G.B1, 1, net->n1, net->f1, d.w1, d.h1,
                                                         batch, L.slab, L.slab_bytes, stream)));
}

int srcnn_train_fwd_bwd(const srcnn_net* net, const float* X, const float* T, uint32_t w,
                        uint32_t h, uint32_t batch, const float* params, float* grads,
                        float* sq_err, void* ws, size_t ws_bytes, srcnn_stream_t stream) {
  return train_impl(net, X, T, w, h, batch, params, grads, sq_err, ws, ws_bytes, stream, nullptr,
                    nullptr);
}

int srcnn_train_step(const srcnn_net* net, const float* X, const float* T, uint32_t w, uint32_t h,
                     uint32_t batch, float* params, float* grads, float* momentum_bufs,
                     float momentum, float wd, const float* lr, uint32_t update_batch,
                     float* sq_err, void* ws, size_t ws_bytes, srcnn_stream_t stream) {
  SRCNN_REQUIRE(net && params && grads && momentum_bufs && lr, "train_step: null argument");
  SRCNN_REQUIRE(update_batch > 0, "train_step: update batch size must be > 0");
  size_t off[6];
  if (int rc = srcnn_net_offsets(net, off)) return rc;
  const size_t total = off[5] + 1;
  SRCNN_REQUIRE(total < (1ull << 32), "train_step: parameter count %zu too large", total);
  srcnn::fused::SlabUpdate u{};
  u.P = params;
  u.G = grads;
  u.M = momentum_bufs;
  for (int k = 0; k < 6; k++) u.off[k] = (uint32_t)off[k];
  u.off[6] = (uint32_t)total;
  for (int k = 0; k < 3; k++) u.lr[k] = lr[k];
  u.mu = momentum;
  u.wd = wd;
  u.batch = (float)update_batch;
  bool updated = false;
  if (int rc = train_impl(net, X, T, w, h, batch, params, grads, sq_err, ws, ws_bytes, stream, &u,
                          &updated))
    return rc;
  if (updated) return SRCNN_OK;
  srcnn::kernels_note("update_all");
  return srcnn_update_all(net, params, grads, momentum_bufs, momentum, wd, lr, update_batch, stream);
}

int srcnn_train_fwd_bwd_lazy(const srcnn_net* net, const float* X, const float* T, uint32_t w,
                             uint32_t h, uint32_t batch, const float* params_in, float* params_out,
                             const float* mom_in, float* mom_out, float* grads, float momentum,
                             float wd, const float* lr, uint32_t update_batch, float* sq_err,
                             void* ws, size_t ws_bytes, srcnn_stream_t stream) {
  SRCNN_REQUIRE(net && params_in && grads, "train_fwd_bwd_lazy: null argument");
  srcnn::kernels_reset();
  size_t off[6];
  if (int rc = srcnn_net_offsets(net, off)) return rc;
  const size_t total = off[5] + 1;
  SRCNN_REQUIRE(total < (1ull << 32), "train_fwd_bwd_lazy: parameter count %zu too large", total);
  srcnn::fused::LazyUpdate u{};
  u.P = params_in;
  u.G = grads;
  if (update_batch > 0) {
    SRCNN_REQUIRE(params_out && mom_in && mom_out && lr, "train_fwd_bwd_lazy: null argument");
    // out of place: the blocks of the first kernel read the old values while
    // others write the new ones
    // every input {params_in, mom_in, grads} against every output
    // {params_out, mom_out}, and the two outputs against each other
    auto disjoint = [total](const float* a, const float* b) { return a + total <= b || b + total <= a; };
    SRCNN_REQUIRE(disjoint(params_in, params_out) && disjoint(params_in, mom_out) &&
                      disjoint(mom_in, params_out) && disjoint(mom_in, mom_out) &&
                      disjoint(grads, params_out) && disjoint(grads, mom_out) && disjoint(params_out, mom_out),
                  "train_fwd_bwd_lazy: params_in / params_out / mom_in / mom_out / grads overlap");
    u.M = mom_in;
    u.Po = params_out;
    u.Mo = mom_out;
    for (int k = 0; k < 6; k++) u.off[k] = (uint32_t)off[k];
    u.off[6] = (uint32_t)total;
    for (int k = 0; k < 3; k++) u.lr[k] = lr[k];
    u.mu = momentum;
    u.wd = wd;
    u.batch = (float)update_batch;
  }
  if (batch == 0) {  // no tiles: the pending update alone, gradients zero
    if (update_batch == 0) return srcnn_fill_f32(grads, 0.0f, total, stream);
    return srcnn::lazy_update(u, srcnn::as_stream(stream));
  }
  return train_impl(net, X, T, w, h, batch, params_in, grads, sq_err, ws, ws_bytes, stream, nullptr,
                    nullptr, &u);
}

int srcnn_train_activations(const srcnn_net* net, uint32_t w, uint32_t h, uint32_t batch,
                            const void* ws, size_t ws_bytes, float* A1, float* A2, float* A3,
                            srcnn_stream_t stream) {
  NetDims d;
  if (int rc = net_dims(net, w, h, &d)) return rc;
  if (batch == 0) return SRCNN_OK;
  SRCNN_REQUIRE(ws && A1 && A2 && A3, "train_activations: null buffer");
  const size_t need = srcnn_train_workspace_bytes(net, w, h, batch);
  if (ws_bytes < need)
    return fail(SRCNN_ERR_WORKSPACE, "train_activations: workspace %zu B < %zu B", ws_bytes, need);
  const srcnn::StepBuffers L = train_ws(d, batch, const_cast<void*>(ws), ws_bytes);
  hipStream_t s = as_stream(stream);
  // the layout the last step on this workspace wrote (recorded when it ran,
  // so an srcnn_set_arith since does not change it); else the current
  // dispatch's: the fused family stores A1 per 32-pixel chunk, blocked or in
  // run order; the wide family and the op-level kernels in HWC
  int layout = srcnn::fused::a1_layout_written(L.A1);
  if (layout < 0) layout = step_need(net, w, h, batch).a1_layout;
  int rc = layout == srcnn::fused::kA1Runs ? srcnn::fused::unrun_a1(L.A1, A1, d.w1, d.h1, batch, s)
           : layout == srcnn::fused::kA1Blocked ? srcnn::fused::unblock_a1(L.A1, A1, net->n1, d.w1 * d.h1, batch, s)
                                                : srcnn_memcpy_d2d(A1, L.A1, d.s1 * batch * sizeof(float), stream);
  if (rc) return rc;
  if ((rc = srcnn_memcpy_d2d(A2, L.A2, d.s2 * batch * sizeof(float), stream))) return rc;
  return srcnn_memcpy_d2d(A3, L.A3, d.s3 * batch * sizeof(float), stream);
}

int srcnn_update_all(const srcnn_net* net, float* params, float* grads, float* momentum_bufs,
                     float momentum, float wd, const float* lr, uint32_t batch,
                     srcnn_stream_t stream) {
  SRCNN_REQUIRE(net && params && grads && momentum_bufs && lr, "update_all: null argument");
  SRCNN_REQUIRE(batch > 0, "update_all: batch size must be > 0");
  size_t off[6];
  srcnn_net_offsets(net, off);
  const size_t total = off[5] + 1;
  SRCNN_REQUIRE(total < (1ull << 32), "update_all: parameter count %zu too large", total);
  // layers 3, 2, 1 + the six zero-fills (ConfigBasedDataPipeline.cpp:325-361) in one launch;
  // every element's arithmetic is that of srcnn_sgd_update
  return srcnn::update_all(params, grads, momentum_bufs, off, total, lr, momentum, wd, batch,
                           srcnn::as_stream(stream));
}

size_t srcnn_forward_workspace_bytes(const srcnn_net* net, uint32_t w, uint32_t h,
                                     uint32_t batch) {
  NetDims d;
  if (net_dims(net, w, h, &d) || batch == 0) return 0;
  size_t generic = align_up(d.s1 * batch * sizeof(float)) + align_up(d.s2 * batch * sizeof(float));
  size_t fused = 0;
  if (fast_enabled()) srcnn::fused::forward_plan(net, w, h, batch, &fused);
  return std::max(generic, fused);
}

int srcnn_forward(const srcnn_net* net, const float* X, uint32_t w, uint32_t h, uint32_t batch,
                  const float* params, float* out, void* ws, size_t ws_bytes,
                  srcnn_stream_t stream) {
  NetDims d;
  if (int rc = net_dims(net, w, h, &d)) return rc;
  if (batch == 0) return SRCNN_OK;
  SRCNN_REQUIRE(X && params && out && ws, "forward: null buffer");
  const size_t need = srcnn_forward_workspace_bytes(net, w, h, batch);
  if (ws_bytes < need)
    return fail(SRCNN_ERR_WORKSPACE, "forward: workspace %zu B < %zu B", ws_bytes, need);
  if (fast_enabled()) {  // fused gfx950 inference (forward_fused.hip)
    int rc = srcnn::fused::forward(net, X, w, h, batch, params, out, ws, ws_bytes, as_stream(stream));
    if (rc != 0) return rc < 0 ? rc : tag("fused", SRCNN_OK);
  }
  const auto P = srcnn::split_params(params, net);
  float* A1 = static_cast<float*>(ws);
  float* A2 = reinterpret_cast<float*>(static_cast<char*>(ws) + align_up(d.s1 * batch * sizeof(float)));
  int rc;
  OpSequence seq;
  if ((rc = srcnn_conv_fwd(X, A1, P.W1, P.B1, w, h, 1, net->n1, net->f1, 1, batch, stream))) return rc;
  if ((rc = srcnn_conv_fwd(A1, A2, P.W2, P.B2, d.w1, d.h1, net->n1, net->n2, net->f2, 1, batch, stream)))
    return rc;
  return seq.done(srcnn_conv_fwd(A2, out, P.W3, P.B3, d.w2, d.h2, net->n2, 1, net->f3, 0, batch, stream));
}

}  // extern "C"
