// abi_upscale.cpp -- extern "C" image-level entry points of srcnn.h: the
// resampling operators (srcnn_upscale_*, srcnn_resize_*, srcnn_yuv_*), the
// upscale of an image or a Y'CbCr frame through the net by a scale or to any
// size (srcnn_upscale, _yuv, _frame, _to, _frame_to), and what prepares and
// judges images around them (srcnn_downscale_rgba, srcnn_gather_*,
// srcnn_make_pairs, srcnn_quality, srcnn_quality_frame, srcnn_evaluate).
//
// Every call validates its arguments before its first launch.  The net-level
// calls are composed of the public operators and of srcnn_sub_mean and
// srcnn_forward (abi.cpp); nothing here knows how those dispatch.
//
// A call either names a scale (1..4: the kernels of upscale.hip and yuv.hip,
// templates over it) or an output size (the general kernels of resize.hip,
// DESIGN.md 16).  Both kinds go through one flow: the kind picks the wording
// of the size errors, the chroma-size rule and the launcher, once per stage.
#include <cstdio>

#include "common.hpp"
#include "ops.hpp"

using srcnn::align_up;
using srcnn::as_stream;
using srcnn::fail;

namespace {

const uint64_t kIndexMax = 0x7fffffffull;  // INT32_MAX: what the kernels' int indices reach

int check_scale(const char* who, uint32_t scale) {
  SRCNN_REQUIRE(scale >= 1 && scale <= 4, "%s: scale %u is not 1, 2, 3 or 4", who, scale);
  return SRCNN_OK;
}

// What a call asks for: `who`, the source w x h, and either a scale or the
// output W x H (by_scale says which; the other is unset).
struct UpRequest {
  const char* who;
  uint32_t w, h;
  bool by_scale;
  uint32_t scale, W, H;
};
UpRequest by_scale(const char* who, uint32_t w, uint32_t h, uint32_t scale) {
  return {who, w, h, true, scale, 0, 0};
}
UpRequest to_size(const char* who, uint32_t w, uint32_t h, uint32_t W, uint32_t H) {
  return {who, w, h, false, 0, W, H};
}

// The sizes of one upscale, checked against what the kernels can index (int
// coordinates and element offsets below 2^31); rgb: the call writes an rgb
// image.  A size within [1x, 4x] of the source per axis.
struct UpDims {
  uint32_t W, H, PW, PH;  // output image, padded plane
};
int up_dims(const UpRequest& r, uint32_t pad, bool rgb, UpDims* d) {
  uint64_t W = r.W, H = r.H;
  if (r.by_scale) {
    if (int rc = check_scale(r.who, r.scale)) return rc;
    SRCNN_REQUIRE(r.w > 0 && r.h > 0, "%s: empty image %ux%u", r.who, r.w, r.h);
    W = (uint64_t)r.w * r.scale;
    H = (uint64_t)r.h * r.scale;
  } else {
    SRCNN_REQUIRE(r.w > 0 && r.h > 0 && r.W > 0 && r.H > 0, "%s: empty image: %ux%u -> %ux%u", r.who, r.w,
                  r.h, r.W, r.H);
    SRCNN_REQUIRE(W >= r.w && W <= 4ull * r.w && H >= r.h && H <= 4ull * r.h,
                  "%s: output %ux%u is outside 1x .. 4x of the source %ux%u on an axis (upscaling only, "
                  "by at most 4)",
                  r.who, r.W, r.H, r.w, r.h);
  }
  const uint64_t PW = W + pad, PH = H + pad;
  if (!(PW <= kIndexMax && PH <= kIndexMax && PW * PH <= kIndexMax && (!rgb || 3 * W * H <= kIndexMax))) {
    // (each kind's own wording: a size names the rgb bytes whether or not they count)
    char what[64];
    if (r.by_scale)
      snprintf(what, sizeof what, "%ux%u x%u", r.w, r.h, r.scale);
    else
      snprintf(what, sizeof what, "%ux%u -> %ux%u", r.w, r.h, r.W, r.H);
    return fail(SRCNN_ERR_INVALID,
                "%s: %s with padding %u exceeds the kernels' 32-bit index: the padded plane's floats%s "
                "number at most 2^31-1",
                r.who, what, pad, rgb || !r.by_scale ? " and the rgb bytes must each" : " must");
  }
  d->W = (uint32_t)W;
  d->H = (uint32_t)H;
  d->PW = (uint32_t)PW;
  d->PH = (uint32_t)PH;
  return SRCNN_OK;
}

// The sizes of one byte plane against what the kernels of yuv.hip and
// resize.hip can index (int coordinates, at most 2^31-1 elements in a plane;
// row offsets are size_t).  A pixel is nch samples of B bytes:
// the pitch is in bytes, and even for two-byte samples.
int plane_dims(const char* who, uint32_t w, uint32_t h, uint32_t pitch, uint32_t B = 1,
               uint32_t nch = 1) {
  SRCNN_REQUIRE(w > 0 && h > 0, "%s: empty plane %ux%u", who, w, h);
  if (B * nch == 1) {
    SRCNN_REQUIRE(pitch >= w, "%s: pitch %u is below the row width %u", who, pitch, w);
  } else {
    SRCNN_REQUIRE(pitch >= (uint64_t)w * nch * B,
                  "%s: pitch %u is below the %llu bytes of a row of %u x %u samples of %u bytes", who,
                  pitch, (unsigned long long)w * nch * B, w, nch, B);
  }
  SRCNN_REQUIRE(B == 1 || pitch % 2 == 0, "%s: pitch %u of two-byte samples is odd", who, pitch);
  SRCNN_REQUIRE((uint64_t)w * h * nch <= kIndexMax,
                "%s: plane %ux%u exceeds the kernels' 32-bit index: a plane's elements must "
                "number at most 2^31-1",
                who, w, h);
  return SRCNN_OK;
}
// the sample format of DESIGN.md 15; *B: bytes per sample
int yuv_samples(const char* who, uint32_t bits, uint32_t msb, uint32_t* B) {
  SRCNN_REQUIRE(bits >= 8 && bits <= 16, "%s: %u bits per sample is outside 8..16", who, bits);
  SRCNN_REQUIRE(msb <= 1, "%s: msb %u is neither 0 nor 1", who, msb);
  SRCNN_REQUIRE(!(msb && bits == 8), "%s: msb 1 with one-byte samples", who);
  *B = bits == 8 ? 1 : 2;
  return SRCNN_OK;
}
bool odd_address(uint32_t B, const void* p) { return B == 2 && ((uintptr_t)p & 1); }
int yuv_range(const char* who, int range) {
  SRCNN_REQUIRE(range == SRCNN_YUV_LIMITED || range == SRCNN_YUV_FULL,
                "%s: range %d is neither SRCNN_YUV_LIMITED nor SRCNN_YUV_FULL", who, range);
  return SRCNN_OK;
}
int yuv_layout(const char* who, uint32_t layout) {
  SRCNN_REQUIRE(layout == SRCNN_YUV_PLANAR || layout == SRCNN_YUV_SEMIPLANAR,
                "%s: layout %u is neither SRCNN_YUV_PLANAR nor SRCNN_YUV_SEMIPLANAR", who, layout);
  return SRCNN_OK;
}

// up_dims for a luma plane of bytes at `pitch`.  The two kinds make the same
// checks in their own order, which decides the message of an input with two
// faults: a scale call looks at the source plane before the sizes, a size call
// after (where every check of the plane but the pitch's has been made).
int luma_dims(const UpRequest& r, uint32_t pitch, uint32_t B, uint32_t pad, UpDims* d) {
  if (r.by_scale) {
    if (int rc = check_scale(r.who, r.scale)) return rc;
    if (int rc = plane_dims(r.who, r.w, r.h, pitch, B)) return rc;
    return up_dims(r, pad, false, d);
  }
  if (int rc = up_dims(r, pad, false, d)) return rc;
  return plane_dims(r.who, r.w, r.h, pitch, B);
}

// How a chroma plane call maps its source to its output: by a scale, the
// output a crop of the scaled source that keeps its last tile (DESIGN.md
// 14.1), or at the source steps rx_num / rx_den and ry_num / ry_den per
// output sample
struct PlaneMap {
  bool by_scale;
  uint32_t scale, rx_num, rx_den, ry_num, ry_den;
};
// one axis of a PlaneMap of ratios: n source samples, N outputs
int resize_axis(const char* who, const char* axis, uint32_t rn, uint32_t rd, uint32_t n, uint32_t N) {
  SRCNN_REQUIRE(rn > 0, "%s: the %s ratio %u/%u has a zero numerator", who, axis, rn, rd);
  SRCNN_REQUIRE(rd >= rn && rd <= 4ull * rn,
                "%s: the %s ratio %u/%u is outside 1x .. 4x (den / num must lie in [1, 4])", who, axis,
                rn, rd);
  const uint64_t bound = ((uint64_t)n * rd + rn - 1) / rn;
  SRCNN_REQUIRE(N <= bound, "%s: %s output size %u exceeds ceil(%u * %u / %u) = %llu", who, axis, N, n,
                rd, rn, (unsigned long long)bound);
  // (2 X' + 1) rn of the map, a signed 64-bit integer in the kernel
  SRCNN_REQUIRE(2ull * N + 1 <= 0x7fffffffffffffffull / rn,
                "%s: the %s ratio %u/%u at %u outputs exceeds the map's 64-bit integers", who, axis, rn,
                rd, N);
  return SRCNN_OK;
}
// the output ow x oh of a source pw x ph under the map (its scale checked before)
int plane_map_dims(const char* who, const PlaneMap& m, uint32_t pw, uint32_t ph, uint32_t ow, uint32_t oh) {
  if (m.by_scale) {
    const uint64_t s = m.scale;
    SRCNN_REQUIRE(s * (pw - 1) < ow && ow <= s * pw && s * (ph - 1) < oh && oh <= s * ph,
                  "%s: output %ux%u is not a crop of the x%u of %ux%u that keeps its last tile", who,
                  ow, oh, m.scale, pw, ph);
    return SRCNN_OK;
  }
  if (int rc = resize_axis(who, "horizontal", m.rx_num, m.rx_den, pw, ow)) return rc;
  return resize_axis(who, "vertical", m.ry_num, m.ry_den, ph, oh);
}

// The Y'CbCr operations, each behind its op-level entry points (the 8-bit
// ones: bits 8, msb 0, planar) and the net-level calls; `who` is the one the
// caller used.
int yuv_luma(const UpRequest& r, const void* y, uint32_t pitch_y, float* luma_padded, uint32_t pad,
             uint32_t bits, uint32_t msb, int range, srcnn_stream_t stream) {
  UpDims d;
  uint32_t B;
  if (int rc = yuv_samples(r.who, bits, msb, &B)) return rc;
  if (int rc = luma_dims(r, pitch_y, B, pad, &d)) return rc;
  if (int rc = yuv_range(r.who, range)) return rc;
  SRCNN_REQUIRE(y && luma_padded, "%s: null buffer", r.who);
  SRCNN_REQUIRE(!odd_address(B, y), "%s: odd address of two-byte samples", r.who);
  const bool full = range == SRCNN_YUV_FULL;
  return r.by_scale ? srcnn::yuv_upscale_luma(y, pitch_y, luma_padded, r.w, r.h, r.scale, pad, bits, msb != 0,
                                              full, as_stream(stream))
                    : srcnn::yuv_resize_luma(y, pitch_y, luma_padded, r.w, r.h, r.W, r.H, pad, bits, msb != 0,
                                             full, as_stream(stream));
}
int yuv_compose_luma(const char* who, const float* luma, void* y, uint32_t pitch_y, uint32_t W,
                     uint32_t H, uint32_t bits, uint32_t msb, int range, srcnn_stream_t stream) {
  uint32_t B;
  if (int rc = yuv_samples(who, bits, msb, &B)) return rc;
  if (int rc = plane_dims(who, W, H, pitch_y, B)) return rc;
  if (int rc = yuv_range(who, range)) return rc;
  SRCNN_REQUIRE(luma && y, "%s: null buffer", who);
  SRCNN_REQUIRE(!odd_address(B, y), "%s: odd address of two-byte samples", who);
  return srcnn::yuv_compose_luma(luma, y, pitch_y, W, H, bits, msb != 0, range == SRCNN_YUV_FULL,
                                 as_stream(stream));
}
int chroma_planes(const char* who, const void* src0, const void* src1, uint32_t src_pitch, uint32_t pw,
                  uint32_t ph, void* dst0, void* dst1, uint32_t dst_pitch, uint32_t ow, uint32_t oh,
                  const PlaneMap& m, uint32_t bits, uint32_t msb, uint32_t layout, srcnn_stream_t stream) {
  uint32_t B;
  if (int rc = yuv_samples(who, bits, msb, &B)) return rc;
  if (int rc = yuv_layout(who, layout)) return rc;
  const bool semi = layout == SRCNN_YUV_SEMIPLANAR;
  if (m.by_scale)
    if (int rc = check_scale(who, m.scale)) return rc;
  if (int rc = plane_dims(who, pw, ph, src_pitch, B, semi ? 2 : 1)) return rc;
  if (int rc = plane_dims(who, ow, oh, dst_pitch, B, semi ? 2 : 1)) return rc;
  if (int rc = plane_map_dims(who, m, pw, ph, ow, oh)) return rc;
  SRCNN_REQUIRE(src0 && dst0, "%s: null buffer", who);
  if (semi) {
    SRCNN_REQUIRE(!src1 && !dst1, "%s: a semi-planar frame has no second chroma plane", who);
  } else {
    SRCNN_REQUIRE(src1 && dst1, "%s: null buffer", who);
  }
  SRCNN_REQUIRE(!odd_address(B, src0) && !odd_address(B, src1) && !odd_address(B, dst0) &&
                    !odd_address(B, dst1),
                "%s: odd address of two-byte samples", who);
  return m.by_scale ? srcnn::upscale_planes(src0, src1, src_pitch, pw, ph, dst0, dst1, dst_pitch, ow, oh,
                                            m.scale, bits, msb != 0, semi, as_stream(stream))
                    : srcnn::resize_planes(src0, src1, src_pitch, pw, ph, dst0, dst1, dst_pitch, ow, oh,
                                           m.rx_num, m.rx_den, m.ry_num, m.ry_den, bits, msb != 0, semi,
                                           as_stream(stream));
}

// the two operations on an rgba image, likewise
int rgba_luma(const UpRequest& r, const uint8_t* rgba, float* luma_padded, uint32_t pad,
              srcnn_stream_t stream) {
  UpDims d;
  if (int rc = up_dims(r, pad, true, &d)) return rc;
  SRCNN_REQUIRE(rgba && luma_padded, "%s: null buffer", r.who);
  return r.by_scale ? srcnn::upscale_luma(rgba, luma_padded, r.w, r.h, r.scale, pad, as_stream(stream))
                    : srcnn::resize_luma(rgba, luma_padded, r.w, r.h, r.W, r.H, pad, as_stream(stream));
}
int rgba_compose(const UpRequest& r, const uint8_t* rgba, const float* new_luma, uint8_t* rgb,
                 srcnn_stream_t stream) {
  UpDims d;
  if (int rc = up_dims(r, 0, true, &d)) return rc;
  SRCNN_REQUIRE(rgba && new_luma && rgb, "%s: null buffer", r.who);
  return r.by_scale ? srcnn::upscale_compose(rgba, new_luma, rgb, r.w, r.h, r.scale, as_stream(stream))
                    : srcnn::resize_compose(rgba, new_luma, rgb, r.w, r.h, r.W, r.H, as_stream(stream));
}

// ---- through the net ----
// the net's total padding (Config::total_padding), and as an int the kernels can index
uint64_t padding(const srcnn_net* net) { return (uint64_t)net->f1 + net->f2 + net->f3 - 3; }
int net_pad(const char* who, const srcnn_net* net, uint32_t* pad) {
  SRCNN_REQUIRE(net, "%s: null srcnn_net", who);
  SRCNN_REQUIRE(padding(net) <= kIndexMax, "%s: total padding %llu too large", who,
                (unsigned long long)padding(net));
  *pad = (uint32_t)padding(net);
  return SRCNN_OK;
}

// regions of the upscale workspace: padded plane | net output | reduction
// scratch | forward workspace, each 256-byte aligned
struct UpWs {
  size_t plane, out, red, fwd, total;  // byte offsets of the regions, and their sum
  size_t red_bytes, fwd_bytes;         // what the reduction and the forward are given
};
bool up_ws(const srcnn_net* net, const UpDims& d, UpWs* L) {
  L->fwd_bytes = srcnn_forward_workspace_bytes(net, d.PW, d.PH, 1);
  if (L->fwd_bytes == 0) return false;
  const size_t plane = (size_t)d.PW * d.PH;
  L->red_bytes = srcnn_reduce_workspace_bytes(plane);
  L->plane = 0;
  L->out = L->plane + align_up(plane * sizeof(float));
  L->red = L->out + align_up((size_t)d.W * d.H * sizeof(float));
  L->fwd = L->red + align_up(L->red_bytes);
  L->total = L->fwd + align_up(L->fwd_bytes);
  return true;
}
// What the net-level calls do between their checks and their composition: the
// workspace carved and measured, fill_plane(plane) for the padded bicubic
// luma, then the plane minus its mean through the net.  *luma: the net's
// output [H][W], in ws.
template <typename FillPlane>
int up_net(const char* who, const srcnn_net* net, const UpDims& d, const float* params, void* ws,
           size_t ws_bytes, srcnn_stream_t stream, FillPlane fill_plane, float** luma) {
  UpWs L;
  if (!up_ws(net, d, &L)) return SRCNN_ERR_INVALID;  // (message from net_dims)
  if (ws_bytes < L.total)
    return fail(SRCNN_ERR_WORKSPACE, "%s: workspace %zu B < %zu B", who, ws_bytes, L.total);
  char* p = static_cast<char*>(ws);
  float* plane = reinterpret_cast<float*>(p + L.plane);
  *luma = reinterpret_cast<float*>(p + L.out);
  int rc;
  if ((rc = fill_plane(plane))) return rc;
  // the mean of what the net sees: the whole padded plane; not added back
  // (the reference flow: cnn.cpp subtracts it and pastes the net's output)
  if ((rc = srcnn_sub_mean(plane, (size_t)d.PW * d.PH, nullptr, p + L.red, L.red_bytes, stream)))
    return rc;
  return srcnn_forward(net, plane, d.PW, d.PH, 1, params, *luma, p + L.fwd, L.fwd_bytes, stream);
}

// srcnn_upscale and srcnn_upscale_to: every check that does not need the
// buffers, the workspace, the call
int image_dims(const UpRequest& r, const srcnn_net* net, uint32_t* pad, UpDims* d) {
  if (int rc = net_pad(r.who, net, pad)) return rc;
  return up_dims(r, *pad, true, d);
}
size_t image_workspace_bytes(const UpRequest& r, const srcnn_net* net) {
  uint32_t pad;
  UpDims d;
  UpWs L;
  return !image_dims(r, net, &pad, &d) && up_ws(net, d, &L) ? L.total : 0;
}
int upscale_image(const UpRequest& r, const srcnn_net* net, const uint8_t* rgba, const float* params,
                  uint8_t* rgb, void* ws, size_t ws_bytes, srcnn_stream_t stream) {
  uint32_t pad;
  UpDims d;
  if (int rc = image_dims(r, net, &pad, &d)) return rc;
  SRCNN_REQUIRE(rgba && params && rgb && ws, "%s: null buffer", r.who);
  float* out;
  const auto luma = [&](float* plane) { return rgba_luma(r, rgba, plane, pad, stream); };
  if (int rc = up_net(r.who, net, d, params, ws, ws_bytes, stream, luma, &out)) return rc;
  return rgba_compose(r, rgba, out, rgb, stream);
}

// srcnn_upscale_yuv (8 bits, planar), srcnn_upscale_frame and
// srcnn_upscale_frame_to, likewise; the chroma sizes of the source (cw x ch)
// and of the output (CW x CH)
struct FrameDims {
  UpDims d;
  uint32_t pad, cw, ch, CW, CH;
};
int frame_dims(const UpRequest& r, const srcnn_net* net, uint32_t cx, uint32_t cy, FrameDims* f) {
  if (int rc = net_pad(r.who, net, &f->pad)) return rc;
  SRCNN_REQUIRE((cx == 2 && cy == 2) || (cx == 2 && cy == 1) || (cx == 1 && cy == 1),
                "%s: chroma subsampling %ux%u is not 2x2 (4:2:0), 2x1 (4:2:2) or 1x1 (4:4:4)", r.who,
                cx, cy);
  // (a luma plane of bytes at its own width: the frames' pitches come later)
  if (int rc = luma_dims(r, r.w, 1, f->pad, &f->d)) return rc;
  f->cw = (r.w - 1) / cx + 1;
  f->ch = (r.h - 1) / cy + 1;
  f->CW = (f->d.W - 1) / cx + 1;
  f->CH = (f->d.H - 1) / cy + 1;
  return SRCNN_OK;
}
size_t frame_workspace_bytes(const UpRequest& r, const srcnn_net* net) {
  FrameDims f;
  UpWs L;
  return !frame_dims(r, net, 1, 1, &f) && up_ws(net, f.d, &L) ? L.total : 0;
}
int upscale_frame(const UpRequest& r, const srcnn_net* net, const srcnn_yuv_format& fmt,
                  const srcnn_yuv_frame* src, const srcnn_yuv_frame* dst, const float* params, void* ws,
                  size_t ws_bytes, srcnn_stream_t stream) {
  const char* who = r.who;
  FrameDims f;
  uint32_t B;
  if (int rc = frame_dims(r, net, fmt.cx, fmt.cy, &f)) return rc;
  if (int rc = yuv_range(who, fmt.range)) return rc;
  if (int rc = yuv_samples(who, fmt.bits, fmt.msb, &B)) return rc;
  if (int rc = yuv_layout(who, fmt.layout)) return rc;
  const bool semi = fmt.layout == SRCNN_YUV_SEMIPLANAR;
  const uint32_t nch = semi ? 2 : 1;
  SRCNN_REQUIRE(src && dst && params && ws, "%s: null buffer", who);
  SRCNN_REQUIRE(src->y && src->u && dst->y && dst->u, "%s: null plane", who);
  if (semi) {
    SRCNN_REQUIRE(!src->v && !dst->v, "%s: a semi-planar frame has no v plane", who);
  } else {
    SRCNN_REQUIRE(src->v && dst->v, "%s: null plane", who);
  }
  SRCNN_REQUIRE(!odd_address(B, src->y) && !odd_address(B, src->u) && !odd_address(B, src->v) &&
                    !odd_address(B, dst->y) && !odd_address(B, dst->u) && !odd_address(B, dst->v),
                "%s: odd address of two-byte samples", who);
  // (the planes again, now with the frames' pitches; the chroma takes the luma's scale or ratios)
  const UpDims& d = f.d;
  const PlaneMap m = r.by_scale ? PlaneMap{true, r.scale, 0, 0, 0, 0} : PlaneMap{false, 0, r.w, d.W, r.h, d.H};
  if (int rc = plane_dims(who, r.w, r.h, src->pitch_y, B)) return rc;
  if (int rc = plane_dims(who, d.W, d.H, dst->pitch_y, B)) return rc;
  if (int rc = plane_dims(who, f.cw, f.ch, src->pitch_c, B, nch)) return rc;
  if (int rc = plane_dims(who, f.CW, f.CH, dst->pitch_c, B, nch)) return rc;
  if (int rc = plane_map_dims(who, m, f.cw, f.ch, f.CW, f.CH)) return rc;
  float* out;
  const auto luma = [&](float* plane) {
    return yuv_luma(r, src->y, src->pitch_y, plane, f.pad, fmt.bits, fmt.msb, fmt.range, stream);
  };
  if (int rc = up_net(who, net, d, params, ws, ws_bytes, stream, luma, &out)) return rc;
  if (int rc = yuv_compose_luma(who, out, dst->y, dst->pitch_y, d.W, d.H, fmt.bits, fmt.msb, fmt.range,
                                stream))
    return rc;
  return chroma_planes(who, src->u, src->v, src->pitch_c, f.cw, f.ch, dst->u, dst->v, dst->pitch_c, f.CW,
                       f.CH, m, fmt.bits, fmt.msb, fmt.layout, stream);
}

// srcnn_downscale_rgba / srcnn_make_pairs / srcnn_evaluate: the source against
// the scale and against what downscale_rgba_kernel can index (pixel offsets
// below 2^31)
int down_dims(const char* who, uint32_t W, uint32_t H, uint32_t scale) {
  if (int rc = check_scale(who, scale)) return rc;
  SRCNN_REQUIRE(W >= scale && H >= scale, "%s: image %ux%u is smaller than the scale %u", who, W, H,
                scale);
  SRCNN_REQUIRE((uint64_t)W * H <= kIndexMax,
                "%s: %ux%u exceeds the kernel's 32-bit index: the source's pixels must number at "
                "most 2^31-1",
                who, W, H);
  return SRCNN_OK;
}

// srcnn_gather_tiles: the grid against the plane and against what
// gather_tiles_kernel can index (int coordinates, one workgroup per tile)
int gather_dims(const char* who, uint32_t pw, uint32_t ph, uint32_t x0, uint32_t y0,
                uint32_t stride, uint32_t nx, uint32_t ny, uint32_t tw, uint32_t th) {
  SRCNN_REQUIRE(stride > 0 && nx > 0 && ny > 0 && tw > 0 && th > 0,
                "%s: stride(%u), grid %ux%u and tile %ux%u must be > 0", who, stride, nx, ny, tw, th);
  SRCNN_REQUIRE((uint64_t)x0 + (uint64_t)(nx - 1) * stride + tw <= pw &&
                    (uint64_t)y0 + (uint64_t)(ny - 1) * stride + th <= ph,
                "%s: %ux%u tiles of %ux%u from (%u, %u) at stride %u leave the %ux%u plane", who, nx,
                ny, tw, th, x0, y0, stride, pw, ph);
  SRCNN_REQUIRE((uint64_t)pw * ph <= kIndexMax && (uint64_t)nx * ny <= kIndexMax,
                "%s: plane %ux%u or grid %ux%u exceeds the kernel's 32-bit index: the plane's floats "
                "and the tiles must each number at most 2^31-1",
                who, pw, ph, nx, ny);
  return SRCNN_OK;
}

// regions of the make_pairs workspace: low-resolution image | X plane
// [Hc][Wc] | T plane [H][W], each 256-byte aligned
struct PairWs {
  uint32_t w, h, Wc, Hc;
  size_t small, xplane, tplane, total;  // byte offsets of the regions, and their sum
};
int pair_ws(const char* who, uint32_t W, uint32_t H, uint32_t scale, PairWs* L) {
  if (int rc = down_dims(who, W, H, scale)) return rc;
  L->w = W / scale;
  L->h = H / scale;
  UpDims u;
  if (int rc = up_dims(by_scale(who, L->w, L->h, scale), 0, true, &u)) return rc;
  L->Wc = u.W;
  L->Hc = u.H;
  L->small = 0;
  L->xplane = L->small + align_up((size_t)L->w * L->h * 4);
  L->tplane = L->xplane + align_up((size_t)L->Wc * L->Hc * sizeof(float));
  L->total = L->tplane + align_up((size_t)W * H * sizeof(float));
  return SRCNN_OK;
}

// srcnn_quality / srcnn_evaluate: the shaved window against the 11 x 11 SSIM
// window and against what quality_tiles_kernel can index (int coordinates)
struct QualityDims {
  uint32_t Ws, Hs;
  size_t partial_bytes;  // two doubles per workgroup
};
bool known_format(int fmt) {
  return fmt == SRCNN_PIX_LUMA_F32 || fmt == SRCNN_PIX_RGB8 || fmt == SRCNN_PIX_RGBA8;
}
int quality_dims(const char* who, uint32_t W, uint32_t H, uint32_t shave, QualityDims* d) {
  SRCNN_REQUIRE(2 * (uint64_t)shave + 11 <= W && 2 * (uint64_t)shave + 11 <= H,
                "%s: image %ux%u with %u pixels shaved per side is smaller than the 11x11 window",
                who, W, H, shave);
  SRCNN_REQUIRE((uint64_t)W * H <= kIndexMax,
                "%s: %ux%u exceeds the kernels' 32-bit index: the pixels must number at most 2^31-1",
                who, W, H);
  d->Ws = W - 2 * shave;
  d->Hs = H - 2 * shave;
  d->partial_bytes = (size_t)srcnn::quality_tile_count(d->Ws, d->Hs) * 2 * sizeof(double);
  return SRCNN_OK;
}
// one image of srcnn_quality: format, pitch, base
int quality_image(const char* who, const void* p, int fmt, uint32_t pitch, uint32_t W, uint32_t H) {
  SRCNN_REQUIRE(known_format(fmt), "quality: image %s has unknown pixel format %d", who, fmt);
  SRCNN_REQUIRE(pitch >= W, "quality: image %s has pitch %u < width %u", who, pitch, W);
  SRCNN_REQUIRE(p, "quality: null buffer (image %s)", who);
  SRCNN_REQUIRE(fmt == SRCNN_PIX_RGB8 || ((uintptr_t)p & 3) == 0,
                "quality: image %s (format %d) is not 4-byte aligned", who, fmt);
  SRCNN_REQUIRE((uint64_t)pitch * H <= kIndexMax,
                "quality: image %s, pitch %u x %u rows, exceeds the kernels' 32-bit index: the "
                "pixels must number at most 2^31-1",
                who, pitch, H);
  return SRCNN_OK;
}
size_t pixel_bytes(int fmt) { return fmt == SRCNN_PIX_RGB8 ? 3 : 4; }

// srcnn_quality_frame: the shaved luma window Ws x Hs of a w x h frame and the
// chroma windows CWs x CHs that sx columns and sy rows per side leave of its
// cw x ch chroma planes, against the SSIM window and the
// kernels' int coordinates
bool known_subsampling(uint32_t cx, uint32_t cy) {
  return (cx == 2 && cy == 2) || (cx == 2 && cy == 1) || (cx == 1 && cy == 1);
}
struct FrameQualityDims {
  uint32_t Ws, Hs, cw, ch, sx, sy, CWs, CHs;
  size_t ws_bytes;  // two words per luma tile, one per chroma tile and plane
};
int quality_frame_dims(const char* who, uint32_t w, uint32_t h, uint32_t cx, uint32_t cy, uint32_t shave,
                       FrameQualityDims* d) {
  SRCNN_REQUIRE(known_subsampling(cx, cy),
                "%s: chroma subsampling %ux%u is not 2x2 (4:2:0), 2x1 (4:2:2) or 1x1 (4:4:4)", who, cx, cy);
  SRCNN_REQUIRE(2 * (uint64_t)shave + 11 <= w && 2 * (uint64_t)shave + 11 <= h,
                "%s: frame %ux%u with %u pixels shaved per side is smaller than the 11x11 window", who, w, h,
                shave);
  SRCNN_REQUIRE((uint64_t)w * h <= kIndexMax,
                "%s: %ux%u exceeds the kernels' 32-bit index: a plane's samples must number at most 2^31-1",
                who, w, h);
  d->Ws = w - 2 * shave;
  d->Hs = h - 2 * shave;
  d->cw = (w - 1) / cx + 1;
  d->ch = (h - 1) / cy + 1;
  d->sx = (shave + cx - 1) / cx;
  d->sy = (shave + cy - 1) / cy;
  SRCNN_REQUIRE(2 * (uint64_t)d->sx < d->cw && 2 * (uint64_t)d->sy < d->ch,
                "%s: %u pixels shaved per side leave nothing of the %ux%u chroma planes", who, shave, d->cw,
                d->ch);
  d->CWs = d->cw - 2 * d->sx;
  d->CHs = d->ch - 2 * d->sy;
  d->ws_bytes = align_up(((size_t)srcnn::quality_tile_count(d->Ws, d->Hs) +
                          (size_t)srcnn::quality_chroma_tile_count(d->CWs, d->CHs)) *
                         2 * sizeof(double));
  return SRCNN_OK;
}
// one frame of srcnn_quality_frame with its format, as srcnn_upscale_frame
// checks a frame; *side: its shaved windows
int quality_frame_side(const char* who, const srcnn_yuv_format* fmt, const srcnn_yuv_frame* f, uint32_t w,
                       uint32_t h, const FrameQualityDims& d, uint32_t shave, srcnn::QualityFrameSide* side) {
  uint32_t B;
  if (int rc = yuv_range(who, fmt->range)) return rc;
  if (int rc = yuv_samples(who, fmt->bits, fmt->msb, &B)) return rc;
  if (int rc = yuv_layout(who, fmt->layout)) return rc;
  const bool semi = fmt->layout == SRCNN_YUV_SEMIPLANAR;
  const uint32_t nch = semi ? 2 : 1;
  SRCNN_REQUIRE(f->y && f->u, "%s: null plane", who);
  if (semi) {
    SRCNN_REQUIRE(!f->v, "%s: a semi-planar frame has no v plane", who);
  } else {
    SRCNN_REQUIRE(f->v, "%s: null plane", who);
  }
  SRCNN_REQUIRE(!odd_address(B, f->y) && !odd_address(B, f->u) && !odd_address(B, f->v),
                "%s: odd address of two-byte samples", who);
  if (int rc = plane_dims(who, w, h, f->pitch_y, B)) return rc;
  if (int rc = plane_dims(who, d.cw, d.ch, f->pitch_c, B, nch)) return rc;
  const size_t oc = (size_t)d.sy * f->pitch_c + (size_t)d.sx * nch * B;
  *side = srcnn::QualityFrameSide{f->y + (size_t)shave * f->pitch_y + (size_t)shave * B,
                                  f->u + oc,
                                  semi ? nullptr : f->v + oc,
                                  f->pitch_y,
                                  f->pitch_c,
                                  fmt->msb != 0,
                                  semi};
  return SRCNN_OK;
}

// regions of the evaluate workspace: low-resolution image | rgb [Hc][Wc][3] |
// luma plane [Hc][Wc] | srcnn_upscale's workspace | srcnn_quality's, each
// 256-byte aligned
struct EvalWs {
  uint32_t w, h, Wc, Hc;
  size_t small, rgb, plane, up, q, total;  // byte offsets of the regions, and their sum
  size_t up_bytes, q_bytes;                // what the upscale and the metric are given
};
// every check of the six calls that does not need the buffers; shave < 0: the
// sizes alone (the workspace query: the metric's workspace does not depend on
// the shave, it is sized for shave = 0)
int eval_ws(const srcnn_net* net, uint32_t W, uint32_t H, uint32_t scale, int64_t shave, EvalWs* L) {
  SRCNN_REQUIRE(net, "evaluate: null srcnn_net");
  if (int rc = down_dims("evaluate", W, H, scale)) return rc;
  L->w = W / scale;
  L->h = H / scale;
  L->up_bytes = srcnn_upscale_workspace_bytes(net, L->w, L->h, scale);
  if (L->up_bytes == 0) return SRCNN_ERR_INVALID;  // (message from net_dims / up_dims)
  L->Wc = L->w * scale;
  L->Hc = L->h * scale;
  QualityDims q;
  if (int rc = quality_dims("evaluate", L->Wc, L->Hc, shave < 0 ? 0 : (uint32_t)shave, &q)) return rc;
  L->q_bytes = srcnn_quality_workspace_bytes(L->Wc, L->Hc, 0);
  L->small = 0;
  L->rgb = L->small + align_up((size_t)L->w * L->h * 4);
  L->plane = L->rgb + align_up((size_t)L->Wc * L->Hc * 3);
  L->up = L->plane + align_up((size_t)L->Wc * L->Hc * sizeof(float));
  L->q = L->up + align_up(L->up_bytes);
  L->total = L->q + align_up(L->q_bytes);
  return SRCNN_OK;
}

// ---- the down direction of the video family ----
// srcnn_downscale_planes behind its entry point and the frame-level calls
int down_planes(const char* who, const void* src0, const void* src1, uint32_t src_pitch, uint32_t pw,
                uint32_t ph, void* dst0, void* dst1, uint32_t dst_pitch, uint32_t ow, uint32_t oh,
                uint32_t scale, uint32_t bits, uint32_t msb, uint32_t layout, srcnn_stream_t stream) {
  uint32_t B;
  if (int rc = yuv_samples(who, bits, msb, &B)) return rc;
  if (int rc = yuv_layout(who, layout)) return rc;
  const bool semi = layout == SRCNN_YUV_SEMIPLANAR;
  if (int rc = check_scale(who, scale)) return rc;
  if (int rc = plane_dims(who, pw, ph, src_pitch, B, semi ? 2 : 1)) return rc;
  if (int rc = plane_dims(who, ow, oh, dst_pitch, B, semi ? 2 : 1)) return rc;
  SRCNN_REQUIRE(ow <= (pw - 1) / scale + 1 && oh <= (ph - 1) / scale + 1,
                "%s: output %ux%u exceeds ceil(%u / %u) x ceil(%u / %u)", who, ow, oh, pw, scale, ph, scale);
  SRCNN_REQUIRE(src0 && dst0, "%s: null buffer", who);
  if (semi) {
    SRCNN_REQUIRE(!src1 && !dst1, "%s: a semi-planar frame has no second chroma plane", who);
  } else {
    SRCNN_REQUIRE(!src1 == !dst1, "%s: exactly one of src1 and dst1 is null", who);
  }
  SRCNN_REQUIRE(!odd_address(B, src0) && !odd_address(B, src1) && !odd_address(B, dst0) &&
                    !odd_address(B, dst1),
                "%s: odd address of two-byte samples", who);
  return srcnn::downscale_planes(src0, src1, src_pitch, pw, ph, dst0, dst1, dst_pitch, ow, oh, scale, bits,
                                 msb != 0, semi, as_stream(stream));
}

// a frame format as srcnn_upscale_frame checks one; *B: bytes per sample,
// *nch: samples per chroma pixel of a chroma plane
int frame_format(const char* who, const srcnn_yuv_format* fmt, uint32_t* B, uint32_t* nch) {
  SRCNN_REQUIRE(fmt, "%s: null srcnn_yuv_format", who);
  SRCNN_REQUIRE(known_subsampling(fmt->cx, fmt->cy),
                "%s: chroma subsampling %ux%u is not 2x2 (4:2:0), 2x1 (4:2:2) or 1x1 (4:4:4)", who, fmt->cx,
                fmt->cy);
  if (int rc = yuv_range(who, fmt->range)) return rc;
  if (int rc = yuv_samples(who, fmt->bits, fmt->msb, B)) return rc;
  if (int rc = yuv_layout(who, fmt->layout)) return rc;
  *nch = fmt->layout == SRCNN_YUV_SEMIPLANAR ? 2 : 1;
  return SRCNN_OK;
}
// the planes of a frame of w x h luma samples: present, aligned, pitched
int frame_planes(const char* who, const srcnn_yuv_format& fmt, const srcnn_yuv_frame* f, uint32_t w,
                 uint32_t h, uint32_t B, uint32_t nch) {
  SRCNN_REQUIRE(f, "%s: null buffer", who);
  SRCNN_REQUIRE(f->y && f->u, "%s: null plane", who);
  if (nch == 2) {
    SRCNN_REQUIRE(!f->v, "%s: a semi-planar frame has no v plane", who);
  } else {
    SRCNN_REQUIRE(f->v, "%s: null plane", who);
  }
  SRCNN_REQUIRE(!odd_address(B, f->y) && !odd_address(B, f->u) && !odd_address(B, f->v),
                "%s: odd address of two-byte samples", who);
  if (int rc = plane_dims(who, w, h, f->pitch_y, B)) return rc;
  return plane_dims(who, (w - 1) / fmt.cx + 1, (h - 1) / fmt.cy + 1, f->pitch_c, B, nch);
}
// the source W x H of a frame-level downscale against the scale (the planes'
// own limits come with their pitches); *w, *h: the small frame
int down_frame_dims(const char* who, uint32_t W, uint32_t H, uint32_t scale, uint32_t* w, uint32_t* h) {
  if (int rc = check_scale(who, scale)) return rc;
  SRCNN_REQUIRE(W >= scale && H >= scale, "%s: frame %ux%u is smaller than the scale %u", who, W, H, scale);
  *w = W / scale;
  *h = H / scale;
  return SRCNN_OK;
}
int downscale_frame(const char* who, const srcnn_yuv_format* fmt, const srcnn_yuv_frame* src,
                    const srcnn_yuv_frame* dst, uint32_t W, uint32_t H, uint32_t scale,
                    srcnn_stream_t stream) {
  uint32_t B, nch, w, h;
  if (int rc = frame_format(who, fmt, &B, &nch)) return rc;
  if (int rc = down_frame_dims(who, W, H, scale, &w, &h)) return rc;
  if (int rc = frame_planes(who, *fmt, src, W, H, B, nch)) return rc;
  if (int rc = frame_planes(who, *fmt, dst, w, h, B, nch)) return rc;
  // (every check of the two calls has been made: the crop rule holds by
  // ceil(floor(W/s)/cx) <= ceil(ceil(W/cx)/s))
  if (int rc = down_planes(who, src->y, nullptr, src->pitch_y, W, H, dst->y, nullptr, dst->pitch_y, w, h, scale,
                           fmt->bits, fmt->msb, SRCNN_YUV_PLANAR, stream))
    return rc;
  return down_planes(who, src->u, src->v, src->pitch_c, (W - 1) / fmt->cx + 1, (H - 1) / fmt->cy + 1, dst->u,
                     dst->v, dst->pitch_c, (w - 1) / fmt->cx + 1, (h - 1) / fmt->cy + 1, scale, fmt->bits,
                     fmt->msb, fmt->layout, stream);
}

// regions of the make_pairs_frame workspace: small Y plane [h][w] at the pitch
// of its row bytes | X plane [Hc][Wc] | T plane [H][W], each 256-byte aligned
struct PairFrameWs {
  uint32_t B, w, h, Wc, Hc;
  size_t small, xplane, tplane, total;
};
int pair_frame_ws(const char* who, const srcnn_yuv_format* fmt, uint32_t W, uint32_t H, uint32_t scale,
                  PairFrameWs* L) {
  uint32_t nch;
  if (int rc = frame_format(who, fmt, &L->B, &nch)) return rc;
  if (int rc = down_frame_dims(who, W, H, scale, &L->w, &L->h)) return rc;
  if (int rc = plane_dims(who, W, H, W * L->B, L->B)) return rc;  // (the frame's pitch comes later)
  UpDims u;
  if (int rc = up_dims(by_scale(who, L->w, L->h, scale), 0, false, &u)) return rc;
  L->Wc = u.W;
  L->Hc = u.H;
  L->small = 0;
  L->xplane = L->small + align_up((size_t)L->w * L->h * L->B);
  L->tplane = L->xplane + align_up((size_t)L->Wc * L->Hc * sizeof(float));
  L->total = L->tplane + align_up((size_t)W * H * sizeof(float));
  return SRCNN_OK;
}

// a frame of w x h luma samples inside a workspace, rows at the pitch of their
// bytes: y | u | v (no v: semi-planar), each 256-byte aligned, from byte `at`
struct WsFrame {
  size_t y, u, v, end;
  uint32_t pitch_y, pitch_c;
};
WsFrame ws_frame(size_t at, const srcnn_yuv_format& fmt, uint32_t w, uint32_t h, uint32_t B, uint32_t nch) {
  const uint32_t cw = (w - 1) / fmt.cx + 1, ch = (h - 1) / fmt.cy + 1;
  WsFrame f;
  f.pitch_y = w * B;
  f.pitch_c = cw * nch * B;
  f.y = at;
  f.u = f.y + align_up((size_t)f.pitch_y * h);
  f.v = f.u + align_up((size_t)f.pitch_c * ch);
  f.end = nch == 2 ? f.v : f.v + align_up((size_t)f.pitch_c * ch);
  return f;
}
srcnn_yuv_frame frame_at(char* p, const WsFrame& f, uint32_t nch) {
  return srcnn_yuv_frame{reinterpret_cast<uint8_t*>(p + f.y), reinterpret_cast<uint8_t*>(p + f.u),
                         nch == 2 ? nullptr : reinterpret_cast<uint8_t*>(p + f.v), f.pitch_y, f.pitch_c};
}
// regions of the evaluate_frame workspace: small frame | output frame | luma
// plane [Hc][Wc] | srcnn_upscale_frame's workspace | srcnn_quality_frame's
struct EvalFrameWs {
  uint32_t B, nch, w, h, Wc, Hc;
  WsFrame small, out;
  size_t plane, up, q, total, up_bytes, q_bytes;
};
// every check of the calls that does not need the buffers; shave < 0: the
// sizes alone (the workspace query: the metric's workspace is sized for shave 0)
int eval_frame_ws(const char* who, const srcnn_net* net, const srcnn_yuv_format* fmt, uint32_t W, uint32_t H,
                  uint32_t scale, int64_t shave, EvalFrameWs* L) {
  SRCNN_REQUIRE(net, "%s: null srcnn_net", who);
  if (int rc = frame_format(who, fmt, &L->B, &L->nch)) return rc;
  if (int rc = down_frame_dims(who, W, H, scale, &L->w, &L->h)) return rc;
  // the truth's planes at the pitch of their bytes (its own pitches come later)
  if (int rc = plane_dims(who, W, H, W * L->B, L->B)) return rc;
  const uint32_t CW = (W - 1) / fmt->cx + 1, CH = (H - 1) / fmt->cy + 1;
  if (int rc = plane_dims(who, CW, CH, CW * L->nch * L->B, L->B, L->nch)) return rc;
  FrameDims f;
  UpWs U;
  if (int rc = frame_dims(by_scale(who, L->w, L->h, scale), net, fmt->cx, fmt->cy, &f)) return rc;
  if (!up_ws(net, f.d, &U)) return SRCNN_ERR_INVALID;  // (message from net_dims)
  L->up_bytes = U.total;
  L->Wc = f.d.W;
  L->Hc = f.d.H;
  FrameQualityDims q;
  if (int rc = quality_frame_dims(who, L->Wc, L->Hc, fmt->cx, fmt->cy, shave < 0 ? 0 : (uint32_t)shave, &q))
    return rc;
  L->q_bytes = srcnn_quality_frame_workspace_bytes(L->Wc, L->Hc, fmt->cx, fmt->cy, 0);
  L->small = ws_frame(0, *fmt, L->w, L->h, L->B, L->nch);
  L->out = ws_frame(L->small.end, *fmt, L->Wc, L->Hc, L->B, L->nch);
  L->plane = L->out.end;
  L->up = L->plane + align_up((size_t)L->Wc * L->Hc * sizeof(float));
  L->q = L->up + align_up(L->up_bytes);
  L->total = L->q + align_up(L->q_bytes);
  return SRCNN_OK;
}

}  // namespace

extern "C" {

// ---------------------------------------------------------------------------
// operator level
// ---------------------------------------------------------------------------
int srcnn_upscale_luma(const uint8_t* rgba, float* luma_padded, uint32_t w, uint32_t h,
                       uint32_t scale, uint32_t pad, srcnn_stream_t stream) {
  return rgba_luma(by_scale("upscale_luma", w, h, scale), rgba, luma_padded, pad, stream);
}

int srcnn_upscale_compose(const uint8_t* rgba, const float* new_luma, uint8_t* rgb, uint32_t w,
                          uint32_t h, uint32_t scale, srcnn_stream_t stream) {
  return rgba_compose(by_scale("upscale_compose", w, h, scale), rgba, new_luma, rgb, stream);
}

int srcnn_resize_luma(const uint8_t* rgba, float* luma_padded, uint32_t w, uint32_t h, uint32_t W,
                      uint32_t H, uint32_t pad, srcnn_stream_t stream) {
  return rgba_luma(to_size("resize_luma", w, h, W, H), rgba, luma_padded, pad, stream);
}

int srcnn_resize_compose(const uint8_t* rgba, const float* new_luma, uint8_t* rgb, uint32_t w,
                         uint32_t h, uint32_t W, uint32_t H, srcnn_stream_t stream) {
  return rgba_compose(to_size("resize_compose", w, h, W, H), rgba, new_luma, rgb, stream);
}

int srcnn_yuv_upscale_luma(const uint8_t* y, uint32_t pitch_y, float* luma_padded, uint32_t w,
                           uint32_t h, uint32_t scale, uint32_t pad, int range,
                           srcnn_stream_t stream) {
  return yuv_luma(by_scale("yuv_upscale_luma", w, h, scale), y, pitch_y, luma_padded, pad, 8, 0, range,
                  stream);
}

int srcnn_yuv_upscale_luma16(const void* y, uint32_t pitch_y, float* luma_padded, uint32_t w,
                             uint32_t h, uint32_t scale, uint32_t pad, uint32_t bits, uint32_t msb,
                             int range, srcnn_stream_t stream) {
  return yuv_luma(by_scale("yuv_upscale_luma16", w, h, scale), y, pitch_y, luma_padded, pad, bits, msb,
                  range, stream);
}

int srcnn_yuv_resize_luma(const void* y, uint32_t pitch_y, float* luma_padded, uint32_t w, uint32_t h,
                          uint32_t W, uint32_t H, uint32_t pad, uint32_t bits, uint32_t msb, int range,
                          srcnn_stream_t stream) {
  return yuv_luma(to_size("yuv_resize_luma", w, h, W, H), y, pitch_y, luma_padded, pad, bits, msb, range,
                  stream);
}

int srcnn_yuv_compose_luma(const float* luma, uint8_t* y, uint32_t pitch_y, uint32_t W, uint32_t H,
                           int range, srcnn_stream_t stream) {
  return yuv_compose_luma("yuv_compose_luma", luma, y, pitch_y, W, H, 8, 0, range, stream);
}

int srcnn_yuv_compose_luma16(const float* luma, void* y, uint32_t pitch_y, uint32_t W, uint32_t H,
                             uint32_t bits, uint32_t msb, int range, srcnn_stream_t stream) {
  return yuv_compose_luma("yuv_compose_luma16", luma, y, pitch_y, W, H, bits, msb, range, stream);
}

int srcnn_upscale_planes_u8(const uint8_t* src0, const uint8_t* src1, uint32_t src_pitch,
                            uint32_t pw, uint32_t ph, uint8_t* dst0, uint8_t* dst1,
                            uint32_t dst_pitch, uint32_t ow, uint32_t oh, uint32_t scale,
                            srcnn_stream_t stream) {
  return chroma_planes("upscale_planes_u8", src0, src1, src_pitch, pw, ph, dst0, dst1, dst_pitch, ow, oh,
                       PlaneMap{true, scale, 0, 0, 0, 0}, 8, 0, SRCNN_YUV_PLANAR, stream);
}

int srcnn_upscale_planes(const void* src0, const void* src1, uint32_t src_pitch, uint32_t pw,
                         uint32_t ph, void* dst0, void* dst1, uint32_t dst_pitch, uint32_t ow,
                         uint32_t oh, uint32_t scale, uint32_t bits, uint32_t msb, uint32_t layout,
                         srcnn_stream_t stream) {
  return chroma_planes("upscale_planes", src0, src1, src_pitch, pw, ph, dst0, dst1, dst_pitch, ow, oh,
                       PlaneMap{true, scale, 0, 0, 0, 0}, bits, msb, layout, stream);
}

int srcnn_resize_planes(const void* src0, const void* src1, uint32_t src_pitch, uint32_t pw,
                        uint32_t ph, void* dst0, void* dst1, uint32_t dst_pitch, uint32_t ow,
                        uint32_t oh, uint32_t rx_num, uint32_t rx_den, uint32_t ry_num,
                        uint32_t ry_den, uint32_t bits, uint32_t msb, uint32_t layout,
                        srcnn_stream_t stream) {
  return chroma_planes("resize_planes", src0, src1, src_pitch, pw, ph, dst0, dst1, dst_pitch, ow, oh,
                       PlaneMap{false, 0, rx_num, rx_den, ry_num, ry_den}, bits, msb, layout, stream);
}

int srcnn_downscale_planes(const void* src0, const void* src1, uint32_t src_pitch, uint32_t pw,
                           uint32_t ph, void* dst0, void* dst1, uint32_t dst_pitch, uint32_t ow,
                           uint32_t oh, uint32_t scale, uint32_t bits, uint32_t msb, uint32_t layout,
                           srcnn_stream_t stream) {
  return down_planes("downscale_planes", src0, src1, src_pitch, pw, ph, dst0, dst1, dst_pitch, ow, oh, scale,
                     bits, msb, layout, stream);
}

int srcnn_downscale_frame(const srcnn_yuv_format* fmt, const srcnn_yuv_frame* src,
                          const srcnn_yuv_frame* dst, uint32_t W, uint32_t H, uint32_t scale,
                          srcnn_stream_t stream) {
  return downscale_frame("downscale_frame", fmt, src, dst, W, H, scale, stream);
}

int srcnn_downscale_rgba(const uint8_t* rgba, uint8_t* small, uint32_t W, uint32_t H,
                         uint32_t scale, srcnn_stream_t stream) {
  if (int rc = down_dims("downscale_rgba", W, H, scale)) return rc;
  SRCNN_REQUIRE(rgba && small, "downscale_rgba: null buffer");
  return srcnn::downscale_rgba(rgba, small, W, H, scale, as_stream(stream));
}

int srcnn_gather_tiles(const float* plane, uint32_t pw, uint32_t ph, uint32_t x0, uint32_t y0,
                       uint32_t stride, uint32_t nx, uint32_t ny, uint32_t tw, uint32_t th,
                       int sub_mean, float* tiles, float* means, srcnn_stream_t stream) {
  if (int rc = gather_dims("gather_tiles", pw, ph, x0, y0, stride, nx, ny, tw, th)) return rc;
  SRCNN_REQUIRE(plane && tiles, "gather_tiles: null buffer");
  return srcnn::gather_tiles(plane, pw, x0, y0, stride, nx, ny, tw, th, sub_mean, tiles, means,
                             as_stream(stream));
}

int srcnn_gather_batch(const srcnn_plane_pair* planes, uint32_t n_planes,
                       const srcnn_tile_ref* refs, uint32_t n, uint32_t tw, uint32_t th, float* X,
                       float* T, float* means, srcnn_stream_t stream) {
  SRCNN_REQUIRE(planes && refs && X && T, "gather_batch: null buffer");
  SRCNN_REQUIRE(n_planes > 0 && tw > 0 && th > 0, "gather_batch: n_planes(%u) and tile %ux%u must be > 0",
                n_planes, tw, th);
  SRCNN_REQUIRE((uint64_t)tw * th <= kIndexMax,
                "gather_batch: tile %ux%u exceeds the kernel's 32-bit index: its floats must number at "
                "most 2^31-1",
                tw, th);
  if (n == 0) return SRCNN_OK;
  return srcnn::gather_batch(planes, n_planes, refs, n, tw, th, X, T, means, as_stream(stream));
}

size_t srcnn_make_pairs_count(uint32_t W, uint32_t H, uint32_t scale, uint32_t tile,
                              uint32_t stride, uint32_t* nx, uint32_t* ny) {
  if (nx) *nx = 0;
  if (ny) *ny = 0;
  if (scale < 1 || scale > 4 || W < scale || H < scale || tile == 0 || stride == 0) return 0;
  const uint32_t Wc = W / scale * scale, Hc = H / scale * scale;
  if (tile > Wc || tile > Hc) return 0;
  const uint32_t gx = (Wc - tile) / stride + 1, gy = (Hc - tile) / stride + 1;
  if ((uint64_t)gx * gy > kIndexMax) return 0;
  if (nx) *nx = gx;
  if (ny) *ny = gy;
  return (size_t)gx * gy;
}

size_t srcnn_make_pairs_workspace_bytes(uint32_t W, uint32_t H, uint32_t scale) {
  PairWs L;
  return pair_ws("make_pairs", W, H, scale, &L) ? 0 : L.total;
}

int srcnn_make_pairs(const uint8_t* rgba, uint32_t W, uint32_t H, uint32_t scale, uint32_t tile,
                     uint32_t stride, float* X, float* T, void* ws, size_t ws_bytes,
                     srcnn_stream_t stream) {
  PairWs L;
  if (int rc = pair_ws("make_pairs", W, H, scale, &L)) return rc;
  SRCNN_REQUIRE(tile > 0 && stride > 0, "make_pairs: tile(%u) and stride(%u) must be > 0", tile,
                stride);
  uint32_t nx, ny;
  SRCNN_REQUIRE(srcnn_make_pairs_count(W, H, scale, tile, stride, &nx, &ny) > 0,
                "make_pairs: image %ux%u at scale %u holds no %ux%u tile (or more than 2^31-1)", W,
                H, scale, tile, tile);
  // (the two gathers' own checks, before the first launch)
  if (int rc = gather_dims("make_pairs", L.Wc, L.Hc, 0, 0, stride, nx, ny, tile, tile)) return rc;
  if (int rc = gather_dims("make_pairs", W, H, 0, 0, stride, nx, ny, tile, tile)) return rc;
  SRCNN_REQUIRE(rgba && X && T && ws, "make_pairs: null buffer");
  if (ws_bytes < L.total)
    return fail(SRCNN_ERR_WORKSPACE, "make_pairs: workspace %zu B < %zu B", ws_bytes, L.total);
  char* p = static_cast<char*>(ws);
  uint8_t* small = reinterpret_cast<uint8_t*>(p + L.small);
  float* xplane = reinterpret_cast<float*>(p + L.xplane);
  float* tplane = reinterpret_cast<float*>(p + L.tplane);
  int rc;
  if ((rc = srcnn_downscale_rgba(rgba, small, W, H, scale, stream))) return rc;
  if ((rc = srcnn_upscale_luma(small, xplane, L.w, L.h, scale, 0, stream))) return rc;
  if ((rc = srcnn_extract_luma(rgba, tplane, W, H, 1, stream))) return rc;
  if ((rc = srcnn_gather_tiles(xplane, L.Wc, L.Hc, 0, 0, stride, nx, ny, tile, tile, 1, X, nullptr,
                               stream)))
    return rc;
  return srcnn_gather_tiles(tplane, W, H, 0, 0, stride, nx, ny, tile, tile, 0, T, nullptr, stream);
}

size_t srcnn_make_pairs_frame_workspace_bytes(const srcnn_yuv_format* fmt, uint32_t W, uint32_t H,
                                              uint32_t scale) {
  PairFrameWs L;
  return pair_frame_ws("make_pairs_frame", fmt, W, H, scale, &L) ? 0 : L.total;
}

int srcnn_make_pairs_frame(const srcnn_yuv_format* fmt, const srcnn_yuv_frame* frame, uint32_t W,
                           uint32_t H, uint32_t scale, uint32_t tile, uint32_t stride, float* X,
                           float* T, void* ws, size_t ws_bytes, srcnn_stream_t stream) {
  const char* who = "make_pairs_frame";
  PairFrameWs L;
  if (int rc = pair_frame_ws(who, fmt, W, H, scale, &L)) return rc;
  SRCNN_REQUIRE(tile > 0 && stride > 0, "%s: tile(%u) and stride(%u) must be > 0", who, tile, stride);
  uint32_t nx, ny;
  SRCNN_REQUIRE(srcnn_make_pairs_count(W, H, scale, tile, stride, &nx, &ny) > 0,
                "%s: frame %ux%u at scale %u holds no %ux%u tile (or more than 2^31-1)", who, W, H, scale,
                tile, tile);
  if (int rc = gather_dims(who, L.Wc, L.Hc, 0, 0, stride, nx, ny, tile, tile)) return rc;
  if (int rc = gather_dims(who, W, H, 0, 0, stride, nx, ny, tile, tile)) return rc;
  SRCNN_REQUIRE(frame && X && T && ws, "%s: null buffer", who);
  SRCNN_REQUIRE(frame->y, "%s: null plane", who);
  SRCNN_REQUIRE(!odd_address(L.B, frame->y) && !odd_address(L.B, ws), "%s: odd address of two-byte samples",
                who);
  if (int rc = plane_dims(who, W, H, frame->pitch_y, L.B)) return rc;
  if (ws_bytes < L.total) return fail(SRCNN_ERR_WORKSPACE, "%s: workspace %zu B < %zu B", who, ws_bytes, L.total);
  char* p = static_cast<char*>(ws);
  uint8_t* small = reinterpret_cast<uint8_t*>(p + L.small);
  float* xplane = reinterpret_cast<float*>(p + L.xplane);
  float* tplane = reinterpret_cast<float*>(p + L.tplane);
  int rc;
  if ((rc = srcnn_downscale_planes(frame->y, nullptr, frame->pitch_y, W, H, small, nullptr, L.w * L.B, L.w, L.h,
                                   scale, fmt->bits, fmt->msb, SRCNN_YUV_PLANAR, stream)))
    return rc;
  if ((rc = srcnn_yuv_upscale_luma16(small, L.w * L.B, xplane, L.w, L.h, scale, 0, fmt->bits, fmt->msb,
                                     fmt->range, stream)))
    return rc;
  if ((rc = srcnn_yuv_upscale_luma16(frame->y, frame->pitch_y, tplane, W, H, 1, 0, fmt->bits, fmt->msb,
                                     fmt->range, stream)))
    return rc;
  if ((rc = srcnn_gather_tiles(xplane, L.Wc, L.Hc, 0, 0, stride, nx, ny, tile, tile, 1, X, nullptr, stream)))
    return rc;
  return srcnn_gather_tiles(tplane, W, H, 0, 0, stride, nx, ny, tile, tile, 0, T, nullptr, stream);
}

size_t srcnn_quality_workspace_bytes(uint32_t W, uint32_t H, uint32_t shave) {
  QualityDims d;
  return quality_dims("quality", W, H, shave, &d) ? 0 : align_up(d.partial_bytes);
}

int srcnn_quality(const void* a, int fmt_a, uint32_t pitch_a, const void* b, int fmt_b,
                  uint32_t pitch_b, uint32_t W, uint32_t H, uint32_t shave, double* result,
                  void* ws, size_t ws_bytes, srcnn_stream_t stream) {
  QualityDims d;
  if (int rc = quality_dims("quality", W, H, shave, &d)) return rc;
  if (int rc = quality_image("a", a, fmt_a, pitch_a, W, H)) return rc;
  if (int rc = quality_image("b", b, fmt_b, pitch_b, W, H)) return rc;
  SRCNN_REQUIRE(result && ws, "quality: null buffer");
  SRCNN_REQUIRE((((uintptr_t)result | (uintptr_t)ws) & 7) == 0,
                "quality: result and workspace hold doubles and must be 8-byte aligned");
  if (ws_bytes < align_up(d.partial_bytes))
    return fail(SRCNN_ERR_WORKSPACE, "quality: workspace %zu B < %zu B", ws_bytes,
                align_up(d.partial_bytes));
  // the shaved window is a pointer offset: the kernels see Ws x Hs alone
  const char* pa = static_cast<const char*>(a) + ((size_t)shave * pitch_a + shave) * pixel_bytes(fmt_a);
  const char* pb = static_cast<const char*>(b) + ((size_t)shave * pitch_b + shave) * pixel_bytes(fmt_b);
  return srcnn::quality(pa, fmt_a, pitch_a, pb, fmt_b, pitch_b, d.Ws, d.Hs, result,
                        static_cast<double*>(ws), as_stream(stream));
}

size_t srcnn_quality_frame_workspace_bytes(uint32_t w, uint32_t h, uint32_t cx, uint32_t cy,
                                           uint32_t shave) {
  FrameQualityDims d;
  return quality_frame_dims("quality_frame", w, h, cx, cy, shave, &d) ? 0 : d.ws_bytes;
}

int srcnn_quality_frame(const srcnn_yuv_format* fmt_a, const srcnn_yuv_frame* a,
                        const srcnn_yuv_format* fmt_b, const srcnn_yuv_frame* b, uint32_t w, uint32_t h,
                        uint32_t shave, double* result, void* ws, size_t ws_bytes,
                        srcnn_stream_t stream) {
  const char* who = "quality_frame";
  SRCNN_REQUIRE(fmt_a && fmt_b, "%s: null srcnn_yuv_format", who);
  SRCNN_REQUIRE(a && b && result && ws, "%s: null buffer", who);
  FrameQualityDims d;
  if (int rc = quality_frame_dims(who, w, h, fmt_a->cx, fmt_a->cy, shave, &d)) return rc;
  SRCNN_REQUIRE(fmt_a->bits == fmt_b->bits && fmt_a->cx == fmt_b->cx && fmt_a->cy == fmt_b->cy &&
                    fmt_a->range == fmt_b->range,
                "%s: the formats differ in bits (%u / %u), subsampling (%ux%u / %ux%u) or range (%d / %d)",
                who, fmt_a->bits, fmt_b->bits, fmt_a->cx, fmt_a->cy, fmt_b->cx, fmt_b->cy, fmt_a->range,
                fmt_b->range);
  srcnn::QualityFrameSide sa, sb;
  if (int rc = quality_frame_side(who, fmt_a, a, w, h, d, shave, &sa)) return rc;
  if (int rc = quality_frame_side(who, fmt_b, b, w, h, d, shave, &sb)) return rc;
  SRCNN_REQUIRE((((uintptr_t)result | (uintptr_t)ws) & 7) == 0,
                "%s: result and workspace hold 8-byte words and must be 8-byte aligned", who);
  if (ws_bytes < d.ws_bytes)
    return fail(SRCNN_ERR_WORKSPACE, "%s: workspace %zu B < %zu B", who, ws_bytes, d.ws_bytes);
  return srcnn::quality_frame(sa, sb, fmt_a->bits, d.Ws, d.Hs, d.CWs, d.CHs, result, ws, as_stream(stream));
}

// ---------------------------------------------------------------------------
// network level
// ---------------------------------------------------------------------------
size_t srcnn_upscale_workspace_bytes(const srcnn_net* net, uint32_t w, uint32_t h,
                                     uint32_t scale) {
  // Not image_workspace_bytes alone: of the five queries only this one leaves
  // srcnn_net_offsets' message for a null net and none for a padding too
  // large (srcnn_evaluate then fails with the message before it).  Kept.
  size_t off[6];
  if (srcnn_net_offsets(net, off) || padding(net) > kIndexMax) return 0;
  return image_workspace_bytes(by_scale("upscale", w, h, scale), net);
}

int srcnn_upscale(const srcnn_net* net, const uint8_t* rgba, uint32_t w, uint32_t h,
                  uint32_t scale, const float* params, uint8_t* rgb, void* ws, size_t ws_bytes,
                  srcnn_stream_t stream) {
  return upscale_image(by_scale("upscale", w, h, scale), net, rgba, params, rgb, ws, ws_bytes, stream);
}

size_t srcnn_upscale_to_workspace_bytes(const srcnn_net* net, uint32_t w, uint32_t h, uint32_t W,
                                        uint32_t H) {
  return image_workspace_bytes(to_size("upscale_to", w, h, W, H), net);
}

int srcnn_upscale_to(const srcnn_net* net, const uint8_t* rgba, uint32_t w, uint32_t h, uint32_t W,
                     uint32_t H, const float* params, uint8_t* rgb, void* ws, size_t ws_bytes,
                     srcnn_stream_t stream) {
  return upscale_image(to_size("upscale_to", w, h, W, H), net, rgba, params, rgb, ws, ws_bytes, stream);
}

size_t srcnn_upscale_yuv_workspace_bytes(const srcnn_net* net, uint32_t w, uint32_t h,
                                         uint32_t scale) {
  return frame_workspace_bytes(by_scale("upscale_yuv", w, h, scale), net);
}

int srcnn_upscale_yuv(const srcnn_net* net, const srcnn_yuv_frame* src, const srcnn_yuv_frame* dst,
                      uint32_t w, uint32_t h, uint32_t cx, uint32_t cy, uint32_t scale, int range,
                      const float* params, void* ws, size_t ws_bytes, srcnn_stream_t stream) {
  const srcnn_yuv_format fmt{8, 0, SRCNN_YUV_PLANAR, cx, cy, range};
  return upscale_frame(by_scale("upscale_yuv", w, h, scale), net, fmt, src, dst, params, ws, ws_bytes,
                       stream);
}

int srcnn_upscale_frame(const srcnn_net* net, const srcnn_yuv_format* fmt,
                        const srcnn_yuv_frame* src, const srcnn_yuv_frame* dst, uint32_t w,
                        uint32_t h, uint32_t scale, const float* params, void* ws, size_t ws_bytes,
                        srcnn_stream_t stream) {
  SRCNN_REQUIRE(fmt, "upscale_frame: null srcnn_yuv_format");
  return upscale_frame(by_scale("upscale_frame", w, h, scale), net, *fmt, src, dst, params, ws, ws_bytes,
                       stream);
}

size_t srcnn_upscale_frame_to_workspace_bytes(const srcnn_net* net, uint32_t w, uint32_t h,
                                              uint32_t W, uint32_t H) {
  return frame_workspace_bytes(to_size("upscale_frame_to", w, h, W, H), net);
}

int srcnn_upscale_frame_to(const srcnn_net* net, const srcnn_yuv_format* fmt,
                           const srcnn_yuv_frame* src, const srcnn_yuv_frame* dst, uint32_t w,
                           uint32_t h, uint32_t W, uint32_t H, const float* params, void* ws,
                           size_t ws_bytes, srcnn_stream_t stream) {
  SRCNN_REQUIRE(fmt, "upscale_frame_to: null srcnn_yuv_format");
  return upscale_frame(to_size("upscale_frame_to", w, h, W, H), net, *fmt, src, dst, params, ws, ws_bytes,
                       stream);
}

size_t srcnn_evaluate_workspace_bytes(const srcnn_net* net, uint32_t W, uint32_t H,
                                      uint32_t scale) {
  EvalWs L;
  return eval_ws(net, W, H, scale, -1, &L) ? 0 : L.total;
}

int srcnn_evaluate(const srcnn_net* net, const uint8_t* rgba, uint32_t W, uint32_t H,
                   uint32_t scale, uint32_t shave, const float* params, double* result, void* ws,
                   size_t ws_bytes, srcnn_stream_t stream) {
  EvalWs L;
  if (int rc = eval_ws(net, W, H, scale, shave, &L)) return rc;
  SRCNN_REQUIRE(rgba && params && result && ws, "evaluate: null buffer");
  SRCNN_REQUIRE((((uintptr_t)rgba & 3) | (((uintptr_t)result | (uintptr_t)ws) & 7)) == 0,
                "evaluate: rgba must be 4-byte, result and workspace 8-byte aligned");
  if (ws_bytes < L.total)
    return fail(SRCNN_ERR_WORKSPACE, "evaluate: workspace %zu B < %zu B", ws_bytes, L.total);
  char* p = static_cast<char*>(ws);
  uint8_t* small = reinterpret_cast<uint8_t*>(p + L.small);
  uint8_t* rgb = reinterpret_cast<uint8_t*>(p + L.rgb);
  float* plane = reinterpret_cast<float*>(p + L.plane);
  int rc;
  if ((rc = srcnn_downscale_rgba(rgba, small, W, H, scale, stream))) return rc;
  // the net's result against the truth's top-left Wc x Hc pixels (pitch W)
  if ((rc = srcnn_upscale(net, small, L.w, L.h, scale, params, rgb, p + L.up, L.up_bytes, stream)))
    return rc;
  if ((rc = srcnn_quality(rgb, SRCNN_PIX_RGB8, L.Wc, rgba, SRCNN_PIX_RGBA8, W, L.Wc, L.Hc, shave,
                          result, p + L.q, L.q_bytes, stream)))
    return rc;
  // plain bicubic: the same resampling without the net
  if ((rc = srcnn_upscale_luma(small, plane, L.w, L.h, scale, 0, stream))) return rc;
  if ((rc = srcnn_upscale_compose(small, plane, rgb, L.w, L.h, scale, stream))) return rc;
  return srcnn_quality(rgb, SRCNN_PIX_RGB8, L.Wc, rgba, SRCNN_PIX_RGBA8, W, L.Wc, L.Hc, shave,
                       result + 3, p + L.q, L.q_bytes, stream);
}

size_t srcnn_evaluate_frame_workspace_bytes(const srcnn_net* net, const srcnn_yuv_format* fmt,
                                            uint32_t W, uint32_t H, uint32_t scale) {
  EvalFrameWs L;
  return eval_frame_ws("evaluate_frame", net, fmt, W, H, scale, -1, &L) ? 0 : L.total;
}

int srcnn_evaluate_frame(const srcnn_net* net, const srcnn_yuv_format* fmt,
                         const srcnn_yuv_frame* truth, uint32_t W, uint32_t H, uint32_t scale,
                         uint32_t shave, const float* params, double* result, void* ws,
                         size_t ws_bytes, srcnn_stream_t stream) {
  const char* who = "evaluate_frame";
  EvalFrameWs L;
  if (int rc = eval_frame_ws(who, net, fmt, W, H, scale, shave, &L)) return rc;
  SRCNN_REQUIRE(truth && params && result && ws, "%s: null buffer", who);
  if (int rc = frame_planes(who, *fmt, truth, W, H, L.B, L.nch)) return rc;
  SRCNN_REQUIRE((((uintptr_t)result | (uintptr_t)ws) & 7) == 0,
                "%s: result and workspace must be 8-byte aligned", who);
  if (ws_bytes < L.total) return fail(SRCNN_ERR_WORKSPACE, "%s: workspace %zu B < %zu B", who, ws_bytes, L.total);
  char* p = static_cast<char*>(ws);
  const srcnn_yuv_frame small = frame_at(p, L.small, L.nch), out = frame_at(p, L.out, L.nch);
  float* plane = reinterpret_cast<float*>(p + L.plane);
  int rc;
  if ((rc = srcnn_downscale_frame(fmt, truth, &small, W, H, scale, stream))) return rc;
  if ((rc = srcnn_upscale_frame(net, fmt, &small, &out, L.w, L.h, scale, params, p + L.up, L.up_bytes, stream)))
    return rc;
  // the net's result against the truth's top-left Wc x Hc samples (its own pitches)
  if ((rc = srcnn_quality_frame(fmt, &out, fmt, truth, L.Wc, L.Hc, shave, result, p + L.q, L.q_bytes, stream)))
    return rc;
  // plain bicubic: the same resampling without the net; the chroma planes stay
  if ((rc = srcnn_yuv_upscale_luma16(small.y, small.pitch_y, plane, L.w, L.h, scale, 0, fmt->bits, fmt->msb,
                                     fmt->range, stream)))
    return rc;
  if ((rc = srcnn_yuv_compose_luma16(plane, out.y, out.pitch_y, L.Wc, L.Hc, fmt->bits, fmt->msb, fmt->range,
                                     stream)))
    return rc;
  return srcnn_quality_frame(fmt, &out, fmt, truth, L.Wc, L.Hc, shave, result + 8, p + L.q, L.q_bytes, stream);
}

}  // extern "C"
