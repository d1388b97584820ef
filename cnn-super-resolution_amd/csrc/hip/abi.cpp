// abi.cpp -- extern "C" operator + network entry points of srcnn.h.
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

size_t align_up(size_t v) { return (v + 255) & ~size_t(255); }

// srcnn_upscale_*: the sizes of one upscale, checked against what the kernels
// of upscale.hip can index (int coordinates and element offsets below 2^31)
struct UpDims {
  uint32_t W, H, PW, PH;  // output image, padded plane
};
int up_dims(const char* who, uint32_t w, uint32_t h, uint32_t scale, uint32_t pad, UpDims* d) {
  SRCNN_REQUIRE(scale >= 1 && scale <= 4, "%s: scale %u is not 1, 2, 3 or 4", who, scale);
  SRCNN_REQUIRE(w > 0 && h > 0, "%s: empty image %ux%u", who, w, h);
  const uint64_t lim = 0x7fffffffull;  // INT32_MAX
  const uint64_t W = (uint64_t)w * scale, H = (uint64_t)h * scale;
  SRCNN_REQUIRE(W + pad <= lim && H + pad <= lim && (W + pad) * (H + pad) <= lim &&
                    3 * W * H <= lim,
                "%s: %ux%u x%u with padding %u exceeds the kernels' 32-bit index: the padded plane's "
                "floats and the rgb bytes must each number at most 2^31-1",
                who, w, h, scale, pad);
  d->W = (uint32_t)W;
  d->H = (uint32_t)H;
  d->PW = (uint32_t)(W + pad);
  d->PH = (uint32_t)(H + pad);
  return SRCNN_OK;
}

// srcnn_yuv_* / srcnn_upscale_planes_u8: the sizes of one byte plane and of
// its resampled counterpart against what the kernels of yuv.hip can index (int
// coordinates, at most 2^31-1 elements in a plane; row offsets are size_t).
// A pixel is nch samples of B bytes: the pitch is in bytes, and
// even for two-byte samples.
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
  SRCNN_REQUIRE((uint64_t)w * h * nch <= 0x7fffffffull,
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
int yuv_luma_dims(const char* who, uint32_t w, uint32_t h, uint32_t pitch, uint32_t scale,
                  uint32_t pad, UpDims* d, uint32_t B = 1) {
  SRCNN_REQUIRE(scale >= 1 && scale <= 4, "%s: scale %u is not 1, 2, 3 or 4", who, scale);
  if (int rc = plane_dims(who, w, h, pitch, B)) return rc;
  const uint64_t lim = 0x7fffffffull;
  const uint64_t W = (uint64_t)w * scale, H = (uint64_t)h * scale;
  SRCNN_REQUIRE(W + pad <= lim && H + pad <= lim && (W + pad) * (H + pad) <= lim,
                "%s: %ux%u x%u with padding %u exceeds the kernels' 32-bit index: the padded "
                "plane's floats must number at most 2^31-1",
                who, w, h, scale, pad);
  d->W = (uint32_t)W;
  d->H = (uint32_t)H;
  d->PW = (uint32_t)(W + pad);
  d->PH = (uint32_t)(H + pad);
  return SRCNN_OK;
}
int planes_dims(const char* who, uint32_t src_pitch, uint32_t pw, uint32_t ph, uint32_t dst_pitch,
                uint32_t ow, uint32_t oh, uint32_t scale, uint32_t B = 1, uint32_t nch = 1) {
  SRCNN_REQUIRE(scale >= 1 && scale <= 4, "%s: scale %u is not 1, 2, 3 or 4", who, scale);
  if (int rc = plane_dims(who, pw, ph, src_pitch, B, nch)) return rc;
  if (int rc = plane_dims(who, ow, oh, dst_pitch, B, nch)) return rc;
  const uint64_t s = scale;
  SRCNN_REQUIRE(s * (pw - 1) < ow && ow <= s * pw && s * (ph - 1) < oh && oh <= s * ph,
                "%s: output %ux%u is not a crop of the x%u of %ux%u that keeps its last tile", who,
                ow, oh, scale, pw, ph);
  return SRCNN_OK;
}

// The three Y'CbCr operations, each behind its 8-bit entry point (bits 8,
// msb 0, planar) and its general one; `who` is the one the caller used.
int yuv_upscale_luma(const char* who, const void* y, uint32_t pitch_y, float* luma_padded,
                     uint32_t w, uint32_t h, uint32_t scale, uint32_t pad, uint32_t bits,
                     uint32_t msb, int range, srcnn_stream_t stream) {
  UpDims d;
  uint32_t B;
  if (int rc = yuv_samples(who, bits, msb, &B)) return rc;
  if (int rc = yuv_luma_dims(who, w, h, pitch_y, scale, pad, &d, B)) return rc;
  if (int rc = yuv_range(who, range)) return rc;
  SRCNN_REQUIRE(y && luma_padded, "%s: null buffer", who);
  SRCNN_REQUIRE(!odd_address(B, y), "%s: odd address of two-byte samples", who);
  return srcnn::yuv_upscale_luma(y, pitch_y, luma_padded, w, h, scale, pad, bits, msb != 0,
                                 range == SRCNN_YUV_FULL, as_stream(stream));
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
int yuv_layout(const char* who, uint32_t layout) {
  SRCNN_REQUIRE(layout == SRCNN_YUV_PLANAR || layout == SRCNN_YUV_SEMIPLANAR,
                "%s: layout %u is neither SRCNN_YUV_PLANAR nor SRCNN_YUV_SEMIPLANAR", who, layout);
  return SRCNN_OK;
}
int upscale_planes(const char* who, const void* src0, const void* src1, uint32_t src_pitch,
                   uint32_t pw, uint32_t ph, void* dst0, void* dst1, uint32_t dst_pitch,
                   uint32_t ow, uint32_t oh, uint32_t scale, uint32_t bits, uint32_t msb,
                   uint32_t layout, srcnn_stream_t stream) {
  uint32_t B;
  if (int rc = yuv_samples(who, bits, msb, &B)) return rc;
  if (int rc = yuv_layout(who, layout)) return rc;
  const bool semi = layout == SRCNN_YUV_SEMIPLANAR;
  if (int rc = planes_dims(who, src_pitch, pw, ph, dst_pitch, ow, oh, scale, B, semi ? 2 : 1))
    return rc;
  SRCNN_REQUIRE(src0 && dst0, "%s: null buffer", who);
  if (semi) {
    SRCNN_REQUIRE(!src1 && !dst1, "%s: a semi-planar frame has no second chroma plane", who);
  } else {
    SRCNN_REQUIRE(src1 && dst1, "%s: null buffer", who);
  }
  SRCNN_REQUIRE(!odd_address(B, src0) && !odd_address(B, src1) && !odd_address(B, dst0) &&
                    !odd_address(B, dst1),
                "%s: odd address of two-byte samples", who);
  return srcnn::upscale_planes(src0, src1, src_pitch, pw, ph, dst0, dst1, dst_pitch, ow, oh, scale,
                               bits, msb != 0, semi, as_stream(stream));
}

// srcnn_resize_* (DESIGN.md 16): the output size W x H of one resampling, each
// axis within [1x, 4x] of the source, against what the kernels of resize.hip
// can index (as up_dims; rgb: the call writes an rgb image)
int resize_dims(const char* who, uint32_t w, uint32_t h, uint32_t W, uint32_t H, uint32_t pad,
                bool rgb, UpDims* d) {
  SRCNN_REQUIRE(w > 0 && h > 0 && W > 0 && H > 0, "%s: empty image: %ux%u -> %ux%u", who, w, h, W, H);
  SRCNN_REQUIRE(W >= w && W <= 4ull * w && H >= h && H <= 4ull * h,
                "%s: output %ux%u is outside 1x .. 4x of the source %ux%u on an axis (upscaling only, "
                "by at most 4)",
                who, W, H, w, h);
  const uint64_t lim = 0x7fffffffull, PW = (uint64_t)W + pad, PH = (uint64_t)H + pad;
  SRCNN_REQUIRE(PW <= lim && PH <= lim && PW * PH <= lim && (!rgb || 3ull * W * H <= lim),
                "%s: %ux%u -> %ux%u with padding %u exceeds the kernels' 32-bit index: the padded "
                "plane's floats and the rgb bytes must each number at most 2^31-1",
                who, w, h, W, H, pad);
  d->W = W;
  d->H = H;
  d->PW = (uint32_t)PW;
  d->PH = (uint32_t)PH;
  return SRCNN_OK;
}
// one axis of srcnn_resize_planes: the source step rn / rd per output sample,
// n source samples, N outputs
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

// The Y'CbCr operations at any output size, each behind its op-level entry
// point and srcnn_upscale_frame_to (`who`)
int yuv_resize_luma(const char* who, const void* y, uint32_t pitch_y, float* luma_padded, uint32_t w,
                    uint32_t h, uint32_t W, uint32_t H, uint32_t pad, uint32_t bits, uint32_t msb,
                    int range, srcnn_stream_t stream) {
  UpDims d;
  uint32_t B;
  if (int rc = yuv_samples(who, bits, msb, &B)) return rc;
  if (int rc = resize_dims(who, w, h, W, H, pad, false, &d)) return rc;
  if (int rc = plane_dims(who, w, h, pitch_y, B)) return rc;
  if (int rc = yuv_range(who, range)) return rc;
  SRCNN_REQUIRE(y && luma_padded, "%s: null buffer", who);
  SRCNN_REQUIRE(!odd_address(B, y), "%s: odd address of two-byte samples", who);
  return srcnn::yuv_resize_luma(y, pitch_y, luma_padded, w, h, W, H, pad, bits, msb != 0,
                                range == SRCNN_YUV_FULL, as_stream(stream));
}
int resize_planes(const char* who, const void* src0, const void* src1, uint32_t src_pitch, uint32_t pw,
                  uint32_t ph, void* dst0, void* dst1, uint32_t dst_pitch, uint32_t ow, uint32_t oh,
                  uint32_t rx_num, uint32_t rx_den, uint32_t ry_num, uint32_t ry_den, uint32_t bits,
                  uint32_t msb, uint32_t layout, srcnn_stream_t stream) {
  uint32_t B;
  if (int rc = yuv_samples(who, bits, msb, &B)) return rc;
  if (int rc = yuv_layout(who, layout)) return rc;
  const bool semi = layout == SRCNN_YUV_SEMIPLANAR;
  if (int rc = plane_dims(who, pw, ph, src_pitch, B, semi ? 2 : 1)) return rc;
  if (int rc = plane_dims(who, ow, oh, dst_pitch, B, semi ? 2 : 1)) return rc;
  if (int rc = resize_axis(who, "horizontal", rx_num, rx_den, pw, ow)) return rc;
  if (int rc = resize_axis(who, "vertical", ry_num, ry_den, ph, oh)) return rc;
  SRCNN_REQUIRE(src0 && dst0, "%s: null buffer", who);
  if (semi) {
    SRCNN_REQUIRE(!src1 && !dst1, "%s: a semi-planar frame has no second chroma plane", who);
  } else {
    SRCNN_REQUIRE(src1 && dst1, "%s: null buffer", who);
  }
  SRCNN_REQUIRE(!odd_address(B, src0) && !odd_address(B, src1) && !odd_address(B, dst0) &&
                    !odd_address(B, dst1),
                "%s: odd address of two-byte samples", who);
  return srcnn::resize_planes(src0, src1, src_pitch, pw, ph, dst0, dst1, dst_pitch, ow, oh, rx_num,
                              rx_den, ry_num, ry_den, bits, msb != 0, semi, as_stream(stream));
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
// What srcnn_upscale, srcnn_upscale_yuv and srcnn_upscale_frame (`who`) do
// between their checks and their composition: the workspace carved and
// measured, fill_plane(plane) for the padded bicubic luma, then the plane
// minus its mean through the net.  *luma: the net's output [H][W], in ws.
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

// srcnn_downscale_rgba / srcnn_make_pairs: the source against the scale and
// against what downscale_rgba_kernel can index (pixel offsets below 2^31)
int down_dims(const char* who, uint32_t W, uint32_t H, uint32_t scale) {
  SRCNN_REQUIRE(scale >= 1 && scale <= 4, "%s: scale %u is not 1, 2, 3 or 4", who, scale);
  SRCNN_REQUIRE(W >= scale && H >= scale, "%s: image %ux%u is smaller than the scale %u", who, W, H,
                scale);
  SRCNN_REQUIRE((uint64_t)W * H <= 0x7fffffffull,
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
  SRCNN_REQUIRE((uint64_t)pw * ph <= 0x7fffffffull && (uint64_t)nx * ny <= 0x7fffffffull,
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
  if (int rc = up_dims(who, L->w, L->h, scale, 0, &u)) return rc;
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
  SRCNN_REQUIRE((uint64_t)W * H <= 0x7fffffffull,
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
  SRCNN_REQUIRE((uint64_t)pitch * H <= 0x7fffffffull,
                "quality: image %s, pitch %u x %u rows, exceeds the kernels' 32-bit index: the "
                "pixels must number at most 2^31-1",
                who, pitch, H);
  return SRCNN_OK;
}
size_t pixel_bytes(int fmt) { return fmt == SRCNN_PIX_RGB8 ? 3 : 4; }

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

int srcnn_upscale_luma(const uint8_t* rgba, float* luma_padded, uint32_t w, uint32_t h,
                       uint32_t scale, uint32_t pad, srcnn_stream_t stream) {
  UpDims d;
  if (int rc = up_dims("upscale_luma", w, h, scale, pad, &d)) return rc;
  SRCNN_REQUIRE(rgba && luma_padded, "upscale_luma: null buffer");
  return srcnn::upscale_luma(rgba, luma_padded, w, h, scale, pad, as_stream(stream));
}

int srcnn_upscale_compose(const uint8_t* rgba, const float* new_luma, uint8_t* rgb, uint32_t w,
                          uint32_t h, uint32_t scale, srcnn_stream_t stream) {
  UpDims d;
  if (int rc = up_dims("upscale_compose", w, h, scale, 0, &d)) return rc;
  SRCNN_REQUIRE(rgba && new_luma && rgb, "upscale_compose: null buffer");
  return srcnn::upscale_compose(rgba, new_luma, rgb, w, h, scale, as_stream(stream));
}

int srcnn_resize_luma(const uint8_t* rgba, float* luma_padded, uint32_t w, uint32_t h, uint32_t W,
                      uint32_t H, uint32_t pad, srcnn_stream_t stream) {
  UpDims d;
  if (int rc = resize_dims("resize_luma", w, h, W, H, pad, true, &d)) return rc;
  SRCNN_REQUIRE(rgba && luma_padded, "resize_luma: null buffer");
  return srcnn::resize_luma(rgba, luma_padded, w, h, W, H, pad, as_stream(stream));
}

int srcnn_resize_compose(const uint8_t* rgba, const float* new_luma, uint8_t* rgb, uint32_t w,
                         uint32_t h, uint32_t W, uint32_t H, srcnn_stream_t stream) {
  UpDims d;
  if (int rc = resize_dims("resize_compose", w, h, W, H, 0, true, &d)) return rc;
  SRCNN_REQUIRE(rgba && new_luma && rgb, "resize_compose: null buffer");
  return srcnn::resize_compose(rgba, new_luma, rgb, w, h, W, H, as_stream(stream));
}

int srcnn_yuv_resize_luma(const void* y, uint32_t pitch_y, float* luma_padded, uint32_t w, uint32_t h,
                          uint32_t W, uint32_t H, uint32_t pad, uint32_t bits, uint32_t msb, int range,
                          srcnn_stream_t stream) {
  return yuv_resize_luma("yuv_resize_luma", y, pitch_y, luma_padded, w, h, W, H, pad, bits, msb, range,
                         stream);
}

int srcnn_resize_planes(const void* src0, const void* src1, uint32_t src_pitch, uint32_t pw,
                        uint32_t ph, void* dst0, void* dst1, uint32_t dst_pitch, uint32_t ow,
                        uint32_t oh, uint32_t rx_num, uint32_t rx_den, uint32_t ry_num,
                        uint32_t ry_den, uint32_t bits, uint32_t msb, uint32_t layout,
                        srcnn_stream_t stream) {
  return resize_planes("resize_planes", src0, src1, src_pitch, pw, ph, dst0, dst1, dst_pitch, ow, oh,
                       rx_num, rx_den, ry_num, ry_den, bits, msb, layout, stream);
}

int srcnn_yuv_upscale_luma(const uint8_t* y, uint32_t pitch_y, float* luma_padded, uint32_t w,
                           uint32_t h, uint32_t scale, uint32_t pad, int range,
                           srcnn_stream_t stream) {
  return yuv_upscale_luma("yuv_upscale_luma", y, pitch_y, luma_padded, w, h, scale, pad, 8, 0, range,
                          stream);
}

int srcnn_upscale_planes_u8(const uint8_t* src0, const uint8_t* src1, uint32_t src_pitch,
                            uint32_t pw, uint32_t ph, uint8_t* dst0, uint8_t* dst1,
                            uint32_t dst_pitch, uint32_t ow, uint32_t oh, uint32_t scale,
                            srcnn_stream_t stream) {
  return upscale_planes("upscale_planes_u8", src0, src1, src_pitch, pw, ph, dst0, dst1, dst_pitch, ow,
                        oh, scale, 8, 0, SRCNN_YUV_PLANAR, stream);
}

int srcnn_yuv_compose_luma(const float* luma, uint8_t* y, uint32_t pitch_y, uint32_t W, uint32_t H,
                           int range, srcnn_stream_t stream) {
  return yuv_compose_luma("yuv_compose_luma", luma, y, pitch_y, W, H, 8, 0, range, stream);
}

int srcnn_yuv_upscale_luma16(const void* y, uint32_t pitch_y, float* luma_padded, uint32_t w,
                             uint32_t h, uint32_t scale, uint32_t pad, uint32_t bits, uint32_t msb,
                             int range, srcnn_stream_t stream) {
  return yuv_upscale_luma("yuv_upscale_luma16", y, pitch_y, luma_padded, w, h, scale, pad, bits, msb,
                          range, stream);
}

int srcnn_yuv_compose_luma16(const float* luma, void* y, uint32_t pitch_y, uint32_t W, uint32_t H,
                             uint32_t bits, uint32_t msb, int range, srcnn_stream_t stream) {
  return yuv_compose_luma("yuv_compose_luma16", luma, y, pitch_y, W, H, bits, msb, range, stream);
}

int srcnn_upscale_planes(const void* src0, const void* src1, uint32_t src_pitch, uint32_t pw,
                         uint32_t ph, void* dst0, void* dst1, uint32_t dst_pitch, uint32_t ow,
                         uint32_t oh, uint32_t scale, uint32_t bits, uint32_t msb, uint32_t layout,
                         srcnn_stream_t stream) {
  return upscale_planes("upscale_planes", src0, src1, src_pitch, pw, ph, dst0, dst1, dst_pitch, ow, oh,
                        scale, bits, msb, layout, stream);
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
  SRCNN_REQUIRE((uint64_t)tw * th <= 0x7fffffffull,
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
  if ((uint64_t)gx * gy > 0x7fffffffull) return 0;
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
      (rc = srcnn::preload_yuv()) < 0 || (rc = srcnn::preload_resize()) < 0)
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

size_t srcnn_upscale_workspace_bytes(const srcnn_net* net, uint32_t w, uint32_t h,
                                     uint32_t scale) {
  size_t off[6];
  UpDims d;
  UpWs L;
  if (srcnn_net_offsets(net, off)) return 0;
  const uint64_t pad = (uint64_t)net->f1 + net->f2 + net->f3 - 3;
  if (pad > 0x7fffffffull || up_dims("upscale", w, h, scale, (uint32_t)pad, &d)) return 0;
  return up_ws(net, d, &L) ? L.total : 0;
}

int srcnn_upscale(const srcnn_net* net, const uint8_t* rgba, uint32_t w, uint32_t h,
                  uint32_t scale, const float* params, uint8_t* rgb, void* ws, size_t ws_bytes,
                  srcnn_stream_t stream) {
  SRCNN_REQUIRE(net, "upscale: null srcnn_net");
  const uint64_t pad64 = (uint64_t)net->f1 + net->f2 + net->f3 - 3;
  SRCNN_REQUIRE(pad64 <= 0x7fffffffull, "upscale: total padding %llu too large",
                (unsigned long long)pad64);
  const uint32_t pad = (uint32_t)pad64;
  UpDims d;
  if (int rc = up_dims("upscale", w, h, scale, pad, &d)) return rc;
  SRCNN_REQUIRE(rgba && params && rgb && ws, "upscale: null buffer");
  float* out;
  const auto luma = [&](float* plane) {
    return srcnn_upscale_luma(rgba, plane, w, h, scale, pad, stream);
  };
  if (int rc = up_net("upscale", net, d, params, ws, ws_bytes, stream, luma, &out)) return rc;
  return srcnn_upscale_compose(rgba, out, rgb, w, h, scale, stream);
}

// srcnn_upscale_yuv: every check that does not need the buffers; the chroma
// sizes of the source (cw x ch) and of the output (CW x CH)
struct YuvDims {
  UpDims d;
  uint32_t pad, cw, ch, CW, CH;
};
static int yuv_dims(const char* who, const srcnn_net* net, uint32_t w, uint32_t h, uint32_t cx,
                    uint32_t cy, uint32_t scale, YuvDims* y) {
  SRCNN_REQUIRE(net, "%s: null srcnn_net", who);
  size_t off[6];
  if (int rc = srcnn_net_offsets(net, off)) return rc;
  const uint64_t pad64 = (uint64_t)net->f1 + net->f2 + net->f3 - 3;
  SRCNN_REQUIRE(pad64 <= 0x7fffffffull, "%s: total padding %llu too large", who,
                (unsigned long long)pad64);
  y->pad = (uint32_t)pad64;
  SRCNN_REQUIRE((cx == 2 && cy == 2) || (cx == 2 && cy == 1) || (cx == 1 && cy == 1),
                "%s: chroma subsampling %ux%u is not 2x2 (4:2:0), 2x1 (4:2:2) or 1x1 (4:4:4)", who,
                cx, cy);
  if (int rc = yuv_luma_dims(who, w, h, w, scale, y->pad, &y->d)) return rc;
  y->cw = (w - 1) / cx + 1;
  y->ch = (h - 1) / cy + 1;
  y->CW = (y->d.W - 1) / cx + 1;
  y->CH = (y->d.H - 1) / cy + 1;
  return SRCNN_OK;
}

size_t srcnn_upscale_yuv_workspace_bytes(const srcnn_net* net, uint32_t w, uint32_t h,
                                         uint32_t scale) {
  YuvDims y;
  UpWs L;
  if (yuv_dims("upscale_yuv", net, w, h, 1, 1, scale, &y)) return 0;
  return up_ws(net, y.d, &L) ? L.total : 0;
}

// srcnn_upscale_yuv (8 bits, planar) and srcnn_upscale_frame: `who`
static int upscale_frame(const char* who, const srcnn_net* net, const srcnn_yuv_format& fmt,
                         const srcnn_yuv_frame* src, const srcnn_yuv_frame* dst, uint32_t w,
                         uint32_t h, uint32_t scale, const float* params, void* ws, size_t ws_bytes,
                         srcnn_stream_t stream) {
  YuvDims y;
  uint32_t B;
  if (int rc = yuv_dims(who, net, w, h, fmt.cx, fmt.cy, scale, &y)) return rc;
  if (int rc = yuv_range(who, fmt.range)) return rc;
  if (int rc = yuv_samples(who, fmt.bits, fmt.msb, &B)) return rc;
  if (int rc = yuv_layout(who, fmt.layout)) return rc;
  const bool semi = fmt.layout == SRCNN_YUV_SEMIPLANAR;
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
  // (the sizes again, now with the frames' pitches)
  UpDims d;
  if (int rc = yuv_luma_dims(who, w, h, src->pitch_y, scale, y.pad, &d, B)) return rc;
  if (int rc = plane_dims(who, d.W, d.H, dst->pitch_y, B)) return rc;
  if (int rc = planes_dims(who, src->pitch_c, y.cw, y.ch, dst->pitch_c, y.CW, y.CH, scale, B,
                           semi ? 2 : 1))
    return rc;
  float* out;
  const auto luma = [&](float* plane) {
    return yuv_upscale_luma(who, src->y, src->pitch_y, plane, w, h, scale, y.pad, fmt.bits, fmt.msb,
                            fmt.range, stream);
  };
  if (int rc = up_net(who, net, d, params, ws, ws_bytes, stream, luma, &out)) return rc;
  if (int rc = yuv_compose_luma(who, out, dst->y, dst->pitch_y, d.W, d.H, fmt.bits, fmt.msb,
                                fmt.range, stream))
    return rc;
  return upscale_planes(who, src->u, src->v, src->pitch_c, y.cw, y.ch, dst->u, dst->v, dst->pitch_c,
                        y.CW, y.CH, scale, fmt.bits, fmt.msb, fmt.layout, stream);
}

int srcnn_upscale_yuv(const srcnn_net* net, const srcnn_yuv_frame* src, const srcnn_yuv_frame* dst,
                      uint32_t w, uint32_t h, uint32_t cx, uint32_t cy, uint32_t scale, int range,
                      const float* params, void* ws, size_t ws_bytes, srcnn_stream_t stream) {
  const srcnn_yuv_format fmt{8, 0, SRCNN_YUV_PLANAR, cx, cy, range};
  return upscale_frame("upscale_yuv", net, fmt, src, dst, w, h, scale, params, ws, ws_bytes, stream);
}

int srcnn_upscale_frame(const srcnn_net* net, const srcnn_yuv_format* fmt,
                        const srcnn_yuv_frame* src, const srcnn_yuv_frame* dst, uint32_t w,
                        uint32_t h, uint32_t scale, const float* params, void* ws, size_t ws_bytes,
                        srcnn_stream_t stream) {
  SRCNN_REQUIRE(fmt, "upscale_frame: null srcnn_yuv_format");
  return upscale_frame("upscale_frame", net, *fmt, src, dst, w, h, scale, params, ws, ws_bytes,
                       stream);
}

// srcnn_upscale_to / srcnn_upscale_frame_to: the net's total padding (`who`)
static int net_pad(const char* who, const srcnn_net* net, uint32_t* pad) {
  SRCNN_REQUIRE(net, "%s: null srcnn_net", who);
  size_t off[6];
  if (int rc = srcnn_net_offsets(net, off)) return rc;
  const uint64_t pad64 = (uint64_t)net->f1 + net->f2 + net->f3 - 3;
  SRCNN_REQUIRE(pad64 <= 0x7fffffffull, "%s: total padding %llu too large", who,
                (unsigned long long)pad64);
  *pad = (uint32_t)pad64;
  return SRCNN_OK;
}

size_t srcnn_upscale_to_workspace_bytes(const srcnn_net* net, uint32_t w, uint32_t h, uint32_t W,
                                        uint32_t H) {
  uint32_t pad;
  UpDims d;
  UpWs L;
  if (net_pad("upscale_to", net, &pad) || resize_dims("upscale_to", w, h, W, H, pad, true, &d)) return 0;
  return up_ws(net, d, &L) ? L.total : 0;
}

int srcnn_upscale_to(const srcnn_net* net, const uint8_t* rgba, uint32_t w, uint32_t h, uint32_t W,
                     uint32_t H, const float* params, uint8_t* rgb, void* ws, size_t ws_bytes,
                     srcnn_stream_t stream) {
  uint32_t pad;
  UpDims d;
  if (int rc = net_pad("upscale_to", net, &pad)) return rc;
  if (int rc = resize_dims("upscale_to", w, h, W, H, pad, true, &d)) return rc;
  SRCNN_REQUIRE(rgba && params && rgb && ws, "upscale_to: null buffer");
  float* out;
  const auto luma = [&](float* plane) {
    return srcnn_resize_luma(rgba, plane, w, h, W, H, pad, stream);
  };
  if (int rc = up_net("upscale_to", net, d, params, ws, ws_bytes, stream, luma, &out)) return rc;
  return srcnn_resize_compose(rgba, out, rgb, w, h, W, H, stream);
}

// srcnn_upscale_frame_to: every check that does not need the buffers; the
// chroma sizes of the source (cw x ch) and of the output (CW x CH)
static int frame_to_dims(const srcnn_net* net, uint32_t w, uint32_t h, uint32_t W, uint32_t H,
                         uint32_t cx, uint32_t cy, YuvDims* y) {
  const char* who = "upscale_frame_to";
  if (int rc = net_pad(who, net, &y->pad)) return rc;
  SRCNN_REQUIRE((cx == 2 && cy == 2) || (cx == 2 && cy == 1) || (cx == 1 && cy == 1),
                "%s: chroma subsampling %ux%u is not 2x2 (4:2:0), 2x1 (4:2:2) or 1x1 (4:4:4)", who,
                cx, cy);
  if (int rc = resize_dims(who, w, h, W, H, y->pad, false, &y->d)) return rc;
  y->cw = (w - 1) / cx + 1;
  y->ch = (h - 1) / cy + 1;
  y->CW = (W - 1) / cx + 1;
  y->CH = (H - 1) / cy + 1;
  return SRCNN_OK;
}

size_t srcnn_upscale_frame_to_workspace_bytes(const srcnn_net* net, uint32_t w, uint32_t h,
                                              uint32_t W, uint32_t H) {
  YuvDims y;
  UpWs L;
  if (frame_to_dims(net, w, h, W, H, 1, 1, &y)) return 0;
  return up_ws(net, y.d, &L) ? L.total : 0;
}

int srcnn_upscale_frame_to(const srcnn_net* net, const srcnn_yuv_format* fmtp,
                           const srcnn_yuv_frame* src, const srcnn_yuv_frame* dst, uint32_t w,
                           uint32_t h, uint32_t W, uint32_t H, const float* params, void* ws,
                           size_t ws_bytes, srcnn_stream_t stream) {
  const char* who = "upscale_frame_to";
  SRCNN_REQUIRE(fmtp, "%s: null srcnn_yuv_format", who);
  const srcnn_yuv_format& fmt = *fmtp;
  YuvDims y;
  uint32_t B;
  if (int rc = frame_to_dims(net, w, h, W, H, fmt.cx, fmt.cy, &y)) return rc;
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
  // (the planes with the frames' pitches; the chroma ratio is the luma's)
  if (int rc = plane_dims(who, w, h, src->pitch_y, B)) return rc;
  if (int rc = plane_dims(who, W, H, dst->pitch_y, B)) return rc;
  if (int rc = plane_dims(who, y.cw, y.ch, src->pitch_c, B, nch)) return rc;
  if (int rc = plane_dims(who, y.CW, y.CH, dst->pitch_c, B, nch)) return rc;
  if (int rc = resize_axis(who, "horizontal", w, W, y.cw, y.CW)) return rc;
  if (int rc = resize_axis(who, "vertical", h, H, y.ch, y.CH)) return rc;
  float* out;
  const auto luma = [&](float* plane) {
    return yuv_resize_luma(who, src->y, src->pitch_y, plane, w, h, W, H, y.pad, fmt.bits, fmt.msb,
                           fmt.range, stream);
  };
  if (int rc = up_net(who, net, y.d, params, ws, ws_bytes, stream, luma, &out)) return rc;
  if (int rc = yuv_compose_luma(who, out, dst->y, dst->pitch_y, W, H, fmt.bits, fmt.msb, fmt.range,
                                stream))
    return rc;
  return resize_planes(who, src->u, src->v, src->pitch_c, y.cw, y.ch, dst->u, dst->v, dst->pitch_c,
                       y.CW, y.CH, w, W, h, H, fmt.bits, fmt.msb, fmt.layout, stream);
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
static int eval_ws(const srcnn_net* net, uint32_t W, uint32_t H, uint32_t scale, int64_t shave,
                   EvalWs* L) {
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

}  // extern "C"
