// yuv.hip -- the device front and back end of srcnn_upscale_yuv
// and of srcnn_upscale_frame:
//   yuv_upscale_luma   Y [h][w] (pitched) -> bicubic x S of the normalised
//                      luma, edge-replicated into the padded plane
//                      [(S*h+P)][(S*w+P)] f32 the net reads
//   upscale_planes     a frame's chroma, [ph][pw] (pitched), as two planes or
//                      as one plane of (U, V) pairs -> bicubic x S, rounded to
//                      nearest and clamped, the top-left ow x oh in the same
//                      layout (pitched)
//   yuv_compose_luma   the net's luma [H][W] f32 -> Y [H][W] (pitched)
// A sample is one byte, or a 16-bit word that holds 9 to 16 bits in its low or
// in its high bits (template parameter B: bytes per sample; struct Fmt,
// samples.hpp, shared with resize.hip).
// The resampling is upscale.hip's (bicubic.hpp holds what the
// two files share): one workgroup per tile of JX x JY source pixels, the
// source patch staged in LDS as floats, a horizontal pass into LDS, a vertical
// pass into registers.  The source here is one or two bytes per sample at an
// arbitrary pitch, so the patch is fetched in aligned words of four samples
// wherever a word lies inside the row, and in clamped single samples at the
// image's edges.
#include "bicubic.hpp"
#include "common.hpp"
#include "ops.hpp"
#include "samples.hpp"

namespace srcnn {
namespace {

template <int S, int B>
__global__ __launch_bounds__(kThreads) void yuv_upscale_luma_kernel(
    const uint8_t* __restrict__ y, size_t pitch, float* __restrict__ out, int w, int h, int P,
    int tiles_x, float off, float div, Fmt<B> f) {
  using T = Tile<S, false>;
  __shared__ float s_src[T::PR][T::PCP];
  __shared__ float s_h[T::PR][T::TX + 1];
  const int tiles_y = gridDim.x / tiles_x;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int j0 = tx * T::JX, i0 = ty * T::JY;

  stage_samples<T, B, 1>(y, pitch, w, h, j0, i0, [&](int r, int c, int, uint32_t v) {
    s_src[r][c] = luma_of_y((float)f.value(v), off, div);
  });
  __syncthreads();
  hpass<S, T, 1>([&](int r, int c, int) { return s_src[r][c]; },
                 [&](int, int r, int x, float v) { s_h[r][x] = v; });
  __syncthreads();

  store_plane_tile<S>(s_h, out, w, h, P, tx, ty, i0, tiles_x, tiles_y);
}

// NCH = 1: two planes, blockIdx.y selects one.  NCH = 2: src0 / dst0 hold
// (U, V) pairs, the two channels of one pass; pw, ow and the tile count pairs.
// The tile is upscale_compose's (64 x 8 source pixels at S <= 2, else 32 x 16):
// an output row of the tile is 64 - 512 bytes.
template <int S, int B, int NCH>
__global__ __launch_bounds__(kThreads) void upscale_planes_kernel(
    const uint8_t* __restrict__ src0, const uint8_t* __restrict__ src1, size_t src_pitch, int pw,
    int ph, uint8_t* __restrict__ dst0, uint8_t* __restrict__ dst1, size_t dst_pitch, int ow, int oh,
    int tiles_x, Fmt<B> f) {
  using T = Tile<S, true>;
  using E = typename Sample<B>::type;
  constexpr int TX = T::TX, TY = T::TY;
  constexpr int RB = kThreads / 32;        // output rows per batch
  constexpr int STG = 16 + TX * NCH * B;   // staged row: up to 15 bytes of skew + the samples
  __shared__ float s_src[NCH][T::PR][T::PCP];
  __shared__ float s_h[NCH][T::PR][TX + 1];
  __shared__ __attribute__((aligned(16))) uint8_t s_out[RB][STG];
  const uint8_t* __restrict__ src = NCH == 1 && blockIdx.y ? src1 : src0;
  uint8_t* __restrict__ dst = NCH == 1 && blockIdx.y ? dst1 : dst0;
  const int tid = threadIdx.x;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int j0 = tx * T::JX, i0 = ty * T::JY;

  stage_samples<T, B, NCH>(src, src_pitch, pw, ph, j0, i0, [&](int r, int c, int ch, uint32_t v) {
    s_src[ch][r][c] = (float)f.value(v);
  });
  __syncthreads();
  hpass<S, T, NCH>([&](int r, int c, int ch) { return s_src[ch][r][c]; },
                   [&](int ch, int r, int x, float v) { s_h[ch][r][x] = v; });
  __syncthreads();

  // the tile's share of the ow x oh output: the last tile of a row or column
  // is cut by the plane (S*pw x S*ph) or by the crop, whichever is smaller
  const int X0 = tx * TX, Y0 = ty * TY;
  const int ncol = min(TX, ow - X0), nrow = min(TY, oh - Y0);  // pixels of a row; rows
  const int nb = ncol * (NCH * B);                             // bytes of a row
  const int c5 = tid & 31, rr = tid >> 5;
  for (int yb = 0; yb < nrow; yb += RB) {
    const bool live = yb + rr < nrow;
    const int Y = Y0 + yb + rr;
    uint8_t* gbytes = dst + (size_t)Y * dst_pitch + (size_t)X0 * (NCH * B);
    // the row is staged in LDS at the skew its global address has, so that
    // 16-byte chunks of the two line up
    const int o = (int)((uintptr_t)gbytes & 15);
    if (live) {
      const int jy = Y / S, ky = Y - jy * S;
      const int rb = jy - i0 + tap_base(S, ky) + 1;
      float wv[4];
      phase_weights<S>(ky, wv);
      const float w0 = wv[0], w1 = wv[1], w2 = wv[2], w3 = wv[3];
#pragma unroll
      for (int i = 0; i < TX / 32; i++) {
        const int cx = c5 + 32 * i;
        if (cx < ncol) {
#pragma unroll
          for (int ch = 0; ch < NCH; ch++)
            *reinterpret_cast<E*>(&s_out[rr][o + (cx * NCH + ch) * B]) =
                (E)quantise<B>(w0 * s_h[ch][rb][cx] + w1 * s_h[ch][rb + 1][cx] +
                                   w2 * s_h[ch][rb + 2][cx] + w3 * s_h[ch][rb + 3][cx],
                               f);
        }
      }
    }
    __syncthreads();
    if (live) {
      // samples up to the first 16-byte boundary, 16-byte chunks, the rest
      // (in bytes: o, nb and head are multiples of B)
      auto copy = [&](int at) {
        *reinterpret_cast<E*>(gbytes + at) = *reinterpret_cast<const E*>(&s_out[rr][o + at]);
      };
      const int head = min((16 - o) & 15, nb);
      if (c5 * B < head) copy(c5 * B);
      const int nch = (nb - head) >> 4;  // <= TX*NCH*B/16 <= 32, the row's lanes
      if (c5 < nch)
        *reinterpret_cast<uint4*>(gbytes + head + 16 * c5) =
            *reinterpret_cast<const uint4*>(&s_out[rr][o + head + 16 * c5]);
      const int t = head + 16 * nch + c5 * B;  // fewer than 16 bytes are left
      if (t < nb) copy(t);
    }
    __syncthreads();
  }
}

// four floats at any 4-byte-aligned address: a row of the luma starts at
// Y * W floats and is read from the pixel where the Y row's address reaches a
// 16-byte boundary, so the loads are 16 bytes wide but not 16-byte aligned
typedef float float4u __attribute__((ext_vector_type(4), aligned(4)));

// One-byte samples: one wavefront per row, four rows per workgroup.  A lane
// takes the 16 / B pixels of one 16-byte store: 16-byte loads, one 16-byte
// store; the samples before the row's first 16-byte boundary and after its
// last go one per lane.  Two-byte samples: the four wavefronts of a workgroup
// share one row, so that twice the output bytes leave in as many passes per
// lane as with bytes.
template <int B>
__global__ __launch_bounds__(kThreads) void yuv_compose_luma_kernel(
    const float* __restrict__ luma, uint8_t* __restrict__ y, size_t pitch, int W, int H, float mul,
    float add, Fmt<B> f) {
  using E = typename Sample<B>::type;
  constexpr int PPL = 16 / B;                  // pixels per lane and store
  constexpr int LPR = B == 1 ? 64 : kThreads;  // lanes per row
  const int Y = blockIdx.x * (kThreads / LPR) + threadIdx.x / LPR;
  if (Y >= H) return;
  const int l = threadIdx.x & (LPR - 1);
  const float* __restrict__ in = luma + (size_t)Y * W;
  uint8_t* __restrict__ obytes = y + (size_t)Y * pitch;
  E* __restrict__ orow = reinterpret_cast<E*>(obytes);
  auto q = [&](float v) { return quantise<B>(fmaf(v, mul, add), f); };
  const int head = min((int)((16 - ((uintptr_t)obytes & 15)) & 15) >> (B - 1), W);
  if (l < head) orow[l] = (E)q(in[l]);
  const int ng = (W - head) >> (B == 1 ? 4 : 3);  // groups of PPL pixels
  for (int g = l; g < ng; g += LPR) {
    const int X = head + PPL * g;
    uint32_t o[4];
    if constexpr (B == 1) {
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const float4u v = *reinterpret_cast<const float4u*>(in + X + 4 * i);
        o[i] = q(v.x) | q(v.y) << 8 | q(v.z) << 16 | q(v.w) << 24;
      }
    } else {
#pragma unroll
      for (int i = 0; i < 2; i++) {
        const float4u v = *reinterpret_cast<const float4u*>(in + X + 4 * i);
        o[2 * i] = q(v.x) | q(v.y) << 16;
        o[2 * i + 1] = q(v.z) | q(v.w) << 16;
      }
    }
    *reinterpret_cast<uint4*>(orow + X) = make_uint4(o[0], o[1], o[2], o[3]);
  }
  const int t = head + PPL * ng + l;  // fewer than 16 / B pixels are left
  if (t < W) orow[t] = (E)q(in[t]);
}

template <int B>
int launch_luma(const uint8_t* y, uint32_t pitch_y, float* plane, uint32_t w, uint32_t h,
                uint32_t scale, uint32_t pad, float off, float div, Fmt<B> f, hipStream_t s) {
#define SRCNN_YUV_LUMA(S)                                                                      \
  {                                                                                            \
    const uint32_t tx = tiles(w, Tile<S, false>::JX), ty = tiles(h, Tile<S, false>::JY);       \
    hipLaunchKernelGGL((yuv_upscale_luma_kernel<S, B>), dim3(tx* ty), dim3(kThreads), 0, s, y, \
                       (size_t)pitch_y, plane, (int)w, (int)h, (int)pad, (int)tx, off, div, f); \
  }
  switch (scale) {
    case 1: SRCNN_YUV_LUMA(1); break;
    case 2: SRCNN_YUV_LUMA(2); break;
    case 3: SRCNN_YUV_LUMA(3); break;
    case 4: SRCNN_YUV_LUMA(4); break;
    default: return fail(SRCNN_ERR_INVALID, "yuv_upscale_luma: scale %u has no kernel", scale);
  }
#undef SRCNN_YUV_LUMA
  SRCNN_LAUNCH_TRY();
  return SRCNN_OK;
}

template <int B>
int launch_planes(const uint8_t* src0, const uint8_t* src1, uint32_t src_pitch, uint32_t pw,
                  uint32_t ph, uint8_t* dst0, uint8_t* dst1, uint32_t dst_pitch, uint32_t ow,
                  uint32_t oh, uint32_t scale, bool semiplanar, Fmt<B> f, hipStream_t s) {
#define SRCNN_YUV_PLANES(S)                                                                       \
  {                                                                                               \
    const uint32_t tx = tiles(pw, Tile<S, true>::JX), ty = tiles(ph, Tile<S, true>::JY);          \
    const auto k = semiplanar ? upscale_planes_kernel<S, B, 2> : upscale_planes_kernel<S, B, 1>;  \
    hipLaunchKernelGGL(k, dim3(tx* ty, semiplanar ? 1 : 2), dim3(kThreads), 0, s, src0, src1,     \
                       (size_t)src_pitch, (int)pw, (int)ph, dst0, dst1, (size_t)dst_pitch,        \
                       (int)ow, (int)oh, (int)tx, f);                                             \
  }
  switch (scale) {
    case 1: SRCNN_YUV_PLANES(1); break;
    case 2: SRCNN_YUV_PLANES(2); break;
    case 3: SRCNN_YUV_PLANES(3); break;
    case 4: SRCNN_YUV_PLANES(4); break;
    default: return fail(SRCNN_ERR_INVALID, "upscale_planes: scale %u has no kernel", scale);
  }
#undef SRCNN_YUV_PLANES
  SRCNN_LAUNCH_TRY();
  return SRCNN_OK;
}

// SRCNN_PROFILE's label of a call: what was there before the deeper formats
//  keeps the name it was first measured under
const char* label(bool first, const char* name8, const char* name) { return first ? name8 : name; }

}  // namespace

int yuv_upscale_luma(const void* y, uint32_t pitch_y, float* plane, uint32_t w, uint32_t h,
                     uint32_t scale, uint32_t pad, uint32_t bits, bool msb, bool full_range,
                     hipStream_t s) {
  SRCNN_PROFILE(label(bits == 8, "yuv_upscale_luma", "yuv_upscale_luma16"), s);
  const uint8_t* src = static_cast<const uint8_t*>(y);
  const Range r = range_of(bits, full_range);
  if (bits == 8)
    return launch_luma<1>(src, pitch_y, plane, w, h, scale, pad, r.off, r.span, Fmt<1>{}, s);
  return launch_luma<2>(src, pitch_y, plane, w, h, scale, pad, r.off, r.span, deep_fmt(bits, msb),
                        s);
}

int upscale_planes(const void* src0, const void* src1, uint32_t src_pitch, uint32_t pw, uint32_t ph,
                   void* dst0, void* dst1, uint32_t dst_pitch, uint32_t ow, uint32_t oh,
                   uint32_t scale, uint32_t bits, bool msb, bool semiplanar, hipStream_t s) {
  SRCNN_PROFILE(label(bits == 8 && !semiplanar, "upscale_planes_u8", "upscale_planes"), s);
  const uint8_t *a = static_cast<const uint8_t*>(src0), *b = static_cast<const uint8_t*>(src1);
  uint8_t *A = static_cast<uint8_t*>(dst0), *Bp = static_cast<uint8_t*>(dst1);
  if (bits == 8)
    return launch_planes<1>(a, b, src_pitch, pw, ph, A, Bp, dst_pitch, ow, oh, scale, semiplanar,
                            Fmt<1>{}, s);
  return launch_planes<2>(a, b, src_pitch, pw, ph, A, Bp, dst_pitch, ow, oh, scale, semiplanar,
                          deep_fmt(bits, msb), s);
}

int yuv_compose_luma(const float* luma, void* y, uint32_t pitch_y, uint32_t W, uint32_t H,
                     uint32_t bits, bool msb, bool full_range, hipStream_t s) {
  SRCNN_PROFILE(label(bits == 8, "yuv_compose_luma", "yuv_compose_luma16"), s);
  uint8_t* dst = static_cast<uint8_t*>(y);
  const Range r = range_of(bits, full_range);
  if (bits == 8)
    hipLaunchKernelGGL(yuv_compose_luma_kernel<1>, dim3(tiles(H, kThreads / 64)), dim3(kThreads), 0,
                       s, luma, dst, (size_t)pitch_y, (int)W, (int)H, r.span, r.off, Fmt<1>{});
  else
    hipLaunchKernelGGL(yuv_compose_luma_kernel<2>, dim3(H), dim3(kThreads), 0, s, luma, dst,
                       (size_t)pitch_y, (int)W, (int)H, r.span, r.off, deep_fmt(bits, msb));
  SRCNN_LAUNCH_TRY();
  return SRCNN_OK;
}

int preload_yuv() {
#define SRCNN_YUV_SCALES(K, ...) \
  (const void*)K<1, __VA_ARGS__>, (const void*)K<2, __VA_ARGS__>, (const void*)K<3, __VA_ARGS__>, (const void*)K<4, __VA_ARGS__>
  const void* k[] = {SRCNN_YUV_SCALES(yuv_upscale_luma_kernel, 1),
                     SRCNN_YUV_SCALES(yuv_upscale_luma_kernel, 2),
                     SRCNN_YUV_SCALES(upscale_planes_kernel, 1, 1),
                     SRCNN_YUV_SCALES(upscale_planes_kernel, 1, 2),
                     SRCNN_YUV_SCALES(upscale_planes_kernel, 2, 1),
                     SRCNN_YUV_SCALES(upscale_planes_kernel, 2, 2),
                     (const void*)yuv_compose_luma_kernel<1>,
                     (const void*)yuv_compose_luma_kernel<2>};
#undef SRCNN_YUV_SCALES
  return resolve_kernels(k, (int)(sizeof(k) / sizeof(k[0])));
}

}  // namespace srcnn
