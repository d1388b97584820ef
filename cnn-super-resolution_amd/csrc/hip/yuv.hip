// yuv.hip -- the device front and back end of srcnn_upscale_yuv:
//   yuv_upscale_luma   Y [h][w] u8 (pitched) -> bicubic x S of the normalised
//                      luma, edge-replicated into the padded plane
//                      [(S*h+P)][(S*w+P)] f32 the net reads
//   upscale_planes_u8  two u8 planes [ph][pw] (pitched) -> bicubic x S, rounded
//                      to nearest and clamped, the top-left ow x oh of each
//                      into two u8 planes (pitched): a frame's chroma
//   yuv_compose_luma   the net's luma [H][W] f32 -> Y [H][W] u8 (pitched)
// The resampling is upscale.hip's (bicubic.hpp holds what the
// two files share): one workgroup per tile of JX x JY source pixels, the
// source patch staged in LDS as floats, a horizontal pass into LDS, a vertical
// pass into registers.  The source here is one byte per pixel at an arbitrary
// pitch, so the patch is fetched in aligned 4-byte words wherever a word lies
// inside the row, and in clamped single bytes at the image's edges.
#include "bicubic.hpp"
#include "common.hpp"
#include "ops.hpp"

namespace srcnn {
namespace {

// clamped fetch of the tile's source patch from a byte plane: lane (r, k)
// takes the k-th 4-byte-aligned word under patch row r
template <typename T, typename Store>
__device__ __forceinline__ void stage_bytes(const uint8_t* __restrict__ src, size_t pitch, int w,
                                            int h, int j0, int i0, Store store) {
  constexpr int NW = (T::PC + 6) / 4;  // words under PC bytes at a skew of up to 3
  const int xs = j0 - 2;               // the column of patch column 0
  for (int it = threadIdx.x; it < T::PR * NW; it += kThreads) {
    const int r = it / NW, k = it - r * NW;
    const int sy = min(max(i0 - 2 + r, 0), h - 1);
    const uint8_t* row = src + (size_t)sy * pitch;
    const int skew = (int)(((uintptr_t)row + (uintptr_t)(intptr_t)xs) & 3);
    const int c0 = 4 * k - skew;  // patch column of the word's first byte
    const int x0 = xs + c0;       // its column: row + x0 is 4-byte aligned
    if (x0 >= 0 && x0 + 3 < w) {
      const uint32_t v = *reinterpret_cast<const uint32_t*>(row + x0);
#pragma unroll
      for (int b = 0; b < 4; b++)
        if (c0 + b >= 0 && c0 + b < T::PC) store(r, c0 + b, (float)((v >> (8 * b)) & 255u));
    } else {
#pragma unroll
      for (int b = 0; b < 4; b++)
        if (c0 + b >= 0 && c0 + b < T::PC) store(r, c0 + b, (float)row[min(max(x0 + b, 0), w - 1)]);
    }
  }
}

// the normalised luma of a Y byte: (Y - off) / div with (off, div) = (0, 255)
// for full range and (16, 219) for limited; a true division, never contracted,
// so that scale 1 at full range gives float(Y) / 255.0f bit for bit
__device__ __forceinline__ float luma_of_y(float y, float off, float div) {
#pragma clang fp contract(off)
  return (y - off) / div;
}

// clamp(rintf(v), 0, 255) as a byte (rintf: round to nearest, ties to even)
__device__ __forceinline__ uint32_t quantise(float v) {
  return (uint32_t)fminf(fmaxf(rintf(v), 0.0f), 255.0f);
}

template <int S>
__global__ __launch_bounds__(kThreads) void yuv_upscale_luma_kernel(
    const uint8_t* __restrict__ y, size_t pitch, float* __restrict__ out, int w, int h, int P,
    int tiles_x, float off, float div) {
  using T = Tile<S, false>;
  __shared__ float s_src[T::PR][T::PCP];
  __shared__ float s_h[T::PR][T::TX + 1];
  const int tiles_y = gridDim.x / tiles_x;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int j0 = tx * T::JX, i0 = ty * T::JY;

  stage_bytes<T>(y, pitch, w, h, j0, i0,
                 [&](int r, int c, float v) { s_src[r][c] = luma_of_y(v, off, div); });
  __syncthreads();
  hpass<S, T, 1>([&](int r, int c, int) { return s_src[r][c]; },
                 [&](int, int r, int x, float v) { s_h[r][x] = v; });
  __syncthreads();

  store_plane_tile<S>(s_h, out, w, h, P, tx, ty, i0, tiles_x, tiles_y);
}

// blockIdx.y selects the plane.  The tile is upscale_compose's (64 x 8 source
// pixels at S <= 2, else 32 x 16): an output row of the tile is 64 - 128 bytes.
template <int S>
__global__ __launch_bounds__(kThreads) void upscale_planes_u8_kernel(
    const uint8_t* __restrict__ src0, const uint8_t* __restrict__ src1, size_t src_pitch, int pw,
    int ph, uint8_t* __restrict__ dst0, uint8_t* __restrict__ dst1, size_t dst_pitch, int ow, int oh,
    int tiles_x) {
  using T = Tile<S, true>;
  constexpr int TX = T::TX, TY = T::TY;
  constexpr int RB = kThreads / 32;  // output rows per batch
  constexpr int STG = 16 + TX;       // staged row: up to 15 bytes of skew + the pixels
  __shared__ float s_src[T::PR][T::PCP];
  __shared__ float s_h[T::PR][TX + 1];
  __shared__ __attribute__((aligned(16))) uint8_t s_out[RB][STG];
  const uint8_t* __restrict__ src = blockIdx.y ? src1 : src0;
  uint8_t* __restrict__ dst = blockIdx.y ? dst1 : dst0;
  const int tid = threadIdx.x;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int j0 = tx * T::JX, i0 = ty * T::JY;

  stage_bytes<T>(src, src_pitch, pw, ph, j0, i0, [&](int r, int c, float v) { s_src[r][c] = v; });
  __syncthreads();
  hpass<S, T, 1>([&](int r, int c, int) { return s_src[r][c]; },
                 [&](int, int r, int x, float v) { s_h[r][x] = v; });
  __syncthreads();

  // the tile's share of the ow x oh output: the last tile of a row or column
  // is cut by the plane (S*pw x S*ph) or by the crop, whichever is smaller
  const int X0 = tx * TX, Y0 = ty * TY;
  const int ncol = min(TX, ow - X0), nrow = min(TY, oh - Y0);  // bytes of a row; rows
  const int c5 = tid & 31, rr = tid >> 5;
  for (int yb = 0; yb < nrow; yb += RB) {
    const bool live = yb + rr < nrow;
    const int Y = Y0 + yb + rr;
    uint8_t* grow = dst + (size_t)Y * dst_pitch + X0;
    // the row is staged in LDS at the skew its global address has, so that
    // 16-byte chunks of the two line up
    const int o = (int)((uintptr_t)grow & 15);
    if (live) {
      const int jy = Y / S, ky = Y - jy * S;
      const int rb = jy - i0 + tap_base(S, ky) + 1;
      float wv[4];
      phase_weights<S>(ky, wv);
      const float w0 = wv[0], w1 = wv[1], w2 = wv[2], w3 = wv[3];
#pragma unroll
      for (int i = 0; i < TX / 32; i++) {
        const int cx = c5 + 32 * i;
        if (cx < ncol)
          s_out[rr][o + cx] = (uint8_t)quantise(w0 * s_h[rb][cx] + w1 * s_h[rb + 1][cx] +
                                                w2 * s_h[rb + 2][cx] + w3 * s_h[rb + 3][cx]);
      }
    }
    __syncthreads();
    if (live) {
      // bytes up to the first 16-byte boundary, 16-byte chunks, the rest
      const int head = min((16 - o) & 15, ncol);
      if (c5 < head) grow[c5] = s_out[rr][o + c5];
      const int nch = (ncol - head) >> 4;  // <= TX/16 <= 8 of the row's 32 lanes
      if (c5 < nch)
        *reinterpret_cast<uint4*>(grow + head + 16 * c5) =
            *reinterpret_cast<const uint4*>(&s_out[rr][o + head + 16 * c5]);
      const int t = head + 16 * nch + c5;
      if (t < ncol) grow[t] = s_out[rr][o + t];
    }
    __syncthreads();
  }
}

// four floats at any 4-byte-aligned address: a row of the luma starts at
// Y * W floats and is read from the pixel where the Y row's address reaches a
// 16-byte boundary, so the loads are 16 bytes wide but not 16-byte aligned
typedef float float4u __attribute__((ext_vector_type(4), aligned(4)));

// One wavefront per row, four rows per workgroup.  A lane takes 16 pixels:
// four 16-byte loads, one 16-byte store; the bytes before the row's first
// 16-byte boundary and after its last go one per lane.
__global__ __launch_bounds__(kThreads) void yuv_compose_luma_kernel(
    const float* __restrict__ luma, uint8_t* __restrict__ y, size_t pitch, int W, int H, float mul,
    float add) {
  const int Y = blockIdx.x * (kThreads / 64) + threadIdx.x / 64;
  if (Y >= H) return;
  const int l = threadIdx.x & 63;
  const float* __restrict__ in = luma + (size_t)Y * W;
  uint8_t* __restrict__ orow = y + (size_t)Y * pitch;
  auto q = [&](float v) { return quantise(fmaf(v, mul, add)); };
  const int head = min((int)((16 - ((uintptr_t)orow & 15)) & 15), W);
  if (l < head) orow[l] = (uint8_t)q(in[l]);
  const int ng = (W - head) >> 4;
  for (int g = l; g < ng; g += 64) {
    const int X = head + 16 * g;
    uint32_t o[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const float4u v = *reinterpret_cast<const float4u*>(in + X + 4 * i);
      o[i] = q(v.x) | q(v.y) << 8 | q(v.z) << 16 | q(v.w) << 24;
    }
    *reinterpret_cast<uint4*>(orow + X) = make_uint4(o[0], o[1], o[2], o[3]);
  }
  const int t = head + 16 * ng + l;  // fewer than 16 pixels are left
  if (t < W) orow[t] = (uint8_t)q(in[t]);
}

}  // namespace

int yuv_upscale_luma(const uint8_t* y, uint32_t pitch_y, float* plane, uint32_t w, uint32_t h,
                     uint32_t scale, uint32_t pad, bool full_range, hipStream_t s) {
  SRCNN_PROFILE("yuv_upscale_luma", s);
  const float off = full_range ? 0.0f : 16.0f, div = full_range ? 255.0f : 219.0f;
#define SRCNN_YUV_LUMA(S)                                                                    \
  {                                                                                          \
    const uint32_t tx = tiles(w, Tile<S, false>::JX), ty = tiles(h, Tile<S, false>::JY);     \
    hipLaunchKernelGGL(yuv_upscale_luma_kernel<S>, dim3(tx* ty), dim3(kThreads), 0, s, y,    \
                       (size_t)pitch_y, plane, (int)w, (int)h, (int)pad, (int)tx, off, div); \
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

int upscale_planes_u8(const uint8_t* src0, const uint8_t* src1, uint32_t src_pitch, uint32_t pw,
                      uint32_t ph, uint8_t* dst0, uint8_t* dst1, uint32_t dst_pitch, uint32_t ow,
                      uint32_t oh, uint32_t scale, hipStream_t s) {
  SRCNN_PROFILE("upscale_planes_u8", s);
#define SRCNN_YUV_PLANES(S)                                                                    \
  {                                                                                            \
    const uint32_t tx = tiles(pw, Tile<S, true>::JX), ty = tiles(ph, Tile<S, true>::JY);       \
    hipLaunchKernelGGL(upscale_planes_u8_kernel<S>, dim3(tx* ty, 2), dim3(kThreads), 0, s,     \
                       src0, src1, (size_t)src_pitch, (int)pw, (int)ph, dst0, dst1,            \
                       (size_t)dst_pitch, (int)ow, (int)oh, (int)tx);                          \
  }
  switch (scale) {
    case 1: SRCNN_YUV_PLANES(1); break;
    case 2: SRCNN_YUV_PLANES(2); break;
    case 3: SRCNN_YUV_PLANES(3); break;
    case 4: SRCNN_YUV_PLANES(4); break;
    default: return fail(SRCNN_ERR_INVALID, "upscale_planes_u8: scale %u has no kernel", scale);
  }
#undef SRCNN_YUV_PLANES
  SRCNN_LAUNCH_TRY();
  return SRCNN_OK;
}

int yuv_compose_luma(const float* luma, uint8_t* y, uint32_t pitch_y, uint32_t W, uint32_t H,
                     bool full_range, hipStream_t s) {
  SRCNN_PROFILE("yuv_compose_luma", s);
  const float mul = full_range ? 255.0f : 219.0f, add = full_range ? 0.0f : 16.0f;
  hipLaunchKernelGGL(yuv_compose_luma_kernel, dim3(tiles(H, kThreads / 64)), dim3(kThreads), 0, s,
                     luma, y, (size_t)pitch_y, (int)W, (int)H, mul, add);
  SRCNN_LAUNCH_TRY();
  return SRCNN_OK;
}

int preload_yuv() {
  const void* k[] = {(const void*)yuv_upscale_luma_kernel<1>,  (const void*)yuv_upscale_luma_kernel<2>,
                     (const void*)yuv_upscale_luma_kernel<3>,  (const void*)yuv_upscale_luma_kernel<4>,
                     (const void*)upscale_planes_u8_kernel<1>, (const void*)upscale_planes_u8_kernel<2>,
                     (const void*)upscale_planes_u8_kernel<3>, (const void*)upscale_planes_u8_kernel<4>,
                     (const void*)yuv_compose_luma_kernel};
  return resolve_kernels(k, 9);
}

}  // namespace srcnn
