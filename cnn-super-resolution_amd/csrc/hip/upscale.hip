// upscale.hip -- the device front and back end of srcnn_upscale:
//   upscale_luma     rgba [h][w][4] u8 -> bicubic x S luma, edge-replicated into
//                    the padded plane [(S*h+P)][(S*w+P)] f32 the net reads
//   upscale_compose  bicubic x S of the source's r, g, b + the net's luma ->
//                    rgb [S*h][S*w][3] u8 (swap_luma's constants and rounding)
// The reference has no counterpart (its README: "application input is already
// scaled image"); the resampling is specified in DESIGN.md 10.1.
//
// Both kernels: one workgroup per tile of JX x JY source pixels, i.e.
// (JX*S) x (JY*S) output pixels (struct Tile).  The source patch the tile's
// taps reach (j-2 .. j+2: (JX+4) x (JY+4), indices clamped to the image) is
// fetched once with one 4-byte load per pixel and kept in LDS (luma as floats,
// colours as the RGBA8 word); the horizontal pass writes JY+4 rows of S*JX
// values to LDS; the vertical pass reads four of those rows per output into
// registers.  S is a template parameter: the only divisions left are by that
// constant, once per output row, and the tile decode once per workgroup.
#include "bicubic.hpp"
#include "common.hpp"
#include "luma.hpp"
#include "ops.hpp"

namespace srcnn {
namespace {

// clamped fetch of the tile's source patch: one uchar4 load per pixel,
// consecutive lanes consecutive pixels of a row
template <typename T, typename Store>
__device__ __forceinline__ void stage_patch(const uint8_t* __restrict__ rgba, int w, int h, int j0,
                                            int i0, Store store) {
  constexpr int LW = T::PC <= 64 ? 64 : 128;  // lanes per patch row
  const int c = threadIdx.x % LW;
  if (c >= T::PC) return;
  const int sx = min(max(j0 - 2 + c, 0), w - 1);
  for (int r = threadIdx.x / LW; r < T::PR; r += kThreads / LW) {
    const int sy = min(max(i0 - 2 + r, 0), h - 1);
    store(r, c, reinterpret_cast<const uchar4*>(rgba)[(size_t)sy * w + sx]);
  }
}

template <int S>
__global__ __launch_bounds__(kThreads) void upscale_luma_kernel(const uint8_t* __restrict__ rgba,
                                                                float* __restrict__ out, int w,
                                                                int h, int P, int tiles_x) {
  using T = Tile<S, false>;
  __shared__ float s_src[T::PR][T::PCP];
  __shared__ float s_h[T::PR][T::TX + 1];
  const int tiles_y = gridDim.x / tiles_x;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int j0 = tx * T::JX, i0 = ty * T::JY;

  stage_patch<T>(rgba, w, h, j0, i0, [&](int r, int c, uchar4 p) {
    s_src[r][c] = luma_of((float)p.x, (float)p.y, (float)p.z);
  });
  __syncthreads();
  hpass<S, T, 1>([&](int r, int c, int) { return s_src[r][c]; },
                 [&](int, int r, int x, float v) { s_h[r][x] = v; });
  __syncthreads();

  store_plane_tile<S>(s_h, out, w, h, P, tx, ty, i0, tiles_x, tiles_y);
}

template <int S>
__global__ __launch_bounds__(kThreads) void upscale_compose_kernel(
    const uint8_t* __restrict__ rgba, const float* __restrict__ nl, uint8_t* __restrict__ rgb,
    int w, int h, int tiles_x) {
  using T = Tile<S, true>;
  constexpr int TX = T::TX, TY = T::TY;
  constexpr int RB = kThreads / 32;    // output rows per batch
  constexpr int STG = 16 + 3 * TX;     // staged row: up to 15 bytes of skew + the pixels
  __shared__ uchar4 s_src[T::PR][T::PCP];
  __shared__ float s_h[3][T::PR][TX + 1];
  __shared__ __attribute__((aligned(16))) uint8_t s_out[RB][STG];
  const int tid = threadIdx.x;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int j0 = tx * T::JX, i0 = ty * T::JY;

  stage_patch<T>(rgba, w, h, j0, i0, [&](int r, int c, uchar4 p) { s_src[r][c] = p; });
  __syncthreads();
  hpass<S, T, 3>(
      [&](int r, int c, int ch) {
        const uchar4 p = s_src[r][c];
        return (float)(ch == 0 ? p.x : ch == 1 ? p.y : p.z);
      },
      [&](int ch, int r, int x, float v) { s_h[ch][r][x] = v; });
  __syncthreads();

  const int W = w * S, H = h * S;
  const int X0 = tx * TX, Y0 = ty * TY;
  const int ncol = min(TX, W - X0), nrow = min(TY, H - Y0);
  const int nb = 3 * ncol;  // bytes of one output row of the tile
  const int c5 = tid & 31, rr = tid >> 5;
  for (int yb = 0; yb < nrow; yb += RB) {
    const bool live = yb + rr < nrow;
    const int Y = Y0 + yb + rr;
    uint8_t* grow = rgb + ((size_t)Y * W + X0) * 3;
    // the row is staged in LDS at the skew its global address has, so that
    // 16-byte chunks of the two line up
    const int o = (int)((uintptr_t)grow & 15);
    if (live) {
      const int jy = Y / S, ky = Y - jy * S;
      const int rb = jy - i0 + tap_base(S, ky) + 1;
      float wv[4];
      phase_weights<S>(ky, wv);
      const float w0 = wv[0], w1 = wv[1], w2 = wv[2], w3 = wv[3];
      const float* lrow = nl + (size_t)Y * W + X0;
#pragma unroll
      for (int i = 0; i < TX / 32; i++) {
        const int cx = c5 + 32 * i;
        if (cx < ncol) {
          auto val = [&](int ch) {
            return w0 * s_h[ch][rb][cx] + w1 * s_h[ch][rb + 1][cx] + w2 * s_h[ch][rb + 2][cx] +
                   w3 * s_h[ch][rb + 3][cx];
          };
          compose_px(val(0), val(1), val(2), lrow[cx], &s_out[rr][o + 3 * cx]);
        }
      }
    }
    __syncthreads();
    if (live) {
      // bytes up to the first 16-byte boundary, 16-byte chunks, the rest
      const int head = min((16 - o) & 15, nb);
      if (c5 < head) grow[c5] = s_out[rr][o + c5];
      const int nch = (nb - head) >> 4;  // <= 3*TX/16 <= 24 of the row's 32 lanes
      if (c5 < nch)
        *reinterpret_cast<uint4*>(grow + head + 16 * c5) =
            *reinterpret_cast<const uint4*>(&s_out[rr][o + head + 16 * c5]);
      const int t = head + 16 * nch + c5;
      if (t < nb) grow[t] = s_out[rr][o + t];
    }
    __syncthreads();
  }
}

}  // namespace

int upscale_luma(const uint8_t* rgba, float* plane, uint32_t w, uint32_t h, uint32_t scale,
                 uint32_t pad, hipStream_t s) {
  SRCNN_PROFILE("upscale_luma", s);
#define SRCNN_UP_LUMA(S)                                                                        \
  {                                                                                             \
    const uint32_t tx = tiles(w, Tile<S, false>::JX), ty = tiles(h, Tile<S, false>::JY); \
    hipLaunchKernelGGL(upscale_luma_kernel<S>, dim3(tx* ty), dim3(kThreads), 0, s, rgba, plane, \
                       (int)w, (int)h, (int)pad, (int)tx);                                      \
  }
  switch (scale) {
    case 1: SRCNN_UP_LUMA(1); break;
    case 2: SRCNN_UP_LUMA(2); break;
    case 3: SRCNN_UP_LUMA(3); break;
    case 4: SRCNN_UP_LUMA(4); break;
    default: return fail(SRCNN_ERR_INVALID, "upscale_luma: scale %u has no kernel", scale);
  }
#undef SRCNN_UP_LUMA
  SRCNN_LAUNCH_TRY();
  return SRCNN_OK;
}

int upscale_compose(const uint8_t* rgba, const float* nl, uint8_t* rgb, uint32_t w, uint32_t h,
                    uint32_t scale, hipStream_t s) {
  SRCNN_PROFILE("upscale_compose", s);
#define SRCNN_UP_COMPOSE(S)                                                                     \
  {                                                                                             \
    const uint32_t tx = tiles(w, Tile<S, true>::JX), ty = tiles(h, Tile<S, true>::JY);   \
    hipLaunchKernelGGL(upscale_compose_kernel<S>, dim3(tx* ty), dim3(kThreads), 0, s, rgba, nl, \
                       rgb, (int)w, (int)h, (int)tx);                                           \
  }
  switch (scale) {
    case 1: SRCNN_UP_COMPOSE(1); break;
    case 2: SRCNN_UP_COMPOSE(2); break;
    case 3: SRCNN_UP_COMPOSE(3); break;
    case 4: SRCNN_UP_COMPOSE(4); break;
    default: return fail(SRCNN_ERR_INVALID, "upscale_compose: scale %u has no kernel", scale);
  }
#undef SRCNN_UP_COMPOSE
  SRCNN_LAUNCH_TRY();
  return SRCNN_OK;
}

int preload_upscale() {
  const void* k[] = {(const void*)upscale_luma_kernel<1>,    (const void*)upscale_luma_kernel<2>,
                     (const void*)upscale_luma_kernel<3>,    (const void*)upscale_luma_kernel<4>,
                     (const void*)upscale_compose_kernel<1>, (const void*)upscale_compose_kernel<2>,
                     (const void*)upscale_compose_kernel<3>, (const void*)upscale_compose_kernel<4>};
  return resolve_kernels(k, 8);
}

}  // namespace srcnn
