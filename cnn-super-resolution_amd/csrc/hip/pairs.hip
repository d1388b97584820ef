// pairs.hip -- training pairs from a full-size image on the device:
//   downscale_rgba  rgba [H][W][4] u8 -> antialiased bicubic / S, [H/S][W/S][4] u8
//                   (the inverse of upscale.hip's resampling: same Keys kernel,
//                   stretched by S, half-pixel centres, replicated edges)
//   gather_tiles    float plane [ph][pw] -> a grid of tiles [n][th][tw], each
//                   optionally minus its own mean (the batch layout
//                   srcnn_train_fwd_bwd reads)
//   gather_batch    planes + a device-side list of {plane, origin, orientation}
//                   records -> the X and T batches of one training chunk, in
//                   one launch
// The reference has no counterpart: its pairs are made on the host, one file
// per sample.  The resampling is specified in DESIGN.md 11.1.
//
// downscale_rgba: one workgroup per tile of TX x TY output pixels (struct
// Tile).  The source patch the tile's taps reach (S*(T-1) + NT per axis,
// indices clamped to the image) is fetched once with one 4-byte load per
// pixel and kept in LDS as the RGBA8 word; the horizontal pass writes the
// patch's rows of TX values per channel to LDS; the vertical pass reads NT of
// those rows per output into registers; one uchar4 store per output pixel.
// The phase is the same for every output, so every weight index is a
// compile-time value (uniform scalar loads from __constant__).
#include "common.hpp"
#include "keys_down.hpp"
#include "ops.hpp"

namespace srcnn {
namespace {

constexpr int kThreads = 256;

// (o_min, n_taps and the weight table c_down: keys_down.hpp, shared with
// yuv_down.hip)

// Tile geometry by LDS budget: 32 output pixels wide, so
// that a tile's output rows are whole 128-byte lines and its patch rows 264 -
// 560 contiguous bytes; 16 rows at S <= 2 (26 KB of LDS at S = 2: 6
// workgroups per CU), 8 at S >= 3, where the patch grows with S^2 (26 / 42 KB
// at S = 3 / 4: 6 / 3 workgroups per CU; 16 rows would be 71 KB at S = 4).
template <int S>
struct Tile {
  static constexpr int TX = 32, TY = S <= 2 ? 16 : 8;  // output pixels
  static constexpr int NT = n_taps(S), O0 = o_min(S);
  static constexpr int PC = S * (TX - 1) + NT, PR = S * (TY - 1) + NT;  // staged patch
};

template <int S>
__global__ __launch_bounds__(kThreads) void downscale_rgba_kernel(const uint8_t* __restrict__ rgba,
                                                                  uint8_t* __restrict__ small,
                                                                  int W, int H, int w, int h,
                                                                  int tiles_x) {
  using T = Tile<S>;
  constexpr int TX = T::TX, TY = T::TY, NT = T::NT, PC = T::PC, PR = T::PR;
  __shared__ uchar4 s_src[PR][PC];
  __shared__ float s_h[3][PR][TX + 1];
  const int tid = threadIdx.x;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int j0 = tx * TX, i0 = ty * TY;

  // clamped fetch of the patch: consecutive lanes consecutive pixels of a row
  const int sx0 = j0 * S + T::O0, sy0 = i0 * S + T::O0;
  for (int e = tid; e < PR * PC; e += kThreads) {
    const int r = e / PC, c = e - r * PC;
    const int sx = min(max(sx0 + c, 0), W - 1), sy = min(max(sy0 + r, 0), H - 1);
    s_src[r][c] = reinterpret_cast<const uchar4*>(rgba)[(size_t)sy * W + sx];
  }
  __syncthreads();

  // horizontal pass: patch row r, output column x -> one value per channel
  const int x = tid % TX;
  for (int r = tid / TX; r < PR; r += kThreads / TX) {
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
#pragma unroll
    for (int t = 0; t < NT; t++) {
      const uchar4 p = s_src[r][S * x + t];
      const float wt = c_down.w[S][t];
      a0 += wt * (float)p.x;
      a1 += wt * (float)p.y;
      a2 += wt * (float)p.z;
    }
    s_h[0][r][x] = a0;
    s_h[1][r][x] = a1;
    s_h[2][r][x] = a2;
  }
  __syncthreads();

  // vertical pass: NT rows per output, round to nearest, alpha 255
  const int j = j0 + x;
  if (j >= w) return;
  for (int y = tid / TX; y < TY; y += kThreads / TX) {
    const int i = i0 + y;
    if (i >= h) break;
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
#pragma unroll
    for (int t = 0; t < NT; t++) {
      const float wt = c_down.w[S][t];
      a0 += wt * s_h[0][S * y + t][x];
      a1 += wt * s_h[1][S * y + t][x];
      a2 += wt * s_h[2][S * y + t][x];
    }
    auto q = [](float v) { return (uint8_t)floorf(fminf(fmaxf(v, 0.0f), 255.0f) + 0.5f); };
    reinterpret_cast<uchar4*>(small)[(size_t)i * w + j] = make_uchar4(q(a0), q(a1), q(a2), 255);
  }
}

// gather_tiles: one workgroup per tile, of any size (nothing of the tile is
// held on chip: the second pass re-reads the plane, from cache).  The mean is
// a fixed-order sum that depends on tw x th alone: thread t adds the tile's
// elements t, t + 256, t + 512, ... (row-major within the tile) in that
// order, then the 256 partial sums meet in a binary tree: six butterfly
// levels inside each wave, two more over the four waves' sums in LDS.
template <bool SUB_MEAN>
__global__ __launch_bounds__(kThreads) void gather_tiles_kernel(
    const float* __restrict__ plane, float* __restrict__ tiles, float* __restrict__ means, int pw,
    int x0, int y0, int stride, int nx, int tw, int th) {
  __shared__ float s_part[kThreads / 64];
  const int tid = threadIdx.x;
  const int iy = blockIdx.x / nx, ix = blockIdx.x - iy * nx;
  const float* src = plane + (size_t)(y0 + iy * stride) * pw + (x0 + ix * stride);
  const uint32_t n = (uint32_t)tw * th, utw = tw;  // n <= 2^31-1: e + 256 stays below 2^32
  float mean = 0.0f;
  if (SUB_MEAN) {
    float acc = 0.0f;
    for (uint32_t e = tid; e < n; e += kThreads) {
      const uint32_t r = e / utw, c = e - r * utw;
      acc += src[(size_t)r * pw + c];
    }
    // butterfly over the wave's 64 lanes (every lane ends with the same
    // bits: a + b == b + a), then the four waves' sums as (0 + 1) + (2 + 3)
#pragma unroll
    for (int k = 32; k > 0; k >>= 1) acc += __shfl_xor(acc, k, 64);
    if ((tid & 63) == 0) s_part[tid >> 6] = acc;
    __syncthreads();
    mean = ((s_part[0] + s_part[1]) + (s_part[2] + s_part[3])) / (float)n;
    if (means && tid == 0) means[blockIdx.x] = mean;
  }
  float* dst = tiles + (size_t)blockIdx.x * n;
  for (uint32_t e = tid; e < n; e += kThreads) {
    const uint32_t r = e / utw, c = e - r * utw;
    const float v = src[(size_t)r * pw + c];
    dst[e] = SUB_MEAN ? v - mean : v;
  }
}

// gather_batch: one workgroup per record of a device-side list
// {plane, x, y, op}; the X tile (minus the footprint's mean) and the T tile
// leave through one of the eight orientations.  The footprint is sw x sh =
// tw x th, swapped when op transposes.  Its mean is gather_tiles' sum with
// (tw, th) := (sw, sh): thread t adds the footprint's elements t, t + 256, ...
// in its own row-major order whatever op says, so the loop that fetches the
// footprint is the loop that sums it.
//
// Footprints of at most kStage floats (rows padded to an odd pitch) are staged
// in LDS, X and T together, all loads in flight before the one barrier: the
// loads run along the footprint's rows, the stores along the tile's rows, and
// a transposing op turns into LDS reads at a stride of the odd pitch, which
// puts any 32 (or 64) consecutive lanes on as many different banks.  8 KB per
// plane: a 45 x 45 footprint fits, and eight workgroups a CU keep their 16 KB
// each with LDS to spare.  Larger footprints read the plane through the
// permutation, a strided read when op transposes, as gather_tiles would.
constexpr uint32_t kStage = 2048;

__device__ __forceinline__ uint32_t batch_src(uint32_t e, uint32_t tw, uint32_t sw, uint32_t sh,
                                              uint32_t op, uint32_t* b) {
  const uint32_t r = e / tw, c = e - r * tw;
  uint32_t a = op & 4 ? c : r;
  *b = op & 4 ? r : c;
  if (op & 2) a = sh - 1 - a;
  if (op & 1) *b = sw - 1 - *b;
  return a;
}

__global__ __launch_bounds__(kThreads) void gather_batch_kernel(
    const srcnn_plane_pair* __restrict__ planes, uint32_t n_planes,
    const srcnn_tile_ref* __restrict__ refs, uint32_t tw, uint32_t th, float* __restrict__ X,
    float* __restrict__ T, float* __restrict__ means) {
  __shared__ float s_x[kStage], s_t[kStage];
  __shared__ float s_part[kThreads / 64];
  const uint32_t tid = threadIdx.x;
  const uint32_t n = tw * th;  // <= 2^31-1: e + 256 stays below 2^32
  const srcnn_tile_ref ref = refs[blockIdx.x];
  float* dx = X + (size_t)blockIdx.x * n;
  float* dt = T + (size_t)blockIdx.x * n;
  const uint32_t op = ref.op;
  const uint32_t sw = op & 4 ? th : tw, sh = op & 4 ? tw : th;
  bool ok = ref.plane < n_planes && op <= 7;
  srcnn_plane_pair p = {};
  if (ok) {
    p = planes[ref.plane];
    ok = (uint64_t)ref.x + sw <= p.w && (uint64_t)ref.y + sh <= p.h;
  }
  if (!ok) {  // (uniform over the workgroup) nothing of any plane is read
    const float q = __builtin_nanf("");
    for (uint32_t e = tid; e < n; e += kThreads) dx[e] = q, dt[e] = q;
    if (means && tid == 0) means[blockIdx.x] = q;
    return;
  }
  const float* sx = p.x + (size_t)ref.y * p.x_pitch + ref.x;
  const float* st = p.t + (size_t)ref.y * p.t_pitch + ref.x;
  const uint32_t lp = sw | 1;  // LDS row pitch: odd
  const bool staged = (uint64_t)sh * lp <= kStage;

  float acc = 0.0f;
  if (staged) {
    for (uint32_t e = tid; e < n; e += kThreads) {
      const uint32_t r = e / sw, c = e - r * sw;
      const float v = sx[(size_t)r * p.x_pitch + c];
      s_t[r * lp + c] = st[(size_t)r * p.t_pitch + c];
      s_x[r * lp + c] = v;
      acc += v;
    }
  } else {
    for (uint32_t e = tid; e < n; e += kThreads) {
      const uint32_t r = e / sw, c = e - r * sw;
      acc += sx[(size_t)r * p.x_pitch + c];
    }
  }
  // gather_tiles' tree: the butterfly over the wave, then (0 + 1) + (2 + 3)
#pragma unroll
  for (int k = 32; k > 0; k >>= 1) acc += __shfl_xor(acc, k, 64);
  if ((tid & 63) == 0) s_part[tid >> 6] = acc;
  __syncthreads();  // (also: the staged footprints are complete)
  const float mean = ((s_part[0] + s_part[1]) + (s_part[2] + s_part[3])) / (float)n;
  if (means && tid == 0) means[blockIdx.x] = mean;

  if (staged) {
    for (uint32_t e = tid; e < n; e += kThreads) {
      uint32_t b;
      const uint32_t a = batch_src(e, tw, sw, sh, op, &b);
      dx[e] = s_x[a * lp + b] - mean;
      dt[e] = s_t[a * lp + b];
    }
  } else {
    for (uint32_t e = tid; e < n; e += kThreads) {
      uint32_t b;
      const uint32_t a = batch_src(e, tw, sw, sh, op, &b);
      dx[e] = sx[(size_t)a * p.x_pitch + b] - mean;
      dt[e] = st[(size_t)a * p.t_pitch + b];
    }
  }
}

}  // namespace

int downscale_rgba(const uint8_t* rgba, uint8_t* small, uint32_t W, uint32_t H, uint32_t scale,
                   hipStream_t s) {
  SRCNN_PROFILE("downscale_rgba", s);
  const uint32_t w = W / scale, h = H / scale;
#define SRCNN_DOWN(S)                                                                           \
  {                                                                                             \
    const uint32_t tx = (w + Tile<S>::TX - 1) / Tile<S>::TX, ty = (h + Tile<S>::TY - 1) / Tile<S>::TY; \
    hipLaunchKernelGGL(downscale_rgba_kernel<S>, dim3(tx* ty), dim3(kThreads), 0, s, rgba, small, \
                       (int)W, (int)H, (int)w, (int)h, (int)tx);                                \
  }
  switch (scale) {
    case 1: SRCNN_DOWN(1); break;
    case 2: SRCNN_DOWN(2); break;
    case 3: SRCNN_DOWN(3); break;
    case 4: SRCNN_DOWN(4); break;
    default: return fail(SRCNN_ERR_INVALID, "downscale_rgba: scale %u has no kernel", scale);
  }
#undef SRCNN_DOWN
  SRCNN_LAUNCH_TRY();
  return SRCNN_OK;
}

int gather_tiles(const float* plane, uint32_t pw, uint32_t x0, uint32_t y0, uint32_t stride,
                 uint32_t nx, uint32_t ny, uint32_t tw, uint32_t th, int sub_mean, float* tiles,
                 float* means, hipStream_t s) {
  SRCNN_PROFILE("gather_tiles", s);
  if (sub_mean)
    hipLaunchKernelGGL(gather_tiles_kernel<true>, dim3(nx * ny), dim3(kThreads), 0, s, plane, tiles,
                       means, (int)pw, (int)x0, (int)y0, (int)stride, (int)nx, (int)tw, (int)th);
  else
    hipLaunchKernelGGL(gather_tiles_kernel<false>, dim3(nx * ny), dim3(kThreads), 0, s, plane, tiles,
                       means, (int)pw, (int)x0, (int)y0, (int)stride, (int)nx, (int)tw, (int)th);
  SRCNN_LAUNCH_TRY();
  return SRCNN_OK;
}

int gather_batch(const srcnn_plane_pair* planes, uint32_t n_planes, const srcnn_tile_ref* refs,
                 uint32_t n, uint32_t tw, uint32_t th, float* X, float* T, float* means,
                 hipStream_t s) {
  SRCNN_PROFILE("gather_batch", s);
  // one workgroup per record; a grid holds at most 2^31-1 of them
  const uint32_t kMaxGrid = 0x7fffffffu;
  const size_t tile = (size_t)tw * th;
  for (uint32_t i = 0; i < n;) {
    const uint32_t m = n - i < kMaxGrid ? n - i : kMaxGrid;
    hipLaunchKernelGGL(gather_batch_kernel, dim3(m), dim3(kThreads), 0, s, planes, n_planes, refs + i,
                       tw, th, X + i * tile, T + i * tile, means ? means + i : nullptr);
    SRCNN_LAUNCH_TRY();
    i += m;
  }
  return SRCNN_OK;
}

int preload_pairs() {
  const void* k[] = {(const void*)downscale_rgba_kernel<1>, (const void*)downscale_rgba_kernel<2>,
                     (const void*)downscale_rgba_kernel<3>, (const void*)downscale_rgba_kernel<4>,
                     (const void*)gather_tiles_kernel<true>, (const void*)gather_tiles_kernel<false>,
                     (const void*)gather_batch_kernel};
  return resolve_kernels(k, 7);
}

}  // namespace srcnn
