// resize.hip -- the upscale front and back end for any output size (DESIGN.md
// 16): the resampling of upscale.hip and yuv.hip with the ratio as a fraction
// per axis instead of a template parameter,
//   resize_luma     rgba [h][w][4] u8, or Y [h][w] of one- or two-byte samples
//                   (pitched) -> bicubic luma W x H, edge-replicated into the
//                   padded plane [(H+P)][(W+P)] f32 the net reads
//   resize_compose  bicubic W x H of the source's r, g, b + the net's luma ->
//                   rgb [H][W][3] u8 (swap_luma's constants and rounding)
//   resize_planes   a frame's chroma [ph][pw] (pitched), as two planes or as
//                   one plane of (U, V) pairs -> the bicubic at the given
//                   ratios, rounded to nearest and clamped, ow x oh
// The 1-D map: the source step per output sample is rn / rd
// with 1 <= rd / rn <= 4; for output index X': n = (2X'+1) rn - rd, D = 2 rd,
// b = floor(n / D), t = (n - b D) / D; taps b-1 .. b+2 clamped to the source,
// weights keys() at t+1, t, 1-t, 2-t in double, rounded once to fp32.
//
// All kernels: one workgroup of 256 threads per tile of TX x TY outputs.  Its
// first TX + TY threads compute the tile's tap tables {b - 1, w[4]} per column
// and per row into LDS.  Because the step is at most 1, the taps of a tile
// span at most (TX + 3) x (TY + 3) source samples: that patch is staged in LDS
// (static arrays, sized for ratio 1), the horizontal pass goes into LDS with a
// thread per (patch row, output column), the vertical pass into registers.
// Nothing in this file is contracted by the compiler, keys() (keys.hpp)
// included: its doubles are the spec's, operation by operation, and the fmas
// of the two passes are the ones dot4 spells out.
#pragma clang fp contract(off)
#include "keys.hpp"
#include "common.hpp"
#include "luma.hpp"
#include "ops.hpp"
#include "samples.hpp"

namespace srcnn {
namespace {

constexpr int kThreads = 256;
// Tile geometry (64 x 32 was measured too): 64 x 16
// outputs.  A row of the tile is 256 bytes of plane floats, 192 of rgb, 64 -
// 256 of chroma; the widest kernel (resize_planes, two channels of two-byte
// samples) takes 24 KB of LDS.
constexpr int TX = 64, TY = 16;
struct Patch {
  static constexpr int PC = TX + 3, PR = TY + 3;  // the staged patch at ratio 1
  static constexpr int PCP = PC + 1;              // its LDS pitch
};
constexpr int RB = kThreads / 32;  // output rows per batch of the byte stores

// one axis: ratio rn / rd, n source samples, N outputs
struct Axis {
  uint32_t rn, rd;
  int n, N;
};

// The tap tables of a tile: for tile column c (row r) the source index of its
// first tap, b - 1 (not clamped: -2 at the least), and the four fp32 weights.
struct Taps {
  int bx[TX], by[TY];
  float4 wx[TX], wy[TY];
};

// entry of output index X (clamped to the axis by the caller)
__device__ __forceinline__ void tap_of(const Axis a, int X, int* b1, float4* w) {
  const int64_t n = (2 * (int64_t)X + 1) * a.rn - a.rd, D = 2 * (int64_t)a.rd;
  // n >= rn - rd > -D, so floor(n / D) is -1 for every negative n
  const int64_t b = n < 0 ? -1 : (int64_t)((uint64_t)n / (uint64_t)D);
  const double t = (double)(n - b * D) / (double)D;
  *b1 = (int)b - 1;
  *w = make_float4((float)keys(t + 1), (float)keys(t), (float)keys(1 - t), (float)keys(2 - t));
}

// Threads 0 .. TX-1 fill the columns, TX .. TX+TY-1 the rows.  X0, Y0: the
// tile's first output; shift: what a coordinate of the tile is moved by before
// it is clamped to the axis (the padded plane's margin, else 0).  Clamping is
// monotone, so b never decreases along the tile and never by more than the
// step: bx[TX-1] - bx[0] <= TX - 1.
__device__ __forceinline__ void fill_taps(Taps& t, const Axis ax, const Axis ay, int X0, int Y0,
                                          int shift) {
  const int tid = threadIdx.x;
  if (tid < TX)
    tap_of(ax, min(max(X0 + tid - shift, 0), ax.N - 1), &t.bx[tid], &t.wx[tid]);
  else if (tid < TX + TY)
    tap_of(ay, min(max(Y0 + tid - TX - shift, 0), ay.N - 1), &t.by[tid - TX], &t.wy[tid - TX]);
}

// w . (a, b, c, d) of both passes: one product and three fmas in this order in
// every kernel, whatever the compiler would contract, so that a semi-planar
// call gives the planar call's samples bit for bit
__device__ __forceinline__ float dot4(float4 w, float a, float b, float c, float d) {
#pragma clang fp contract(off)
  return fmaf(w.w, d, fmaf(w.z, c, fmaf(w.y, b, w.x * a)));
}

// horizontal pass over the pr patch rows the tile's taps reach: tap(r, c, ch)
// is the staged value of channel ch at patch column c, put(ch, r, x, v) stores
template <int NCH, typename Tap, typename Put>
__device__ __forceinline__ void hpass(const Taps& t, int pr, Tap tap, Put put) {
  const int x = threadIdx.x % TX;
  const int c = t.bx[x] - t.bx[0];
  const float4 w = t.wx[x];
  for (int r = threadIdx.x / TX; r < pr; r += kThreads / TX) {
#pragma unroll
    for (int ch = 0; ch < NCH; ch++)
      put(ch, r, x, dot4(w, tap(r, c, ch), tap(r, c + 1, ch), tap(r, c + 2, ch), tap(r, c + 3, ch)));
  }
}

// The luma tile: the plane is tiled in its own (padded) coordinates, X' =
// clamp(X - P/2, 0, W - 1), so the margins need no tiles of their own.
// stage(x0, y0, pc, pr, store) fetches the patch whose first sample is source
// (x0, y0); pc x pr of it are in use.
template <typename Stage>
__device__ __forceinline__ void luma_tile(float* __restrict__ out, const Axis ax, const Axis ay,
                                          int P, int tiles_x, Stage stage) {
  __shared__ Taps s_t;
  __shared__ float s_src[Patch::PR][Patch::PCP];
  __shared__ float s_h[Patch::PR][TX + 1];
  const int tid = threadIdx.x;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int X0 = tx * TX, Y0 = ty * TY, m = P / 2;
  fill_taps(s_t, ax, ay, X0, Y0, m);
  __syncthreads();
  const int x0 = s_t.bx[0], y0 = s_t.by[0];
  const int pc = s_t.bx[TX - 1] + 4 - x0, pr = s_t.by[TY - 1] + 4 - y0;  // <= TX + 3, TY + 3
  stage(x0, y0, pc, pr, [&](int r, int c, float v) { s_src[r][c] = v; });
  __syncthreads();
  hpass<1>(s_t, pr, [&](int r, int c, int) { return s_src[r][c]; },
           [&](int, int r, int x, float v) { s_h[r][x] = v; });
  __syncthreads();

  // vertical pass: 16 lanes share a row, each stores 16 bytes where the row's
  // address allows
  const int PW = ax.N + P, PH = ay.N + P;
  const int n = min(TX, PW - X0), nrow = min(TY, PH - Y0);
  constexpr int LPR = TX / 4, RPI = kThreads / LPR;
  const int l = tid % LPR;
  for (int r = tid / LPR; r < nrow; r += RPI) {
    const int rb = s_t.by[r] - y0;
    const float4 w = s_t.wy[r];
    auto val = [&](int c) { return dot4(w, s_h[rb][c], s_h[rb + 1][c], s_h[rb + 2][c], s_h[rb + 3][c]); };
    float* orow = out + (size_t)(Y0 + r) * PW + X0;
    // floats up to the first 16-byte boundary, float4 groups, the rest
    const int head = min((int)(((16 - ((uintptr_t)orow & 15)) & 15) >> 2), n);
    if (l < head) orow[l] = val(l);
    const int ng = (n - head) >> 2;  // <= TX / 4 = LPR
    if (l < ng) {
      const int c = head + 4 * l;
      *reinterpret_cast<float4*>(orow + c) = make_float4(val(c), val(c + 1), val(c + 2), val(c + 3));
    }
    const int c = head + 4 * ng + l;  // fewer than 4 floats are left
    if (c < n) orow[c] = val(c);
  }
}

__global__ __launch_bounds__(kThreads) void resize_luma_rgba_kernel(
    const uint8_t* __restrict__ rgba, float* __restrict__ out, Axis ax, Axis ay, int P, int tiles_x) {
  luma_tile(out, ax, ay, P, tiles_x, [&](int x0, int y0, int pc, int pr, auto store) {
    // one uchar4 load per pixel, consecutive lanes consecutive pixels of a row
    const int c = threadIdx.x % 128;
    if (c >= pc) return;
    const int sx = min(max(x0 + c, 0), ax.n - 1);
    for (int r = threadIdx.x / 128; r < pr; r += kThreads / 128) {
      const int sy = min(max(y0 + r, 0), ay.n - 1);
      const uchar4 p = reinterpret_cast<const uchar4*>(rgba)[(size_t)sy * ax.n + sx];
      store(r, c, luma_of((float)p.x, (float)p.y, (float)p.z));
    }
  });
}

template <int B>
__global__ __launch_bounds__(kThreads) void resize_luma_y_kernel(
    const uint8_t* __restrict__ y, size_t pitch, float* __restrict__ out, Axis ax, Axis ay, int P,
    int tiles_x, float off, float div, Fmt<B> f) {
  luma_tile(out, ax, ay, P, tiles_x, [&](int x0, int y0, int, int pr, auto store) {
    stage_samples<Patch, B, 1>(
        y, pitch, ax.n, ay.n, x0 + 2, y0 + 2,
        [&](int r, int c, int, uint32_t v) { store(r, c, luma_of_y((float)f.value(v), off, div)); }, pr);
  });
}

// One output row of a tile, nb bytes staged in LDS at the skew o its global
// address has, to global memory: bytes (B = 1) or words up to the first
// 16-byte boundary, 16-byte chunks, the rest; c5: the lane of the row's 32.
// o, nb and the row's address are multiples of B.
template <int B>
__device__ __forceinline__ void store_row(uint8_t* __restrict__ g, const uint8_t* s, int o, int nb,
                                          int c5) {
  using E = typename Sample<B>::type;
  auto copy = [&](int at) { *reinterpret_cast<E*>(g + at) = *reinterpret_cast<const E*>(s + o + at); };
  const int head = min((16 - o) & 15, nb);
  if (c5 * B < head) copy(c5 * B);
  const int nch = (nb - head) >> 4;  // <= 4 * TX / 16 = 16 of the row's 32 lanes
  if (c5 < nch)
    *reinterpret_cast<uint4*>(g + head + 16 * c5) = *reinterpret_cast<const uint4*>(s + o + head + 16 * c5);
  const int t = head + 16 * nch + c5 * B;  // fewer than 16 bytes are left
  if (t < nb) copy(t);
}

__global__ __launch_bounds__(kThreads) void resize_compose_kernel(
    const uint8_t* __restrict__ rgba, const float* __restrict__ nl, uint8_t* __restrict__ rgb, Axis ax,
    Axis ay, int tiles_x) {
  constexpr int STG = 16 + 3 * TX;  // staged row: up to 15 bytes of skew + the pixels
  __shared__ Taps s_t;
  __shared__ uchar4 s_src[Patch::PR][Patch::PCP];
  __shared__ float s_h[3][Patch::PR][TX + 1];
  __shared__ __attribute__((aligned(16))) uint8_t s_out[RB][STG];
  const int tid = threadIdx.x;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int X0 = tx * TX, Y0 = ty * TY;
  fill_taps(s_t, ax, ay, X0, Y0, 0);
  __syncthreads();
  const int x0 = s_t.bx[0], y0 = s_t.by[0];
  const int pc = s_t.bx[TX - 1] + 4 - x0, pr = s_t.by[TY - 1] + 4 - y0;  // the patch in use
  {
    const int c = tid % 128;
    if (c < pc) {
      const int sx = min(max(x0 + c, 0), ax.n - 1);
      for (int r = tid / 128; r < pr; r += kThreads / 128) {
        const int sy = min(max(y0 + r, 0), ay.n - 1);
        s_src[r][c] = reinterpret_cast<const uchar4*>(rgba)[(size_t)sy * ax.n + sx];
      }
    }
  }
  __syncthreads();
  hpass<3>(
      s_t, pr,
      [&](int r, int c, int ch) {
        const uchar4 p = s_src[r][c];
        return (float)(ch == 0 ? p.x : ch == 1 ? p.y : p.z);
      },
      [&](int ch, int r, int x, float v) { s_h[ch][r][x] = v; });
  __syncthreads();

  const int W = ax.N;
  const int ncol = min(TX, W - X0), nrow = min(TY, ay.N - Y0);
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
      const int rb = s_t.by[yb + rr] - y0;
      const float4 w = s_t.wy[yb + rr];
      const float* lrow = nl + (size_t)Y * W + X0;
#pragma unroll
      for (int i = 0; i < TX / 32; i++) {
        const int cx = c5 + 32 * i;
        if (cx < ncol) {
          auto val = [&](int ch) {
            return dot4(w, s_h[ch][rb][cx], s_h[ch][rb + 1][cx], s_h[ch][rb + 2][cx], s_h[ch][rb + 3][cx]);
          };
          compose_px(val(0), val(1), val(2), lrow[cx], &s_out[rr][o + 3 * cx]);
        }
      }
    }
    __syncthreads();
    if (live) store_row<1>(grow, s_out[rr], o, nb, c5);
    __syncthreads();
  }
}

// NCH = 1: two planes, blockIdx.y selects one.  NCH = 2: src0 / dst0 hold
// (U, V) pairs, the two channels of one pass; the axes count pairs.
template <int B, int NCH>
__global__ __launch_bounds__(kThreads) void resize_planes_kernel(
    const uint8_t* __restrict__ src0, const uint8_t* __restrict__ src1, size_t src_pitch,
    uint8_t* __restrict__ dst0, uint8_t* __restrict__ dst1, size_t dst_pitch, Axis ax, Axis ay,
    int tiles_x, Fmt<B> f) {
  using E = typename Sample<B>::type;
  constexpr int STG = 16 + TX * NCH * B;  // staged row: up to 15 bytes of skew + the samples
  __shared__ Taps s_t;
  __shared__ float s_src[NCH][Patch::PR][Patch::PCP];
  __shared__ float s_h[NCH][Patch::PR][TX + 1];
  __shared__ __attribute__((aligned(16))) uint8_t s_out[RB][STG];
  const uint8_t* __restrict__ src = NCH == 1 && blockIdx.y ? src1 : src0;
  uint8_t* __restrict__ dst = NCH == 1 && blockIdx.y ? dst1 : dst0;
  const int tid = threadIdx.x;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int X0 = tx * TX, Y0 = ty * TY;
  fill_taps(s_t, ax, ay, X0, Y0, 0);
  __syncthreads();
  const int x0 = s_t.bx[0], y0 = s_t.by[0];
  const int pr = s_t.by[TY - 1] + 4 - y0;  // patch rows in use
  stage_samples<Patch, B, NCH>(
      src, src_pitch, ax.n, ay.n, x0 + 2, y0 + 2,
      [&](int r, int c, int ch, uint32_t v) { s_src[ch][r][c] = (float)f.value(v); }, pr);
  __syncthreads();
  hpass<NCH>(s_t, pr, [&](int r, int c, int ch) { return s_src[ch][r][c]; },
             [&](int ch, int r, int x, float v) { s_h[ch][r][x] = v; });
  __syncthreads();

  const int ncol = min(TX, ax.N - X0), nrow = min(TY, ay.N - Y0);  // pixels of a row; rows
  const int nb = ncol * (NCH * B);                                 // bytes of a row
  const int c5 = tid & 31, rr = tid >> 5;
  for (int yb = 0; yb < nrow; yb += RB) {
    const bool live = yb + rr < nrow;
    uint8_t* gbytes = dst + (size_t)(Y0 + yb + rr) * dst_pitch + (size_t)X0 * (NCH * B);
    const int o = (int)((uintptr_t)gbytes & 15);  // (as in resize_compose)
    if (live) {
      const int rb = s_t.by[yb + rr] - y0;
      const float4 w = s_t.wy[yb + rr];
#pragma unroll
      for (int i = 0; i < TX / 32; i++) {
        const int cx = c5 + 32 * i;
        if (cx < ncol) {
#pragma unroll
          for (int ch = 0; ch < NCH; ch++)
            *reinterpret_cast<E*>(&s_out[rr][o + (cx * NCH + ch) * B]) =
                (E)quantise<B>(dot4(w, s_h[ch][rb][cx], s_h[ch][rb + 1][cx], s_h[ch][rb + 2][cx],
                                    s_h[ch][rb + 3][cx]),
                               f);
        }
      }
    }
    __syncthreads();
    if (live) store_row<B>(gbytes, s_out[rr], o, nb, c5);
    __syncthreads();
  }
}

uint32_t tiles(uint32_t n, int t) { return (n + t - 1) / t; }
Axis axis(uint32_t rn, uint32_t rd, uint32_t n, uint32_t N) { return Axis{rn, rd, (int)n, (int)N}; }

}  // namespace

int resize_luma(const uint8_t* rgba, float* plane, uint32_t w, uint32_t h, uint32_t W, uint32_t H,
                uint32_t pad, hipStream_t s) {
  SRCNN_PROFILE("resize_luma", s);
  const uint32_t tx = tiles(W + pad, TX), ty = tiles(H + pad, TY);
  hipLaunchKernelGGL(resize_luma_rgba_kernel, dim3(tx * ty), dim3(kThreads), 0, s, rgba, plane,
                     axis(w, W, w, W), axis(h, H, h, H), (int)pad, (int)tx);
  SRCNN_LAUNCH_TRY();
  return SRCNN_OK;
}

int resize_compose(const uint8_t* rgba, const float* nl, uint8_t* rgb, uint32_t w, uint32_t h,
                   uint32_t W, uint32_t H, hipStream_t s) {
  SRCNN_PROFILE("resize_compose", s);
  const uint32_t tx = tiles(W, TX), ty = tiles(H, TY);
  hipLaunchKernelGGL(resize_compose_kernel, dim3(tx * ty), dim3(kThreads), 0, s, rgba, nl, rgb,
                     axis(w, W, w, W), axis(h, H, h, H), (int)tx);
  SRCNN_LAUNCH_TRY();
  return SRCNN_OK;
}

int yuv_resize_luma(const void* y, uint32_t pitch_y, float* plane, uint32_t w, uint32_t h, uint32_t W,
                    uint32_t H, uint32_t pad, uint32_t bits, bool msb, bool full_range, hipStream_t s) {
  SRCNN_PROFILE("yuv_resize_luma", s);
  const uint8_t* src = static_cast<const uint8_t*>(y);
  const Range r = range_of(bits, full_range);
  const uint32_t tx = tiles(W + pad, TX), ty = tiles(H + pad, TY);
  const Axis ax = axis(w, W, w, W), ay = axis(h, H, h, H);
  if (bits == 8)
    hipLaunchKernelGGL(resize_luma_y_kernel<1>, dim3(tx * ty), dim3(kThreads), 0, s, src,
                       (size_t)pitch_y, plane, ax, ay, (int)pad, (int)tx, r.off, r.span, Fmt<1>{});
  else
    hipLaunchKernelGGL(resize_luma_y_kernel<2>, dim3(tx * ty), dim3(kThreads), 0, s, src,
                       (size_t)pitch_y, plane, ax, ay, (int)pad, (int)tx, r.off, r.span,
                       deep_fmt(bits, msb));
  SRCNN_LAUNCH_TRY();
  return SRCNN_OK;
}

int resize_planes(const void* src0, const void* src1, uint32_t src_pitch, uint32_t pw, uint32_t ph,
                  void* dst0, void* dst1, uint32_t dst_pitch, uint32_t ow, uint32_t oh, uint32_t rx_num,
                  uint32_t rx_den, uint32_t ry_num, uint32_t ry_den, uint32_t bits, bool msb,
                  bool semiplanar, hipStream_t s) {
  SRCNN_PROFILE("resize_planes", s);
  const uint8_t *a = static_cast<const uint8_t*>(src0), *b = static_cast<const uint8_t*>(src1);
  uint8_t *A = static_cast<uint8_t*>(dst0), *Bp = static_cast<uint8_t*>(dst1);
  const uint32_t tx = tiles(ow, TX), ty = tiles(oh, TY);
  const Axis ax = axis(rx_num, rx_den, pw, ow), ay = axis(ry_num, ry_den, ph, oh);
  const dim3 grid(tx * ty, semiplanar ? 1 : 2);
#define SRCNN_RESIZE_PLANES(B, F)                                                                  \
  {                                                                                                \
    const auto k = semiplanar ? resize_planes_kernel<B, 2> : resize_planes_kernel<B, 1>;           \
    hipLaunchKernelGGL(k, grid, dim3(kThreads), 0, s, a, b, (size_t)src_pitch, A, Bp,              \
                       (size_t)dst_pitch, ax, ay, (int)tx, F);                                     \
  }
  if (bits == 8) SRCNN_RESIZE_PLANES(1, Fmt<1>{})
  else SRCNN_RESIZE_PLANES(2, deep_fmt(bits, msb))
#undef SRCNN_RESIZE_PLANES
  SRCNN_LAUNCH_TRY();
  return SRCNN_OK;
}

int preload_resize() {
  const void* k[] = {(const void*)resize_luma_rgba_kernel,    (const void*)resize_luma_y_kernel<1>,
                     (const void*)resize_luma_y_kernel<2>,    (const void*)resize_compose_kernel,
                     (const void*)resize_planes_kernel<1, 1>, (const void*)resize_planes_kernel<1, 2>,
                     (const void*)resize_planes_kernel<2, 1>, (const void*)resize_planes_kernel<2, 2>};
  return resolve_kernels(k, (int)(sizeof(k) / sizeof(k[0])));
}

}  // namespace srcnn
