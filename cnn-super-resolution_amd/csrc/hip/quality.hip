// quality.hip -- PSNR and SSIM of two images on the device:
//   quality_tiles  two images (RGB8 / RGBA8 / normalised f32 luma, each with
//                  its own pitch) -> per workgroup two doubles: the sum of its
//                  windows' SSIM values and of its owned pixels' squared luma
//                  differences
//   quality_final  those partials, added in a fixed order -> {mse, psnr, ssim}
// and of two Y'CbCr frames of any srcnn_yuv_format:
//   quality_frame_tiles   quality_tiles on two Y planes of 8- or 16-bit
//                         samples: the same tile body behind another loader;
//                         the squared differences are integers of the code
//                         values, summed in a 64-bit integer
//   quality_frame_chroma  the integer squared-difference sums of both chroma
//                         planes, planar or semi-planar, one per workgroup
//   quality_frame_final   all partials -> the 8 doubles of srcnn_quality_frame
// The reference has no metric code; the metrics are specified in DESIGN.md
// 12.1 and 17.1.
//
// quality_tiles: one workgroup per tile of TX x TY windows of the SSIM map
// (valid placement: window (i, j) covers pixels j .. j+10, i .. i+10).  The
// (TX+10) x (TY+10) pixels the tile's windows reach are fetched once, luma
// formed on load and centred (- 128), and kept in LDS for both images;
// positions past the image hold 0 and feed only windows that do not exist.
// The horizontal pass writes TY+10 rows of TX values of the five planes
// (xa, xb, xa*xa, xb*xb, xa*xb) to LDS, every tap one fma; in the vertical pass a thread owns
// one column and kOut vertically adjacent windows, which share kOut+10 rows:
// per plane those rows are read once into registers and slid over, 3.5 LDS
// reads per window and plane instead of 11.  A tile owns the pixels at its
// windows' centres, edge tiles the 5-pixel rim besides, so every pixel's
// squared difference is added exactly once.  Both sums are doubles: each
// thread adds its own values in a fixed order, a butterfly joins the wave's
// 64 lanes, and the four waves' sums are added in order.  Which thread adds
// what depends on the window's size alone, never on the pitches, the formats
// or what lies around the window.
#include <cmath>

#include "common.hpp"
#include "luma.hpp"
#include "ops.hpp"

namespace srcnn {
namespace {

constexpr int kThreads = 256;
constexpr int kWin = 11, kHalo = kWin - 1, kRim = kWin / 2;
// Tile geometry: 32 x 32 windows, i.e. one column and kOut = 4
// rows per thread; 42 x 42 staged pixels per image, 41 KB of LDS in all
// (three workgroups per CU)
constexpr int TX = 32, TY = 32, kOut = 4;
constexpr int PC = TX + kHalo, PR = TY + kHalo;
static_assert(TX * (TY / kOut) == kThreads, "one column and kOut rows per thread");

// the 11-tap Gaussian window, sigma = 1.5: g[i] = exp(-(i-5)^2 / 4.5) / sum,
// computed in double and rounded once to fp32 (tests/test_quality_cpu.py
// checks these constants against the formula)
__constant__ float c_gauss[kWin] = {
    0.00102838012f, 0.00759875821f, 0.0360007733f, 0.109360687f, 0.213005543f, 0.266011715f,
    0.213005543f, 0.109360687f, 0.0360007733f, 0.00759875821f, 0.00102838012f};

// luma on the 0 - 255 scale of pixel `i` (row-major offset in pixels) of an
// image of format FMT; the RGB8 loader reads single bytes, whatever the
// alignment of the base.  Contraction is off: Y = 255.0f * v is a rounded
// product of its own.  Left to -ffp-contract=fast it fused into its uses, and
// differently for the two images (Ya - Yb became an fma on b's product, so
// that xb came from the unrounded 255 v and xa from the rounded one: two
// identical planes then scored 1.0000001).
template <int FMT>
__device__ __forceinline__ float load_luma(const void* __restrict__ img, size_t i) {
#pragma clang fp contract(off)
  if (FMT == SRCNN_PIX_RGBA8) {
    const uchar4 p = reinterpret_cast<const uchar4*>(img)[i];
    return luma255_of((float)p.x, (float)p.y, (float)p.z);
  } else if (FMT == SRCNN_PIX_RGB8) {
    const uint8_t* p = reinterpret_cast<const uint8_t*>(img) + 3 * i;
    return luma255_of((float)p[0], (float)p[1], (float)p[2]);
  } else {
    return 255.0f * reinterpret_cast<const float*>(img)[i];
  }
}

// one window's SSIM from its five filtered values.  Contraction is off so
// that the operands are formed the same way in a and b: for identical images
// (ma == mb, saa == sbb == sab bit for bit) numerator and denominator are the
// same two factors and the quotient is exactly 1
__device__ __forceinline__ float ssim_of(float ma, float mb, float saa, float sbb, float sab) {
#pragma clang fp contract(off)
  const float C1 = (0.01f * 255.0f) * (0.01f * 255.0f), C2 = (0.03f * 255.0f) * (0.03f * 255.0f);
  const float va = saa - ma * ma, vb = sbb - mb * mb, cab = sab - ma * mb;
  const float Ma = ma + 128.0f, Mb = mb + 128.0f;
  const float num = (2.0f * (Ma * Mb) + C1) * (2.0f * cab + C2);
  const float den = ((Ma * Ma + Mb * Mb) + C1) * ((va + vb) + C2);
  return num / den;
}

// sum over the workgroup, as gather_tiles (pairs.hip) forms it: six butterfly
// levels inside each wave (a + b == b + a, so every lane ends with the same
// bits), then the four waves' sums in order; every thread returns the same bits
template <typename T>
__device__ __forceinline__ T block_sum(T v, T* s_part) {
#pragma unroll
  for (int k = 32; k > 0; k >>= 1) v += __shfl_xor(v, k, 64);
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((s_part[0] + s_part[1]) + s_part[2]) + s_part[3];
}

// The two images of a tile body: load() gives the lumas of pixel (px, py) on
// the 0 - 255 scale and, for a pixel the tile owns, adds its squared
// difference to `sq`.
// Two images of SRCNN_PIX_* formats; a, b: the window's first pixel; pitches
// in pixels; the square is formed in fp32 and summed in double
template <int FA, int FB>
struct PixelPair {
  using Sum = double;
  const void* __restrict__ a;
  const void* __restrict__ b;
  int pitch_a, pitch_b;
  __device__ __forceinline__ void load(int px, int py, bool own, float& Ya, float& Yb, Sum& sq) const {
    Ya = load_luma<FA>(a, (size_t)py * pitch_a + px);
    Yb = load_luma<FB>(b, (size_t)py * pitch_b + px);
    if (own) {
      const float d = Ya - Yb;
      sq += (double)(d * d);
    }
  }
};
// Two Y planes of samples T (uint8_t, or uint16_t with the code in the bits
// above shift_*); a, b: the window's first sample; pitches in
// bytes.  The luma is the code times to8 = 2^-(bits-8), exact in fp32; the
// square is the integer (xa - xb)^2 < 2^32
template <typename T>
struct SamplePair {
  using Sum = unsigned long long;
  const uint8_t* __restrict__ a;
  const uint8_t* __restrict__ b;
  uint32_t pitch_a, pitch_b;
  int shift_a, shift_b;
  float to8;
  __device__ __forceinline__ void load(int px, int py, bool own, float& Ya, float& Yb, Sum& sq) const {
    const uint32_t xa = (uint32_t)reinterpret_cast<const T*>(a + (size_t)py * pitch_a)[px] >> shift_a;
    const uint32_t xb = (uint32_t)reinterpret_cast<const T*>(b + (size_t)py * pitch_b)[px] >> shift_b;
    if (own) {
      const uint32_t d = xa > xb ? xa - xb : xb - xa;
      sq += d * d;
    }
    Ya = (float)xa * to8;
    Yb = (float)xb * to8;
  }
};

// a workgroup's two sums side by side: the SSIM sum, a double, then the sum of
// squared differences, a double or a 64-bit integer in the same 8 bytes
__device__ __forceinline__ void store_sums(double* __restrict__ p, double ss, double sq) {
  p[0] = ss;
  p[1] = sq;
}
__device__ __forceinline__ void store_sums(double* __restrict__ p, double ss, unsigned long long sq) {
  p[0] = ss;
  reinterpret_cast<unsigned long long*>(p)[1] = sq;
}

// the tile of blockIdx.x of a Ws x Hs window of `pair`'s two images
template <typename Pair>
__device__ __forceinline__ void quality_tile(const Pair& pair, int Ws, int Hs, int tiles_x,
                                             double* __restrict__ partial) {
  using Sum = typename Pair::Sum;
  __shared__ float s_a[PR][PC], s_b[PR][PC];
  __shared__ float s_h[5][PR][TX];
  __shared__ double s_part[kThreads / 64];
  __shared__ Sum s_part_sq[kThreads / 64];
  const int tid = threadIdx.x;
  const int tiles_y = gridDim.x / tiles_x;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int X0 = tx * TX, Y0 = ty * TY;

  // the pixels this tile owns, in staged coordinates
  const int oc0 = tx == 0 ? 0 : kRim, oc1 = tx == tiles_x - 1 ? Ws - X0 : TX + kRim;
  const int or0 = ty == 0 ? 0 : kRim, or1 = ty == tiles_y - 1 ? Hs - Y0 : TY + kRim;

  // stage: consecutive lanes consecutive pixels of a row
  Sum sq = 0;
  for (int e = tid; e < PR * PC; e += kThreads) {
    const int r = e / PC, c = e - r * PC;
    const int px = X0 + c, py = Y0 + r;
    float xa = 0.0f, xb = 0.0f;
    if (px < Ws && py < Hs) {
      float Ya, Yb;
      pair.load(px, py, c >= oc0 && c < oc1 && r >= or0 && r < or1, Ya, Yb, sq);
      xa = Ya - 128.0f;
      xb = Yb - 128.0f;
    }
    s_a[r][c] = xa;
    s_b[r][c] = xb;
  }
  __syncthreads();

  // horizontal pass: staged row r, window column x, taps in ascending order.
  // Every tap of both passes is an explicit fma: left to -ffp-contract=fast
  // the compiler fused the taps of the five planes differently (four planes
  // as packed fmas, xa*xb's partly as products and adds), and identical
  // images then scored 1 + 1e-7 in some windows; with one fixed form the five
  // planes of identical images are the same bits and the quotient is 1
  for (int p = tid; p < PR * TX; p += kThreads) {
    const int r = p / TX, x = p - r * TX;
    float ha = 0.0f, hb = 0.0f, haa = 0.0f, hbb = 0.0f, hab = 0.0f;
#pragma unroll
    for (int t = 0; t < kWin; t++) {
      const float g = c_gauss[t], va = s_a[r][x + t], vb = s_b[r][x + t];
      const float aa = va * va, bb = vb * vb, ab = va * vb;  // each product rounded once
      ha = fmaf(g, va, ha);
      hb = fmaf(g, vb, hb);
      haa = fmaf(g, aa, haa);
      hbb = fmaf(g, bb, hbb);
      hab = fmaf(g, ab, hab);
    }
    s_h[0][r][x] = ha;
    s_h[1][r][x] = hb;
    s_h[2][r][x] = haa;
    s_h[3][r][x] = hbb;
    s_h[4][r][x] = hab;
  }
  __syncthreads();

  // vertical pass: column x, windows y0 .. y0 + kOut - 1 from rows y0 .. y0 + kOut + 9
  const int x = tid % TX, y0 = (tid / TX) * kOut;
  float f[5][kOut];
#pragma unroll
  for (int pl = 0; pl < 5; pl++) {
    float v[kOut + kHalo];
#pragma unroll
    for (int i = 0; i < kOut + kHalo; i++) v[i] = s_h[pl][y0 + i][x];
#pragma unroll
    for (int k = 0; k < kOut; k++) {
      float acc = 0.0f;
#pragma unroll
      for (int t = 0; t < kWin; t++) acc = fmaf(c_gauss[t], v[k + t], acc);
      f[pl][k] = acc;
    }
  }
  const int nwx = Ws - kHalo, nwy = Hs - kHalo;  // windows of the map
  double ss = 0.0;
#pragma unroll
  for (int k = 0; k < kOut; k++) {
    const float s = ssim_of(f[0][k], f[1][k], f[2][k], f[3][k], f[4][k]);
    if (X0 + x < nwx && Y0 + y0 + k < nwy) ss += (double)s;
  }

  ss = block_sum(ss, s_part);
  sq = block_sum(sq, s_part_sq);
  if (tid == 0) store_sums(partial + 2 * (size_t)blockIdx.x, ss, sq);
}

// a, b: the window's first pixel; Ws x Hs: the window; pitches in pixels
template <int FA, int FB>
__global__ __launch_bounds__(kThreads) void quality_tiles_kernel(
    const void* __restrict__ a, const void* __restrict__ b, int pitch_a, int pitch_b, int Ws, int Hs,
    int tiles_x, double* __restrict__ partial) {
  quality_tile(PixelPair<FA, FB>{a, b, pitch_a, pitch_b}, Ws, Hs, tiles_x, partial);
}

// One side of srcnn_quality_frame as the kernels take it: the first samples of
// the shaved windows of its planes (c1: the second chroma plane, or c0 again
// for a semi-planar frame), pitches in bytes; chroma sample (r, c) of plane p
// is element c * stride + p * off of row r; a code is its word >> shift
struct FrameSide {
  const uint8_t *y, *c0, *c1;
  uint32_t pitch_y, pitch_c;
  int stride, off, shift;
};

template <typename T>
__global__ __launch_bounds__(kThreads) void quality_frame_tiles_kernel(FrameSide a, FrameSide b, float to8,
                                                                       int Ws, int Hs, int tiles_x,
                                                                       double* __restrict__ partial) {
  quality_tile(SamplePair<T>{a.y, b.y, a.pitch_y, b.pitch_y, a.shift, b.shift, to8}, Ws, Hs, tiles_x, partial);
}

// Chroma: blockIdx.y is the plane, blockIdx.x a tile of CTX columns x CTY rows
// of its CWs x CHs window; a thread owns one column of the tile, so consecutive
// lanes read consecutive samples of a row.  partial [2][gridDim.x]
constexpr int CTX = kThreads, CTY = 16;
template <typename T>
__global__ __launch_bounds__(kThreads) void quality_frame_chroma_kernel(
    FrameSide a, FrameSide b, int CWs, int CHs, int tiles_x, unsigned long long* __restrict__ partial) {
  __shared__ unsigned long long s_part[kThreads / 64];
  const int plane = blockIdx.y;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int c = tx * CTX + (int)threadIdx.x;
  const int r0 = ty * CTY, r1 = min(r0 + CTY, CHs);
  const uint8_t* __restrict__ pa = plane ? a.c1 : a.c0;
  const uint8_t* __restrict__ pb = plane ? b.c1 : b.c0;
  const int ea = c * a.stride + plane * a.off, eb = c * b.stride + plane * b.off;
  unsigned long long sq = 0;
  if (c < CWs) {
    for (int r = r0; r < r1; r++) {
      const uint32_t xa = (uint32_t)reinterpret_cast<const T*>(pa + (size_t)r * a.pitch_c)[ea] >> a.shift;
      const uint32_t xb = (uint32_t)reinterpret_cast<const T*>(pb + (size_t)r * b.pitch_c)[eb] >> b.shift;
      const uint32_t d = xa > xb ? xa - xb : xb - xa;
      sq += d * d;
    }
  }
  sq = block_sum(sq, s_part);
  if (threadIdx.x == 0) partial[(size_t)plane * gridDim.x + blockIdx.x] = sq;
}

// one workgroup: thread t adds the partials t, t + 256, ... in that order,
// then the 256 sums meet as in quality_tiles
__global__ __launch_bounds__(kThreads) void quality_final_kernel(const double* __restrict__ partial,
                                                                 uint32_t n, double pixels,
                                                                 double windows,
                                                                 double* __restrict__ result) {
  __shared__ double s_part[2][kThreads / 64];
  double ss = 0.0, sq = 0.0;
  for (uint32_t i = threadIdx.x; i < n; i += kThreads) {
    ss += partial[2 * (size_t)i];
    sq += partial[2 * (size_t)i + 1];
  }
  ss = block_sum(ss, s_part[0]);
  sq = block_sum(sq, s_part[1]);
  if (threadIdx.x == 0) {
    const double mse = sq / pixels;
    result[0] = mse;
    result[1] = mse == 0.0 ? (double)INFINITY : 10.0 * log10(65025.0 / mse);
    result[2] = ss / windows;
  }
}

__device__ __forceinline__ double psnr_of(double peak2, double mse) {
  return mse == 0.0 ? (double)INFINITY : 10.0 * log10(peak2 / mse);
}

// one workgroup: the n luma partials as quality_final adds them (the SSIM sums
// in its order; the integer sums have none), the nc chroma partials of each
// plane likewise -> {mse_y, psnr_y, ssim_y, mse_u, psnr_u, mse_v, psnr_v,
// psnr_all}; Ny, Nc: the samples of the luma window and of one chroma window
__global__ __launch_bounds__(kThreads) void quality_frame_final_kernel(
    const double* __restrict__ partial, uint32_t n, const unsigned long long* __restrict__ cpartial,
    uint32_t nc, uint32_t Ny, uint32_t Nc, double windows, double peak2, double* __restrict__ result) {
  __shared__ double s_part[kThreads / 64];
  __shared__ unsigned long long s_part_sq[3][kThreads / 64];
  double ss = 0.0;
  unsigned long long sy = 0, su = 0, sv = 0;
  for (uint32_t i = threadIdx.x; i < n; i += kThreads) {
    ss += partial[2 * (size_t)i];
    sy += reinterpret_cast<const unsigned long long*>(partial)[2 * (size_t)i + 1];
  }
  for (uint32_t i = threadIdx.x; i < nc; i += kThreads) {
    su += cpartial[i];
    sv += cpartial[(size_t)nc + i];
  }
  ss = block_sum(ss, s_part);
  sy = block_sum(sy, s_part_sq[0]);
  su = block_sum(su, s_part_sq[1]);
  sv = block_sum(sv, s_part_sq[2]);
  if (threadIdx.x == 0) {
    const double mse_y = (double)sy / (double)Ny, mse_u = (double)su / (double)Nc, mse_v = (double)sv / (double)Nc;
    const double mse_all = (((double)sy + (double)su) + (double)sv) / (double)((unsigned long long)Ny + Nc + Nc);
    result[0] = mse_y;
    result[1] = psnr_of(peak2, mse_y);
    result[2] = ss / windows;
    result[3] = mse_u;
    result[4] = psnr_of(peak2, mse_u);
    result[5] = mse_v;
    result[6] = psnr_of(peak2, mse_v);
    result[7] = psnr_of(peak2, mse_all);
  }
}

template <int FA>
void* tiles_kernel_of(int fb) {
  switch (fb) {
    case SRCNN_PIX_LUMA_F32: return (void*)quality_tiles_kernel<FA, SRCNN_PIX_LUMA_F32>;
    case SRCNN_PIX_RGB8: return (void*)quality_tiles_kernel<FA, SRCNN_PIX_RGB8>;
    case SRCNN_PIX_RGBA8: return (void*)quality_tiles_kernel<FA, SRCNN_PIX_RGBA8>;
  }
  return nullptr;
}
void* tiles_kernel_of(int fa, int fb) {
  switch (fa) {
    case SRCNN_PIX_LUMA_F32: return tiles_kernel_of<SRCNN_PIX_LUMA_F32>(fb);
    case SRCNN_PIX_RGB8: return tiles_kernel_of<SRCNN_PIX_RGB8>(fb);
    case SRCNN_PIX_RGBA8: return tiles_kernel_of<SRCNN_PIX_RGBA8>(fb);
  }
  return nullptr;
}

}  // namespace

uint64_t quality_tile_count(uint32_t Ws, uint32_t Hs) {
  const uint64_t tx = ((uint64_t)Ws - kHalo + TX - 1) / TX, ty = ((uint64_t)Hs - kHalo + TY - 1) / TY;
  return tx * ty;
}

int quality(const void* a, int fmt_a, uint32_t pitch_a, const void* b, int fmt_b, uint32_t pitch_b,
            uint32_t Ws, uint32_t Hs, double* result, double* partial, hipStream_t s) {
  SRCNN_PROFILE("quality", s);
  void* kernel = tiles_kernel_of(fmt_a, fmt_b);
  if (!kernel) return fail(SRCNN_ERR_INVALID, "quality: formats %d / %d have no kernel", fmt_a, fmt_b);
  int pa = (int)pitch_a, pb = (int)pitch_b, ws = (int)Ws, hs = (int)Hs;
  int tiles_x = (int)((Ws - kHalo + TX - 1) / TX);
  const uint32_t n = (uint32_t)quality_tile_count(Ws, Hs);
  void* args[] = {&a, &b, &pa, &pb, &ws, &hs, &tiles_x, &partial};
  SRCNN_HIP_TRY(hipLaunchKernel(kernel, dim3(n), dim3(kThreads), args, 0, s));
  hipLaunchKernelGGL(quality_final_kernel, dim3(1), dim3(kThreads), 0, s, (const double*)partial, n,
                     (double)Ws * Hs, (double)(Ws - kHalo) * (Hs - kHalo), result);
  SRCNN_LAUNCH_TRY();
  return SRCNN_OK;
}

uint64_t quality_chroma_tile_count(uint32_t CWs, uint32_t CHs) {
  return (((uint64_t)CWs + CTX - 1) / CTX) * (((uint64_t)CHs + CTY - 1) / CTY);
}

namespace {
template <typename T>
int quality_frame_of(const FrameSide& a, const FrameSide& b, uint32_t bits, uint32_t Ws, uint32_t Hs,
                     uint32_t CWs, uint32_t CHs, double* result, void* ws, hipStream_t s) {
  const uint32_t n = (uint32_t)quality_tile_count(Ws, Hs), nc = (uint32_t)quality_chroma_tile_count(CWs, CHs);
  double* partial = static_cast<double*>(ws);
  unsigned long long* cpartial = reinterpret_cast<unsigned long long*>(partial + 2 * (size_t)n);
  const int tiles_x = (int)((Ws - kHalo + TX - 1) / TX), ctiles_x = (int)((CWs + CTX - 1) / CTX);
  const double peak = (double)((1u << bits) - 1);
  hipLaunchKernelGGL(quality_frame_tiles_kernel<T>, dim3(n), dim3(kThreads), 0, s, a, b,
                     ldexpf(1.0f, 8 - (int)bits), (int)Ws, (int)Hs, tiles_x, partial);
  SRCNN_LAUNCH_TRY();
  hipLaunchKernelGGL(quality_frame_chroma_kernel<T>, dim3(nc, 2), dim3(kThreads), 0, s, a, b, (int)CWs,
                     (int)CHs, ctiles_x, cpartial);
  SRCNN_LAUNCH_TRY();
  hipLaunchKernelGGL(quality_frame_final_kernel, dim3(1), dim3(kThreads), 0, s, (const double*)partial, n,
                     (const unsigned long long*)cpartial, nc, Ws * Hs, CWs * CHs,
                     (double)(Ws - kHalo) * (Hs - kHalo), peak * peak, result);
  SRCNN_LAUNCH_TRY();
  return SRCNN_OK;
}
}  // namespace

int quality_frame(const QualityFrameSide& a, const QualityFrameSide& b, uint32_t bits, uint32_t Ws,
                  uint32_t Hs, uint32_t CWs, uint32_t CHs, double* result, void* ws, hipStream_t s) {
  SRCNN_PROFILE("quality_frame", s);
  const auto side = [bits](const QualityFrameSide& f) {
    const uint8_t* c0 = static_cast<const uint8_t*>(f.c0);
    return FrameSide{static_cast<const uint8_t*>(f.y), c0, f.semiplanar ? c0 : static_cast<const uint8_t*>(f.c1),
                     f.pitch_y, f.pitch_c, f.semiplanar ? 2 : 1, f.semiplanar ? 1 : 0,
                     f.msb ? 16 - (int)bits : 0};
  };
  return bits == 8 ? quality_frame_of<uint8_t>(side(a), side(b), bits, Ws, Hs, CWs, CHs, result, ws, s)
                   : quality_frame_of<uint16_t>(side(a), side(b), bits, Ws, Hs, CWs, CHs, result, ws, s);
}

int preload_quality() {
  const int fmts[3] = {SRCNN_PIX_LUMA_F32, SRCNN_PIX_RGB8, SRCNN_PIX_RGBA8};
  const void* k[15];
  int n = 0;
  for (int fa : fmts)
    for (int fb : fmts) k[n++] = tiles_kernel_of(fa, fb);
  k[n++] = (const void*)quality_final_kernel;
  k[n++] = (const void*)quality_frame_tiles_kernel<uint8_t>;
  k[n++] = (const void*)quality_frame_tiles_kernel<uint16_t>;
  k[n++] = (const void*)quality_frame_chroma_kernel<uint8_t>;
  k[n++] = (const void*)quality_frame_chroma_kernel<uint16_t>;
  k[n++] = (const void*)quality_frame_final_kernel;
  return resolve_kernels(k, n);
}

}  // namespace srcnn
