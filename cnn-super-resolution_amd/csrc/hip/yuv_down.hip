// yuv_down.hip -- the planes of a Y'CbCr frame made smaller on the device
// (DESIGN.md 18), the down direction's counterpart of yuv.hip's upscale_planes:
//   downscale_planes   one or two planes [ph][pw] (pitched), or one plane of
//                      (U, V) pairs -> the antialiased Keys bicubic / S of
//                      the code values, rounded to nearest (ties to even) and
//                      clamped, [oh][ow] in the same layout (pitched), with
//                      ow <= ceil(pw / S), oh <= ceil(ph / S)
// A sample is one byte, or a 16-bit word that holds 9 to 16 bits in its low or
// in its high bits (template parameter B: bytes per sample; struct Fmt,
// samples.hpp).  The resampling is pairs.hip's downscale_rgba (DESIGN.md 11.1;
// keys_down.hpp holds the taps and the weight table the two files share): one
// workgroup per tile of output samples, the source patch its taps reach staged
// once in LDS as floats (aligned words of four samples wherever a word lies
// inside the row, clamped single samples at the plane's edges: stage_samples),
// a horizontal pass into LDS, a vertical pass of NT rows per output into
// registers.  The phase is the same for every output, so every weight index is
// a compile-time value.  Output rows leave as upscale_planes' do: quantised
// into an LDS row at the byte skew of their global address, then stored as
// head samples, 16-byte chunks and a tail.
#include "common.hpp"
#include "keys_down.hpp"
#include "ops.hpp"
#include "samples.hpp"

namespace srcnn {
namespace {

constexpr int kThreads = 256;

// Tile geometry by LDS budget: a tile row is 32 output
// samples, one per lane of half a wavefront (32 pixels of a plane, or 16 (U, V)
// pairs kept interleaved, so that the two layouts stage the same number of
// floats); 16 rows at S <= 2, 8 at S >= 3, where the patch grows with S^2.
template <int S, int NCH>
struct DownTile {
  static constexpr int TE = 32;                               // output samples of a tile row
  static constexpr int TX = TE / NCH, TY = S <= 2 ? 16 : 8;   // output pixels
  static constexpr int NT = n_taps(S), O0 = o_min(S);
  static constexpr int PC = S * (TX - 1) + NT, PR = S * (TY - 1) + NT;  // staged patch, pixels
  static constexpr int PCP = PC * NCH + 1;                    // its LDS pitch, floats
};

// NCH = 1: one or two planes, blockIdx.y selects one.  NCH = 2: src0 / dst0
// hold (U, V) pairs; pw, ow and the tile count pairs.
template <int S, int B, int NCH>
__global__ __launch_bounds__(kThreads) void downscale_planes_kernel(
    const uint8_t* __restrict__ src0, const uint8_t* __restrict__ src1, size_t src_pitch, int pw,
    int ph, uint8_t* __restrict__ dst0, uint8_t* __restrict__ dst1, size_t dst_pitch, int ow, int oh,
    int tiles_x, Fmt<B> f) {
  using T = DownTile<S, NCH>;
  using E = typename Sample<B>::type;
  constexpr int TE = T::TE, TX = T::TX, TY = T::TY, NT = T::NT, PR = T::PR;
  constexpr int RB = kThreads / TE;  // rows per batch
  constexpr int STG = 16 + TE * B;   // staged row: up to 15 bytes of skew + the samples
  __shared__ float s_src[PR][T::PCP];  // [row][pixel * NCH + channel]
  __shared__ float s_h[PR][TE + 1];
  __shared__ __attribute__((aligned(16))) uint8_t s_out[RB][STG];
  const uint8_t* __restrict__ src = NCH == 1 && blockIdx.y ? src1 : src0;
  uint8_t* __restrict__ dst = NCH == 1 && blockIdx.y ? dst1 : dst0;
  const int tid = threadIdx.x;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int X0 = tx * TX, Y0 = ty * TY;

  // the patch from (S*X0 + O0, S*Y0 + O0), clamped to the plane (stage_samples
  // counts from two pixels before its origin)
  stage_samples<T, B, NCH>(src, src_pitch, pw, ph, S * X0 + T::O0 + 2, S * Y0 + T::O0 + 2,
                           [&](int r, int c, int ch, uint32_t v) {
                             s_src[r][c * NCH + ch] = (float)f.value(v);
                           });
  __syncthreads();

  // horizontal pass: patch row r, output sample e (pixel e / NCH, channel e % NCH)
  const int e = tid % TE, rr = tid / TE;
  const int cb = S * (e / NCH) * NCH + e % NCH;
  for (int r = rr; r < PR; r += RB) {
    float a = 0.0f;
#pragma unroll
    for (int t = 0; t < NT; t++) a += c_down.w[S][t] * s_src[r][cb + t * NCH];
    s_h[r][e] = a;
  }
  __syncthreads();

  // the tile's share of the ow x oh output
  const int ncol = min(TX, ow - X0), nrow = min(TY, oh - Y0);  // pixels of a row; rows
  const int ne = ncol * NCH, nb = ne * B;                      // samples, bytes of a row
  for (int yb = 0; yb < nrow; yb += RB) {
    const bool live = yb + rr < nrow;
    const int y = yb + rr;
    uint8_t* gbytes = dst + (size_t)(Y0 + y) * dst_pitch + (size_t)X0 * (NCH * B);
    // the row is staged in LDS at the skew its global address has, so that
    // 16-byte chunks of the two line up
    const int o = (int)((uintptr_t)gbytes & 15);
    if (live && e < ne) {
      float a = 0.0f;
#pragma unroll
      for (int t = 0; t < NT; t++) a += c_down.w[S][t] * s_h[S * y + t][e];
      *reinterpret_cast<E*>(&s_out[rr][o + e * B]) = (E)quantise<B>(a, f);
    }
    __syncthreads();
    if (live) {
      // samples up to the first 16-byte boundary, 16-byte chunks, the rest
      // (in bytes: o, nb and head are multiples of B)
      auto copy = [&](int at) {
        *reinterpret_cast<E*>(gbytes + at) = *reinterpret_cast<const E*>(&s_out[rr][o + at]);
      };
      const int head = min((16 - o) & 15, nb);
      if (e * B < head) copy(e * B);
      const int nch = (nb - head) >> 4;  // <= TE*B/16 <= 4
      if (e < nch)
        *reinterpret_cast<uint4*>(gbytes + head + 16 * e) =
            *reinterpret_cast<const uint4*>(&s_out[rr][o + head + 16 * e]);
      const int t = head + 16 * nch + e * B;  // fewer than 16 bytes are left
      if (t < nb) copy(t);
    }
    __syncthreads();
  }
}

inline uint32_t tiles(uint32_t n, int t) { return (n + t - 1) / t; }

template <int B>
int launch_down(const uint8_t* src0, const uint8_t* src1, uint32_t src_pitch, uint32_t pw, uint32_t ph,
                uint8_t* dst0, uint8_t* dst1, uint32_t dst_pitch, uint32_t ow, uint32_t oh,
                uint32_t scale, bool semiplanar, Fmt<B> f, hipStream_t s) {
  const uint32_t planes = !semiplanar && src1 ? 2 : 1;
#define SRCNN_YUV_DOWN(S, NCH)                                                                     \
  {                                                                                                \
    const uint32_t tx = tiles(ow, DownTile<S, NCH>::TX), ty = tiles(oh, DownTile<S, NCH>::TY);     \
    hipLaunchKernelGGL((downscale_planes_kernel<S, B, NCH>), dim3(tx* ty, planes), dim3(kThreads), \
                       0, s, src0, src1, (size_t)src_pitch, (int)pw, (int)ph, dst0, dst1,          \
                       (size_t)dst_pitch, (int)ow, (int)oh, (int)tx, f);                           \
  }
#define SRCNN_YUV_DOWN_S(S) \
  if (semiplanar) SRCNN_YUV_DOWN(S, 2) else SRCNN_YUV_DOWN(S, 1)
  switch (scale) {
    case 1: SRCNN_YUV_DOWN_S(1); break;
    case 2: SRCNN_YUV_DOWN_S(2); break;
    case 3: SRCNN_YUV_DOWN_S(3); break;
    case 4: SRCNN_YUV_DOWN_S(4); break;
    default: return fail(SRCNN_ERR_INVALID, "downscale_planes: scale %u has no kernel", scale);
  }
#undef SRCNN_YUV_DOWN_S
#undef SRCNN_YUV_DOWN
  SRCNN_LAUNCH_TRY();
  return SRCNN_OK;
}

}  // namespace

int downscale_planes(const void* src0, const void* src1, uint32_t src_pitch, uint32_t pw, uint32_t ph,
                     void* dst0, void* dst1, uint32_t dst_pitch, uint32_t ow, uint32_t oh,
                     uint32_t scale, uint32_t bits, bool msb, bool semiplanar, hipStream_t s) {
  SRCNN_PROFILE("downscale_planes", s);
  const uint8_t *a = static_cast<const uint8_t*>(src0), *b = static_cast<const uint8_t*>(src1);
  uint8_t *A = static_cast<uint8_t*>(dst0), *Bp = static_cast<uint8_t*>(dst1);
  if (bits == 8)
    return launch_down<1>(a, b, src_pitch, pw, ph, A, Bp, dst_pitch, ow, oh, scale, semiplanar,
                          Fmt<1>{}, s);
  return launch_down<2>(a, b, src_pitch, pw, ph, A, Bp, dst_pitch, ow, oh, scale, semiplanar,
                        deep_fmt(bits, msb), s);
}

int preload_yuv_down() {
#define SRCNN_YUV_SCALES(K, ...) \
  (const void*)K<1, __VA_ARGS__>, (const void*)K<2, __VA_ARGS__>, (const void*)K<3, __VA_ARGS__>, (const void*)K<4, __VA_ARGS__>
  const void* k[] = {SRCNN_YUV_SCALES(downscale_planes_kernel, 1, 1),
                     SRCNN_YUV_SCALES(downscale_planes_kernel, 1, 2),
                     SRCNN_YUV_SCALES(downscale_planes_kernel, 2, 1),
                     SRCNN_YUV_SCALES(downscale_planes_kernel, 2, 2)};
#undef SRCNN_YUV_SCALES
  return resolve_kernels(k, (int)(sizeof(k) / sizeof(k[0])));
}

}  // namespace srcnn
