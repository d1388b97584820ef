// samples.hpp -- the sample formats of DESIGN.md 15 as the kernels of yuv.hip
//  and resize.hip see them: a sample is one
// byte, or a 16-bit word that holds 9 to 16 bits in its low or in its high
// bits (template parameter B: bytes per sample; struct Fmt); the word-aligned
// clamped fetch of a patch of such samples into LDS; the luma of a Y sample
// and the way back.  Everything sits in an unnamed namespace, as in
// bicubic.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace srcnn {
namespace {

template <int B>
struct Sample {
  using type = uint8_t;
};
template <>
struct Sample<2> {
  using type = uint16_t;
};

// How a two-byte sample sits in its word: the value is word >> sh (sh = 0: in
// the low bits, nothing masked; sh = 16 - bits: in the high bits) and at most
// maxv = 2^bits - 1 when written.  A one-byte sample is the byte, at most 255.
template <int B>
struct Fmt {
  __device__ __forceinline__ uint32_t value(uint32_t word) const { return word; }
};
template <>
struct Fmt<2> {
  int sh;
  float maxv;
  __device__ __forceinline__ uint32_t value(uint32_t word) const { return word >> sh; }
};

// clamped fetch of a patch of T::PC x T::PR pixels (a 256-thread workgroup),
// its first at (j0 - 2, i0 - 2) of the plane (either may lie outside it), from
// a plane of B-byte samples, NCH of them interleaved per pixel: lane (r, k)
// takes the k-th aligned word of four samples (4 bytes, or 8 of two-byte
// samples) under patch row r; store(r, c, ch, word) receives the sample's
// word of channel ch of patch column c.  A word is loaded whole only where it
// lies inside the row's w * NCH * B bytes, else its samples singly with
// clamped indices: no load leaves the row.  pr: the patch rows to fetch, the
// first pr <= T::PR of them.
template <typename T, int B, int NCH, typename Store>
__device__ __forceinline__ void stage_samples(const uint8_t* __restrict__ src, size_t pitch, int w,
                                              int h, int j0, int i0, Store store, int pr = T::PR) {
  using E = typename Sample<B>::type;
  constexpr int EW = 4;                       // samples in a word
  constexpr int PE = T::PC * NCH;             // samples under a patch row
  constexpr int NW = (PE + 2 * EW - 2) / EW;  // words under them at a skew of up to EW - 1
  constexpr uint32_t mask = B == 1 ? 255u : 65535u;
  const int ne = w * NCH;         // samples in a row
  const int xs = (j0 - 2) * NCH;  // the sample of patch column 0, channel 0
  for (int it = threadIdx.x; it < pr * NW; it += 256) {
    const int r = it / NW, k = it - r * NW;
    const int sy = min(max(i0 - 2 + r, 0), h - 1);
    const uint8_t* row = src + (size_t)sy * pitch;
    const int skew = (int)(((uintptr_t)row + (uintptr_t)((intptr_t)xs * B)) & (EW * B - 1)) / B;
    const int c0 = EW * k - skew;  // patch sample of the word's first sample
    const int x0 = xs + c0;        // its index in the row: row + x0 * B is aligned to the word
    if (x0 >= 0 && x0 + EW - 1 < ne) {
      uint32_t v[B];
      if constexpr (B == 1) {
        v[0] = *reinterpret_cast<const uint32_t*>(row + x0);
      } else {
        const uint2 t = *reinterpret_cast<const uint2*>(row + (size_t)x0 * B);
        v[0] = t.x;
        v[1] = t.y;
      }
#pragma unroll
      for (int b = 0; b < EW; b++)
        if (c0 + b >= 0 && c0 + b < PE)
          store(r, (int)((unsigned)(c0 + b) / NCH), (int)((unsigned)(c0 + b) % NCH),
                (v[b * B / 4] >> (8 * B * b % 32)) & mask);
    } else {
#pragma unroll
      for (int b = 0; b < EW; b++)
        if (c0 + b >= 0 && c0 + b < PE) {
          // the pixel is clamped, the channel kept (x0 + b may be negative)
          const int e = x0 + b;
          const int ec = NCH == 1 ? min(max(e, 0), w - 1) : min(max(e >> 1, 0), w - 1) * 2 + (e & 1);
          store(r, (int)((unsigned)(c0 + b) / NCH), (int)((unsigned)(c0 + b) % NCH),
                (uint32_t) reinterpret_cast<const E*>(row)[ec]);
        }
    }
  }
}

// the normalised luma of a Y sample: (Y - off) / div with (off, div) = (0, 255)
// for full range and (16, 219) for limited at 8 bits, both times 2^(bits-8)
// (full range: 2^bits - 1) above; a true division, never contracted, so that
// scale 1 at full range gives float(Y) / float(2^bits - 1) bit for bit
__device__ __forceinline__ float luma_of_y(float y, float off, float div) {
#pragma clang fp contract(off)
  return (y - off) / div;
}

// clamp(rintf(v), 0, 2^bits - 1) as the sample's word (rintf: round to
// nearest, ties to even)
template <int B>
__device__ __forceinline__ uint32_t quantise(float v, Fmt<B> f) {
  if constexpr (B == 1)
    return (uint32_t)fminf(fmaxf(rintf(v), 0.0f), 255.0f);
  else
    return (uint32_t)fminf(fmaxf(rintf(v), 0.0f), f.maxv) << f.sh;
}

inline Fmt<2> deep_fmt(uint32_t bits, bool msb) {
  return Fmt<2>{msb ? (int)(16 - bits) : 0, (float)((1u << bits) - 1u)};
}

// the range of a Y sample of `bits` bits: Y = off + span * luma, with
// (off, span) = (16, 219) times up = 2^(bits-8) for limited range, exactly the
// 8-bit pair at 8 bits, and (0, 2^bits - 1) for full range
struct Range {
  float off, span;
};
inline Range range_of(uint32_t bits, bool full_range) {
  const float up = (float)(1u << (bits - 8));  // exact
  return full_range ? Range{0.0f, (float)((1u << bits) - 1u)} : Range{16.0f * up, 219.0f * up};
}

}  // namespace
}  // namespace srcnn
