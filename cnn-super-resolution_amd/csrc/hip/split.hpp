// split.hpp -- fp32 products on the gfx950 bf16 matrix cores in exact-split
// form (used by l12x6.hpp's layer 2, d1x6.hpp, forward_fused.hip and the wide
// family's wl1x6.hpp, wg1x6.hpp, wl2x6.hpp and wgrad2x6.hpp), and in the
// two-part fp16 form below (d1x6.hpp's gW1 / gB1, l12x6.hpp's layer 1).
//
// a = a0 + a1 + a2 with a0 = bf16(a), a1 = bf16(a - a0), a2 = bf16(a - a0 - a1)
// (round to nearest even; every residual is exact in fp32), so
// |a - a0 - a1 - a2| <= 2^-27 |a|.  The product a . b keeps the six part
// products of order >= 2^-16 (a0b0, a0b1, a1b0, a0b2, a1b1, a2b0); the three
// dropped ones are <= 2^-26 |a b| together, below an fp32 product's 2^-24
// rounding.  Each part product is exact in fp32 (8 x 8 significant bits) and
// v_mfma_f32_32x32x16_bf16 sums them into an fp32 accumulator, so a 32x32x16
// block is 6 bf16 MFMAs (6 x 32 cycles) instead of 8 fp32 32x32x2 MFMAs
// (8 x 64 cycles) at fp32 accuracy (tools/micro/split_bf16.hip measures it).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mfma.hpp"

namespace srcnn {
namespace mfma {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void split3(float a, __bf16& p0, __bf16& p1, __bf16& p2) {
  p0 = (__bf16)a;
  const float r = a - (float)p0;
  p1 = (__bf16)r;
  p2 = (__bf16)(r - (float)p1);
}

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

// split8 with the residual subtractions as packed v_pk_add_f32 (d1x6, one
// wave per SIMD: the fewer VALU instructions won there, same-box A/B)
__device__ __forceinline__ void split8_pk(const float (&v)[8], bf16x8 (&o)[3]) {
#pragma unroll
  for (int j = 0; j < 8; j += 2) {
    const f32x2 a = {v[j], v[j + 1]};
    const bf16x2 p0 = __builtin_convertvector(a, bf16x2);
    const f32x2 r = a - __builtin_convertvector(p0, f32x2);
    const bf16x2 p1 = __builtin_convertvector(r, bf16x2);
    const bf16x2 p2 = __builtin_convertvector(r - __builtin_convertvector(p1, f32x2), bf16x2);
    o[0][j] = p0[0];
    o[0][j + 1] = p0[1];
    o[1][j] = p1[0];
    o[1][j + 1] = p1[1];
    o[2][j] = p2[0];
    o[2][j + 1] = p2[1];
  }
}

// eight values -> the three part operands of one 32x32x16 fragment, two
// values per conversion (one v_cvt_pk_bf16_f32 per pair and part)
__device__ __forceinline__ void split8(const float (&v)[8], bf16x8 (&o)[3]) {
#pragma unroll
  for (int j = 0; j < 8; j += 2) {
    const bf16x2 p0 = __builtin_convertvector((f32x2){v[j], v[j + 1]}, bf16x2);
    const f32x2 h0 = __builtin_convertvector(p0, f32x2);
    // (scalar subtractions: v_pk_add_f32 beside MFMAs costs more issue time)
    const float r0 = v[j] - h0[0], r1 = v[j + 1] - h0[1];
    const bf16x2 p1 = __builtin_convertvector((f32x2){r0, r1}, bf16x2);
    const f32x2 h1 = __builtin_convertvector(p1, f32x2);
    const bf16x2 p2 = __builtin_convertvector((f32x2){r0 - h1[0], r1 - h1[1]}, bf16x2);
    o[0][j] = p0[0];
    o[0][j + 1] = p0[1];
    o[1][j] = p1[0];
    o[1][j + 1] = p1[1];
    o[2][j] = p2[0];
    o[2][j + 1] = p2[1];
  }
}

// the three part dwords (bf16 pairs, a in the low half) of the pair (a, b)
__device__ __forceinline__ void split_pair(float a, float b, uint32_t (&o)[3]) {
  float v[8] = {a, b, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  bf16x8 r[3];
  split8(v, r);
#pragma unroll
  for (int q = 0; q < 3; q++) o[q] = __builtin_bit_cast(u32x4, r[q])[0];
}

// max(x, 0) as one v_max_i32 on the bit pattern (a negative float is a
// negative int32; fmaxf adds a canonicalising v_max per value)
__device__ __forceinline__ float relu1(float x) {
  const int b = __builtin_bit_cast(int, x);
  return __builtin_bit_cast(float, b > 0 ? b : 0);
}

__device__ __forceinline__ f32x16 mma_bf16(const bf16x8& a, const bf16x8& b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

// c += a . b over a 16-slot k-step, the six part products, small ones first
__device__ __forceinline__ f32x16 mma_x6(const bf16x8 (&a)[3], const bf16x8 (&b)[3], f32x16 c) {
  c = mma_bf16(a[2], b[0], c);
  c = mma_bf16(a[1], b[1], c);
  c = mma_bf16(a[0], b[2], c);
  c = mma_bf16(a[1], b[0], c);
  c = mma_bf16(a[0], b[1], c);
  return mma_bf16(a[0], b[0], c);
}

// the same on v_mfma_f32_16x16x32_bf16 (a 32-slot k-step, 16x16 C)
__device__ __forceinline__ f32x4 mma16_bf16(const bf16x8& a, const bf16x8& b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ f32x4 mma16_x6(const bf16x8 (&a)[3], const bf16x8 (&b)[3], f32x4 c) {
  c = mma16_bf16(a[2], b[0], c);
  c = mma16_bf16(a[1], b[1], c);
  c = mma16_bf16(a[0], b[2], c);
  c = mma16_bf16(a[1], b[0], c);
  c = mma16_bf16(a[0], b[1], c);
  return mma16_bf16(a[0], b[0], c);
}

// ---- the two-part fp16 form (tools/micro/split_f16.hip measures it;
// tests/test_split_f16_cpu.py restates it in numpy) ----
// A value scaled by a power of two so that its bound lands on 2^15 at most,
// xs = x 2^e, is p0 + p1 with p0 = f16(xs), p1 = f16(xs - p0) (round to
// nearest even, the residual exact in fp32): 22-23 significant bits while xs
// stays above 2^-2 or so, fewer below (p1 reaches fp16's subnormals, which
// the conversion and the matrix cores keep).  A product keeps p0 q0, p0 q1
// and p1 q0; p1 q1 <= 2^-22 |x y| is dropped.  Each part product is exact in
// fp32 (11 x 11 bits), so a 32x32x16 block is 3 v_mfma_f32_32x32x16_f16 where
// the bf16 form takes 6, and the result carries the factor 2^(ea + eb).
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

// eight scaled values -> the two part operands of one 32x32x16 fragment (one
// conversion per pair and part, scalar subtractions, as split8)
__device__ __forceinline__ void split8_h(const float (&v)[8], f16x8 (&o)[2]) {
#pragma unroll
  for (int j = 0; j < 8; j += 2) {
    const f16x2 p0 = __builtin_convertvector((f32x2){v[j], v[j + 1]}, f16x2);
    const f32x2 h0 = __builtin_convertvector(p0, f32x2);
    const f16x2 p1 = __builtin_convertvector((f32x2){v[j] - h0[0], v[j + 1] - h0[1]}, f16x2);
    o[0][j] = p0[0];
    o[0][j + 1] = p0[1];
    o[1][j] = p1[0];
    o[1][j + 1] = p1[1];
  }
}

// the two part dwords (fp16 pairs, a in the low half) of the scaled pair (a, b)
__device__ __forceinline__ void split_pair_h(float a, float b, uint32_t (&o)[2]) {
  const f16x2 p0 = __builtin_convertvector((f32x2){a, b}, f16x2);
  const f32x2 h0 = __builtin_convertvector(p0, f32x2);
  const f16x2 p1 = __builtin_convertvector((f32x2){a - h0[0], b - h0[1]}, f16x2);
  o[0] = __builtin_bit_cast(uint32_t, p0);
  o[1] = __builtin_bit_cast(uint32_t, p1);
}

// the power-of-two scale of a bound: e with bound 2^e in [2^14, 2^15), 0 for
// a zero bound, always in [kScaleMin, kScaleMax] (so 2^e is a normal fp32
// even for a non-finite or absurd bound, which takes the exponent field as it
// stands)
constexpr int kScaleMin = -126, kScaleMax = 60;
__device__ __forceinline__ int scale_exp_h(float bound) {
  const int field = (__builtin_bit_cast(uint32_t, bound) >> 23) & 0xFF;  // 0: zero or subnormal
  if (bound == 0.0f) return 0;
  const int e = 14 - (field - 127);
  return e < kScaleMin ? kScaleMin : e > kScaleMax ? kScaleMax : e;
}
// 2^e for e in [-126, 127]
__device__ __forceinline__ float pow2_h(int e) { return __builtin_bit_cast(float, (uint32_t)(e + 127) << 23); }

__device__ __forceinline__ f32x16 mma_f16(const f16x8& a, const f16x8& b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}

// c += a . b over a 16-slot k-step, the three part products, small ones first
__device__ __forceinline__ f32x16 mma_x3_h(const f16x8 (&a)[2], const f16x8 (&b)[2], f32x16 c) {
  c = mma_f16(a[1], b[0], c);
  c = mma_f16(a[0], b[1], c);
  return mma_f16(a[0], b[0], c);
}

// c0 += a0 . b0 and c1 += a1 . b1 (two x3 chains interleaved, so no MFMA
// waits on its predecessor's result)
__device__ __forceinline__ void mma_x3_h_2(const f16x8 (&a0)[2], const f16x8 (&b0)[2], f32x16& c0,
                                           const f16x8 (&a1)[2], const f16x8 (&b1)[2], f32x16& c1) {
  c0 = mma_f16(a0[1], b0[0], c0);
  c1 = mma_f16(a1[1], b1[0], c1);
  c0 = mma_f16(a0[0], b0[1], c0);
  c1 = mma_f16(a1[0], b1[1], c1);
  c0 = mma_f16(a0[0], b0[0], c0);
  c1 = mma_f16(a1[0], b1[0], c1);
}

}  // namespace mfma
}  // namespace srcnn
