// luma.hpp -- the project's full-range luma of an 8-bit pixel, shared by
// upscale.hip, resize.hip and quality.hip
// (DESIGN.md 12.1), and the way back from a luma and the pixel's colours
// (compose_px, upscale.hip and resize.hip).
//
// srcnn_upscale_luma's scale-1 anchor is bit-exact against
// extract_luma_kernel (ops_generic.hip).  Under -ffp-contract=fast the
// compiler chooses which of that kernel's products fuse into an fma, and the
// choice shows in the last bit; these helpers spell out the operations
// extract_luma_kernel is built from, with contraction off, so that the context
// they are inlined into cannot change them (tests/test_upscale_gpu.py pins
// luma_of against the kernel itself).
#pragma once

#include <hip/hip_runtime.h>

namespace srcnn {

// extract_luma_kernel without normalize: the 0 - 255 scale
__device__ __forceinline__ float luma255_of(float r, float g, float b) {
#pragma clang fp contract(off)
  return fmaf(b, 0.114f, r * 0.299f + g * 0.587f);
}
// extract_luma_kernel with normalize
__device__ __forceinline__ float luma_of(float r, float g, float b) {
#pragma clang fp contract(off)
  return luma255_of(r, g, b) / 255.0f;
}

// The composition of upscale.hip and resize.hip: at ratio 1
// it is srcnn_swap_luma byte for byte, so it spells out the operations
// swap_luma_kernel (ops_generic.hip) is built from in the same way
// (tests/test_upscale_gpu.py and tests/test_resize_gpu.py pin it against the
// kernel itself).
__device__ __forceinline__ void compose_px(float r, float g, float b, float nl, uint8_t* q) {
#pragma clang fp contract(off)
  const float Cb = fmaf(b, 0.5f, fmaf(r, -0.1687f, g * -0.3312f));
  const float Cr = fmaf(b, -0.0813f, fmaf(r, 0.5f, g * -0.4186f));
  // Y = nl * 255 is never rounded on its own: Y + Cb * k is one fma
  const float R = Cr * 1.4f + fmaf(nl, 255.0f, Cb * 0.0f);
  const float G = fmaf(nl, 255.0f, Cb * -0.343f) - Cr * 0.711f;
  const float B = Cr * 0.0f + fmaf(nl, 255.0f, Cb * 1.765f);
  q[0] = (uint8_t)(unsigned)fminf(fmaxf(R, 0.0f), 255.0f);
  q[1] = (uint8_t)(unsigned)fminf(fmaxf(G, 0.0f), 255.0f);
  q[2] = (uint8_t)(unsigned)fminf(fmaxf(B, 0.0f), 255.0f);
}

}  // namespace srcnn
