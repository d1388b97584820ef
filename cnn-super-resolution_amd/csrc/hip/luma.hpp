// luma.hpp -- the project's full-range luma of an 8-bit pixel, shared by
// upscale.hip and quality.hip.
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

}  // namespace srcnn
