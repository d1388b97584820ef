// lds_dma.hpp -- gfx950 LDS-DMA (global_load_lds: 16 or 4 B per lane from
// global memory into LDS at M0 + 16 / 4 * lane) for the kernels that stage
// their operand images with it: the wide family (wconv_mfma.hpp, wd1g16.hpp,
// wgrad2.hpp) and the fused step's d1c.hpp.
//
// Inline asm, not __builtin_amdgcn_global_load_lds: issued through the
// builtin, the compiler cannot tell the in-flight DMA into the NEXT buffer
// from reads of the current one and puts an s_waitcnt vmcnt(0) before every
// later LDS read, which drains the whole prefetch each k-step.  Hidden from
// it, its own vmcnt waits only under-count (stay safe); every consumer
// reaches the data through an explicit s_waitcnt vmcnt(0) + barrier.
#pragma once

#include <hip/hip_runtime.h>

// M0 is written only by the asm below; the compiler sets it itself around its own uses
#pragma clang diagnostic ignored "-Winline-asm"

namespace srcnn {
namespace lds_dma {

typedef __attribute__((address_space(3))) void lds_void;

// the LDS byte address of a destination (per lane)
__device__ __forceinline__ uint32_t lds_addr(const float* p) {
  return (uint32_t)reinterpret_cast<uintptr_t>((lds_void*)p);
}
// the wave's M0 value: the first lane's destination
__device__ __forceinline__ uint32_t m0_of(const float* lds_dst) {
  return __builtin_amdgcn_readfirstlane(lds_addr(lds_dst));
}

// 16 B per lane from a 64-bit per-lane address
__device__ __forceinline__ void dma16(const float* src, float* lds_dst) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off"
               :
               : "s"(m0_of(lds_dst)), "v"(src)
               : "m0");
}
// 4 B per lane from a 64-bit per-lane address
__device__ __forceinline__ void dma4(const float* src, float* lds_dst) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dword %1, off"
               :
               : "s"(m0_of(lds_dst)), "v"(src)
               : "m0");
}
// 16 B / 4 B per lane from a wave-uniform base + 32-bit per-lane byte offset
__device__ __forceinline__ void dma16s(const float* base, uint32_t off, float* lds_dst) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2"
               :
               : "s"(m0_of(lds_dst)), "v"(off), "s"(base)
               : "m0");
}
__device__ __forceinline__ void dma4s(const float* base, uint32_t off, float* lds_dst) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dword %1, %2"
               :
               : "s"(m0_of(lds_dst)), "v"(off), "s"(base)
               : "m0");
}

}  // namespace lds_dma
}  // namespace srcnn
