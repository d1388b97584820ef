// Probe: fp32 GEMM tiles through the two-part fp16 split (split.hpp: split8_h,
// mma_x3_h) on gfx950, beside the six-product bf16 form and
// v_mfma_f32_32x32x2_f32, against an fp64 host product.  Prints
//   1. whether v_mfma_f32_32x32x16_f16 keeps fp16 subnormal operands (and
//      whether the fp32 -> fp16 conversion of the split produces them),
//   2. per data set and K the normwise and max elementwise relative error of
//      f32 / bf16 x6 / f16 x3 (the f16 operands scaled by powers of two: the
//      exact scale, and the A scale 2^7 and 2^12 too small),
//   3. cycles per MFMA back to back (s_memtime around a register-fed loop, one
//      wave) and the matrix-pipe rate with every SIMD busy, f16 beside bf16.
// Build: hipcc --offload-arch=gfx950 -O3 -I cnn-super-resolution_amd/csrc/hip
//        tools/micro/split_f16.hip -o tools/micro/split_f16
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "split.hpp"

using namespace srcnn::mfma;

#define CHECK(x)                                                                  \
  do {                                                                            \
    hipError_t e_ = (x);                                                          \
    if (e_ != hipSuccess) {                                                       \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); \
      exit(1);                                                                    \
    }                                                                             \
  } while (0)

// one wave: D[32][32] = A[32][K] . B[K][32] (K a multiple of 16).
// mode 0 f32, 6 bf16 x6, 3 f16 x3 with A scaled by 2^ea and B by 2^eb
__global__ void tile_gemm(const float* A, const float* B, float* D, int K, int mode, int ea, int eb) {
  const int l = threadIdx.x, col = l & 31, hh = l >> 5;
  f32x16 acc = zero16();
  if (mode == 0) {
    for (int k = 0; k < K; k += 2) acc = mma(A[col * K + k + hh], B[(k + hh) * 32 + col], acc);
  } else {
    const float sa = pow2_h(ea), sb = pow2_h(eb);
    for (int k = 0; k < K; k += 16) {
      float av[8], bv[8];
      for (int j = 0; j < 8; j++) {
        const int kk = k + 8 * hh + j;
        av[j] = A[col * K + kk];
        bv[j] = B[kk * 32 + col];
      }
      if (mode == 6) {
        bf16x8 a[3], b[3];
        split8(av, a);
        split8(bv, b);
        acc = mma_x6(a, b, acc);
      } else {
        for (int j = 0; j < 8; j++) av[j] *= sa, bv[j] *= sb;
        f16x8 a[2], b[2];
        split8_h(av, a);
        split8_h(bv, b);
        acc = mma_x3_h(a, b, acc);
      }
    }
    if (mode == 3) {
      // (two exact steps: 2^-(ea + eb) alone may leave fp32's normal range)
      const float ua = pow2_h(-ea), ub = pow2_h(-eb);
      for (int r = 0; r < 16; r++) acc[r] = acc[r] * ua * ub;
    }
  }
  for (int r = 0; r < 16; r++) D[crow(r, hh) * 32 + col] = acc[r];
}

// subnormal operands: out[0] = sum_k a b with a = 2^-20 (an fp16 subnormal,
// handed over as bits) and b = 2^10 on every slot: 16 x 2^-10 if kept, 0 if
// flushed.  out[1] = the same with the subnormal coming out of split8_h
// (p1 of 1 + 2^-20 is 2^-20): tells whether the conversion keeps them.
__global__ void subnormal_probe(float* out, float x) {
  f16x8 a, b, one;
  const uint16_t sub = 0x0010;  // 2^-24 x 16 = 2^-20
  for (int j = 0; j < 8; j++) {
    a[j] = __builtin_bit_cast(_Float16, sub);
    b[j] = (_Float16)1024.0f;
    one[j] = (_Float16)1.0f;
  }
  f32x16 acc = mma_f16(a, b, zero16());
  float v[8];
  for (int j = 0; j < 8; j++) v[j] = x;  // (an argument: nothing folded on the host)
  f16x8 p[2];
  split8_h(v, p);
  f32x16 acc2 = mma_f16(p[1], b, zero16());
  f32x16 acc3 = mma_f16(p[0], one, zero16());
  if (threadIdx.x == 0) {
    out[0] = acc[0];
    out[1] = acc2[0];
    out[2] = acc3[0];
  }
}

// cycles per MFMA back to back: one wave, kChains independent accumulators,
// s_memtime (the shader clock, common.hpp) around the loop
template <bool kF16, int kChains>
__global__ void cycles(unsigned long long* out, float* sink, int iters) {
  f32x16 acc[kChains];
  for (int c = 0; c < kChains; c++) acc[c] = zero16();
  bf16x8 av, bv;
  f16x8 ah, bh;
  for (int j = 0; j < 8; j++) {
    av[j] = (__bf16)(threadIdx.x * 1e-3f + j), bv[j] = (__bf16)(1.0f - j);
    ah[j] = (_Float16)(threadIdx.x * 1e-3f + j), bh[j] = (_Float16)(1.0f - j);
  }
  const unsigned long long t0 = __builtin_amdgcn_s_memtime();
  for (int it = 0; it < iters; it++) {
#pragma unroll
    for (int k = 0; k < 8; k++)
#pragma unroll
      for (int c = 0; c < kChains; c++) acc[c] = kF16 ? mma_f16(ah, bh, acc[c]) : mma_bf16(av, bv, acc[c]);
  }
  float s = 0.0f;
  for (int c = 0; c < kChains; c++)
    for (int i = 0; i < 16; i++) s += acc[c][i];
  const unsigned long long t1 = __builtin_amdgcn_s_memtime();
  sink[threadIdx.x] = s;
  if (threadIdx.x == 0) out[0] = t1 - t0;
}

// matrix-pipe rate: independent accumulators, operands in registers
template <bool kF16>
__global__ __launch_bounds__(256) void rate(float* out, int iters) {
  f32x16 acc[4];
  for (int c = 0; c < 4; c++) acc[c] = zero16();
  bf16x8 av, bv;
  f16x8 ah, bh;
  for (int j = 0; j < 8; j++) {
    av[j] = (__bf16)(threadIdx.x * 1e-3f + j), bv[j] = (__bf16)(1.0f - j);
    ah[j] = (_Float16)(threadIdx.x * 1e-3f + j), bh[j] = (_Float16)(1.0f - j);
  }
  for (int it = 0; it < iters; it++) {
#pragma unroll
    for (int k = 0; k < 8; k++)
#pragma unroll
      for (int c = 0; c < 4; c++) acc[c] = kF16 ? mma_f16(ah, bh, acc[c]) : mma_bf16(av, bv, acc[c]);
  }
  float s = 0.0f;
  for (int c = 0; c < 4; c++)
    for (int i = 0; i < 16; i++) s += acc[c][i];
  out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

// e with m 2^e in [2^14, 2^15) for the data's maximum m (0 for all zeros)
static int host_scale(const std::vector<float>& v) {
  float m = 0.0f;
  for (float x : v) m = std::fmax(m, std::fabs(x));
  if (m == 0.0f) return 0;
  int ex;
  std::frexp(m, &ex);  // m = f 2^ex, f in [0.5, 1)
  return 15 - ex;
}

static void errors(const char* tag, const std::vector<float>& A, const std::vector<float>& B, int K) {
  std::vector<double> ref(32 * 32);
  double rn = 0.0;
  for (int i = 0; i < 32; i++)
    for (int j = 0; j < 32; j++) {
      double s = 0.0;
      for (int k = 0; k < K; k++) s += (double)A[i * K + k] * B[k * 32 + j];
      ref[i * 32 + j] = s;
      rn += s * s;
    }
  rn = std::sqrt(rn);
  float *dA, *dB, *dD;
  CHECK(hipMalloc(&dA, A.size() * 4));
  CHECK(hipMalloc(&dB, B.size() * 4));
  CHECK(hipMalloc(&dD, 32 * 32 * 4));
  CHECK(hipMemcpy(dA, A.data(), A.size() * 4, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(dB, B.data(), B.size() * 4, hipMemcpyHostToDevice));
  const int ea = host_scale(A), eb = host_scale(B);
  printf("%-10s K=%4d", tag, K);
  struct Form {
    const char* name;
    int mode, shorter;
  };
  for (const Form& f : {Form{"f32", 0, 0}, Form{"bf16x6", 6, 0}, Form{"f16x3", 3, 0}, Form{"f16x3/2^7", 3, 7},
                        Form{"f16x3/2^12", 3, 12}}) {
    hipLaunchKernelGGL(tile_gemm, dim3(1), dim3(64), 0, 0, dA, dB, dD, K, f.mode, ea - f.shorter, eb);
    CHECK(hipGetLastError());
    std::vector<float> D(32 * 32);
    CHECK(hipMemcpy(D.data(), dD, 32 * 32 * 4, hipMemcpyDeviceToHost));
    double en = 0.0, emax = 0.0;
    for (int i = 0; i < 32 * 32; i++) {
      const double e = D[i] - ref[i];
      en += e * e;
      emax = std::fmax(emax, std::fabs(e) / (std::fabs(ref[i]) + 1e-30));
    }
    printf("  %s norm %.2e max %.2e", f.name, std::sqrt(en) / rn, emax);
  }
  printf("\n");
  CHECK(hipFree(dA));
  CHECK(hipFree(dB));
  CHECK(hipFree(dD));
}

int main() {
  float* out;
  CHECK(hipMalloc(&out, 1024 * 256 * 4));
  {
    hipLaunchKernelGGL(subnormal_probe, dim3(1), dim3(64), 0, 0, out, 1.0f + 0x1p-20f);
    float r[3];
    CHECK(hipMemcpy(r, out, sizeof r, hipMemcpyDeviceToHost));
    const float kept = 16.0f * 0x1p-10f;
    printf("subnormal fp16 operand (2^-20 x 2^10 x 16 = %g): MFMA gives %g -> %s\n", kept, r[0],
           r[0] == kept ? "kept" : r[0] == 0.0f ? "flushed" : "other");
    printf("subnormal part out of split8_h (1 + 2^-20: p0 sum %g, p1 . 2^10 sum %g) -> conversion %s\n", r[2], r[1],
           r[1] == kept ? "keeps them" : r[1] == 0.0f ? "flushes them (or the MFMA does)" : "other");
  }
  std::mt19937 rng(7);
  std::normal_distribution<float> nd(0.f, 1.f);
  std::uniform_real_distribution<float> ud(0.f, 1.f);
  std::lognormal_distribution<float> ln(0.f, 3.f);
  for (int K : {96, 640}) {
    std::vector<float> A(32 * K), B(K * 32);
    for (auto& v : A) v = nd(rng);
    for (auto& v : B) v = nd(rng);
    errors("normal", A, B, K);
    for (auto& v : A) v = 1e-3f * nd(rng);
    for (auto& v : B) v = 1e-5f * nd(rng);
    errors("1e-3x1e-5", A, B, K);
    // delta1-like (half zeros, lognormal magnitudes) against pixels in [0, 1)
    for (auto& v : A) v = ud(rng) < 0.5f ? 0.0f : 1e-6f * ln(rng) * (ud(rng) < 0.5f ? -1.0f : 1.0f);
    for (auto& v : B) v = ud(rng);
    errors("delta1*x", A, B, K);
  }
  {
    unsigned long long* cyc;
    CHECK(hipMalloc(&cyc, 8));
    const int iters = 2000;
    for (int f16 = 0; f16 < 2; f16++)
      for (int chains : {1, 2, 4}) {
        auto k = f16 ? (chains == 1 ? cycles<true, 1> : chains == 2 ? cycles<true, 2> : cycles<true, 4>)
                     : (chains == 1 ? cycles<false, 1> : chains == 2 ? cycles<false, 2> : cycles<false, 4>);
        unsigned long long c = 0;
        for (int rep = 0; rep < 2; rep++) {  // (the second launch: warm)
          hipLaunchKernelGGL(k, dim3(1), dim3(64), 0, 0, cyc, out, iters);
          CHECK(hipMemcpy(&c, cyc, 8, hipMemcpyDeviceToHost));
        }
        printf("%s, %d chain%s: %.1f cycles per MFMA back to back\n", f16 ? "32x32x16 f16 " : "32x32x16 bf16", chains,
               chains > 1 ? "s" : " ", (double)c / ((double)iters * 8 * chains));
      }
    CHECK(hipFree(cyc));
  }
  for (int waves : {1, 2}) {
    const int blocks = 256 * waves, iters = 4000;
    for (int f16 = 0; f16 < 2; f16++) {
      auto k = f16 ? rate<true> : rate<false>;
      hipLaunchKernelGGL(k, dim3(blocks), dim3(256), 0, 0, out, 10);
      CHECK(hipDeviceSynchronize());
      hipEvent_t e0, e1;
      CHECK(hipEventCreate(&e0));
      CHECK(hipEventCreate(&e1));
      CHECK(hipEventRecord(e0));
      hipLaunchKernelGGL(k, dim3(blocks), dim3(256), 0, 0, out, iters);
      CHECK(hipEventRecord(e1));
      CHECK(hipEventSynchronize(e1));
      float ms;
      CHECK(hipEventElapsedTime(&ms, e0, e1));
      const double per_simd = (double)iters * 32 * waves;
      printf("%s waves/SIMD=%d: %.2f ns per MFMA per SIMD\n", f16 ? "32x32x16 f16 " : "32x32x16 bf16", waves,
             ms * 1e6 / per_simd);
    }
  }
  CHECK(hipFree(out));
  return 0;
}
