// wl1x6.hpp -- wl1x6_fwd, the split-bf16 layer-1 forward of the wide step
// (LDS layout: W1x6Lds, wide_layout.hpp; pixel order: runs.hpp).  Included by
// train_wide.hip inside namespace srcnn::wide.

// ---------------------------------------------------------------------------
// wl1x6: the L1 forward of the step with split-bf16 products (split.hpp),
// l12x6's layer 1 (fused, l12x6.hpp) with the operands swapped so the
// accumulator holds [pixel][channel] and A1 leaves as HWC rows:
//   A1[p][n] = relu(B1[n] + sum_tap X[p + off(tap)] W1[tap][n])   (layer_uber_kernel.cl:36-96)
// GEMM M = the 32 pixel slots of a chunk (runs.hpp order), N = 32 channels
// per wave (four waves: n1 = 128), K = taps: taps 0-79 in 5 bf16 k-steps of
// 16 (slot 8h + j of k-step s: group g = 2s + h <= 8 is tap (g, j), g = 9 is
// tap (j, 8)), tap 80 and the bias in one fp32 32x32x2 MFMA that starts the
// accumulator.  A: X windows -- k-steps 0-3 one row of 8 pixels = 4 pair
// dwords per part of the pair image (l12x6's X6Lds layout: the three part
// rows side by side, row stride rs3 = 4 (ow / 4) (mod 32), so a half-wave's
// 32 slots hit 32 banks), k-step 4 the fp32 tile split in registers.  B: the
// wave's W1 parts, register-resident (5 k-steps x 3 parts).  Per chunk 30
// bf16 MFMAs + 1 fp32 where wl1_fwd_kernel issues 82 fp32 32x32x2 (two
// 16-pixel halves of 41 k-pairs); four blocks per CU.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256, 4) void wl1x6_fwd_kernel(const float* __restrict__ X,
                                                          const float* __restrict__ W1,
                                                          const float* __restrict__ B1,
                                                          float* __restrict__ A1, WGeom g, RunGeom rg) {
  using mfma::bf16x8;
  using mfma::mma_x6;
  using mfma::split3;
  using mfma::split8;
  using mfma::u32x4;
  constexpr int N1 = 128, F1 = 9, K1 = F1 * F1;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const W1x6Lds L(g.w, g.h, rg);
  char* const base = reinterpret_cast<char*>(smem);
  uint32_t* const rimg = reinterpret_cast<uint32_t*>(smem);
  float* const xs = reinterpret_cast<float*>(base + L.xs);
  int* const rbt = reinterpret_cast<int*>(base + L.rb);
  int* const pxt = reinterpret_cast<int*>(base + L.px);
  const int lane = lane_id(), wave = wave_id(), h = lane >> 5, li = lane & 31;
  const int W = g.w, xn = g.w * g.h, npx = g.w1 * g.h1, nch = rg.nch, rs3 = L.rs3;
  const int n = 32 * wave + li;  // this lane's channel (B operand column, output column)

  float xr[kW1x6Regs];
  auto xload = [&](int smp) {
    const float* src = X + (size_t)smp * xn;
#pragma unroll
    for (int k = 0; k < kW1x6Regs; k++) {
      const int i = threadIdx.x + 256 * k;
      xr[k] = i < xn ? src[i] : 0.0f;
    }
  };
  if ((int)blockIdx.x < g.batch) xload(blockIdx.x);

  // W1 parts: k-step s, lane (n, h), element j <-> tap of group g = 2s + h
  bf16x8 wb[5][3];
#pragma unroll
  for (int s_ = 0; s_ < 5; s_++) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const int gg = 2 * s_ + h, tap = gg <= 8 ? gg * F1 + j : j * F1 + 8;
      v[j] = W1[tap * N1 + n];
    }
    split8(v, wb[s_]);
  }
  // tap 80 (half 0) and the bias (half 1): the fp32 MFMA's B operand
  const float b88 = h ? B1[n] : W1[(K1 - 1) * N1 + n];

  for (int i = threadIdx.x; i < nch * 32; i += 256) {
    int iy, ix;
    slot_coord(rg, i >> 5, i & 31, iy, ix);
    rbt[2 * i] = iy * rs3 + ix;
    rbt[2 * i + 1] = iy * W + ix;
    // [chunk][half][register]: register r of half hh is slot crow(r, hh)
    const int c = i >> 5, hh = (i >> 4) & 1, r = i & 15;
    pxt[i] = slot_pixel(rg, c, crow(r, hh));
  }

  for (int sample = blockIdx.x; sample < g.batch; sample += gridDim.x) {
    __syncthreads();  // the previous sample's readers are done with the images
    {
      uint16_t* const r16 = reinterpret_cast<uint16_t*>(rimg);
#pragma unroll
      for (int k = 0; k < kW1x6Regs; k++) {
        const int i = threadIdx.x + 256 * k;
        if (i < xn) {
          xs[i] = xr[k];
          const int y = i / W, x = i - y * W, d = y * rs3 + x;
          __bf16 p[3];
          split3(xr[k], p[0], p[1], p[2]);
#pragma unroll
          for (int q = 0; q < 3; q++) {
            const uint16_t b = __builtin_bit_cast(uint16_t, p[q]);
            r16[2 * (d + W * q)] = b;                 // low half of pair x
            if (x > 0) r16[2 * (d + W * q) - 1] = b;  // high half of pair x - 1
          }
        }
      }
    }
    __syncthreads();
    if (sample + (int)gridDim.x < g.batch) xload(sample + gridDim.x);
    // A1 rows of this sample through a range-checked buffer: a dummy slot's
    // offset (pixel -1) lies outside it and its store is dropped, no branch
    const auto a1rs = __builtin_amdgcn_make_buffer_rsrc(A1 + (size_t)sample * npx * N1, 0, npx * N1 * 4, 0x00020000);

    for (int c = 0; c < nch; c++) {
      const int rb = rbt[2 * (32 * c + li)] + h * rs3, xy = rbt[2 * (32 * c + li) + 1];
      f32x16 acc = mma(h ? 1.0f : xs[xy + 8 * W + 8], b88, zero16());
      auto xop = [&](int s_, bf16x8 (&a)[3]) {
#pragma unroll
        for (int q = 0; q < 3; q++) {
          const uint32_t* r = rimg + W * q + rb + 2 * s_ * rs3;
          u32x4 d;
          d[0] = r[0];
          d[1] = r[2];
          d[2] = r[4];
          d[3] = r[6];
          a[q] = __builtin_bit_cast(bf16x8, d);
        }
      };
#pragma unroll
      for (int s_ = 0; s_ < 4; s_++) {
        bf16x8 a[3];
        xop(s_, a);
        acc = mma_x6(a, wb[s_], acc);
      }
      {
        // k-step 4: half 0 row 8 (dx 0..7), half 1 column 8 (dy 0..7)
        const int b4 = h ? xy + 8 : xy + 8 * W, st4 = h ? W : 1;
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; j++) v[j] = xs[b4 + j * st4];
        bf16x8 a[3];
        split8(v, a);
        acc = mma_x6(a, wb[4], acc);
      }
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int4 t = *reinterpret_cast<const int4*>(pxt + 32 * c + 16 * h + 4 * k);
        const int pr[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
        for (int e = 0; e < 4; e++)
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, mfma::relu1(acc[4 * k + e])), a1rs,
                                                pr[e] * (N1 * 4) + 4 * n, 0, 0);
      }
    }
  }
}
