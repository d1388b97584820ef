// wl1.hpp -- wl1_fwd, the fp32 layer-1 forward of the wide step (its X tile:
// kXS, kXTile, wide_layout.hpp).  Included by train_wide.hip inside namespace
// srcnn::wide.

// ---------------------------------------------------------------------------
// L1 forward: A1 = relu(B1 + conv9x9(X, W1))   (layer_uber_kernel.cl:36-96)
// GEMM M = pixels (32-row tiles), N = 4 x 32 channels (one tile per wave),
// K = 81 taps (+1 zero tap).  The k-slot pairing gives half h the taps
// [KP*h, KP*h + KP), so every A operand is one ds_read_b32 at a per-half base
// plus an immediate.  Four blocks per CU (launch bound: 120 VGPRs), so the
// 1024-block grid is resident at once and every block gets the same number
// of samples (at three blocks per CU, 256 of the 1024 ran after the rest:
// 0.509 -> 0.486 ms, profiles/r03_ab_wl1).
// ---------------------------------------------------------------------------
template <int N1, int F1>
__global__ __launch_bounds__(256, 4) void wl1_fwd_kernel(const float* __restrict__ X,
                                                      const float* __restrict__ W1,
                                                      const float* __restrict__ B1,
                                                      float* __restrict__ A1, WGeom g) {
  static_assert(N1 == 128, "four waves x 32 output channels");
  constexpr int NT = F1 * F1, KP = (NT + 1) / 2;
  constexpr int Q = KP / F1, R = KP % F1;
  __shared__ float xs[kXTile];
  const int lane = lane_id(), wave = wave_id(), j = lane & 31, h = lane >> 5;
  const int n = 32 * wave + j;
  float wb[KP];
#pragma unroll
  for (int kp = 0; kp < KP; kp++) {
    const int t = kp + KP * h;
    wb[kp] = t < NT ? W1[t * N1 + n] : 0.0f;
  }
  const float bias = B1[n];
  for (int i = threadIdx.x; i < kXTile; i += 256) xs[i] = 0.0f;
  const int npx = g.w1 * g.h1, mtiles = (npx + 31) / 32;
  // tap kp + KP (half 1) sits at one of two fixed offsets from tap kp
  const int dA = h * (Q * kXS + R), dB = h * ((Q + 1) * kXS + R - F1);
  for (int s = blockIdx.x; s < g.batch; s += gridDim.x) {
    __syncthreads();
    const float* xsrc = X + (size_t)s * g.w * g.h;
    for (int i = threadIdx.x; i < g.w * g.h; i += 256) {
      const int y = i / g.w;
      xs[y * kXS + i - y * g.w] = xsrc[i];
    }
    __syncthreads();
    float* dst = A1 + (size_t)s * npx * N1 + n;
    for (int m = 0; m < mtiles; m += 2) {
      int base[2];
#pragma unroll
      for (int u = 0; u < 2; u++) {
        const int o = min(32 * (m + u) + j, npx - 1), oy = o / g.w1;
        base[u] = oy * kXS + o - oy * g.w1;
      }
      f32x16 acc0 = zero16(), acc1 = zero16();
#pragma unroll
      for (int kp = 0; kp < KP; kp++) {
        const int toff = (kp / F1) * kXS + kp % F1;
        const int d = (kp % F1 + R < F1) ? dA : dB;
        acc0 = mma(xs[base[0] + d + toff], wb[kp], acc0);
        acc1 = mma(xs[base[1] + d + toff], wb[kp], acc1);
      }
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int p0 = 32 * m + crow(r, h), p1 = p0 + 32;
        if (p0 < npx) dst[(size_t)p0 * N1] = fmaxf(acc0[r] + bias, 0.0f);
        if (p1 < npx) dst[(size_t)p1 * N1] = fmaxf(acc1[r] + bias, 0.0f);
      }
    }
  }
}
