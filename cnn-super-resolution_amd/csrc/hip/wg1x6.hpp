// wg1x6.hpp -- wg1x6, the split-bf16 gW1 / gB1 of the wide step after wd1x6
// (LDS layout: G1x6Lds, wide_layout.hpp; pixel order: runs.hpp).  Included by
// train_wide.hip inside namespace srcnn::wide.

// ---------------------------------------------------------------------------
// wg1x6: gW1 / gB1 of the step with split-bf16 products -- d1x6's gW1
// contraction (fused, d1x6.hpp) with delta1 read from HBM (D1, written by
// wd1x6 before its ReLU' factor) and the factor from A1:
//   gW1[t][n] += sum_p X[p + off(t)] [A1[p][n] > 0] D1[p][n],   gB1[n] += sum_p ...
// (backpropagate.cl:56-114 for layer 1).  Written as gW1^T: M = channels
// (one tile of 32 per wave, four waves = n1 128), N = taps (three tiles: 81
// taps, the ones column of gB1, zeros), K = the 32 slots of a chunk
// (runs.hpp order) in 2 k-steps; A = the wave's masked delta1 (lane =
// channel, 8 slots per lane half: runs 4m + h and 4m + 2 + h), split in
// registers; B = X windows from d1x6's part-interleaved pair images (row
// runs: R, rows padded to rs = 9 (mod 64); column runs: T, column-major),
// double-buffered per sample.  The next item's 32 delta1 / A1 loads (range-
// checked buffer loads: a dummy slot's offset lies outside and reads 0) are
// in flight under the current item's 36 MFMAs.  Every wave owns its channel
// tile, so the block writes its slab with no cross-wave reduction; two
// blocks per CU.  (l1_grad_kernel<MASK> did this on fp32 16x16x4 MFMAs.)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void wg1x6_kernel(const float* __restrict__ X,
                                                      const float* __restrict__ D1,
                                                      const float* __restrict__ A1,
                                                      float* __restrict__ slab, WGeom g, RunGeom rg) {
  using mfma::bf16x8;
  using mfma::mma_x6;
  using mfma::split3;
  using mfma::split8;
  using mfma::u32x4;
  constexpr int N1 = 128, F1 = 9, K1 = F1 * F1, P1 = K1 * N1 + N1;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const G1x6Lds L(g.w, g.h, rg);
  char* const base = reinterpret_cast<char*>(smem);
  uint32_t* const u32 = reinterpret_cast<uint32_t*>(smem);
  int* const offs = reinterpret_cast<int*>(base + L.offs);
  int* const runs = reinterpret_cast<int*>(base + L.runs);
  const int lane = lane_id(), wave = wave_id(), h = lane >> 5, li = lane & 31;
  const int W = g.w, xn = g.w * g.h, npx = g.w1 * g.h1, nch = rg.nch;
  const int x0col = 4 * rg.a;
  const int n = 32 * wave + li;  // this lane's channel (A operand row)

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

  // per-block tables: element e = 8m + j of lane half hh of chunk c is slot
  // 16m + 8 (j >> 2) + 4 hh + (j & 3) (runs 4m + hh, 4m + 2 + hh)
  for (int i = threadIdx.x; i < nch * 32; i += 256) {
    const int c = i >> 5, hh = (i >> 4) & 1, e = i & 15, m = e >> 3, j = e & 7;
    const int pix = slot_pixel(rg, c, 16 * m + 8 * (j >> 2) + 4 * hh + (j & 3));
    offs[i] = pix >= 0 ? pix * (N1 * 4) : (int)0x80000000;
  }
  for (int k = threadIdx.x; k < nch * 8; k += 256) {
    int iy, ix;
    bool col;
    run_origin(rg, k < rg.nrun ? k : 0, iy, ix, col);
    runs[k] = col ? ~(L.rdw + 3 * ((ix - x0col) * L.st + iy)) : 3 * (iy * L.rs + ix);
  }
  for (int i = threadIdx.x; i < 2 * L.xbuf; i += 256) u32[i] = 0u;
  if (threadIdx.x < 32) u32[L.cst / 4 + threadIdx.x] = threadIdx.x == 0 || threadIdx.x == 6 ? 0x3F803F80u : 0u;

  int offR3[3], offT3[3];
#pragma unroll
  for (int u = 0; u < 3; u++) {
    const int tap = 32 * u + li;
    const int dy = tap < K1 ? tap / F1 : 0, dx = tap < K1 ? tap - dy * F1 : 0;
    offR3[u] = 3 * (dy * L.rs + dx);
    offT3[u] = 3 * (dx * L.st + dy);
  }
  const int spec = li == K1 - 64 ? L.cst / 4 : li > K1 - 64 ? L.cst / 4 + 16 : -1;

  f32x16 g1[3] = {zero16(), zero16(), zero16()};
  // items k = (sample it, chunk c) of the block, it = k / nch; their delta1
  // and A1 values (element e = 8m + j) are loaded two items ahead into two
  // register buffers (one item of MFMAs did not cover the HBM latency)
  float dv[2][16], mv[2][16];
  const int nsmp = (g.batch - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x, nit = nsmp * nch;
  const float inv_nch = 1.0f / (float)nch;
  auto ldi = [&](int k, float (&dd)[16], float (&mm)[16]) __attribute__((always_inline)) {
    if (k >= nit) return;
    const int it = run_div(k, inv_nch), c = k - it * nch, smp = blockIdx.x + it * gridDim.x;
    const auto rd = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(D1) + (size_t)smp * npx * N1, 0,
                                                      npx * N1 * 4, 0x00020000);
    const auto ra = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(A1) + (size_t)smp * npx * N1, 0,
                                                      npx * N1 * 4, 0x00020000);
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int4 o = *reinterpret_cast<const int4*>(offs + 32 * c + 16 * h + 4 * q);
      const int oo[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
      for (int e = 0; e < 4; e++) {
        dd[4 * q + e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rd, oo[e] + 4 * n, 0, 0));
        mm[4 * q + e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ra, oo[e] + 4 * n, 0, 0));
      }
    }
  };
  bf16x8 da[2][3];  // the current item's masked delta1 parts [m]
  auto mask_split = [&](const float (&dd)[16], const float (&mm)[16]) __attribute__((always_inline)) {
#pragma unroll
    for (int m = 0; m < 2; m++) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; j++) v[j] = mm[8 * m + j] > 0.0f ? dd[8 * m + j] : 0.0f;
      split8(v, da[m]);
    }
  };
  // item k: at a sample's first chunk its X pair images (buffer it & 1) and
  // the barrier; then the loads of item k + 2 into the buffer item k came
  // from, the MFMAs, and the split of item k + 1
  auto step = [&](int k, float (&ld)[16], float (&lm)[16], const float (&sd)[16], const float (&sm)[16])
      __attribute__((always_inline)) {
    const int it = run_div(k, inv_nch), c = k - it * nch, smp = blockIdx.x + it * gridDim.x;
    if (c == 0) {
      uint32_t* const xi = u32 + (it & 1) * L.xbuf;
      uint16_t* const x16 = reinterpret_cast<uint16_t*>(xi);
#pragma unroll
      for (int q = 0; q < kW1x6Regs; q++) {
        const int i = threadIdx.x + 256 * q;
        if (i < xn) {
          __bf16 p[3];
          split3(xr[q], p[0], p[1], p[2]);
          const int y = i / W, x = i - y * W, ri = y * L.rs + x;
          const int ti = L.rdw + 3 * ((x - x0col) * L.st + y);
#pragma unroll
          for (int pq = 0; pq < 3; pq++) {
            const uint16_t b = __builtin_bit_cast(uint16_t, p[pq]);
            x16[2 * (3 * ri + pq)] = b;
            if (ri > 0) x16[2 * (3 * (ri - 1) + pq) + 1] = b;
            if (L.tcols && x >= x0col) {
              x16[2 * (ti + pq)] = b;
              if (y > 0) x16[2 * (ti - 3 + pq) + 1] = b;
            }
          }
        }
      }
      __syncthreads();  // images of buffer it & 1 complete; every wave is past sample it - 1
      if (it + 1 < nsmp) xload(smp + gridDim.x);
    }
    ldi(k + 2, ld, lm);
    const int xo = (it & 1) * L.xbuf;
    int rc4[2][2];
#pragma unroll
    for (int m = 0; m < 2; m++)
#pragma unroll
      for (int e = 0; e < 2; e++) rc4[m][e] = runs[8 * c + 4 * m + 2 * e + h];
#pragma unroll
    for (int m = 0; m < 2; m++)
#pragma unroll
      for (int u = 0; u < 3; u++) {
        u32x4 d[3];
#pragma unroll
        for (int e = 0; e < 2; e++) {
          const int code = rc4[m][e];
          int a = xo + (code >= 0 ? code + offR3[u] : ~code + offT3[u]);
          if (u == 2) a = spec >= 0 ? spec : a;
#pragma unroll
          for (int q = 0; q < 3; q++) {
            d[q][2 * e] = u32[a + q];
            d[q][2 * e + 1] = u32[a + q + 6];
          }
        }
        bf16x8 bx[3];
#pragma unroll
        for (int q = 0; q < 3; q++) bx[q] = __builtin_bit_cast(bf16x8, d[q]);
        g1[u] = mma_x6(da[m], bx, g1[u]);
      }
    if (k + 1 < nit) mask_split(sd, sm);
  };

  __syncthreads();  // tables
  ldi(0, dv[0], mv[0]);
  ldi(1, dv[1], mv[1]);
  if (nit > 0) mask_split(dv[0], mv[0]);
  for (int k = 0; k < nit; k += 2) {
    step(k, dv[0], mv[0], dv[1], mv[1]);
    if (k + 1 < nit) step(k + 1, dv[1], mv[1], dv[0], mv[0]);
  }

  // the block's slab [gW1 | gB1]: wave w's channels 32 w .. 32 w + 31
  float* const out = slab + (size_t)blockIdx.x * P1;
#pragma unroll
  for (int u = 0; u < 3; u++) {
    const int tap = 32 * u + li;
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int ch = 32 * wave + crow(r, h);
      if (tap < K1)
        out[tap * N1 + ch] = g1[u][r];
      else if (tap == K1)
        out[K1 * N1 + ch] = g1[u][r];
    }
  }
}
