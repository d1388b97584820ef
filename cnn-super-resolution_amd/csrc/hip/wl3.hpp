// wl3.hpp -- layer 3 of the wide step, forward and backward in one kernel: wl3
// (A2 from HBM twice) and wl3l (A2 resident in LDS).  LDS layouts: Wl3Lds,
// Wl3lLds (wide_layout.hpp).  Included by train_wide.hip inside namespace
// srcnn::wide.

// ---------------------------------------------------------------------------
// wl3: per sample
//   1. Q[p][t] = sum_c A2[p][c] W3[t][c]      (MFMA: M = pixels, N = taps, K = n2)
//   2. A3[o] = B3 + sum_t Q[o + off(t)][t]; delta3 = (A3 - T[o + pad]) [A3 > 0]
//      (last_layer_delta.cl:34-48, relu' quirk kept); squared error
//      (squared_error.cl); delta3 written into a zero-bordered grid Gd
//   3. delta2[p][c] = [A2 > 0] sum_t Gd[p - off(t)] W3[t][c]   (MFMA, K = taps)
//   4. gW3[t][c] += sum_p Gd[p - off(t)] A2[p][c]              (MFMA, K = pixels)
// gW3 / gB3 / squared error accumulate in registers across the block's
// samples and leave as one slab per block.
// ---------------------------------------------------------------------------
// Operands run ahead of their use (round 3, -18% wl3): each wave's next Q
// tile (across samples: the next sample's first tile) is in flight under the
// current tile's MFMAs, and gW3's A2 pixel pairs come in batches of kWl3B, the
// next batch in flight under the current one.  Two blocks per CU, every
// accumulator in VGPRs (launch bound).
constexpr int kWl3B = 4;  // gW3 pixel pairs per prefetch batch
template <int N2, int F3>
__global__ __launch_bounds__(256, 2) void wl3_kernel(const float* __restrict__ A2,
                                                  const float* __restrict__ T,
                                                  const float* __restrict__ W3,
                                                  const float* __restrict__ B3,
                                                  float* __restrict__ D2, float* __restrict__ slab3,
                                                  float* __restrict__ sqs, float* __restrict__ A3out,
                                                  WGeom g, int qfloats) {
  static_assert(N2 == 64 && F3 * F3 <= 32, "shape");
  constexpr int FF = F3 * F3, KP3 = (FF + 1) / 2, P3 = FF * N2 + 1;
  extern __shared__ float smem[];
  const Wl3Lds L(g, F3, qfloats);
  float* Qs = smem;             // [npx2][FF], later the cross-wave reduction
  float* Gd = smem + L.gd;      // [(h3 + 2(F3-1))][(w3 + 2(F3-1))]
  // relu' mask of A2 as bits, built from the step-1 operand registers so step
  // 3 does not re-read A2 from HBM: word [p][h] bit 4kk + jj <-> channel 8kk + 4h + jj
  unsigned* mbits = reinterpret_cast<unsigned*>(smem + L.mbits);
  __shared__ float red_s[2][4];
  const int lane = lane_id(), wave = wave_id(), j = lane & 31, h = lane >> 5;
  const int npx2 = g.w2 * g.h2, mt2 = (npx2 + 31) / 32, npx3 = g.w3 * g.h3;
  const int GW = g.w3 + 2 * (F3 - 1), GH = g.h3 + 2 * (F3 - 1);
  const int padT = (g.w - g.w3) / 2;  // last_layer_delta.cl:25 (from the width)
  const uint32_t w2_mag = (1u << 20) / (uint32_t)g.w2 + 1u;  // p / w2 as a multiply (p < 4096)
  auto row_of = [&](int p) { return (int)(((uint32_t)p * w2_mag) >> 20); };
  for (int i = threadIdx.x; i < GW * GH; i += 256) Gd[i] = 0.0f;
  // step 1 B operand: W3[t = j][c = 8kk + 4h + jj]
  float wq[8][4];
#pragma unroll
  for (int kk = 0; kk < 8; kk++)
#pragma unroll
    for (int jj = 0; jj < 4; jj++) wq[kk][jj] = j < FF ? W3[j * N2 + 8 * kk + 4 * h + jj] : 0.0f;
  // step 3: wave = (N tile nt, M group mg); taps kp + KP3*h
  const int nt = wave & 1, mg = wave >> 1;
  float wd[KP3];
  int goff[KP3];
#pragma unroll
  for (int kp = 0; kp < KP3; kp++) {
    const int t = kp + KP3 * h, tc = min(t, FF - 1);
    wd[kp] = t < FF ? W3[t * N2 + 32 * nt + j] : 0.0f;
    goff[kp] = -((tc / F3) * GW + tc % F3);
  }
  // step 4: row = tap j
  const int tA = min(j, FF - 1);
  const int goffA = -((tA / F3) * GW + tA % F3);
  const bool tapA = j < FF;
  f32x16 gacc0 = zero16(), gacc1 = zero16();
  float sq = 0.0f, gb3 = 0.0f;
  const float b3 = B3[0];
  // step 1 operands of tile mt: lane (j, h) reads pixel 32 mt + j, channels
  // 8 kk + 4 h + jj.  The next tile's (across samples: the next sample's first
  // tile's) loads are in flight under the current tile's MFMAs.
  float4 vn[8];
  auto ldq = [&](const float* a2s_, int mt_) {
    const int p = min(32 * mt_ + j, npx2 - 1);
    const float4* src = reinterpret_cast<const float4*>(a2s_ + (size_t)p * N2) + h;
#pragma unroll
    for (int kk = 0; kk < 8; kk++) vn[kk] = src[2 * kk];
  };
  if ((int)blockIdx.x < g.batch && wave < mt2) ldq(A2 + (size_t)blockIdx.x * npx2 * N2, wave);
  for (int s = blockIdx.x; s < g.batch; s += gridDim.x) {
    const float* a2s = A2 + (size_t)s * npx2 * N2;
    __syncthreads();  // previous sample's Gd / Qs readers are done
    // 1. Q
    for (int mt = wave; mt < mt2; mt += 4) {
      float4 v[8];
#pragma unroll
      for (int kk = 0; kk < 8; kk++) v[kk] = vn[kk];
      if (mt + 4 < mt2) ldq(a2s, mt + 4);
      f32x16 acc = zero16();
#pragma unroll
      for (int kk = 0; kk < 8; kk++)
#pragma unroll
        for (int jj = 0; jj < 4; jj++) acc = mma(v[kk][jj], wq[kk][jj], acc);
      {
        unsigned m = 0;
#pragma unroll
        for (int kk = 0; kk < 8; kk++)
#pragma unroll
          for (int jj = 0; jj < 4; jj++) m |= (v[kk][jj] > 0.0f ? 1u : 0u) << (4 * kk + jj);
        if (32 * mt + j < npx2) mbits[2 * (32 * mt + j) + h] = m;
      }
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int pix = 32 * mt + crow(r, h);
        if (pix < npx2 && j < FF) Qs[pix * FF + j] = acc[r];
      }
    }
    __syncthreads();
    // 2. A3, last delta, squared error
    const float* ts = T + (size_t)s * g.w * g.h;
    for (int o = threadIdx.x; o < npx3; o += 256) {
      const int oy = o / g.w3, ox = o - oy * g.w3;
      const float* q0 = Qs + (oy * g.w2 + ox) * FF;
      float v = 0.0f;
#pragma unroll
      for (int t = 0; t < FF; t++) v += q0[((t / F3) * g.w2 + t % F3) * FF + t];
      const float a3 = v + b3;
      A3out[(size_t)s * npx3 + o] = a3;  // to the workspace (srcnn_train_activations)
      const float diff = a3 - ts[(oy + padT) * g.w + ox + padT];
      const float d = a3 > 0.0f ? diff : 0.0f;
      sq += diff * diff;
      gb3 += d;
      Gd[(oy + F3 - 1) * GW + ox + F3 - 1] = d;
    }
    __syncthreads();
    // 3. delta2 (channel 32nt + j: mask word half mh, bit mbit)
    const int mc = 32 * nt + j, mh = (mc >> 2) & 1, mbit = 4 * (mc >> 3) + (mc & 3);
    for (int mt = mg; mt < mt2; mt += 2) {
      const int p = min(32 * mt + j, npx2 - 1), py = row_of(p), px = p - py * g.w2;
      const int gb = (py + F3 - 1) * GW + px + F3 - 1;
      f32x16 acc = zero16();
#pragma unroll
      for (int kp = 0; kp < KP3; kp++) acc = mma(Gd[gb + goff[kp]], wd[kp], acc);
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int pix = 32 * mt + crow(r, h);
        if (pix < npx2) {
          const size_t idx = ((size_t)s * npx2 + pix) * N2 + 32 * nt + j;
          D2[idx] = (mbits[2 * pix + mh] >> mbit) & 1u ? acc[r] : 0.0f;
        }
      }
    }
    // the next sample's first Q tile, in flight under delta2 / gW3
    if (s + (int)gridDim.x < g.batch && wave < mt2) ldq(a2s + (size_t)gridDim.x * npx2 * N2, wave);
    // 4. gW3 (K = pixel pairs kp = wave + 4 i split over the waves; B columns:
    // channel 2j + tile), in batches of kWl3B pairs: the next batch's A2 loads
    // and delta3-window reads are issued before the current batch's MFMAs
    // (two named register sets); pairs past the wave's count are not issued
    const int niter = (npx2 + 1) / 2 > wave ? ((npx2 + 1) / 2 - wave + 3) / 4 : 0;
    float2 bb[2][kWl3B];
    float ab[2][kWl3B];
    auto ldb = [&](int i0, float2 (&b_)[kWl3B], float (&a_)[kWl3B]) {
#pragma unroll
      for (int u = 0; u < kWl3B; u++) {
        const int pk = 2 * (wave + 4 * (i0 + u)) + h;
        const bool pok = pk < npx2;
        const int p = pok ? pk : npx2 - 1, py = row_of(p), px = p - py * g.w2;
        const float av = Gd[(py + F3 - 1) * GW + px + F3 - 1 + goffA];
        a_[u] = (tapA && pok) ? av : 0.0f;
        b_[u] = *reinterpret_cast<const float2*>(a2s + (size_t)p * N2 + 2 * j);
      }
    };
    auto mmb = [&](int i0, const float2 (&b_)[kWl3B], const float (&a_)[kWl3B]) {
#pragma unroll
      for (int u = 0; u < kWl3B; u++)
        if (i0 + u < niter) {
          gacc0 = mma(a_[u], b_[u].x, gacc0);
          gacc1 = mma(a_[u], b_[u].y, gacc1);
        }
    };
    if (niter > 0) ldb(0, bb[0], ab[0]);
    for (int i0 = 0; i0 < niter; i0 += 2 * kWl3B) {
      if (i0 + kWl3B < niter) ldb(i0 + kWl3B, bb[1], ab[1]);
      mmb(i0, bb[0], ab[0]);
      if (i0 + kWl3B >= niter) break;
      if (i0 + 2 * kWl3B < niter) ldb(i0 + 2 * kWl3B, bb[0], ab[0]);
      mmb(i0 + kWl3B, bb[1], ab[1]);
    }
  }
  // cross-wave reduction of gW3 (fixed order), gB3, squared error
  __syncthreads();
  float* red = Qs;  // 4 waves x 2 tiles x 16 regs x 64 lanes
#pragma unroll
  for (int r = 0; r < 16; r++) {
    red[((wave * 2 + 0) * 16 + r) * 64 + lane] = gacc0[r];
    red[((wave * 2 + 1) * 16 + r) * 64 + lane] = gacc1[r];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sq += __shfl_down(sq, o, 64);
    gb3 += __shfl_down(gb3, o, 64);
  }
  if (lane == 0) {
    red_s[0][wave] = sq;
    red_s[1][wave] = gb3;
  }
  __syncthreads();
  float* out = slab3 + (size_t)blockIdx.x * P3;
  for (int e = threadIdx.x; e < 2 * 16 * 64; e += 256) {
    const int tile = e / (16 * 64), r = (e / 64) % 16, l = e & 63;
    const int tap = crow(r, l >> 5), c = 2 * (l & 31) + tile;
    float v = 0.0f;
    for (int w = 0; w < 4; w++) v += red[((w * 2 + tile) * 16 + r) * 64 + l];
    if (tap < FF) out[tap * N2 + c] = v;
  }
  if (threadIdx.x == 0) {
    out[FF * N2] = red_s[1][0] + red_s[1][1] + red_s[1][2] + red_s[1][3];
    sqs[blockIdx.x] = red_s[0][0] + red_s[0][1] + red_s[0][2] + red_s[0][3];
  }
}

// ---------------------------------------------------------------------------
// wl3l: wl3 with the sample's A2 resident in LDS (round 3).  The Q phase
// writes the A2 operands it loaded into a quad-swizzled LDS image, so the
// delta2 mask and gW3's operand come from LDS and A2 is read from HBM once
// (wl3 read it twice: 1.51x the fused-minimum bytes).  A2 (441 x 64 floats,
// 112.9 KB) + Q (44.1 KB) + the delta3 grid fill the LDS, so one block of 8
// waves per CU; the next sample's first Q tile is loaded before the delta2
// stores (a store counts in vmcnt too) and lands under delta2 / gW3.
// ---------------------------------------------------------------------------
template <int N2>
__device__ __forceinline__ int wl3l_at(int p, int c) {  // A2 image float index, quads XOR-swizzled by pixel
  return p * N2 + 4 * ((c >> 2) ^ (p & (N2 / 4 - 1))) + (c & 3);
}
template <int N2, int F3>
__global__ __launch_bounds__(512, 1) void wl3l_kernel(const float* __restrict__ A2,
                                                     const float* __restrict__ T,
                                                     const float* __restrict__ W3,
                                                     const float* __restrict__ B3,
                                                     float* __restrict__ D2, float* __restrict__ slab3,
                                                     float* __restrict__ sqs, float* __restrict__ A3out,
                                                     WGeom g) {
  static_assert(N2 == 64 && F3 * F3 <= 32, "shape");
  constexpr int FF = F3 * F3, KP3 = (FF + 1) / 2, P3 = FF * N2 + 1, NW = 8;
  extern __shared__ float smem[];
  const int npx2 = g.w2 * g.h2, mt2 = (npx2 + 31) / 32, npx3 = g.w3 * g.h3;
  const int GW = g.w3 + 2 * (F3 - 1), GH = g.h3 + 2 * (F3 - 1);
  const Wl3lLds L(g, N2, F3);
  float* a2i = smem;                  // [npx2][N2], swizzled; the end-of-kernel reduction
  float* Qs = smem + L.q;             // [npx2][FF]
  float* Gd = smem + L.gd;            // [GH][GW]
  __shared__ float red_s[2][NW];
  static_assert(sizeof(red_s) == Wl3lLds::kStatic, "the plan counts this beside the dynamic LDS");
  const int lane = lane_id(), wave = wave_id(), j = lane & 31, h = lane >> 5;
  const int padT = (g.w - g.w3) / 2;  // last_layer_delta.cl:25 (from the width)
  // p / w2 as a multiply by a 20-bit reciprocal (exact for p < 4096; a runtime
  // division costs ~15 VALU per pixel pair in the gW3 loop)
  const uint32_t w2_mag = (1u << 20) / (uint32_t)g.w2 + 1u;
  auto row_of = [&](int p) { return (int)(((uint32_t)p * w2_mag) >> 20); };
  for (int i = threadIdx.x; i < GW * GH; i += 512) Gd[i] = 0.0f;
  float wq[8][4];
#pragma unroll
  for (int kk = 0; kk < 8; kk++)
#pragma unroll
    for (int jj = 0; jj < 4; jj++) wq[kk][jj] = j < FF ? W3[j * N2 + 8 * kk + 4 * h + jj] : 0.0f;
  const int nt = wave & 1, mg = wave >> 1;  // delta2: N tile, M group (4)
  float wd[KP3];
  int goff[KP3];
#pragma unroll
  for (int kp = 0; kp < KP3; kp++) {
    const int t = kp + KP3 * h, tc = min(t, FF - 1);
    wd[kp] = t < FF ? W3[t * N2 + 32 * nt + j] : 0.0f;
    goff[kp] = -((tc / F3) * GW + tc % F3);
  }
  const int tA = min(j, FF - 1);
  const int goffA = -((tA / F3) * GW + tA % F3);
  const bool tapA = j < FF;
  f32x16 gacc0 = zero16(), gacc1 = zero16();
  float sq = 0.0f, gb3 = 0.0f;
  const float b3 = B3[0];
  float4 vn[8];
  auto ldq = [&](const float* a2s_, int mt_) {
    const int p = min(32 * mt_ + j, npx2 - 1);
    const float4* src = reinterpret_cast<const float4*>(a2s_ + (size_t)p * N2) + h;
#pragma unroll
    for (int kk = 0; kk < 8; kk++) vn[kk] = src[2 * kk];
  };
  if ((int)blockIdx.x < g.batch && wave < mt2) ldq(A2 + (size_t)blockIdx.x * npx2 * N2, wave);
  for (int s = blockIdx.x; s < g.batch; s += gridDim.x) {
    const float* a2s = A2 + (size_t)s * npx2 * N2;
    const float* ts = T + (size_t)s * g.w * g.h;
    __syncthreads();  // the previous sample's readers of every LDS region are done
    float tv = 0.0f;  // this thread's target pixel (outputs past 512: loaded in place)
    {
      const int o = min((int)threadIdx.x, npx3 - 1), oy = o / g.w3, ox = o - oy * g.w3;
      tv = ts[(oy + padT) * g.w + ox + padT];
    }
    // 1. Q, and the A2 image
    for (int mt = wave; mt < mt2; mt += NW) {
      float4 v[8];
#pragma unroll
      for (int kk = 0; kk < 8; kk++) v[kk] = vn[kk];
      if (mt + NW < mt2) ldq(a2s, mt + NW);
      f32x16 acc = zero16();
#pragma unroll
      for (int kk = 0; kk < 8; kk++)
#pragma unroll
        for (int jj = 0; jj < 4; jj++) acc = mma(v[kk][jj], wq[kk][jj], acc);
      const int p = 32 * mt + j;
      if (p < npx2)
#pragma unroll
        for (int kk = 0; kk < 8; kk++) *reinterpret_cast<float4*>(a2i + wl3l_at<N2>(p, 8 * kk + 4 * h)) = v[kk];
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int pix = 32 * mt + crow(r, h);
        if (pix < npx2 && j < FF) Qs[pix * FF + j] = acc[r];
      }
    }
    __syncthreads();
    // 2. A3, last delta, squared error
    for (int o = threadIdx.x; o < npx3; o += 512) {
      const int oy = o / g.w3, ox = o - oy * g.w3;
      const float* q0 = Qs + (oy * g.w2 + ox) * FF;
      float v = 0.0f;
#pragma unroll
      for (int t = 0; t < FF; t++) v += q0[((t / F3) * g.w2 + t % F3) * FF + t];
      const float a3 = v + b3;
      A3out[(size_t)s * npx3 + o] = a3;  // to the workspace (srcnn_train_activations)
      const float tgt = o == (int)threadIdx.x ? tv : ts[(oy + padT) * g.w + ox + padT];
      const float diff = a3 - tgt;
      const float d = a3 > 0.0f ? diff : 0.0f;
      sq += diff * diff;
      gb3 += d;
      Gd[(oy + F3 - 1) * GW + ox + F3 - 1] = d;
    }
    __syncthreads();
    // the next sample's first Q tile, issued before the delta2 stores
    if (s + (int)gridDim.x < g.batch && wave < mt2) ldq(a2s + (size_t)gridDim.x * npx2 * N2, wave);
    // 3. delta2 = [A2 > 0] sum_t Gd W3 (channel 32 nt + j)
    const int mc = 32 * nt + j;
    for (int mt = mg; mt < mt2; mt += NW / 2) {
      const int p = min(32 * mt + j, npx2 - 1), py = row_of(p), px = p - py * g.w2;
      const int gb = (py + F3 - 1) * GW + px + F3 - 1;
      f32x16 acc = zero16();
#pragma unroll
      for (int kp = 0; kp < KP3; kp++) acc = mma(Gd[gb + goff[kp]], wd[kp], acc);
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int pix = 32 * mt + crow(r, h);
        if (pix < npx2) {
          const size_t idx = ((size_t)s * npx2 + pix) * N2 + mc;
          D2[idx] = a2i[wl3l_at<N2>(pix, mc)] > 0.0f ? acc[r] : 0.0f;
        }
      }
    }
    // 4. gW3 (K = pixel pairs kp = wave + NW i; B columns: channel 2j + tile);
    // batching the LDS reads of 4 or 8 pairs ahead of their MFMAs measured
    // slower (0.349 / 0.356 vs 0.341 ms)
    for (int kp = wave; 2 * kp < npx2; kp += NW) {
      const int pk = 2 * kp + h;
      const bool pok = pk < npx2;
      const int p = pok ? pk : npx2 - 1, py = row_of(p), px = p - py * g.w2;
      const float av = Gd[(py + F3 - 1) * GW + px + F3 - 1 + goffA];
      const float a = (tapA && pok) ? av : 0.0f;
      const float2 bv = *reinterpret_cast<const float2*>(a2i + wl3l_at<N2>(p, 2 * j));
      gacc0 = mma(a, bv.x, gacc0);
      gacc1 = mma(a, bv.y, gacc1);
    }
  }
  // cross-wave reduction of gW3 (fixed wave order), gB3, squared error
  __syncthreads();
  float* red = a2i;  // NW waves x 2 tiles x 16 regs x 64 lanes
#pragma unroll
  for (int r = 0; r < 16; r++) {
    red[((wave * 2 + 0) * 16 + r) * 64 + lane] = gacc0[r];
    red[((wave * 2 + 1) * 16 + r) * 64 + lane] = gacc1[r];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sq += __shfl_down(sq, o, 64);
    gb3 += __shfl_down(gb3, o, 64);
  }
  if (lane == 0) {
    red_s[0][wave] = sq;
    red_s[1][wave] = gb3;
  }
  __syncthreads();
  float* out = slab3 + (size_t)blockIdx.x * P3;
  for (int e = threadIdx.x; e < 2 * 16 * 64; e += 512) {
    const int tile = e / (16 * 64), r = (e / 64) % 16, l = e & 63;
    const int tap = crow(r, l >> 5), c = 2 * (l & 31) + tile;
    float v = 0.0f;
    for (int w = 0; w < NW; w++) v += red[((w * 2 + tile) * 16 + r) * 64 + l];
    if (tap < FF) out[tap * N2 + c] = v;
  }
  if (threadIdx.x == 0) {
    float b = 0.0f, q = 0.0f;
    for (int w = 0; w < NW; w++) {
      b += red_s[1][w];
      q += red_s[0][w];
    }
    out[FF * N2] = b;
    sqs[blockIdx.x] = q;
  }
}
