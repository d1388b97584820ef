// l12.hpp -- kernel 1 of the fused step (L1 + L2 forward) on fp32 MFMAs, for
// every net of the family (the plan takes it where x6 is off: fp32 arithmetic,
// the minor nets, tiles l12x6 does not fit).  Included by train_fused.hip
// inside namespace srcnn::fused, after fused_layout.hpp (Geom, kL12S,
// kL12Tile, kL12Regs); uses train_fused.hip's mfma names, g_clk and kNtMask,
// and ops.hpp's LazyUpdate.
// ---------------------------------------------------------------------------
// Kernel 1: L1 (+ L2) forward, one sample per work item
// ---------------------------------------------------------------------------
// Both layers run TRANSPOSED (rows = channels, cols = the chunk's 32 pixels):
//   L1^T: A1^T[ch][p] = sum_tap W1[tap][ch] X[p + off(tap)]   A = W1 (registers),
//         B = X gathers from LDS; the padded k-slot (tap 81) reads 1.0 against
//         B1, so the bias rides in the GEMM
//   L2^T: A2^T[n][p] = sum_c W2[c][n] A1^T[c][p]   B = the L1 accumulator
//         registers as they stand (register s of half h is channel crow(s, h),
//         mfma.hpp), A = W2 (registers); one extra MFMA adds B2
// so L2 needs no LDS transpose at all, and each lane ends with consecutive
// channels of ONE pixel: A1 / A2 leave as 16-B stores straight from registers.
// L1 X-gather prefetch distance (k-steps), pinned by sched barriers
constexpr int kL12PD = 4;
// A2 leaves l12 as whole 128-B pixel rows (n2 = 32): at each chunk end the
// wave regroups its A2 tile through a 4.6 KB LDS scratch into row order (one
// write and one read per quad, a single LDS round trip per chunk), and the
// stores inside the next chunk's MFMA stream write 1 KB contiguous each.  As
// held, each store wrote 32 rows x 32 B; those stores cost 6% of l12
// (round-4 diagnostic build).  Same-box A/B (profiles/r04_ab_a2rows): l12
// 0.3068 -> 0.3049 ms, l3 0.1559 -> 0.1547 ms, step 0.8668 -> 0.8641 ms at
// batch 4096; the 512-tile shard unchanged (l12 +0.4 us)
constexpr int kL12A2S = 36;  // A2 scratch row stride (floats)
// kLazy (srcnn_train_fwd_bwd_lazy): the previous data-parallel step's SGD
// update rides in the prologue.  Every block forms the updated W1 / B1 / W2 /
// B2 it needs in registers from lz's (P, M, G) -- the same sgd_step as
// update_all_kernel, so every block holds the same values -- and writes its
// slice of the updated parameters and momentum (all six segments) to lz.Po /
// lz.Mo, which l3 and d1 read after this kernel.  No update launch between
// the gradient all-reduce and the next step.
template <int N1, int N2, int F1, bool kLazy = false>
__global__ __launch_bounds__(256, 2) void l12_fwd_kernel(
    const float* __restrict__ X, const float* __restrict__ W1, const float* __restrict__ B1,
    const float* __restrict__ W2, const float* __restrict__ B2, float* __restrict__ A1,
    float* __restrict__ A2, Geom g, LazyUpdate lz) {
  constexpr int K1 = F1 * F1, KS1 = (K1 + 1) / 2, NT1 = N1 / 32;
  static_assert(N2 <= 32 && N2 % 8 == 0 && K1 % 2 == 1 && N1 % 32 == 0,
                "transposed l12: one 32-row L2 tile, odd tap count");
  __shared__ float xs[kL12Tile];  // X tile at the fixed row stride kL12S (+ zero rows)
  constexpr bool kA2Rows = N2 == 32;  // (a row = 8 quads)
  __shared__ __attribute__((aligned(16))) float a2sc[kA2Rows ? 4 * 32 * kL12A2S : 4];
  // L2 bias as the accumulator's initial value: register r of half h is
  // channel crow(r, h) (one 16x32 image, read as 4 broadcast 16-B loads)
  // instead of one more MFMA (b2 x 1) per chunk; the same fp32 values
  __shared__ __attribute__((aligned(16))) float b2i[2][16];

  SRCNN_CLOCK_BEGIN();
  const int lane = mfma::lane_id(), wave = mfma::wave_id();
  const int h = lane >> 5, li = lane & 31;
  const int npx = g.ow * g.oh;
  const int nch = (npx + 31) / 32;
  // The next sample's X tile is register-staged during the current sample
  // (its loads retire under the MFMAs instead of stalling both barriers);
  // the LDS copy uses a fixed row stride so every L1 B operand is a per-half
  // base + immediate (tap 2s+1 sits 1 or kL12S - F1 + 1 floats past tap 2s).
  for (int i = threadIdx.x; i < kL12Tile; i += blockDim.x) xs[i] = 0.0f;
  const int xn = g.W * g.H;
  float xr[kL12Regs];
  auto xload = [&](int smp) {
    const float* src = X + (size_t)smp * xn;
#pragma unroll
    for (int k = 0; k < kL12Regs; k++) {
      const int i = threadIdx.x + 256 * k;
      xr[k] = i < xn ? src[i] : 0.0f;
    }
  };
  // (issued first: its loads are in flight under the parameter loads)
  if ((int)blockIdx.x < g.batch) xload(blockIdx.x);
  // kLazy: the updated W1 | B1 | W2 | B2 (the flat buffer's first P12
  // floats) are formed once per block into LDS, each by one thread with
  // coalesced loads; the register operands below are read from there
  constexpr int P12 = F1 * F1 * N1 + N1 + N1 * N2 + N2;
  __shared__ float lzs[kLazy ? P12 : 1];
  if constexpr (kLazy) {
    // every load of the thread in flight at once (a rolled loop waited out
    // one L2 round trip per element: l12 +9 us at one sample per block)
    constexpr int kIt = (P12 + 255) / 256;
    float lw[kIt], lm[kIt], lgr[kIt];
#pragma unroll
    for (int k = 0; k < kIt; k++) {
      const int i = threadIdx.x + 256 * k;
      if (i < P12) {
        lw[k] = lz.P[i];
        lm[k] = lz.M[i];
        lgr[k] = lz.G[i];
      }
    }
    lazy_write_slice(lz);
#pragma unroll
    for (int k = 0; k < kIt; k++) {
      const int i = threadIdx.x + 256 * k;
      if (i < P12) {
        const int seg = param_seg(lz.off, i);
        sgd_step(lw[k], lm[k], seg, lgr[k], lz.lr[seg >> 1], lz.mu, lz.wd, lz.batch);
        lzs[i] = lw[k];
      }
    }
    __syncthreads();
  }
  // parameter i of segment seg (W1 0, B1 1, W2 2, B2 3) as this step uses it
  auto prm = [&](int seg, int i) -> float {
    if constexpr (kLazy) return lzs[(seg > 0 ? K1 * N1 : 0) + (seg > 1 ? N1 : 0) + (seg > 2 ? N1 * N2 : 0) + i];
    return (seg == 0 ? W1 : seg == 1 ? B1 : seg == 2 ? W2 : B2)[i];
  };

  // A operands of L1^T: W1[tap = 2s + h][ch = 32t + li]; tap K1 is the bias slot
  // (W1 in registers: read from LDS at each MFMA instead, for a third wave
  // per SIMD, l12 ran 0.323-0.325 vs 0.307 ms)
  float w1f[KS1][NT1];
#pragma unroll
  for (int s = 0; s < KS1; s++)
#pragma unroll
    for (int t = 0; t < NT1; t++) {
      const int tap = 2 * s + h;
      w1f[s][t] = tap < K1 ? prm(0, tap * N1 + 32 * t + li) : prm(1, 32 * t + li);
    }
  // A operands of L2^T: W2[c = 32t + crow(s, h)][n = li]; bias MFMA: B2[li] (half 0)
  float w2f[NT1][16];
#pragma unroll
  for (int t = 0; t < NT1; t++)
#pragma unroll
    for (int s = 0; s < 16; s++) w2f[t][s] = li < N2 ? prm(2, (32 * t + crow(s, h)) * N2 + li) : 0.0f;
  if (threadIdx.x < 32) {
    const int c_ = crow(threadIdx.x & 15, threadIdx.x >> 4);
    b2i[threadIdx.x >> 4][threadIdx.x & 15] = c_ < N2 ? prm(3, c_) : 0.0f;
  }

  for (int sample = blockIdx.x; sample < g.batch; sample += gridDim.x) {
    __syncthreads();  // previous sample's readers are done with xs
#pragma unroll
    for (int k = 0; k < kL12Regs; k++) {
      const int i = threadIdx.x + 256 * k;
      if (i < xn) {
        const int y = i / g.W;
        xs[y * kL12S + i - y * g.W] = xr[k];
      }
    }
    __syncthreads();
    if (sample + (int)gridDim.x < g.batch) xload(sample + gridDim.x);

    // Software-pipelined stores: chunk c's A1 / A2 rows (12 16-B stores per
    // lane) are issued one at a time inside chunk c+1's L1 MFMA stream, so
    // the write traffic streams out under the matrix core instead of in a
    // burst that stalls the wave between chunks.
    constexpr int NST = 4 * NT1 + N2 / 8;  // 16-B stores per lane per chunk
    f32x16 pa1[NT1], pa2 = zero16();
#pragma unroll
    for (int t = 0; t < NT1; t++) pa1[t] = zero16();
    bool pok = false;    // a chunk is pending (wave-uniform)
    bool pval = false;   // ... and this lane's pixel is inside the sample (A2)
    float* pa1p = A1;
    float* pa2p = A2;
    int pc0 = 0;  // kA2Rows: the pending chunk's first pixel
    auto store_prev = [&](int k) {  // store k of the pending chunk (exec-masked)
      if (pok) {
        if (k < 4 * NT1) {
          // blocked A1 (internal to the fused step, read only by d1): block k
          // of a chunk is 64 lanes x 16 B in lane order, one contiguous 1-KB
          // store; lanes past the sample store their clamped pixel's copy
          const int t = k / 4, q = k % 4;
          if (kNtMask & 8) {
            f32x4 v_;
#pragma unroll
            for (int e = 0; e < 4; e++) v_[e] = pa1[t][4 * q + e];
            __builtin_nontemporal_store(v_, reinterpret_cast<f32x4*>(pa1p + 256 * k));
          } else {
            *reinterpret_cast<float4*>(pa1p + 256 * k) =
                make_float4(pa1[t][4 * q], pa1[t][4 * q + 1], pa1[t][4 * q + 2], pa1[t][4 * q + 3]);
          }
        } else if (kA2Rows && k >= 4 * NT1) {
          // row store q: pixels 8q .. 8q + 7 of the chunk, lane L -> pixel
          // 8q + L / 8, quad L % 8 (already relu'd, in pa2's quad q)
          const int q = k - 4 * NT1;
          if (pc0 + 8 * q + (lane >> 3) < npx) {
            f32x4 v_;
#pragma unroll
            for (int e = 0; e < 4; e++) v_[e] = pa2[4 * q + e];
            *reinterpret_cast<f32x4*>(pa2p + (8 * q + (lane >> 3)) * N2 + 4 * (lane & 7)) = v_;
          }
        } else if (!kA2Rows && k >= 4 * NT1 && pval) {
          const int q = k - 4 * NT1;
          *reinterpret_cast<float4*>(pa2p + 8 * q) =
              make_float4(fmaxf(pa2[4 * q], 0.0f), fmaxf(pa2[4 * q + 1], 0.0f),
                          fmaxf(pa2[4 * q + 2], 0.0f), fmaxf(pa2[4 * q + 3], 0.0f));
        }
      }
    };
    for (int c = wave; c < nch; c += 4) {
      // this lane's pixel (B-operand column li)
      const int pl = c * 32 + li;
      const int pc = min(pl, npx - 1);
      const int iy = pc / g.ow, ix = pc - iy * g.ow;
      const int xbA = iy * kL12S + ix + h, xbB = xbA + h * (kL12S - F1);

      f32x16 acc1[NT1];
#pragma unroll
      for (int t = 0; t < NT1; t++) acc1[t] = zero16();
      constexpr int kStoreEvery = (KS1 - 1) / NST;
      // B operand of k-step s (tap K1 = the bias slot)
      auto xg = [&](int s) {
        const int k0 = 2 * s;
        const int o0 = (k0 / F1) * kL12S + (k0 % F1);
        const float v = xs[((k0 % F1) + 1 < F1 ? xbA : xbB) + o0];
        return s == KS1 - 1 ? (h ? 1.0f : v) : v;
      };
      // gathers run kL12PD k-steps ahead of their MFMAs, pinned by sched
      // barriers: left alone, the scheduler issues each one just before its
      // MFMA pair and the wave waits out the full LDS latency every step
      float xq[KS1];
#pragma unroll
      for (int s = 0; s < kL12PD && s < KS1; s++) xq[s] = xg(s);
#pragma unroll
      for (int s = 0; s < KS1; s++) {
        if (s + kL12PD < KS1) xq[s + kL12PD] = xg(s + kL12PD);
        if (kL12PD > 0) __builtin_amdgcn_sched_barrier(0);
        const float xv = kL12PD > 0 ? xq[s] : xg(s);
#pragma unroll
        for (int t = 0; t < NT1; t++) acc1[t] = mma(w1f[s][t], xv, acc1[t]);
        if (s % kStoreEvery == kStoreEvery - 1 && s / kStoreEvery < NST) store_prev(s / kStoreEvery);
      }
      // ReLU (layer_uber_kernel.cl:88-95); the bias is already in
#pragma unroll
      for (int t = 0; t < NT1; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc1[t][r] = fmaxf(acc1[t][r], 0.0f);
      f32x16 acc2;
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const f32x4 v_ = *reinterpret_cast<const f32x4*>(&b2i[h][4 * q]);
#pragma unroll
        for (int e = 0; e < 4; e++) acc2[4 * q + e] = v_[e];
      }
#pragma unroll
      for (int t = 0; t < NT1; t++)
#pragma unroll
        for (int s = 0; s < 16; s++) acc2 = mma(w2f[t][s], acc1[t][s], acc2);
      // this chunk becomes the pending one; registers 4q..4q+3 of tile t are
      // channels 32t + 8q + 4h .. +3 of pixel pl
#pragma unroll
      for (int t = 0; t < NT1; t++) pa1[t] = acc1[t];
      if (kA2Rows) {
        // A2 tile -> row order through this wave's scratch: register 4m + e
        // of half h is channel 8m + 4h + e of pixel li (written relu'd); read
        // back, quad q of this lane is pixel 8q + lane/8, channels 4 (lane%8)..
        float* sc = a2sc + wave * 32 * kL12A2S;
#pragma unroll
        for (int m = 0; m < 4; m++) {
          f32x4 v_;
#pragma unroll
          for (int e = 0; e < 4; e++) v_[e] = fmaxf(acc2[4 * m + e], 0.0f);
          *reinterpret_cast<f32x4*>(sc + li * kL12A2S + 8 * m + 4 * h) = v_;
        }
        // other lanes' values are read back: no compiler motion across this
        // point (the wave's LDS operations themselves complete in order)
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const f32x4 v_ = *reinterpret_cast<const f32x4*>(sc + (8 * q + (lane >> 3)) * kL12A2S + 4 * (lane & 7));
#pragma unroll
          for (int e = 0; e < 4; e++) pa2[4 * q + e] = v_[e];
        }
        pc0 = c * 32;
      } else {
        pa2 = acc2;
      }
      pok = true;
      pval = pl < npx;
      pa1p = A1 + ((size_t)sample * nch + c) * (32 * N1) + 4 * lane;
      pa2p = kA2Rows ? A2 + ((size_t)sample * npx + c * 32) * N2 : A2 + ((size_t)sample * npx + pc) * N2 + 4 * h;
    }
#pragma unroll
    for (int k = 0; k < NST; k++) store_prev(k);
    pok = false;
  }
  SRCNN_CLOCK_END(g_clk, 0);
}
