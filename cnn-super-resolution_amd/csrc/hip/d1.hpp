// d1.hpp -- kernel 3 of the fused step (delta1 + gW2/gB2 + gW1/gB1) on fp32
// MFMAs, one wave per chunk, for every net of the family (the plan takes it
// where neither d1x6 nor d1c serves: the minor nets, tiles past d1c's).
// Included by train_fused.hip inside namespace srcnn::fused, after
// fused_layout.hpp (Geom, kXsMax); uses train_fused.hip's mfma names, g_clk
// and kNtMask.  Reads the blocked A1 that l12_fwd_kernel writes (l12.hpp).
// ---------------------------------------------------------------------------
// Kernel 3: delta1 + gW2/gB2 + gW1/gB1
//
// Per 32-pixel chunk (one wave):
//   delta1 = delta2 . W2^T      16x16x4 MFMA, M = pixels (2 tiles), N = n1
//                               channels (n1/16 tiles), K = n2
//   gW2 += A1^T . delta2        32x32x2 MFMA, M = n1, N = n2, K = pixels
//   relu' mask of delta1        A1 from the same LDS image
//   gW1 += Xwin^T . delta1      16x16x4 MFMA, M = taps 0..16*MT-1, N = n1,
//                               K = pixels; delta1's C registers are the B
//                               operand as they stand (register i of lane
//                               group j is pixel 4j + i of the tile)
//   the f1*f1 - 16*MT remaining taps and gB1 (= the ones row) by VALU FMAs
//                               on the same registers
// With f1 = 9 that is 80 MFMA taps + 1 VALU tap, where a 32-row tap tiling
// issues 96 rows (81 taps + ones row + 14 pad): 1/6 fewer gW1 MFMA cycles.
// ---------------------------------------------------------------------------
// gW1 k-steps the next work item's operand DMA is spread over (1, 2 or 4
// measured 0.4-0.7% slower)
constexpr int kD1DmaSteps = 8;
template <int N1, int N2, int F1>
__global__ __launch_bounds__(256, 2) void d1_grad12_kernel(
    const float* __restrict__ X, const float* __restrict__ A1, const float* __restrict__ D2,
    const float* __restrict__ W2, float* __restrict__ slab, Geom g) {
  constexpr int K1 = F1 * F1, NT1 = N1 / 32, NT2 = (N2 + 31) / 32;
  // quad swizzle of A1 image row r (bits 2 and 3 of r -> quad bits 3 and 2)
  auto a1sw = [](int r) { return ((((r >> 2) & 1) << 3) | (((r >> 3) & 1) << 2)) & (N1 / 4 - 1); };
  // quad swizzle of delta2 image row r
  auto d2sw = [](int r) { return (r >> 1) & (N2 / 4 - 1); };
  constexpr int NQ = N1 / 16;             // 16-wide channel tiles
  constexpr int MT = K1 / 16;             // 16-tap MFMA tiles
  constexpr int KR = K1 - 16 * MT;        // taps left to the VALU
  constexpr int KD = N2 / 4;              // delta1 k-steps (over n)
  // delta2 LDS image rows: N2 floats, quads of row r XOR-swizzled by
  // d2sw(r) = (r >> 1) mod N2/4 (a padded image cost one DMA per chunk more)
  constexpr int DS = N2;
  constexpr int WS = N2 + 1;              // W2 image (N1 * N2 floats) within N1 * WS
  constexpr int NW1 = K1 * N1, NW2 = N1 * N2;
  constexpr int P12 = NW1 + N1 + NW2 + N2;  // [gW1 | gB1 | gW2 | gB2]
  static_assert(N2 % 4 == 0 && N1 % 32 == 0 && KR <= 4, "d1 tile shape");
  constexpr int RED1 = MT * NQ * 4 * 64, RED2 = NT1 * NT2 * 16 * 64, REDV = (KR + 1) * NQ * 64;
  constexpr int RED = RED1 + RED2 + REDV;
  // A1 LDS image rows: N1 floats with the 16-B quads of row r XOR-swizzled
  // by a1sw(r) (8 * bit 2 + 4 * bit 3 of r): the gW2 and mask reads are
  // conflict-free, one DMA instruction per chunk fewer than padded rows
  constexpr int A1P = N1;
  constexpr int A1K = (32 * A1P + 255) / 256;  // 16-byte DMA instructions per A1 chunk
  constexpr int A1S = 256 * A1K;               // per-wave A1 staging
  constexpr int D2S = 32 * DS;                 // per-wave delta2 chunk image [32][DS]
  constexpr int D2K = (D2S + 255) / 256;       // 16-byte DMA instructions per chunk
  constexpr int D2P = 256 * D2K;               // per-wave staging stride (whole DMA instructions)
  constexpr int LDS_MAIN = 4 * A1S + 2 * kXsMax + N1 * WS + 4 * D2P;
  constexpr int LDS_TOTAL = LDS_MAIN > RED ? LDS_MAIN : RED;
  __shared__ __attribute__((aligned(16))) float smem[LDS_TOTAL];
  float* a1s = smem;                   // [4][32][A1P], lane-linear DMA image of A1 rows
  float* xsb = smem + 4 * A1S;         // [2][kXsMax]: X tile, double-buffered over samples
  float* w2s = xsb + 2 * kXsMax;       // [N1][WS]: W2[c][n]
  float* d2w = w2s + N1 * WS;          // [4][32][DS]

  SRCNN_CLOCK_BEGIN();
  const int lane = mfma::lane_id(), wave = mfma::wave_id();
  const int h = lane >> 5, li = lane & 31;
  const int lq = lane & 15, lg = lane >> 4;  // 16x16x4 operand row / k group
  const int npx = g.ow * g.oh;
  // (q + 0.5) / ow in fp32 is at least 0.5/ow away from an integer for the
  // pixel counts here, so the truncation is an exact q / ow
  const float inv_ow = 1.0f / (float)g.ow;

  // W2 as the delta1 B-operand image: [k-step s][lane][channel tile t] holds
  // W2[c = 16t + lq][n = 4s + lg], so each k-step's NQ operands of a lane are
  // one contiguous (conflict-free) 16-B read (NQ = 4) instead of NQ 2-way
  // conflicted 4-B reads
  for (int i = threadIdx.x; i < N1 * N2; i += blockDim.x) {
    const int t = i % NQ, l = (i / NQ) % 64, sk = i / (NQ * 64);
    w2s[i] = W2[(16 * t + (l & 15)) * N2 + 4 * sk + (l >> 4)];
  }
  // gW1 A-operand rows of this lane: taps 16m + lq
  int toff[MT];
#pragma unroll
  for (int m = 0; m < MT; m++) {
    const int tap = 16 * m + lq;
    toff[m] = (tap / F1) * g.W + (tap % F1);
  }

  f32x4 g1[MT][NQ];
  f32x16 g2[NT1][NT2];
#pragma unroll
  for (int m = 0; m < MT; m++)
#pragma unroll
    for (int t = 0; t < NQ; t++) g1[m][t] = mfma::zero4();
#pragma unroll
  for (int t = 0; t < NT1; t++)
#pragma unroll
    for (int u = 0; u < NT2; u++) g2[t][u] = zero16();
  float gb2[NT2], gv[KR + 1][NQ];  // gv[r < KR]: tap 16*MT + r; gv[KR]: gB1
#pragma unroll
  for (int u = 0; u < NT2; u++) gb2[u] = 0.0f;
#pragma unroll
  for (int r = 0; r <= KR; r++)
#pragma unroll
    for (int t = 0; t < NQ; t++) gv[r][t] = 0.0f;

  float* d2me = d2w + wave * D2P;
  float* a1me = a1s + wave * A1S;
  // One LDS-DMA instruction K of a chunk's operands (no registers):
  //   K < A1K: A1 block K of the chunk (blocked layout, see l12) -> this
  //            wave's image, one 1-KB block per instruction (16 B / lane;
  //            the 4-float pad of each row re-reads its first quad)
  //   K >= A1K: delta2 rows -> this wave's padded [32][DS] image (16 B / lane;
  //            the pad quad re-reads quad 0, lanes past the image write into
  //            the staging padding; 2-way bank conflicts on the 16 delta1
  //            operand reads per chunk, 13 fewer DMA instructions)
  // Rows past the sample re-read its last row (A1: finite, and the delta2
  // rows there are zeroed in LDS before use).
  constexpr int kDmaK = A1K + D2K;
#define SRCNN_D1_DMA_K(SMP, C, K)                                                 \
  do {                                                                            \
    int l_ = lane; /* opaque: the address is formed here, never held */           \
    asm volatile("" : "+v"(l_));                                                  \
    /* wave-uniform chunk bases (SGPRs) + 32-bit per-lane offsets: the DMA */     \
    /* takes the saddr form, no 64-bit address math per instruction */           \
    const int rmax_ = npx - 1 - (C) * 32;                                         \
    const size_t px0_ = (size_t)(SMP) * npx + (size_t)(C) * 32;                   \
    if ((K) < A1K) {                                                              \
      /* image quad f = row r, slot q of the [32][A1P] image (slot q holds */   \
      /* quad q ^ a1sw(r)); in the blocked chunk, quad j of pixel r is lane */   \
      /* r + 32(j & 1) of block j >> 1: 64-B runs of 4 pixels per half-block */  \
      const uint32_t f_ = (K) * 64 + (uint32_t)l_;                                \
      const uint32_t r_ = f_ / (A1P / 4), j0_ = f_ - r_ * (A1P / 4);              \
      const uint32_t j_ = j0_ ^ (uint32_t)a1sw(r_);                              \
      const uint32_t off_ = (j_ >> 1) * 256 + 4 * (min(r_, 31u) + 32 * (j_ & 1u)); \
      __builtin_amdgcn_global_load_lds(                                           \
          (const void*)(A1 + ((size_t)(SMP) * nch + (C)) * (32 * N1) + off_),     \
          (__attribute__((address_space(3))) void*)(a1me + (K) * 256), 16, 0,      \
          (kNtMask & 4) ? 2 : 0);                                                 \
    } else {                                                                      \
      /* delta2 rows, 16 B / lane: slot quad Q of the [32][DS] image is row */   \
      /* Q / (DS/4), slot Q % (DS/4) holding quad slot ^ d2sw(row) */            \
      const uint32_t q_ = 64 * ((K) - A1K) + (uint32_t)l_;                        \
      const uint32_t r_ = q_ / (DS / 4), j0_ = q_ - r_ * (DS / 4);                \
      const uint32_t j_ = j0_ ^ (uint32_t)d2sw(r_);                               \
      const uint32_t off_ = (uint32_t)min((int)r_, rmax_) * N2 + (j_ < N2 / 4 ? 4 * j_ : 0u); \
      __builtin_amdgcn_global_load_lds(                                           \
          (const void*)(D2 + px0_ * N2 + off_),                                   \
          (__attribute__((address_space(3))) void*)(d2me + 256 * ((K) - A1K)), 16, 0, \
          (kNtMask & 4) ? 2 : 0);                                                 \
    }                                                                             \
  } while (0)
#define SRCNN_D1_DMA_ALL(SMP, C)                                                  \
  do {                                                                            \
    _Pragma("unroll") for (int k_ = 0; k_ < kDmaK; k_++) SRCNN_D1_DMA_K(SMP, C, k_); \
  } while (0)
  const int nch = (npx + 31) / 32;

  // X tile of a sample -> xs buffer by 4-byte LDS-DMA (lane-linear)
  const int xn = g.W * g.H, xk = (xn + 63) / 64;
#define SRCNN_D1_X_DMA(SMP, DST)                                                  \
  do {                                                                            \
    int l_ = lane;                                                                \
    asm volatile("" : "+v"(l_));                                                  \
    const float* src_ = X + (size_t)(SMP) * xn;                                   \
    for (int k_ = wave; k_ < xk; k_ += 4)                                         \
      if (64 * k_ + l_ < xn)                                                      \
        __builtin_amdgcn_global_load_lds(                                         \
            (const void*)(src_ + 64 * k_ + l_),                                   \
            (__attribute__((address_space(3))) void*)((DST) + 64 * k_), 4, 0, 0); \
  } while (0)

  // software pipeline across samples: a wave's next (sample, chunk) operands
  // are always in flight while it computes the current one; the next
  // sample's X tile streams into the other buffer meanwhile
  if ((int)blockIdx.x < g.batch) {
    SRCNN_D1_X_DMA(blockIdx.x, xsb);
    if (wave < nch) SRCNN_D1_DMA_ALL(blockIdx.x, wave);
  }
  int xbuf = 0;
  for (int sample = blockIdx.x; sample < g.batch; sample += gridDim.x, xbuf ^= 1) {
    // this sample's X tile (every wave's share) has landed; the previous
    // sample's readers of the other X buffer are done.  A wave with chunks
    // issued its share of this X tile before at least kDmaK operand DMAs
    // (those of its next chunk are the most recent), so vmcnt(kDmaK) is
    // enough: the next chunk's operands need not land before the barrier.
    // (__syncthreads() would add its own vmcnt(0): a bare s_barrier after
    // explicit waits; lgkmcnt(0) retires this wave's X reads of the buffer
    // the others are about to refill)
    if (wave >= nch) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    } else {
      asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(kDmaK) : "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
    }
    const float* xs = xsb + xbuf * kXsMax;
    const int next = sample + (int)gridDim.x;
    const bool has_next = next < g.batch;
    if (has_next && wave >= nch) SRCNN_D1_X_DMA(next, xsb + (xbuf ^ 1) * kXsMax);

    for (int c = wave; c < nch; c += 4) {
      // this chunk's operand DMA has landed
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_wave_barrier();
      if (c == wave && has_next) SRCNN_D1_X_DMA(next, xsb + (xbuf ^ 1) * kXsMax);
      if (c * 32 + 32 > npx) {  // delta2 rows past the sample -> 0 (one contiguous range)
        int l_ = lane;
        asm volatile("" : "+v"(l_));
        for (int i = (npx - c * 32) * DS + l_; i < D2S; i += 64) d2me[i] = 0.0f;
      }

      // delta1[p][c] = sum_n delta2[p][n] * W2[c][n]  (layer_deltas.cl, f=1)
      f32x4 d1[2][NQ];
#pragma unroll
      for (int pm = 0; pm < 2; pm++)
#pragma unroll
        for (int t = 0; t < NQ; t++) d1[pm][t] = mfma::zero4();
      // (Measured slower: these operands read one delta1/gW2 super-step ahead
      // into two register sets pinned by sched barriers -- 3 VGPR spills.)
      // swizzled delta2 image: row 16pm + lq, channel 4s + lg at dab ^ 4s + 16pm DS
      int dab = lq * DS + 4 * d2sw(lq) + lg;
      asm volatile("" : "+v"(dab));
#pragma unroll
      for (int s = 0; s < KD; s++) {
        float a[2], b[NQ];
#pragma unroll
        for (int pm = 0; pm < 2; pm++)
          a[pm] = d2me[(dab ^ (4 * s)) + 16 * pm * DS];
        if constexpr (NQ == 4) {
          const f32x4 bv = *reinterpret_cast<const f32x4*>(w2s + (s * 64 + lane) * NQ);
#pragma unroll
          for (int t = 0; t < NQ; t++) b[t] = bv[t];
        } else {
#pragma unroll
          for (int t = 0; t < NQ; t++) b[t] = w2s[(s * 64 + lane) * NQ + t];
        }
#pragma unroll
        for (int pm = 0; pm < 2; pm++)
#pragma unroll
          for (int t = 0; t < NQ; t++)
            d1[pm][t] = mfma::mma16(a[pm], b[t], d1[pm][t]);
      }
      // gW2[c][n] += sum_p A1[p][c] delta2[p][n]; gB2[n] += sum_p delta2[p][n]
      // swizzled image: pixel crow(s, h), channel 32t + li sits at
      // gw2b[t][bit 2 of s] + ((s & 3) + 8 (s >> 2)) A1P (crow's bit 2 is h)
      // swizzled delta2 image: pixel pr0 + 4h, channel li at gdb ^ 4 d2sw(pr0) + pr0 DS
      int gdb = 4 * h * DS + 4 * ((li >> 2) ^ ((2 * h) & (N2 / 4 - 1))) + (li & 3);
      asm volatile("" : "+v"(gdb));
      int gw2b[NT1][2];
      {
        int li_ = li;
        asm volatile("" : "+v"(li_));
#pragma unroll
        for (int t = 0; t < NT1; t++)
#pragma unroll
          for (int sb = 0; sb < 2; sb++)
            gw2b[t][sb] = 4 * h * A1P + 4 * ((8 * t + (li_ >> 2)) ^ a1sw(4 * h + 8 * sb)) + (li_ & 3);
      }
#pragma unroll
      for (int s = 0; s < 16; s++) {
#pragma unroll
        for (int u = 0; u < NT2; u++) {
          const int n = 32 * u + li;
          const int pr0 = (s & 3) + 8 * (s >> 2);  // crow(s, 0); pr = pr0 + 4h
          const float b = n < N2 ? d2me[(gdb ^ (4 * d2sw(pr0))) + pr0 * DS] : 0.0f;
          gb2[u] += b;
#pragma unroll
          for (int t = 0; t < NT1; t++)
            g2[t][u] = mma(a1me[gw2b[t][(s >> 2) & 1] + ((s & 3) + 8 * (s >> 2)) * A1P], b, g2[t][u]);
        }
      }

      // relu' mask of delta1 (after the independent gW2 MFMAs, so the delta1
      // chain has drained without stalling the matrix core); swizzled image:
      // row 16pm + 4lg + i, channel 16t + lq sits at mskb ^ 16t + (16pm + i) A1P
      int mskb = 4 * lg * A1P + 16 * (a1sw(4 * lg) >> 2) + 4 * (lq >> 2) + (lq & 3);
      asm volatile("" : "+v"(mskb));

#pragma unroll
      for (int pm = 0; pm < 2; pm++)
#pragma unroll
        for (int t = 0; t < NQ; t++)
#pragma unroll
          for (int i = 0; i < 4; i++)
            d1[pm][t][i] = a1me[(mskb ^ (16 * t)) + (16 * pm + i) * A1P] > 0.0f ? d1[pm][t][i] : 0.0f;

      // next chunk's operand DMA overlaps the gW1 MFMAs (the images' reads retired)
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      // gW1[tap][c] += sum_p X[p + tap] delta1[p][c].  K-step (pm, i): lane
      // group lg supplies pixel 16pm + 4lg + i.  Hand-pipelined: the X
      // gathers of step s+1 are issued before the MFMAs of step s, and the
      // operand DMA of this wave's next work item (the next chunk, or its
      // first chunk of the next sample, or when neither exists a harmless
      // re-read of this one) is spread over the steps.
      {
        const bool more = c + 4 < nch;
        const int dsmp = more ? sample : (has_next ? next : sample);
        const int dch = more ? c + 4 : (has_next ? wave : c);
        // X offset of this lane's pixel in step S (rows past the sample clamp
        // to its last pixel: their delta1 is 0)
#define SRCNN_D1_XB(S)                                                              \
  ([&]() {                                                                          \
    const int q_ = min(c * 32 + 16 * ((S) >> 2) + 4 * lg + ((S) & 3), npx - 1);    \
    const int y_ = (int)(((float)q_ + 0.5f) * inv_ow);                              \
    return q_ + y_ * (g.W - g.ow);                                                  \
  }())
        constexpr int kDmaPerStep = (kDmaK + kD1DmaSteps - 1) / kD1DmaSteps;
        float acur[MT], rcur[KR > 0 ? KR : 1];
        {
          const int xb = SRCNN_D1_XB(0);
#pragma unroll
          for (int m = 0; m < MT; m++) acur[m] = xs[xb + toff[m]];
#pragma unroll
          for (int r = 0; r < KR; r++) {
            const int tap = 16 * MT + r;
            rcur[r] = xs[xb + (tap / F1) * g.W + (tap % F1)];
          }
        }
#pragma unroll
        for (int s = 0; s < 8; s++) {
          const int pm = s >> 2, i = s & 3;
          float anxt[MT], rnxt[KR > 0 ? KR : 1];
          if (s + 1 < 8) {
            const int xb = SRCNN_D1_XB(s + 1);
#pragma unroll
            for (int m = 0; m < MT; m++) anxt[m] = xs[xb + toff[m]];
#pragma unroll
            for (int r = 0; r < KR; r++) {
              const int tap = 16 * MT + r;
              rnxt[r] = xs[xb + (tap / F1) * g.W + (tap % F1)];
            }
          }
#pragma unroll
          for (int m = 0; m < MT; m++)
#pragma unroll
            for (int t = 0; t < NQ; t++)
              g1[m][t] = mfma::mma16(acur[m], d1[pm][t][i], g1[m][t]);
#pragma unroll
          for (int t = 0; t < NQ; t++) {
#pragma unroll
            for (int r = 0; r < KR; r++) gv[r][t] = fmaf(rcur[r], d1[pm][t][i], gv[r][t]);
            gv[KR][t] += d1[pm][t][i];
          }
#pragma unroll
          for (int k = 0; k < kDmaPerStep; k++)
            if (kDmaPerStep * s + k < kDmaK) SRCNN_D1_DMA_K(dsmp, dch, kDmaPerStep * s + k);
          if (s + 1 < 8) {
#pragma unroll
            for (int m = 0; m < MT; m++) acur[m] = anxt[m];
#pragma unroll
            for (int r = 0; r < KR; r++) rcur[r] = rnxt[r];
          }
        }
#undef SRCNN_D1_XB
      }
      __builtin_amdgcn_wave_barrier();
    }
  }
#undef SRCNN_D1_DMA_K
#undef SRCNN_D1_DMA_ALL
#undef SRCNN_D1_X_DMA

  SRCNN_CLOCK_END(g_clk, 2);
  // ---- block reduction (waves in order) into LDS, then one slab per block ----
  __syncthreads();
  float* red = smem;
  for (int w = 0; w < 4; w++) {
    if (wave == w) {
      int k = 0;
#pragma unroll
      for (int m = 0; m < MT; m++)
#pragma unroll
        for (int t = 0; t < NQ; t++, k++)
#pragma unroll
          for (int r = 0; r < 4; r++) {
            float* d = red + (k * 4 + r) * 64 + lane;
            *d = (w == 0 ? 0.0f : *d) + g1[m][t][r];
          }
      k = 0;
#pragma unroll
      for (int t = 0; t < NT1; t++)
#pragma unroll
        for (int u = 0; u < NT2; u++, k++)
#pragma unroll
          for (int r = 0; r < 16; r++) {
            float* d = red + RED1 + (k * 16 + r) * 64 + lane;
            *d = (w == 0 ? 0.0f : *d) + g2[t][u][r];
          }
#pragma unroll
      for (int r = 0; r <= KR; r++)
#pragma unroll
        for (int t = 0; t < NQ; t++) {
          float* d = red + RED1 + RED2 + (r * NQ + t) * 64 + lane;
          *d = (w == 0 ? 0.0f : *d) + gv[r][t];
        }
    }
    __syncthreads();
  }
  float* out = slab + (size_t)blockIdx.x * P12;
  for (int i = threadIdx.x; i < RED1; i += blockDim.x) {  // taps 0 .. 16*MT-1
    const int k = i >> 8, r = (i >> 6) & 3, l = i & 63;
    const int m = k / NQ, t = k - m * NQ;
    out[(16 * m + 4 * (l >> 4) + r) * N1 + 16 * t + (l & 15)] = red[i];
  }
  for (int i = threadIdx.x; i < RED2; i += blockDim.x) {  // gW2
    const int k = i / 1024, r = (i >> 6) & 15, l = i & 63;
    const int t = k / NT2, u = k - t * NT2;
    const int ch = 32 * t + crow(r, l >> 5), n = 32 * u + (l & 31);
    if (n < N2) out[NW1 + N1 + ch * N2 + n] = red[RED1 + i];
  }
  for (int i = threadIdx.x; i < (KR + 1) * N1; i += blockDim.x) {  // VALU taps, gB1
    const int r = i / N1, ch = i - r * N1, t = ch >> 4;
    const float* v = red + RED1 + RED2 + (r * NQ + t) * 64 + (ch & 15);
    const float sum = ((v[0] + v[16]) + v[32]) + v[48];
    out[r < KR ? (16 * MT + r) * N1 + ch : NW1 + ch] = sum;
  }
  // gB2: combine the two lane halves, then waves in order
  __syncthreads();
#pragma unroll
  for (int u = 0; u < NT2; u++) {
    const float v = gb2[u] + __shfl_down(gb2[u], 32, 64);
    if (h == 0) red[(wave * NT2 + u) * 32 + li] = v;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < NT2 * 32; i += blockDim.x) {
    const int u = i / 32, n = 32 * u + (i & 31);
    if (n < N2) {
      float v = 0.f;
      for (int w = 0; w < 4; w++) v += red[(w * NT2 + u) * 32 + (i & 31)];
      out[NW1 + N1 + NW2 + n] = v;
    }
  }
}
