// fwd_l123.hpp -- the fused forward's region kernel on fp32 MFMAs, for every
// net of the forward (the plan takes it where x6 is off: fp32 arithmetic, the
// example net).  Included by forward_fused.hip inside namespace srcnn::fused,
// after fwd_layout.hpp (FwdGeom, FwdLds, kFwdXs) and fwd_region.hpp (what it
// shares with fwd_l123x6); uses forward_fused.hip's mfma names and g_clk_fwd.
// The file comment of forward_fused.hip describes the region scheme.
constexpr int kFwdPD = 4;      // L1 X-gather prefetch distance (k-steps), pinned by sched barriers

template <int N1, int N2, int F1, int F3>
__global__ __launch_bounds__(256, 2) void fwd_l123_kernel(
    const float* __restrict__ X, const float* __restrict__ W1, const float* __restrict__ B1,
    const float* __restrict__ W2, const float* __restrict__ B2, const float* __restrict__ W3,
    float* __restrict__ part, FwdGeom g) {
  using L = FwdLds<F3>;  // the four static arrays' extents; why Q^T's row stride is 52 stands there
  constexpr int K1 = F1 * F1, KS1 = (K1 + 1) / 2, NT1 = N1 / 32;
  constexpr int K3 = F3 * F3;
  constexpr int TW = kFwdRW + F1 - 1;  // LDS row stride of the input tile
  constexpr int EW = L::EW, EHM = L::EHM, QTS = L::QTS;
  static_assert(K3 <= 32 && N2 <= 32 && N2 % 2 == 0 && K1 % 2 == 1, "Q tile shape");
  __shared__ float xs[L::xs];
  // L2 bias as the accumulator's initial value: register r of half h is
  // channel crow(r, h) (one 16x32 image, read as 4 broadcast 16-B loads)
  // instead of one more MFMA (b2 x 1) per chunk; the same fp32 values
  __shared__ __attribute__((aligned(16))) float b2i[2][L::b2i / 2];
  __shared__ __attribute__((aligned(16))) float qs[L::kWaves][32][QTS];
  __shared__ float accs[F3][EHM][EW];  // [dy][partial row][partial col]
  static_assert(sizeof(xs) + sizeof(b2i) + sizeof(qs) + sizeof(accs) == L::bytes, "FwdLds");

  SRCNN_CLOCK_BEGIN();
  const int lane = mfma::lane_id(), wave = mfma::wave_id();
  const int h = lane >> 5, li = lane & 31;
  const int EH = g.rh + F3 - 1;
  for (int i = threadIdx.x; i < 4 * 32 * 2 * (F3 - 1); i += 256) {  // the zero columns (never written again)
    const int w = i / (64 * (F3 - 1)), r = (i / (2 * (F3 - 1))) % 32, col = i % (2 * (F3 - 1));
    qs[w][r][col < F3 - 1 ? col : kFwdRW + col] = 0.0f;
  }
  // L3 window sums (fwd_region.hpp): this lane's items k of the F3 x EW (tap row
  // dy, column e) per chunk, as a base into the wave's Q image (32 rows a wave;
  // taps dx follow at a stride of QTS + 1 floats) and into the partial-sum
  // accumulator (+ chunk row c * EW)
  constexpr int kWin = fwd_win_items<F3>();
  int wrb[kWin], wwb[kWin];
#pragma unroll
  for (int k = 0; k < kWin; k++) {
    const int it = min(lane + 64 * k, F3 * EW - 1), dy = it / EW, e = it - dy * EW;
    wrb[k] = (wave * 32 + dy * F3) * QTS + e;
    wwb[k] = (dy * EHM + F3 - 1 - dy) * EW + e;
  }

  // All three GEMMs run TRANSPOSED (rows = channels / taps, cols = the
  // chunk's 32 pixels), so each layer's accumulator registers are the next
  // layer's B operand as they stand (register s of half h is row crow(s, h),
  // mfma.hpp) -- no LDS transposes between L1, L2 and Q:
  //   A operands: W1[tap = 2s+h][ch = 32t+li] (tap K1 = the bias slot, X = 1),
  //               W2[c = 32t + crow(s,h)][n = li] (+ one bias MFMA),
  //               W3[tap = li][c = crow(s,h)]
  float w1f[KS1][NT1];
#pragma unroll
  for (int s = 0; s < KS1; s++)
#pragma unroll
    for (int t = 0; t < NT1; t++) {
      const int tap = 2 * s + h;
      w1f[s][t] = tap < K1 ? W1[tap * N1 + 32 * t + li] : B1[32 * t + li];
    }
  float w2f[NT1][16];
#pragma unroll
  for (int t = 0; t < NT1; t++)
#pragma unroll
    for (int s = 0; s < 16; s++) w2f[t][s] = li < N2 ? W2[(32 * t + crow(s, h)) * N2 + li] : 0.0f;
  if (threadIdx.x < 32) {
    const int c_ = crow(threadIdx.x & 15, threadIdx.x >> 4);
    b2i[threadIdx.x >> 4][threadIdx.x & 15] = c_ < N2 ? B2[c_] : 0.0f;
  }
  float w3f[16];
#pragma unroll
  for (int s = 0; s < 16; s++) {
    const int cc = crow(s, h);
    w3f[s] = (li < K3 && cc < N2) ? W3[li * N2 + cc] : 0.0f;
  }

  const int per_frame = g.nrx * g.nry;
  const int n_items = g.batch * per_frame;
  // The next region's input tile is register-staged while this region's
  // chunks run (its loads retire under the MFMAs instead of stalling the
  // block between regions).
  constexpr int kXR = (kFwdXs + 255) / 256;
  float xr[kXR];
  auto xload = [&](int wi) { fwd_xload<256, TW, F1>(X, g, per_frame, wi, xr); };
  if ((int)blockIdx.x < n_items) xload(blockIdx.x);
  for (int wi = blockIdx.x; wi < n_items; wi += gridDim.x) {
    const int crh = fwd_item_rows(g, per_frame, wi);

    __syncthreads();  // the previous region's readers are done with xs / accs
#pragma unroll
    for (int k = 0; k < kXR; k++) {
      const int i = threadIdx.x + 256 * k;
      if (i < kFwdXs) xs[i] = xr[k];
    }
    __syncthreads();
    if (wi + (int)gridDim.x < n_items) xload(wi + gridDim.x);

    // The L3 window sums of a chunk run inside this wave's NEXT chunk's L1
    // MFMA stream (its Q^T stays in the wave's scratch until that chunk's own
    // Q overwrites it): read at k-steps kWinS + kWinD k, summed and stored
    // kWinD / 2 steps later.  Issued after the Q MFMAs they were a ~500-cycle
    // LDS / VALU tail per chunk with no MFMA of this wave behind it.
    constexpr int kWinS = 2, kWinD = (KS1 - kWinS - 4) / kWin;
    static_assert(kWinD >= 2 && kWinS + kWinD * kWin + kWinD / 2 < KS1, "window sums fit the L1 stream");
    auto win_read = [&](int k, float* v) { fwd_win_read<F3, QTS>(&qs[0][0][0], wrb[k], v); };
    auto win_store = [&](int k, const float* v, int pc) {
      fwd_win_store<F3, kWin>(&accs[0][0][0], lane, k, wwb[k], v, pc);
    };
    int pc = -1;  // this wave's chunk whose window sums are pending (wave-uniform)
    float wv_last[F3];
    for (int c = wave; c < crh; c += 4) {  // chunk = region row c, pixel li
      // tap 2s+1 sits 1 or TW - F1 + 1 floats past tap 2s: two per-half bases,
      // every gather is base + immediate
      const int xbA = c * TW + li + h, xbB = xbA + h * (TW - F1);
      f32x16 acc1[NT1];
#pragma unroll
      for (int t = 0; t < NT1; t++) acc1[t] = zero16();
      // B operand of k-step s (tap K1 = the bias slot)
      auto xg = [&](int s) {
        const int k0 = 2 * s;
        const int o0 = (k0 / F1) * TW + (k0 % F1);
        const float v = xs[((k0 % F1) + 1 < F1 ? xbA : xbB) + o0];
        return s == KS1 - 1 ? (h ? 1.0f : v) : v;
      };
      // gathers run kFwdPD k-steps ahead of their MFMAs, pinned by sched
      // barriers: left alone, the scheduler issues each one just before its
      // MFMA pair and the wave waits out the full LDS latency every step
      float xq[KS1];
      float wv[F3];
#pragma unroll
      for (int s = 0; s < kFwdPD && s < KS1; s++) xq[s] = xg(s);
#pragma unroll
      for (int s = 0; s < KS1; s++) {
        if (s + kFwdPD < KS1) xq[s + kFwdPD] = xg(s + kFwdPD);
        if (pc >= 0 && s >= kWinS && (s - kWinS) % kWinD == 0 && (s - kWinS) / kWinD < kWin)
          win_read((s - kWinS) / kWinD, wv);
        __builtin_amdgcn_sched_barrier(0);
        const float xv = xq[s];
#pragma unroll
        for (int t = 0; t < NT1; t++) acc1[t] = mma(w1f[s][t], xv, acc1[t]);
        if (pc >= 0 && s >= kWinS + kWinD / 2 && (s - kWinS - kWinD / 2) % kWinD == 0 &&
            (s - kWinS - kWinD / 2) / kWinD < kWin)
          win_store((s - kWinS - kWinD / 2) / kWinD, wv, pc);
        __builtin_amdgcn_sched_barrier(0);
      }
      // L1 ReLU (layer_uber_kernel.cl:88-95; bias already in)
#pragma unroll
      for (int t = 0; t < NT1; t++)
#pragma unroll
        for (int r = 0; r < 16; r++)
          acc1[t][r] = fmaxf(acc1[t][r], 0.0f);
      // L2^T: A2^T[n][p] = B2[n] + sum_c W2[c][n] A1^T[c][p], then ReLU
      f32x16 acc2;
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const mfma::f32x4 v_ = *reinterpret_cast<const mfma::f32x4*>(&b2i[h][4 * q]);
#pragma unroll
        for (int e = 0; e < 4; e++) acc2[4 * q + e] = v_[e];
      }
#pragma unroll
      for (int t = 0; t < NT1; t++)
#pragma unroll
        for (int s = 0; s < 16; s++) acc2 = mma(w2f[t][s], acc1[t][s], acc2);
#pragma unroll
      for (int r = 0; r < 16; r++)
        acc2[r] = fmaxf(acc2[r], 0.0f);
      // Q^T[tap][p] = sum_c W3[tap][c] A2^T[c][p]
      f32x16 accq = zero16();
#pragma unroll
      for (int s = 0; s < 16; s++) accq = mma(w3f[s], acc2[s], accq);
      // Q^T[taps crow(r, h)][pixel li]: 16 rows per lane, lanes consecutive
      // (the pending window sums above read the previous Q^T: their values
      // are summed, so those reads have completed)
#pragma unroll
      for (int r = 0; r < 16; r++) qs[wave][crow(r, h)][li + F3 - 1] = accq[r];
      __builtin_amdgcn_wave_barrier();
      pc = c;
    }
    // the window sums of this wave's last chunk (fwd_region.hpp has the indexing)
    if (pc >= 0) {
#pragma unroll
      for (int k = 0; k < kWin; k++) {
        win_read(k, wv_last);
        win_store(k, wv_last, pc);
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __syncthreads();
    float* dst = part + (size_t)wi * EH * EW;
    for (int i = threadIdx.x; i < EH * EW; i += 256) dst[i] = fwd_part_sum<F3, EHM>(accs, i, crh);
  }
  SRCNN_CLOCK_END(g_clk_fwd, 0);
}
