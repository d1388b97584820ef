// l3r.hpp -- fused kernel 2 of train_fused.hip for n2 = 32 (round 4; included
// inside namespace srcnn::fused after fused_layout.hpp -- its LDS layout
// L3RLds, the kL3R* sizes, L3Geom -- and l3_delta.hpp, whose l3_order it
// shares; uses train_fused.hip's g_clk).  Same mathematics and outputs as
// l3_delta_kernel:
//   L3 forward       layer_uber_kernel.cl:70-91 (SKIP_RELU), Q trick
//   last delta       last_layer_delta.cl:34-48 (relu' quirk on a linear layer)
//   squared error    squared_error.cl:60-69
//   delta2           layer_deltas.cl:79-123, MFMA over the f3*f3 taps
//   gW3 / gB3        backpropagate.cl:89-112, MFMA over the A2 pixels
// but with the sample's A2 tile held in REGISTERS instead of an LDS image.
//
// Why: l3_delta keeps two 80 KB A2 images in LDS (this sample's and the next
// one's, filled by DMA), so it runs one block per CU and its three
// barrier-separated phases (Q MFMAs, window sums, delta2/gW3 MFMAs) never
// overlap anything: 0.47 of its HBM roof.  Every A2 access of the kernel is
// per pixel except gW3's B operand (K = pixels), so A2 need not be in LDS at
// all:
//   - lane (lq, lg) of the wave owning 16-pixel unit u holds pixel 16u + lq,
//     channels [4lg, 4lg+4) and [16+4lg, 16+4lg+4) (two 16-B loads);
//   - those eight registers are the A operand of Q = A2 . W3^T (k-step s
//     <-> channel chan(s, lg)) AND, in the delta2 phase, exactly the relu'
//     mask of the transposed delta2 tile the same lane holds;
//   - gW3's B operand is made per unit through a 2.5 KB per-wave transpose
//     scratch (eight ds_write_b32, two ds_read_b128), aliased onto the Q image
//     that the window sums have consumed by then.
// LDS is then the Q image (62.5 KB), W3 as the Q B operand image (3.6 KB) and
// the delta3 grid: 70 KB, so TWO blocks share a CU and one block's barrier
// phases run under the other's MFMAs.  A2 of the block's next sample is
// loaded into the same registers unit by unit as the delta2 phase releases
// them, so the loads overlap the delta2 / gW3 MFMAs and the window sums.
//
// n2 = 32 and tiles of up to 40 16-pixel units (625-pixel A2: 33x33 samples
// at f1 = 9); other shapes keep l3_delta_kernel.

// delta2 k-slot (s, lg) -> tap, chosen so that the delta3 window offset of a
// slot is a per-lane base plus an immediate: for s < F3, lane group lg takes
// tap row dy = lg, dx = s; f3 = 5 puts row 4 in slots s = 5, 6 (dx = 4(s-5) + lg).
// -1: an unused slot (zero weight).
template <int F3>
__host__ __device__ constexpr int l3r_tap(int s, int lg) {
  return s < F3 ? (lg < F3 ? lg * F3 + s : -1)
                : (F3 == 5 && s < 7 && 4 * (s - 5) + lg < 5 ? 20 + 4 * (s - 5) + lg : -1);
}
template <int F3>
constexpr int l3r_kt() { return F3 == 5 ? 7 : F3; }

// A2 loads and D2 stores with the nontemporal hint (A2 is read once here,
// D2 once by d1): l3 0.1578 / 0.1577 -> 0.1555 / 0.1552 ms against plain
// ones (same-box A/B, profiles/r04_ab_l3r/ab_l3r6)
__device__ __forceinline__ f32x4 ld_a2(const float* p) {
  return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
}
__device__ __forceinline__ void st_d2(float* p, f32x4 v) {
  __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(p));
}

// kD3Out (the split-bf16 step): no delta2 here -- the kernel writes the
// last delta (delta3, w3 x h3 per sample) to D2 instead and d1x6 forms delta2
// from it (d1x6.hpp), so the 328 MB of delta2 per 4096-tile step never make
// an HBM round trip and this kernel keeps Q, the window sums and gW3.  It
// also writes M2, layer 2's relu' mask as one dword per A2 pixel (bit n =
// A2[pixel][n] > 0), so d1x6 need not read A2 for it, and d3max[block], the
// largest |delta3| over the block's samples, for d1x6's launch scale.
template <int F3, bool kD3Out>
__global__ __launch_bounds__(kL3RThreads, 4) void l3r_delta_kernel(  // two 8-wave blocks per CU (128 VGPRs)
    const float* __restrict__ A2, const float* __restrict__ T, const float* __restrict__ W3,
    const float* __restrict__ B3, float* __restrict__ D2, float* __restrict__ slab3,
    float* __restrict__ sq_slab, float* __restrict__ A3out, uint32_t* __restrict__ M2,
    float* __restrict__ d3max, L3Geom g) {
  constexpr int N2 = 32;
  constexpr int K3 = F3 * F3;
  constexpr int TT = (K3 + 15) / 16;  // 16-wide tap tiles
  constexpr int NT = 2;               // 16-wide channel tiles
  constexpr int KT = l3r_kt<F3>();    // delta2 k-steps (over tap slots)
  constexpr int NW3 = K3 * N2;        // gW3 size; slab row = NW3 + 1 (gB3)
  constexpr int nwaves = kL3RThreads / 64;
  static_assert(K3 <= 32, "taps must fit two 16-wide MFMA tiles");
  SRCNN_CLOCK_BEGIN();
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int npx2 = g.w2 * g.h2;
  const L3RLds<F3> L(g.w2, g.h2);
  const int d3off = L.d3off;
  float* qs = smem;                        // Q[q][tap]
  float* w3s = smem + L.qreg;              // W3[tap][c] at row stride kL3RW3S
  float* wds = w3s + L.w3img;              // W3[tap(s, lg)][c] at c * kL3RWdS + 8 lg + s
  float* d3g = wds + L.wdimg + 4;          // delta3 on the A2 grid (l3_delta.hpp)
  float* red = smem;                       // end-of-kernel reduction scratch

  const int tid = threadIdx.x;
  const int lane = mfma::lane_id(), wave = mfma::wave_id();
  const int lq = lane & 15, lg = lane >> 4;
  const int pad = (g.W - g.w3) / 2;  // last_layer_delta.cl:25
  const int nout = g.w3 * g.h3;

  for (int i = tid - 4; i < L.nd3 - 4; i += kL3RThreads) d3g[i] = 0.0f;
  // kD3Out: Q in split-bf16 products on v_mfma_f32_16x16x32_bf16 (one
  // k-step over the 32 channels): its B operand W3 as a split image, lane
  // (tap 16t + lq, lg), element j <-> channel chan(j, lg) = 4lg + j (j < 4),
  // 16 + 4lg + j - 4, in the space of the fp32 images (not used then).  Only
  // the TT tap tiles that Q reads are written: a second tile at f3 <= 4 would
  // run past the fp32 images of that F3 into the delta3 grid.
  __bf16* const w3q = reinterpret_cast<__bf16*>(w3s);
  static_assert(TT * 3 * 512 * 2 <= (K3 * kL3RW3S + 32 * kL3RWdS) * 4, "split Q image in the fp32 images' space");
  if constexpr (kD3Out) {
    for (int e = tid; e < TT * 64 * 8; e += kL3RThreads) {
      const int j = e & 7, L_ = (e >> 3) & 63, t = e >> 9, lq_ = L_ & 15, lg_ = L_ >> 4;
      const int ch = j < 4 ? 4 * lg_ + j : 16 + 4 * lg_ + j - 4, tq = 16 * t + lq_;
      __bf16 p[3];
      mfma::split3(tq < K3 ? W3[tq * N2 + ch] : 0.0f, p[0], p[1], p[2]);
#pragma unroll
      for (int q = 0; q < 3; q++) w3q[(t * 3 + q) * 512 + L_ * 8 + j] = p[q];
    }
  }
  for (int i = tid; i < K3 * N2; i += kL3RThreads) {
    if constexpr (kD3Out) break;
    w3s[(i / N2) * kL3RW3S + i % N2] = W3[i];
  }
  for (int i = tid; i < 32 * 32; i += kL3RThreads) {
    if constexpr (kD3Out) break;
    const int c = i >> 5, gs = i & 31, tap = l3r_tap<F3>(gs & 7, gs >> 3);
    // slot s = gs & 7 of lane group lg = gs >> 3 at 16 (s >> 2) + 4 lg + (s & 3)
    wds[c * kL3RWdS + 16 * ((gs & 7) >> 2) + 4 * (gs >> 3) + (gs & 3)] =
        (gs & 7) < KT && tap >= 0 ? W3[tap * N2 + c] : 0.0f;
  }

  auto tap_off = [&](int tap) { return tap < K3 ? (tap / F3) * g.w2 + tap % F3 : 0; };
  const float b3 = B3[0];
  // delta2^T B operand, pixel u0 + lq, slot (s, lg): delta3 at
  //   d3b0 - s            (s < F3: tap row lg, dx = s)
  //   d3b1 - 4 (s - 5)    (f3 = 5, s = 5, 6: tap row 4, dx = 4(s-5) + lg)
  // unused slots read finite values (zero weight); lanes past the tap rows
  // (f3 = 3, lg = 3) read row 0's windows
  const int d3b0 = lq + d3off - (lg < F3 ? lg : 0) * g.w2;
  const int d3b1 = lq + d3off - (F3 - 1) * g.w2 - lg;
  //  goff[t]: delta3 window of tap 16t + lq (gW3 A operand; lanes past the
  //           taps read a real window: their gW3 rows are discarded)
  int goff[TT];
#pragma unroll
  for (int t = 0; t < TT; t++) goff[t] = d3off - tap_off(16 * t + lq);
  // per-lane LDS bases of this wave's units (unit j adds the immediate 128 j;
  // LDS offsets are unsigned, so the bases sit at the lowest address read)
  int adb0 = d3b0 - (F3 - 1) + 16 * wave, adb1 = d3b1 - 4 + 16 * wave, agb[TT];
  asm volatile("" : "+v"(adb0), "+v"(adb1));
#pragma unroll
  for (int t = 0; t < TT; t++) {
    agb[t] = goff[t] + 4 * lg + 16 * wave;
    asm volatile("" : "+v"(agb[t]));
  }
  // delta2^T A operand W3[tap(s, lg)][16t + lq]: two 16-B reads per channel tile

  // Q B operand W3[tap 16t + lq][chan(s, lg)] with chan(s, lg) = 4lg + s for
  // s < 4 and 16 + 4lg + s - 4 above: two 16-B reads per tap tile
  const int wqo = lq * kL3RW3S + 4 * lg;
  // transpose scratch of this wave (channel-major, row stride kL3RScS):
  // written as channel 4lg + i (+16) of pixel lq, read as pixels 4lg..4lg+3
  // of channel 16t + lq (one 16-B read per channel tile)
  float* scw = smem + wave * (32 * kL3RScS);
  // (the three images share the row stride 36, so one lane base wqo serves
  // the Q and delta2 W3 operands and the scratch reads)
  static_assert(kL3RW3S == kL3RWdS && kL3RW3S == kL3RScS, "shared lane base");
  const int sco_w = 4 * lg * kL3RScS + lq;
  // the same scratch as [pixel][kL3RScS] rows for the D2 stores: this lane's
  // quads of pixel lq (write), whole-row quads of pixels lq & 7 (+8) (read)
  const int srw = lq * kL3RScS + 4 * lg;
  const int srr = (lq & 7) * kL3RScS + 4 * (lg + 4 * (lq >> 3));

  f32x4 gacc[TT][NT];
#pragma unroll
  for (int t3 = 0; t3 < TT; t3++)
#pragma unroll
    for (int t = 0; t < NT; t++) gacc[t3][t] = mfma::zero4();
  // kD3Out: gW3 as one 32x32 tile (lane (channel li, h), register r <-> tap
  // crow(r, h)); g3b: the delta3 window base of tap li (taps past K3 read
  // tap 0's: their rows are discarded), pixels 8h ..; g3s: scratch row li
  f32x16 g3x = zero16();
  // the split delta3 pair images (kD3Out), in the Q image past the scratches
  uint32_t* const d3p = reinterpret_cast<uint32_t*>(smem + 8 * 32 * kL3RScS);

  const int li32 = lane & 31, h32 = lane >> 5;
  const int g3b = d3off - tap_off(li32 < K3 ? li32 : 0) + 16 * wave + 8 * h32;
  const int g3s = li32 * kL3RScS + 8 * h32;
  float gb3 = 0.0f, sq = 0.0f;
  float dmx = 0.0f;  // kD3Out: this thread's largest |delta3|

  // this lane's A2 registers: unit j = wave + 8j, pixel 16u + lq, channel
  // quads lg and 4 + lg.  Past the sample's pixels a lane loads pixel lq
  // instead (finite values; no branch): such pixels' Q rows are never read,
  // their delta2 is not stored, and their delta3 windows lie past every
  // written delta3 (index >= npx2 in the zeroed grid), so they add exactly 0
  // to gW3
  f32x4 a2r[kL3RUnits][2];
  // (addresses: a wave-uniform base + one 32-bit lane offset, re-formed at
  // each use; precomputed 64-bit pointers per unit cost registers)
  // (A2 loads / D2 stores: pixel lq & 7, quad lg (lq < 8) or 4 + lg of the row)
  const bool lo8 = lq < 8;
#define SRCNN_L3R_LOAD(J, SAMPLE)                                                       \
  do {                                                                                  \
    /* formed here from an opaque lane id: hoisted out of the sample loop,  */          \
    /* the ten per-unit offsets would be held (spilled) across it           */          \
    int l_ = lane;                                                                      \
    asm volatile("" : "+v"(l_));                                                        \
    const int lo_ = ((l_ & 7) * N2 + 4 * ((l_ >> 4) + 4 * ((l_ >> 3) & 1)));            \
    const int pa_ = 16 * (wave + nwaves * (J)) + (l_ & 7);                              \
    const float* b_ = A2 + (size_t)(SAMPLE)*npx2 * N2;                                  \
    const unsigned w_ = 16 * (wave + nwaves * (J)) * N2 + lo_;                          \
    const unsigned oa_ = pa_ < npx2 ? w_ : lo_; /* else pixel lq & 7 of the sample */   \
    const unsigned ob_ = pa_ + 8 < npx2 ? w_ + 8 * N2 : lo_;                            \
    a2r[J][0] = ld_a2(b_ + oa_);                                                        \
    a2r[J][1] = ld_a2(b_ + ob_);                                                        \
  } while (0)
  // loaded as whole 128-B pixel rows (store A / B of the D2 layout below);
  // at first use the lanes lq, lq ^ 8 swap one quad so that lane (lq, lg)
  // holds quads lg and 4 + lg of pixel lq
#define SRCNN_L3R_SWAP(J)                                                               \
  do {                                                                                  \
    _Pragma("unroll") for (int i_ = 0; i_ < 4; i_++) {                                  \
      const float a_ = a2r[J][0][i_], b_ = a2r[J][1][i_];                               \
      const float r_ = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(               \
          __builtin_bit_cast(int, lo8 ? b_ : a_), 0x128, 0xF, 0xF, false));              \
      a2r[J][0][i_] = lo8 ? a_ : r_;                                                    \
      a2r[J][1][i_] = lo8 ? r_ : b_;                                                    \
    }                                                                                   \
  } while (0)

  // ground truth of this thread's L3 outputs, prefetched one sample ahead
  // (tof: the output's offset in its sample, -1 past the outputs)
  int tof[kL3RTPF];
#pragma unroll
  for (int k = 0; k < kL3RTPF; k++) {
    const int t_ = tid + k * kL3RThreads;
    const int y_ = t_ / g.w3, x_ = t_ - y_ * g.w3;
    tof[k] = t_ < nout ? (y_ + pad) * g.W + x_ + pad : -1;
  }
  float tpf[kL3RTPF];
#define SRCNN_L3R_T_PREFETCH(SAMPLE)                                                   \
  do {                                                                                 \
    const float* b_ = T + (size_t)(SAMPLE)*g.W * g.H;                                  \
    _Pragma("unroll") for (int k = 0; k < kL3RTPF; k++) {                              \
      const float x_ = b_[tof[k] >= 0 ? tof[k] : 0];                                   \
      tpf[k] = tof[k] >= 0 ? x_ : 0.f;                                                 \
    }                                                                                  \
  } while (0)

  if ((int)blockIdx.x < g.batch) {
    const int s0 = l3_order(blockIdx.x, g.batch);
#pragma unroll
    for (int j = 0; j < kL3RUnits; j++) SRCNN_L3R_LOAD(j, s0);
    SRCNN_L3R_T_PREFETCH(s0);
  }

  for (int sample = blockIdx.x; sample < g.batch; sample += gridDim.x) {
    // the previous sample's readers of the transpose scratch (= Q image) and
    // of the delta3 grid are done; a bare barrier: the next sample's A2
    // loads and this sample's D2 stores stay in flight
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    const int smp = l3_order(sample, g.batch);
    float tcur[kL3RTPF];
#pragma unroll
    for (int k = 0; k < kL3RTPF; k++) tcur[k] = tpf[k];
    const int next = sample + (int)gridDim.x;
    const bool has_next = next < g.batch;
    const int nsmp = has_next ? l3_order(next, g.batch) : smp;
    SRCNN_L3R_T_PREFETCH(nsmp);  // (a harmless re-read without a next sample)

    // ---- Q = A2 . W3^T per 16-pixel unit, A operand from registers ----
#pragma unroll
    for (int j = 0; j < kL3RUnits; j++) {
      __builtin_amdgcn_sched_barrier(0);  // no operand motion across units (registers)
      const int u = wave + nwaves * j;
      {  // every slot, also past the sample's units (zero A2, stores masked)
        const int u0 = 16 * u;
        SRCNN_L3R_SWAP(j);
        f32x4 acc[TT];
        if constexpr (kD3Out) {
          // A: the lane's 8 A2 registers (k-slot 8lg + i <-> channel chan(i, lg)), split
          mfma::bf16x8 aq[3];
          {
            float v[8];
#pragma unroll
            for (int i = 0; i < 8; i++) v[i] = a2r[j][i >> 2][i & 3];
            mfma::split8(v, aq);
          }
          const uint16_t* const wq16 = reinterpret_cast<const uint16_t*>(w3q) + lane * 8;
#pragma unroll
          for (int t = 0; t < TT; t++) {
            mfma::bf16x8 b[3];
#pragma unroll
            for (int q = 0; q < 3; q++) b[q] = *reinterpret_cast<const mfma::bf16x8*>(wq16 + (t * 3 + q) * 512);
            acc[t] = mfma::mma16_x6(aq, b, mfma::zero4());
          }
        } else {
        f32x4 wv[TT][2];
#pragma unroll
        for (int t = 0; t < TT; t++)
#pragma unroll
          for (int h = 0; h < 2; h++)
            wv[t][h] = *reinterpret_cast<const f32x4*>(w3s + wqo + 16 * t * kL3RW3S + 16 * h);
#pragma unroll
        for (int t = 0; t < TT; t++) acc[t] = mfma::zero4();
#pragma unroll
        for (int s = 0; s < 8; s++)
#pragma unroll
          for (int t = 0; t < TT; t++) acc[t] = mfma::mma16(a2r[j][s >> 2][s & 3], wv[t][s >> 2][s & 3], acc[t]);
        }
        // Q[u0 + 4lg + i][tap = 16t + lq] (rows past the sample are written
        // too, never read)
#pragma unroll
        for (int t = 0; t < TT; t++) {
          const int tap = 16 * t + lq;
          if (tap < K3) {
            float* qd = qs + (u0 + 4 * lg) * K3 + tap;
#pragma unroll
            for (int i = 0; i < 4; i++) qd[i * K3] = acc[t][i];
          }
        }
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");

    // ---- L3 = B3 + diagonal sums of Q; last delta; squared error ----
#pragma unroll
    for (int k = 0; k < kL3RTPF; k++) {
      const int t = tid + k * kL3RThreads;
      if (t < nout) {
        const int y = t / g.w3, x = t - y * g.w3;
        const float* qrow = qs + (y * g.w2 + x) * K3;
        float acc = 0.0f;
#pragma unroll
        for (int dy = 0; dy < F3; dy++)
#pragma unroll
          for (int dx = 0; dx < F3; dx++) acc += qrow[(dy * g.w2 + dx) * K3 + dy * F3 + dx];
        const float a3 = acc + b3;
        A3out[(size_t)smp * nout + t] = a3;
        const float diff = a3 - tcur[k];
        const float d3 = diff * (a3 > 0.0f ? 1.0f : 0.0f);
        d3g[y * g.w2 + x + d3off] = d3;
        if constexpr (kD3Out) {
          D2[(size_t)smp * nout + t] = d3;
          dmx = fmaxf(dmx, fabsf(d3));
        }
        gb3 += d3;
        sq += diff * diff;
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if constexpr (kD3Out) {
      // gW3's A operand pre-split once per sample: the delta3 grid as three
      // part images of bf16 pairs (dword g of part q = parts of grid g, g + 1)
      // in the Q image past the transpose scratches (Q is consumed)
      for (int gi = tid - 4; gi < L.nd3 - 5; gi += kL3RThreads) {
        uint32_t pp[3];
        mfma::split_pair(d3g[gi], d3g[gi + 1], pp);
#pragma unroll
        for (int q = 0; q < 3; q++) d3p[q * L.nd3 + gi + 4] = pp[q];
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
    }

    // ---- per 16-pixel unit: delta2 and gW3 MFMAs ----
    //   delta2[q][n] = [A2 > 0] * sum_tap delta3(q - off(tap)) W3[tap][n]
    //   gW3[tap][n] += sum_p delta3(p - off(tap)) A2[p][n]
    // delta2 runs transposed (M = channels, N = pixels): C register i of lane
    // (lq, lg) in tile t is delta2[u0 + lq][16t + 4lg + i], whose relu' mask
    // is a2r[j][t][i].  Then this unit's registers take the next sample's A2.
    float* d2s = D2 + (kD3Out ? 0 : ((size_t)smp * npx2 + 16 * wave) * N2);
#pragma unroll
    for (int j = 0; j < kL3RUnits; j++) {
      __builtin_amdgcn_sched_barrier(0);  // no operand motion across units (registers)
      const int u = wave + nwaves * j;
      {  // every slot, also past the sample's units (zero A2, stores masked)
        const int u0 = 16 * u;
        // delta2, its masked stores, then gW3, fenced apart so that the
        // groups' operands are never live at once (a 128-VGPR budget: 40 hold
        // the A2 of this wave's units, 16 the gW3 accumulators)
        if constexpr (!kD3Out) {
        float ad[KT];
#pragma unroll
        for (int s = 0; s < KT; s++)
          ad[s] = s < F3 ? d3g[adb0 + 128 * j + (F3 - 1 - s)] : d3g[adb1 + 128 * j + 4 * (6 - s)];
        f32x4 wv[NT][2];
#pragma unroll
        for (int t = 0; t < NT; t++)
#pragma unroll
          for (int h = 0; h < 2; h++)
            wv[t][h] = *reinterpret_cast<const f32x4*>(wds + wqo + 16 * t * kL3RWdS + 16 * h);
        f32x4 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; t++) acc[t] = mfma::zero4();
#pragma unroll
        for (int s = 0; s < KT; s++)
#pragma unroll
          for (int t = 0; t < NT; t++)
            acc[t] = mfma::mma16(wv[t][s >> 2][s & 3], ad[s], acc[t]);
        __builtin_amdgcn_sched_barrier(0);
        // masked delta2; lane (lq, lg) holds quads lg (t = 0) and 4 + lg (t = 1)
        // of pixel u0 + lq.  Two stores of WHOLE 128-B pixel rows: store A
        // writes pixels u0 .. u0+7 and store B pixels u0+8 .. u0+15, 1 KB
        // contiguous each (as held, each store covered half of 16 rows: the
        // stores cost 43% of the kernel, round-4 timing build without them)
#pragma unroll
        for (int t = 0; t < NT; t++)
#pragma unroll
          for (int i = 0; i < 4; i++) acc[t][i] = a2r[j][t][i] > 0.0f ? acc[t][i] : 0.0f;
        {
          // through the scratch as [pixel][kL3RScS] rows: written as this
          // lane's two quads, read back as whole rows
#pragma unroll
          for (int t = 0; t < NT; t++) *reinterpret_cast<f32x4*>(scw + srw + 16 * t) = acc[t];
          __builtin_amdgcn_wave_barrier();  // (cross-lane read-back: no compiler motion across)
          const f32x4 sa = *reinterpret_cast<const f32x4*>(scw + srr);
          const f32x4 sb = *reinterpret_cast<const f32x4*>(scw + srr + 8 * kL3RScS);
          int l_ = lane;
          asm volatile("" : "+v"(l_));  // (formed at the store, not held across the loop)
          const unsigned o_ = (l_ & 7) * N2 + 4 * ((l_ >> 4) + 4 * ((l_ >> 3) & 1)) + 16 * nwaves * N2 * j;
          if (u0 + (lq & 7) < npx2) st_d2(d2s + o_, sa);
          if (u0 + 8 + (lq & 7) < npx2) st_d2(d2s + o_ + 8 * N2, sb);
        }
        }
        __builtin_amdgcn_sched_barrier(0);
        // gW3's B operand A2[u0 + 4lg + s][16t + lq] through the scratch
#pragma unroll
        for (int h = 0; h < 2; h++)
#pragma unroll
          for (int i = 0; i < 4; i++)
            scw[sco_w + (16 * h + i) * kL3RScS] = a2r[j][h][i];
        __builtin_amdgcn_wave_barrier();  // (cross-lane read-back below)
        if constexpr (kD3Out) {
          // gW3 in split-bf16 products on v_mfma_f32_32x32x16_bf16: M = 32
          // tap rows, N = the 32 channels, K = the unit's 16 pixels; A = the
          // delta3 windows of tap (li) at pixels 8h .. 8h+7 of the unit, B =
          // A2[pixel][channel li] from the scratch rows
          float vb[8];
#pragma unroll
          for (int q = 0; q < 2; q++) {
            const f32x4 b_ = *reinterpret_cast<const f32x4*>(scw + g3s + 4 * q);
#pragma unroll
            for (int i = 0; i < 4; i++) vb[4 * q + i] = b_[i];
          }
          // layer 2's relu' mask for d1x6 (M2: one dword per A2 pixel, bit n
          // = A2[pixel][n] > 0): vb[q] is channel li32 of pixel u0 + 8 h32 + q,
          // so the wave mask of vb[q] > 0 IS the dwords of pixels u0 + q (low
          // half) and u0 + 8 + q (high half); lane l < 16 takes pixel u0 + l's
          // and the unit leaves as one 64-B row (substitute pixels, past the
          // sample, are not written)
          {
            uint32_t m_ = 0;
            // (the wave masks are uniform, SGPR pairs: of mask q one half goes
            // into lane q, one into lane 8 + q.  All eight are inputs of ONE
            // statement that opens with the wait states: the compiler adds
            // none for inline assembly, and a v_writelane straight after the
            // v_cmp that wrote its source read the PREVIOUS mask -- every low
            // half came out one pixel late.  One statement per mask, each with
            // its own wait, cost l3r 6%: 0.0947 -> 0.1006 ms)
            uint64_t w_[8];
#pragma unroll
            for (int q = 0; q < 8; q++) w_[q] = __builtin_amdgcn_ballot_w64(vb[q] > 0.0f);
#define SRCNN_L3R_LO(Q) "s"((uint32_t)w_[Q])
#define SRCNN_L3R_HI(Q) "s"((uint32_t)(w_[Q] >> 32))
            asm volatile(
                "s_nop 3\n\t"
                "v_writelane_b32 %0, %1, 0\n\tv_writelane_b32 %0, %2, 1\n\t"
                "v_writelane_b32 %0, %3, 2\n\tv_writelane_b32 %0, %4, 3\n\t"
                "v_writelane_b32 %0, %5, 4\n\tv_writelane_b32 %0, %6, 5\n\t"
                "v_writelane_b32 %0, %7, 6\n\tv_writelane_b32 %0, %8, 7\n\t"
                "v_writelane_b32 %0, %9, 8\n\tv_writelane_b32 %0, %10, 9\n\t"
                "v_writelane_b32 %0, %11, 10\n\tv_writelane_b32 %0, %12, 11\n\t"
                "v_writelane_b32 %0, %13, 12\n\tv_writelane_b32 %0, %14, 13\n\t"
                "v_writelane_b32 %0, %15, 14\n\tv_writelane_b32 %0, %16, 15"
                : "+v"(m_)
                : SRCNN_L3R_LO(0), SRCNN_L3R_LO(1), SRCNN_L3R_LO(2), SRCNN_L3R_LO(3), SRCNN_L3R_LO(4),
                  SRCNN_L3R_LO(5), SRCNN_L3R_LO(6), SRCNN_L3R_LO(7), SRCNN_L3R_HI(0), SRCNN_L3R_HI(1),
                  SRCNN_L3R_HI(2), SRCNN_L3R_HI(3), SRCNN_L3R_HI(4), SRCNN_L3R_HI(5), SRCNN_L3R_HI(6),
                  SRCNN_L3R_HI(7));
#undef SRCNN_L3R_LO
#undef SRCNN_L3R_HI
            if (lane < 16 && u0 + lane < npx2) M2[(size_t)smp * npx2 + u0 + lane] = m_;
          }
          mfma::bf16x8 pa[3], pb[3];
#pragma unroll
          for (int q = 0; q < 3; q++) {
            const uint32_t* r_ = d3p + q * L.nd3 + 4 + g3b + 128 * j;
            mfma::u32x4 d_;
            d_[0] = r_[0];
            d_[1] = r_[2];
            d_[2] = r_[4];
            d_[3] = r_[6];
            pa[q] = __builtin_bit_cast(mfma::bf16x8, d_);
          }
          mfma::split8(vb, pb);
          g3x = mfma::mma_x6(pa, pb, g3x);
        } else {
        float ag[4][TT];
#pragma unroll
        for (int s = 0; s < 4; s++)
#pragma unroll
          for (int t3 = 0; t3 < TT; t3++) ag[s][t3] = d3g[agb[t3] + 128 * j + s];
        f32x4 bg[NT];
#pragma unroll
        for (int t = 0; t < NT; t++) bg[t] = *reinterpret_cast<const f32x4*>(scw + wqo + 16 * t * kL3RScS);
#pragma unroll
        for (int s = 0; s < 4; s++)
#pragma unroll
          for (int t3 = 0; t3 < TT; t3++)
#pragma unroll
            for (int t = 0; t < NT; t++)
              gacc[t3][t] = mfma::mma16(ag[s][t3], bg[t][s], gacc[t3][t]);
        }
        // the next sample's A2 into the registers this unit no longer needs
        // (issued here rather than at the sample top: 0.158 vs 0.174 ms)
        SRCNN_L3R_LOAD(j, nsmp);
      }
    }
  }
#undef SRCNN_L3R_LOAD
#undef SRCNN_L3R_SWAP
#undef SRCNN_L3R_T_PREFETCH
  SRCNN_CLOCK_END(g_clk, 1);

  // ---- block reduction of the partial gradients: every wave parks its 16
  // registers in LDS, then each thread adds its elements over the waves in
  // wave order (the sums of the former wave-by-wave accumulation, with one
  // barrier instead of eight) ----
  constexpr int kRed = TT * NT * 4 * 64;  // elements per wave
  __syncthreads();
#pragma unroll
  for (int t3 = 0; t3 < TT; t3++)
#pragma unroll
    for (int t = 0; t < NT; t++)
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int idx = (t3 * NT + t) * 4 + i;
        red[wave * kRed + idx * 64 + lane] = kD3Out ? g3x[idx] : gacc[t3][t][i];
      }
  __syncthreads();
  float* out = slab3 + (size_t)blockIdx.x * (NW3 + 1);
  for (int i = tid; i < kRed; i += kL3RThreads) {
    float v = red[i];
    for (int w = 1; w < nwaves; w++) v += red[w * kRed + i];
    const int k = i >> 8, r = (i >> 6) & 3, l = i & 63;
    const int t3 = k / NT, t = k - t3 * NT;
    const int tap = kD3Out ? crow(i >> 6, l >> 5) : 16 * t3 + 4 * (l >> 4) + r;
    const int n = kD3Out ? (l & 31) : 16 * t + (l & 15);
    if (tap < K3) out[tap * N2 + n] = v;
  }
  // gB3 and squared error: per-wave shuffle trees, then waves in order
  for (int off = 32; off > 0; off >>= 1) {
    gb3 += __shfl_down(gb3, off, 64);
    sq += __shfl_down(sq, off, 64);
    if constexpr (kD3Out) dmx = fmaxf(dmx, __shfl_down(dmx, off, 64));
  }
  __syncthreads();
  if (lane == 0) {
    red[2 * wave] = gb3;
    red[2 * wave + 1] = sq;
    if constexpr (kD3Out) red[2 * nwaves + wave] = dmx;
  }
  __syncthreads();
  if (tid == 0) {
    float tb = 0.f, ts = 0.f;
    for (int w = 0; w < nwaves; w++) {
      tb += red[2 * w];
      ts += red[2 * w + 1];
    }
    out[NW3] = tb;
    sq_slab[blockIdx.x] = ts;
    // (a block without a sample writes nothing: d1x6 reads the first min(grid, batch) slots)
    if constexpr (kD3Out) {
      float tm = 0.f;
      for (int w = 0; w < nwaves; w++) tm = fmaxf(tm, red[2 * nwaves + w]);
      if ((int)blockIdx.x < g.batch) d3max[blockIdx.x] = tm;
    }
  }
}
