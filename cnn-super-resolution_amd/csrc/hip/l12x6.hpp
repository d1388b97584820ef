// l12x6.hpp -- kernel 1 of the fused step (L1 + L2 forward) for the reference
// default net (n1 = 64, n2 = 32, f1 = 9) with its products on the matrix cores
// in exact-split form.  Included by train_fused.hip inside namespace
// srcnn::fused, after fused_layout.hpp (its LDS layout H6Lds, the rule X6Lds
// by which a tile takes it, Geom, RunGeom, kL12Regs); uses train_fused.hip's
// g_clk and ops.hpp's LazyUpdate.  Same outputs (blocked A1, A2 rows) and the same mathematics as
// l12_fwd_kernel (layer_uber_kernel.cl:36-96 for layers 1 and 2).
//
// Split products (split.hpp).  Layer 2 is in the bf16 form ("x6"): every fp32
// operand is the sum of three bf16 parts (round-to-nearest residuals, exact to
// 2^-27 relative), and a product a . b is formed from the six part products
// whose order is at most 2^-16; the dropped ones are below 2^-26 relative,
// under the 2^-24 rounding of an fp32 product.  v_mfma_f32_32x32x16_bf16 forms
// exact part products and sums them in fp32, so a 32x32x16 block costs 6 x 32
// cycles against 8 x 64 for v_mfma_f32_32x32x2_f32, at fp32 accuracy
// (profiles/r05_x6: normwise error against an fp64 product 1.45e-7 vs 1.79e-7
// for the fp32 MFMA chain at K = 96).
// Layer 1 is in the two-part fp16 form: W1 2^ew and x 2^ex (powers of two
// that put the largest |W1| of the launch, after the lazy update, and the
// largest |x| of the sample into [2^14, 2^15); scale_exp_h) are each the sum
// of two fp16 parts, and a product keeps a1 b0, a0 b1 and a0 b0 -- three
// v_mfma_f32_32x32x16_f16 per k-step, 1.35e-7 at K = 96
// (profiles/r10_f16/accuracy.md, profiles/r12_l12_f16/accuracy.md).  The
// accumulator carries 2^(ew + ex): the fp32 MFMA that starts it has 2^ew on
// its A side (W1's tap 80 and B1) and 2^ex on its B side (x88 from the scaled
// fp32 tile, 2^ex where the bias column had 1.0), and after the ten groups
// every register is multiplied by 2^-(ew + ex), exactly, ahead of the ReLU.
// Nothing of a sample's scale outlives the sample: a non-finite or absurd
// sample (scale_exp_h returns a usable exponent for any bit pattern) stays
// its own.
//
// Layer 1, transposed as in l12_fwd (rows = channels, cols = the chunk's 32
// pixels), K = taps: 80 taps in 5 k-steps of 16 slots, tap (8, 8) and the
// bias in one fp32 32x32x2 MFMA that starts the accumulator.  Slot
// 8h + j of k-step s (lane half h, element j) is
//   group g = 2s + h <= 8: tap (dy = g, dx = j)       (a row run of X)
//   group g = 9:           tap (dy = j, dx = 8)       (column 8)
// so a lane's 8 B-operand values are 8 consecutive X pixels of one row for
// k-steps 0-3: four dwords of the PAIR image R (dword i = parts of x_i and
// x_{i+1}), i.e. two ds_read2_b32 per part.  K-step 4 (row 8 / column 8)
// reads the scaled fp32 tile and splits in registers.
// Layer 2: the L1 accumulator after ReLU is split in registers (k-step m:
// registers 8(m&1) .. +7 of tile m>>1, the channel order of mfma.hpp's crow)
// against W2 split images; the accumulator starts from zero and B2 is added
// to the finished sum (one rounding at the result's own magnitude).
// W1 and W2 live in LDS as split operand images (one ds_read_b128 per part
// and tile), formed once per block, with the lazy update folded in.
using mfma::bf16x8;
using mfma::f16x8;
using mfma::mma_x3_h;
using mfma::mma_x6;
using mfma::relu1;
using mfma::split3;
using mfma::split8;
using mfma::split8_h;
using mfma::split8_pk;
using mfma::u32x4;

template <bool kLazy>
__global__ __launch_bounds__(256, 2) void l12x6_fwd_kernel(const float* __restrict__ X,
                                                            const float* __restrict__ W1,
                                                            const float* __restrict__ B1,
                                                            const float* __restrict__ W2,
                                                            const float* __restrict__ B2,
                                                            float* __restrict__ A1,
                                                            float* __restrict__ A2, Geom g, RunGeom rg,
                                                            LazyUpdate lz, float* __restrict__ xmax) {
  constexpr int N1 = 64, N2 = 32, F1 = 9, NT1 = 2;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const H6Lds L(g.W, g.H);
  _Float16* const w1i = reinterpret_cast<_Float16*>(smem);
  _Float16* const w2i = w1i + kH6W1;
  float* const a88s = reinterpret_cast<float*>(w2i + kH6W2);  // 2^ew [W1 tap 80 | B1]
  float* const b2i = a88s + 128;                              // [2][16]: 2^ew2 B2
  float* const b2s = b2i + 32;                                // [2][16]: 2^(ea + ew2) B2 of the sample
  float* const wmx = b2s + 32;                                // [4]: the waves' max |W1|
  float* const w2mx = wmx + 4;                                // [4]: the waves' max |W2|
  float* const xmx = w2mx + 4;                                // [4]: the waves' max |X| of the sample
  uint32_t* const rimg = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(smem) + L.r);
  float* const xs = reinterpret_cast<float*>(reinterpret_cast<char*>(smem) + L.xs);
  const int rs = L.rs;
  float* const a2sc = reinterpret_cast<float*>(reinterpret_cast<char*>(smem) + L.a2sc);

  SRCNN_CLOCK_BEGIN();
  const int lane = mfma::lane_id(), wave = mfma::wave_id();
  const int h = lane >> 5, li = lane & 31;
  const int W = g.W, xn = g.W * g.H;
  const int npx = g.ow * g.oh, nch = rg.nch;

  float xr[kL12Regs];
  auto xload = [&](int smp) {
    const float* src = X + (size_t)smp * xn;
#pragma unroll
    for (int k = 0; k < kL12Regs; k++) {
      const int i = threadIdx.x + 256 * k;
      xr[k] = i < xn ? src[i] : 0.0f;
    }
  };
  if ((int)blockIdx.x < g.batch) xload(blockIdx.x);
  auto wave_max = [&](float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
  };
  auto max4 = [&](const float* slot) {
    const f32x4 m = *reinterpret_cast<const f32x4*>(slot);
    return fmaxf(fmaxf(m[0], m[1]), fmaxf(m[2], m[3]));
  };

  // ---- split operand images of W1 / W2 (with the pending update folded in) ----
  // Each thread takes 4 consecutive parameters per 16-B load (W1 taps 0-79:
  // 5 loads, W2: 2 loads; with the lazy update the same from P, M and G, all
  // in flight at once) and scatters their parts into the images.
  if constexpr (kLazy) lazy_write_slice(lz);
  auto prm = [&](int seg, int i) -> float {
    if constexpr (kLazy) return lazy_param(lz, seg, i);
    return (seg == 0 ? W1 : seg == 1 ? B1 : seg == 2 ? W2 : B2)[i];
  };
  // 4 consecutive parameters of segment seg from index i (16-B aligned)
  auto prm4 = [&](int seg, int i, f32x4& v, f32x4& m, f32x4& gr) {
    if constexpr (kLazy) {
      const uint32_t gi = lz.off[seg] + i;
      v = *reinterpret_cast<const f32x4*>(lz.P + gi);
      m = *reinterpret_cast<const f32x4*>(lz.M + gi);
      gr = *reinterpret_cast<const f32x4*>(lz.G + gi);
    } else {
      v = *reinterpret_cast<const f32x4*>((seg == 0 ? W1 : W2) + i);
    }
  };
  auto upd4 = [&](int seg, f32x4& v, f32x4& m, const f32x4& gr) {
    if constexpr (kLazy) {
#pragma unroll
      for (int e = 0; e < 4; e++) {
        float w_ = v[e], m_ = m[e];
        sgd_step(w_, m_, seg, gr[e], lz.lr[seg >> 1], lz.mu, lz.wd, lz.batch);
        v[e] = w_;
      }
    }
  };
  // The scales come first: ew = scale_exp_h(max |W1|) over its 5,184 weights
  // and ew2 = scale_exp_h(max |W2|), as they stand after the update (a wave
  // reduction and four slots each), so the images are split behind a barrier
  // of their own.  The same barrier serves layer 2's bound on |A1|: wnorm =
  // max over channels of sum over taps of |W1|, the waves' partial sums over
  // their taps in the A2 scratch (unused until the first chunk); every wave
  // then forms wnorm and max |B1| for itself.
  constexpr int kQ1 = 5120 / 4 / 256, kQ2 = 2048 / 4 / 256;
  f32x4 v1[kQ1], v2[kQ2];
  float a88v = 0.0f, b2v = 0.0f, wm = 0.0f, w2m = 0.0f;
  {
    // W1 taps 0-79 (5120 parameters, 5 quads per thread): every quad of a
    // thread holds the channels 4 (lane & 15) .. + 3 of another tap
    f32x4 m[kQ1], gr[kQ1];
#pragma unroll
    for (int k = 0; k < kQ1; k++) prm4(0, 4 * (threadIdx.x + 256 * k), v1[k], m[k], gr[k]);
    if (threadIdx.x < 128) a88v = threadIdx.x < 64 ? prm(0, 80 * N1 + threadIdx.x) : prm(1, threadIdx.x - 64);
    if (threadIdx.x < 64) wm = fabsf(a88v);
    f32x4 ns = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < kQ1; k++) {
      upd4(0, v1[k], m[k], gr[k]);
#pragma unroll
      for (int e = 0; e < 4; e++) {
        wm = fmaxf(wm, fabsf(v1[k][e]));
        ns[e] += fabsf(v1[k][e]);
      }
    }
#pragma unroll
    for (int e = 0; e < 4; e++) {
      ns[e] += __shfl_xor(ns[e], 16, 64);
      ns[e] += __shfl_xor(ns[e], 32, 64);
    }
    if (lane < 16) *reinterpret_cast<f32x4*>(a2sc + wave * kX6Sc + 4 * lane) = ns;
  }
  {
    f32x4 m[kQ2], gr[kQ2];
#pragma unroll
    for (int k = 0; k < kQ2; k++) prm4(2, 4 * (threadIdx.x + 256 * k), v2[k], m[k], gr[k]);
#pragma unroll
    for (int k = 0; k < kQ2; k++) {
      upd4(2, v2[k], m[k], gr[k]);
#pragma unroll
      for (int e = 0; e < 4; e++) w2m = fmaxf(w2m, fabsf(v2[k][e]));
    }
  }
  wm = wave_max(wm);
  w2m = wave_max(w2m);
  if (lane == 0) {
    wmx[wave] = wm;
    w2mx[wave] = w2m;
  }
  if (threadIdx.x >= 128 && threadIdx.x < 160) {
    const int i = threadIdx.x - 128;
    b2v = prm(3, crow(i & 15, i >> 4));
  }
  const float a80 = fabsf(prm(0, 80 * N1 + lane)), b1a = fabsf(prm(1, lane));
  __syncthreads();
  const int ew = mfma::scale_exp_h(max4(wmx)), ew2 = mfma::scale_exp_h(max4(w2mx));
  const float wnorm = wave_max(a80 + ((a2sc[lane] + a2sc[kX6Sc + lane]) + (a2sc[2 * kX6Sc + lane] + a2sc[3 * kX6Sc + lane])));
  const float b1max = wave_max(b1a);
  {
    // parameter tap * 64 + ch sits at k-step s, tile ch / 32, lane (ch % 32)
    // + 32 h, element j with (g = 2s + h, j) = (dy, dx) for dx < 8, (9, dy)
    // for dx = 8
    const float sw = mfma::pow2_h(ew);
#pragma unroll
    for (int k = 0; k < kQ1; k++) {
      const int p0 = 4 * (threadIdx.x + 256 * k), tap = p0 >> 6, dy = tap / F1, dx = tap - dy * F1;
      const int gg = dx < 8 ? dy : 9, j = dx < 8 ? dx : dy, s_ = gg >> 1, hh = gg & 1;
#pragma unroll
      for (int e = 0; e < 4; e++) {
        const int ch = (p0 & 63) + e, t = ch >> 5, L_ = (ch & 31) + 32 * hh;
        const float ws_ = v1[k][e] * sw;
        const _Float16 q0 = (_Float16)ws_, q1 = (_Float16)(ws_ - (float)q0);
        w1i[((s_ * 2 + t) * 2 + 0) * 512 + L_ * 8 + j] = q0;
        w1i[((s_ * 2 + t) * 2 + 1) * 512 + L_ * 8 + j] = q1;
      }
    }
    // the fp32 MFMA's A side carries 2^ew, its B side 2^ex
    if (threadIdx.x < 128) a88s[threadIdx.x] = a88v * sw;
  }
  {
    // W2 (2048 parameters, 2 quads per thread): parameter c * 32 + n sits at
    // k-step m, lane n + 32 h, element j with c = 32 (m >> 1) + crow(8 (m & 1) + j, h)
    const float sw2 = mfma::pow2_h(ew2);
#pragma unroll
    for (int k = 0; k < kQ2; k++) {
      const int p0 = 4 * (threadIdx.x + 256 * k), c = p0 >> 5, r = c & 31;
      const int hh = (r >> 2) & 1, rr = (r & 3) + 4 * (r >> 3), mm = 2 * (c >> 5) + (rr >> 3), j = rr & 7;
#pragma unroll
      for (int e = 0; e < 4; e++) {
        const int L_ = (p0 & 31) + e + 32 * hh;
        const float ws_ = v2[k][e] * sw2;
        const _Float16 q0 = (_Float16)ws_, q1 = (_Float16)(ws_ - (float)q0);
        w2i[(mm * 2 + 0) * 512 + L_ * 8 + j] = q0;
        w2i[(mm * 2 + 1) * 512 + L_ * 8 + j] = q1;
      }
    }
    if (threadIdx.x >= 128 && threadIdx.x < 160) b2i[threadIdx.x - 128] = b2v * sw2;
  }
  __syncthreads();
  // fp32 MFMA operand of tap (8, 8) (half 0) and the bias (half 1)
  float a88r[NT1];
#pragma unroll
  for (int t = 0; t < NT1; t++) a88r[t] = a88s[64 * h + 32 * t + li];

  // ---- software-pipelined stores of the previous chunk (as in l12_fwd) ----
  // A1 leaves TRANSPOSED per chunk, [chunk][64 channels][32 slots] (d1x6
  // reads a channel's slots as 16-B runs): store k < 32 is register k & 15
  // of tile k >> 4, every half-wave writing one channel's 128 B.  A2 leaves
  // as whole 128-B pixel rows at the slots' pixels (runs.hpp order).
  constexpr int NST = 32 * NT1 / 2 + N2 / 8;
  f32x16 pa1[NT1], pa2 = zero16();
#pragma unroll
  for (int t = 0; t < NT1; t++) pa1[t] = zero16();
  bool pok = false;
  float* pa1p = A1;
  float* pa2p = A2;
  int ppx[4] = {-1, -1, -1, -1};  // pixels of the A2 row stores (-1: dummy slot)
  auto store_prev = [&](int k) {
    if (pok) {
      if (k < 16 * NT1) {
        const int t = k >> 4, r = k & 15;
        __builtin_nontemporal_store(pa1[t][r], pa1p + (32 * t + crow(r, h)) * 32);
      } else {
        const int q = k - 16 * NT1;
        if (ppx[q] >= 0) {
          f32x4 v_;
#pragma unroll
          for (int e = 0; e < 4; e++) v_[e] = pa2[4 * q + e];
          *reinterpret_cast<f32x4*>(pa2p + (size_t)ppx[q] * N2 + 4 * (lane & 7)) = v_;
        }
      }
    }
  };

  const uint16_t* const wl1 = reinterpret_cast<const uint16_t*>(w1i) + lane * 8;
  const uint16_t* const wl2 = reinterpret_cast<const uint16_t*>(w2i) + lane * 8;
  auto w1op = [&](int s, int t, f16x8 (&a)[2]) {
#pragma unroll
    for (int q = 0; q < 2; q++) a[q] = *reinterpret_cast<const f16x8*>(wl1 + ((s * 2 + t) * 2 + q) * 512);
  };

  // the largest max |X| over this block's samples, for d1x6's launch scale
  // (xmax: one slot per block, or null)
  float xrun = 0.0f;
  for (int sample = blockIdx.x; sample < g.batch; sample += gridDim.x) {
    // The sample's scale: ex = scale_exp_h(max |X|) from the registers that
    // hold it, a wave reduction and one slot per wave.  The slots are
    // written ahead of the barrier the images need anyway and read behind
    // it; a wave writes the next sample's only past this sample's second
    // barrier, which every reader reaches with the slots read.
    {
      float xm = 0.0f;
#pragma unroll
      for (int k = 0; k < kL12Regs; k++) xm = fmaxf(xm, fabsf(xr[k]));
      xm = wave_max(xm);
      if (lane == 0) xmx[wave] = xm;
    }
    __syncthreads();  // previous sample's readers are done with the images
    const int ex = mfma::scale_exp_h(max4(xmx));
    xrun = fmaxf(xrun, max4(xmx));
    const float sx = mfma::pow2_h(ex);
    // the accumulators carry 2^(ew + ex); -(ew + ex) lies in [-120, 228], so
    // the factor is taken out in one exact step, or two where it passes 2^127
    const int eu = -(ew + ex), eu1 = eu > 127 ? 127 : eu;
    const float un1 = mfma::pow2_h(eu1), un2 = mfma::pow2_h(eu - eu1);
    // Layer 2's operand scale from a bound instead of a pass over A1:
    // |A1| <= max |X| wnorm + max |B1|, ea = scale_exp_h of it; W2 carries
    // 2^ew2, so B2 enters times 2^(ea + ew2) (the sample's copy, written
    // here): it is added to the finished sum of products, not put in front
    // of it, and the result is unscaled like layer 1's.
    const int ea = mfma::scale_exp_h(max4(xmx) * wnorm + b1max);
    const float sa = mfma::pow2_h(ea);
    const int ev = -(ea + ew2), ev1 = ev > 127 ? 127 : ev;
    const float vn1 = mfma::pow2_h(ev1), vn2 = mfma::pow2_h(ev - ev1);
    if (threadIdx.x < 32) b2s[threadIdx.x] = b2i[threadIdx.x] * sa;
    {
      uint16_t* const r16 = reinterpret_cast<uint16_t*>(rimg);
#pragma unroll
      for (int k = 0; k < kL12Regs; k++) {
        const int i = threadIdx.x + 256 * k;
        if (i < xn) {
          const float xv = xr[k] * sx;
          xs[i] = xv;
          const int y = i / W, x = i - y * W, d = y * rs + x;
          const _Float16 q0 = (_Float16)xv, q1 = (_Float16)(xv - (float)q0);
          const uint16_t b0 = __builtin_bit_cast(uint16_t, q0), b1 = __builtin_bit_cast(uint16_t, q1);
          r16[2 * d] = b0;  // low half of pair x
          r16[2 * (d + W)] = b1;
          if (x > 0) {      // high half of pair x - 1
            r16[2 * d - 1] = b0;
            r16[2 * (d + W) - 1] = b1;
          }
        }
      }
    }
    __syncthreads();
    if (sample + (int)gridDim.x < g.batch) xload(sample + gridDim.x);

    for (int c = wave; c < nch; c += 4) {
      int iy, ix;
      const bool pv = slot_coord(rg, c, li, iy, ix);
      const int rb = (iy + h) * rs + ix;  // row 2s + h of k-steps 0-3
      // k-step 4: half 0 row 8 (dx 0..7), half 1 column 8 (dy 0..7)
      const int b4 = h ? iy * W + ix + 8 : (iy + 8) * W + ix, st4 = h ? W : 1;

      f32x16 acc1[NT1];
      {
        const float bx = h ? sx : xs[(iy + 8) * W + ix + 8];
#pragma unroll
        for (int t = 0; t < NT1; t++) acc1[t] = mma(a88r[t], bx, zero16());
      }
      // B operand of k-steps 0-3: rows 2s + h of the pair image
      auto xop = [&](int s, f16x8 (&b)[2]) {
#pragma unroll
        for (int q = 0; q < 2; q++) {
          const uint32_t* r = rimg + W * q + rb + 2 * s * rs;
          u32x4 d;
          d[0] = r[0];
          d[1] = r[2];
          d[2] = r[4];
          d[3] = r[6];
          b[q] = __builtin_bit_cast(f16x8, d);
        }
      };
      // Operand pipeline over the 10 (k-step, tile) groups of 6 MFMAs: the
      // next group's W1 parts (and at t = 0 the next k-step's X parts) are
      // read before this group's MFMAs, pinned by sched barriers (left
      // alone, the scheduler reads each operand just before its MFMA and the
      // wave waits out the LDS latency every group).  K-step 4's fp32 X
      // values are read at group 4 and split at group 6.
      f16x8 wa[2][2], xb[2][2];
      float x4[8];
      xop(0, xb[0]);
      w1op(0, 0, wa[0]);
#pragma unroll
      for (int gi = 0; gi < 2 * kX6KS; gi++) {
        const int s = gi >> 1, t = gi & 1;
        if (gi + 1 < 2 * kX6KS) w1op((gi + 1) >> 1, (gi + 1) & 1, wa[(gi + 1) & 1]);
        if (t == 0 && s + 1 < 4) xop(s + 1, xb[(s + 1) & 1]);
        if (gi == 4) {
#pragma unroll
          for (int j = 0; j < 8; j++) x4[j] = xs[b4 + j * st4];
        }
        if (gi == 6) split8_h(x4, xb[0]);
        __builtin_amdgcn_sched_barrier(0);
        acc1[t] = mma_x3_h(wa[gi & 1], xb[s & 1], acc1[t]);
#pragma unroll
        for (int k = 3 * gi; k < 3 * gi + 3; k++) store_prev(k);
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int t = 0; t < NT1; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc1[t][r] *= un1;
      if (eu != eu1) {
#pragma unroll
        for (int t = 0; t < NT1; t++)
#pragma unroll
          for (int r = 0; r < 16; r++) acc1[t][r] *= un2;
      }
#pragma unroll
      for (int t = 0; t < NT1; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc1[t][r] = relu1(acc1[t][r]);
      f32x16 acc2 = zero16();  // (B2 is added to the finished sum, below)
      // L2: k-step m's A1 parts are split while k-step m - 1's MFMAs run
      f16x8 wb[2][2], bb[2][2];
      auto a1split = [&](int m, f16x8 (&b)[2]) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; j++) v[j] = acc1[m >> 1][8 * (m & 1) + j] * sa;
        split8_h(v, b);
      };
      auto w2op = [&](int m, f16x8 (&a)[2]) {
#pragma unroll
        for (int q = 0; q < 2; q++) a[q] = *reinterpret_cast<const f16x8*>(wl2 + (m * 2 + q) * 512);
      };
      w2op(0, wb[0]);
      a1split(0, bb[0]);
#pragma unroll
      for (int m = 0; m < 4; m++) {
        if (m + 1 < 4) w2op(m + 1, wb[(m + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);
        acc2 = mma_x3_h(wb[m & 1], bb[m & 1], acc2);
        if (m + 1 < 4) a1split(m + 1, bb[(m + 1) & 1]);
        if (m < 3) {
          store_prev(30 + 2 * m);
          store_prev(31 + 2 * m);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int r = 0; r < 16; r++) acc2[r] = (acc2[r] + b2s[16 * h + r]) * vn1;
      if (ev != ev1) {
#pragma unroll
        for (int r = 0; r < 16; r++) acc2[r] *= vn2;
      }
#pragma unroll
      for (int t = 0; t < NT1; t++) pa1[t] = acc1[t];
      {
        float* sc = a2sc + wave * kX6Sc;
        int* scp = reinterpret_cast<int*>(sc + 32 * 32);
#pragma unroll
        for (int m = 0; m < 4; m++) {
          f32x4 v_;
#pragma unroll
          for (int e = 0; e < 4; e++) v_[e] = relu1(acc2[4 * m + e]);
          *reinterpret_cast<f32x4*>(sc + li * 32 + 4 * ((2 * m + h) ^ (li & 7))) = v_;
        }
        if (h == 0) scp[li] = pv ? iy * g.ow + ix : -1;
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const int p_ = 8 * q + (lane >> 3);
          const f32x4 v_ = *reinterpret_cast<const f32x4*>(sc + p_ * 32 + 4 * ((lane & 7) ^ (p_ & 7)));
#pragma unroll
          for (int e = 0; e < 4; e++) pa2[4 * q + e] = v_[e];
          ppx[q] = scp[8 * q + (lane >> 3)];
        }
      }
      pok = true;
      pa1p = A1 + ((size_t)sample * nch + c) * (32 * N1) + li;
      pa2p = A2 + (size_t)sample * npx * N2;
    }
  }
  // (a sample's last chunk is stored under the next sample's first one)
#pragma unroll
  for (int k = 0; k < NST; k++) store_prev(k);
  // (a block without a sample writes nothing: d1x6 reads the first min(grid, batch) slots)
  if (xmax != nullptr && threadIdx.x == 0 && (int)blockIdx.x < g.batch) xmax[blockIdx.x] = xrun;
  SRCNN_CLOCK_END(g_clk, 0);
}
