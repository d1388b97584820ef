// wconv_mfma.hpp -- the fp32 MFMA convolution of the wide middle layer over an
// LDS-DMA'd chunk image (layout: DmaImgLds, wide_layout.hpp): prepack_w2 (the
// W2 operand images) and conv_mfma (L2 forward; delta1 of the op-level call).
// Included by train_wide.hip inside namespace srcnn::wide.
//
// (conv_mfma / d1g16 stage their input images with the default cache policy:
// with the nontemporal hint the L2 forward's HBM bytes went 2.21 -> 3.09 GB
// per launch and delta1's 2.23 -> 2.78 GB, profiles/r04_ab_widedmant)

// ---------------------------------------------------------------------------
// W2 operand images.  conv_mfma's k-step ks = (chunk, tap, g) contracts input
// channels c = 16*chunk + 8*g + 4*half + jj (jj = MFMA slot 0..3, one
// ds_read_b128 per lane); the B operand of that k-step for output tile nt is
// one float4 per lane: Wimg[((nt * KS) + ks) * 64 + lane].
//   forward: B = W2[tap][c][n]                     (n = 32 nt + j, N2 outputs)
//   delta1:  B = W2[flip(tap)][n][c]               (n = 32 nt + j in n1, c in n2)
// (layer_deltas.cl:83-105: delta_curr[y,x,n] = sum delta_next[y-dy,x-dx,k] W[dy,dx,n,k];
//  as a correlation over delta_next padded by f-1 the tap is flipped.)
// ---------------------------------------------------------------------------
// D16: the delta1 image for d1g16_kernel instead: [n16][chunk][tap][lane][jj],
// lane (n = lane & 15, g = lane >> 4) holding W2[flip(tap)][16 n16 + n][16 chunk + 4 g + jj]
template <int CIN, int COUT, int F, bool D16 = false>
__global__ void prepack_w2_kernel(const float* __restrict__ W2, float* __restrict__ Wf,
                                  float* __restrict__ Wd) {
  constexpr int FF = F * F, TOT = FF * CIN * COUT;
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 2 * TOT) return;
  const bool delta = i >= TOT;
  if (delta) i -= TOT;
  const int jj = i & 3, lane = (i >> 2) & 63, j = lane & 31, hh = lane >> 5;
  const int rest = i >> 8;
  constexpr int KSC = FF * (kCC / 8);
  if (D16 && delta) {
    constexpr int NCH = COUT / kCC;  // delta2 channel chunks
    const int t = rest % FF, chunk = (rest / FF) % NCH, n16 = rest / (FF * NCH);
    const int dy = t / F, dx = t - (t / F) * F, tf = (F - 1 - dy) * F + (F - 1 - dx);
    const int c = chunk * kCC + 4 * (lane >> 4) + jj;  // delta2 channel (n2)
    const int n = 16 * n16 + (lane & 15);               // delta1 channel (n1)
    Wd[i] = W2[((size_t)tf * CIN + n) * COUT + c];
    return;
  }
  if (!delta) {
    constexpr int KS = (CIN / kCC) * KSC;
    const int ks = rest % KS, nt = rest / KS;
    const int chunk = ks / KSC, r2 = ks - chunk * KSC, t = r2 >> 1, gq = r2 & 1;
    const int c = chunk * kCC + 8 * gq + 4 * hh + jj, n = 32 * nt + j;
    Wf[i] = W2[((size_t)t * CIN + c) * COUT + n];
  } else {
    constexpr int KS = (COUT / kCC) * KSC;
    const int ks = rest % KS, nt = rest / KS;
    const int chunk = ks / KSC, r2 = ks - chunk * KSC, t = r2 >> 1, gq = r2 & 1;
    const int dy = t / F, dx = t - (t / F) * F, tf = (F - 1 - dy) * F + (F - 1 - dx);
    const int c = chunk * kCC + 8 * gq + 4 * hh + jj;  // delta2 channel (n2)
    const int n = 32 * nt + j;                          // delta1 channel (n1)
    Wd[i] = W2[((size_t)tf * CIN + n) * COUT + c];
  }
}

// ---------------------------------------------------------------------------
// conv_mfma: out[s][p][n] = epi( sum_{tap, c} img_s[p + off(tap)][c] * W(tap, c, n) )
//   forward (DELTA = false): img = A1, epi = relu(v + B2[n])   (layer_uber_kernel.cl)
//   delta1  (DELTA = true):  img = delta2 zero-padded by F-1, W flipped and
//                            transposed, epi = [A1 > 0] * v     (layer_deltas.cl)
// Work item = (sample, 64 output channels).  4 waves: wave = (N tile nt of 32
// channels, M group mg: the MT 32-pixel tiles 2m + mg, interleaved so both
// groups skip equally many border tap rows in delta1); the whole item's accumulators
// live in registers across the K loop (CIN/16 chunks x F*F taps x 2).
// Each chunk's image (img_w x img_h pixels x 16 channels, 80-B rows) is
// staged by LDS-DMA into the other buffer while the current one is consumed;
// the DMA instructions go out as one burst in the chunk's first tap, after
// that tap's B loads, so only the B waits of tap 4 cover them.
// ---------------------------------------------------------------------------
// Work item `it` = (image s, output window, 64-channel part).  The window's
// staged image is the padded input over [x0, x0 + iw) x [y0, y0 + ih) (padded
// coordinates; real = padded - pad, zero outside the input), iw x ih = the
// largest window's image.
struct CWin {
  int s, part, x0, y0, ow, oh, iw, ih;
};
template <int F, int NP>
__device__ __forceinline__ CWin conv_win(int it, const CGeom& g) {
  CWin w;
  const int rest = it / NP;
  w.part = it - rest * NP;
  if (g.wo == 0) {
    w.s = rest;
    w.x0 = w.y0 = 0;
    w.ow = g.out_w;
    w.oh = g.out_h;
  } else {
    const int nwx = (g.out_w + g.wo - 1) / g.wo, nwin = nwx * ((g.out_h + g.wo - 1) / g.wo);
    w.s = rest / nwin;
    const int wi = rest - w.s * nwin, wy = wi / nwx;
    w.x0 = (wi - wy * nwx) * g.wo;
    w.y0 = wy * g.wo;
    w.ow = min(g.wo, g.out_w - w.x0);
    w.oh = min(g.wo, g.out_h - w.y0);
  }
  // every window stages the full img_w x img_h image (the tap offsets are
  // formed with img_w); an edge window's columns / rows past the input read
  // the zero source
  w.iw = g.img_w;
  w.ih = g.img_h;
  return w;
}

template <int CIN, int COUT, int F, int MT, bool DELTA>
__global__ __launch_bounds__(256, 1) void conv_mfma_kernel(const float* __restrict__ in,
                                                          const float* __restrict__ Wimg,
                                                          const float* __restrict__ bias,
                                                          const float* __restrict__ ycur,
                                                          float* __restrict__ out, CGeom g) {
  constexpr int NCH = CIN / kCC, FF = F * F, KSC = FF * (kCC / 8), KS = NCH * KSC;
  constexpr int NP = COUT / 64;
  static_assert(CIN % kCC == 0 && COUT % 64 == 0 && kCC == 16, "shape");
  extern __shared__ float smem[];
  const int lane = lane_id(), wave = wave_id(), j = lane & 31, h = lane >> 5;
  const int nt = wave & 1, mg = wave >> 1;
  const int buf_floats = DmaImgLds(g).buf_floats;  // the largest window image
  const int nitems = g.batch * NP * conv_windows(g);
  int abase[MT];
  // delta1: a tap row dy whose image rows are zero border for every pixel of
  // tile m (dy outside [dlo, dhi]) is skipped for that tile (wave-uniform
  // branches around MFMA groups that hold no memory operations)
  int dlo[MT], dhi[MT];
  // the image pixel of M-tile slot `slot` (raster order)
  auto pix_of = [&](int slot, int npxw_) { return min(slot, npxw_ - 1); };
  // one LDS-DMA instruction k (64 slots of 16 B) of chunk c of window wn
  // (every window's image is img_w wide: pix / img_w as a multiply, exact for
  // pix < 4096; the predicate is formed without short-circuit branches).
  // d1g16 keeps its own copy of this lambda (whole images only): staged
  // through one shared helper, both conv_mfma instances compile to other code.
  const uint32_t iw_mag = (1u << 20) / (uint32_t)g.img_w + 1u;
  auto dma = [&](const CWin& wn, int c, float* buf, int k) {
    const int slot = k * 64 + lane;
    const int pix = slot / 5, q = slot - 5 * pix;
    const int iy = (int)(((uint32_t)pix * iw_mag) >> 20), ix = pix - iy * wn.iw;
    const int y = wn.y0 + iy - g.pad, x = wn.x0 + ix - g.pad;
    const bool ok = (q < 4) & (slot < wn.iw * wn.ih * 5) & ((unsigned)y < (unsigned)g.in_h) &
                    ((unsigned)x < (unsigned)g.in_w);
    const float* base = in + ((size_t)wn.s * g.in_h * g.in_w) * CIN + c * kCC;
    const float* src = ok ? base + (y * g.in_w + x) * CIN + 4 * q : g_zero_src;
    dma16(src, buf + k * 256);
  };
  auto kdma_of = [](const CWin& wn) { return (wn.iw * wn.ih * 5 + 63) / 64; };
  float* const buf0 = smem;
  float* const buf1 = smem + buf_floats;
  if ((int)blockIdx.x < nitems) {
    const CWin w0 = conv_win<F, NP>(blockIdx.x, g);
    for (int k = wave; k < kdma_of(w0); k += 4) dma(w0, 0, buf0, k);
  }
  wait_vm0();
  __syncthreads();
  int bsel = 0;
  for (int it = blockIdx.x; it < nitems; it += gridDim.x) {
    const CWin cw = conv_win<F, NP>(it, g);
    const int s = cw.s, part = cw.part, npxw = cw.ow * cw.oh;
    // the next item's window (its first chunk is staged under this item's last)
    const CWin wnext = conv_win<F, NP>(min(it + (int)gridDim.x, nitems - 1), g);
#pragma unroll
    for (int m = 0; m < MT; m++) {
      const int o = pix_of(32 * (2 * m + mg) + j, npxw), oy = o / cw.ow;
      abase[m] = (oy * cw.iw + o - oy * cw.ow) * kPS + 4 * h;
      const int pa = min(32 * (2 * m + mg), npxw - 1), pb = min(pa + 31, npxw - 1);
      dlo[m] = __builtin_amdgcn_readfirstlane(g.pad - (cw.y0 + pb / cw.ow));
      dhi[m] = __builtin_amdgcn_readfirstlane(g.pad + g.in_h - 1 - (cw.y0 + pa / cw.ow));
    }
    const float4* wp = reinterpret_cast<const float4*>(Wimg) + (size_t)(part * 2 + nt) * KS * 64 + lane;
    f32x16 acc[MT];
#pragma unroll
    for (int m = 0; m < MT; m++) acc[m] = zero16();
    // B operands: a ring of 5 taps (2 k-steps each), tap t in slot t % F;
    // the loads run 4 taps ahead and land straight in their slot (the dx
    // loop is unrolled, so no register moves wait on a pending load)
    static_assert(F == 5, "B ring sized for 5x5 taps");
    float4 bq[F][2];
#pragma unroll
    for (int d = 0; d < F - 1; d++)
#pragma unroll
      for (int q = 0; q < 2; q++) bq[d][q] = wp[(size_t)(2 * d + q) * 64];
    for (int c = 0; c < NCH; c++) {
      const float* cur = bsel ? buf1 : buf0;
      float* nxt = bsel ? buf0 : buf1;
      int nit = it, nc = c + 1;
      if (nc == NCH) {
        nit = it + gridDim.x;
        nc = 0;
      }
      const bool stage = nit < nitems;
      const CWin& wd = nc == 0 ? wnext : cw;  // the window the staged chunk belongs to
      const int kdma = kdma_of(wd);
      float4 a[MT], an[MT];
#pragma unroll
      for (int m = 0; m < MT; m++) a[m] = *reinterpret_cast<const float4*>(cur + abase[m]);
#pragma unroll 1
      for (int dy = 0; dy < F; dy++) {
#pragma unroll
        for (int dx = 0; dx < F; dx++) {
          const int t = dy * F + dx;
          const int toff = (dy * g.img_w + dx) * kPS;
          const int tn = dx + 1 < F ? t + 1 : (dy + 1 < F ? t + 1 : t);
          const int toffn = ((tn / F) * g.img_w + (tn % F)) * kPS;
          // B of tap t + 4 into the slot tap t - 1 used
          const int ksb = c * KSC + 2 * (t + F - 1);
#pragma unroll
          for (int q = 0; q < 2; q++)
            bq[(dx + F - 1) % F][q] = wp[(size_t)min(ksb + q, KS - 1) * 64];
          // the next chunk's whole DMA in the first tap, after its B loads.
          // The DMA is inline asm, invisible to the compiler's vmcnt counting,
          // so each vmcnt(8) it emits for a B-ring load 4 taps back also
          // waits for every DMA issued after that load: spread over the first
          // taps (2 per tap), the DMAs were waited on 3 taps after issue; as
          // one burst at tap 0 only the B loads of tap 4 wait for them
          // (same-box A/B: delta1 + gW1 -1.0%, L2 forward -1.0%)
          if (stage && t == 0)
            for (int k = wave; k < kdma; k += 4) dma(wd, nc, nxt, k);
          // k-step (t, 0) while (t, 1) loads; k-step (t, 1) while (t + 1, 0)
          // loads.  sched_barriers pin the order: left alone, the scheduler
          // sinks the prefetch reads below the MFMAs and exposes LDS latency.
#pragma unroll
          for (int m = 0; m < MT; m++)
            an[m] = *reinterpret_cast<const float4*>(cur + abase[m] + toff + 8);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int m = 0; m < MT; m++)
            if (!DELTA || (dy >= dlo[m] && dy <= dhi[m])) {
#pragma unroll
              for (int jj = 0; jj < 4; jj++) acc[m] = mma(a[m][jj], bq[dx][0][jj], acc[m]);
            }
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int m = 0; m < MT; m++)
            a[m] = *reinterpret_cast<const float4*>(cur + abase[m] + toffn);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int m = 0; m < MT; m++)
            if (!DELTA || (dy >= dlo[m] && dy <= dhi[m])) {
#pragma unroll
              for (int jj = 0; jj < 4; jj++) acc[m] = mma(an[m][jj], bq[dx][1][jj], acc[m]);
            }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      wait_vm0();
      __syncthreads();
      bsel ^= 1;
    }
    const int n = part * 64 + nt * 32 + j;
    // output pixels of the window, from its origin
    const size_t obase = ((size_t)s * g.npx + (size_t)cw.y0 * g.out_w + cw.x0) * COUT + n;
    {
      const float bn = DELTA ? 0.0f : bias[n];
      const uint32_t ow_mag = (1u << 20) / (uint32_t)cw.ow + 1u;  // exact for pix < 4096
      // one 32-pixel tile at a time; the lane index is made opaque per tile so
      // the compiler cannot hoist all 16*MT store addresses out of the item loop
#pragma unroll
      for (int m = 0; m < MT; m++) {
        int hl = h;
        asm volatile("" : "+v"(hl));
        const int p0 = 32 * (2 * m + mg) + 4 * hl;
#pragma unroll
        for (int r = 0; r < 16; r++) {
          const int pix = p0 + crow(r, 0);
          if (pix < npxw) {
            // window pixel -> image pixel (row by a reciprocal multiply; 0 for
            // full-width windows, where the runtime division used to run anyway)
            const int py = cw.ow == g.out_w ? 0 : (int)(((uint32_t)pix * ow_mag) >> 20);
            const size_t idx = obase + (size_t)(pix + py * (g.out_w - cw.ow)) * COUT;
            if (DELTA)
              out[idx] = ycur[idx] > 0.0f ? acc[m][r] : 0.0f;
            else
              out[idx] = fmaxf(acc[m][r] + bn, 0.0f);
          }
        }
      }
    }
  }
}
