// wl2x6.hpp -- the split-bf16 convolutions of the wide step over a split chunk
// image of 112-B pixel rows (layout: SplitImgLds, w6_pitch, wide_layout.hpp):
// the W2 prep kernels, wl2x6_fwd (L2 forward, two images) and wd1x6 (delta1,
// one image).  Included by train_wide.hip inside namespace srcnn::wide.

// ---------------------------------------------------------------------------
// wl2x6: the L2 forward of the step (conv_mfma_kernel<.., false> over the
// whole image) with its products in split-bf16 form (split.hpp): per tap and
// 16-channel chunk ONE 32x32x16 k-step of six part products instead of 8
// fp32 32x32x2 MFMAs (6 x 32 against 8 x 64 matrix cycles).
//   A: the chunk's image split once into LDS, [pixel][part][16 ch] bf16 rows
//      of 112 B (16-lane groups of ds_read_b128 conflict-free); lane (pixel
//      j, half h) reads channels 8h .. 8h+7 of each part: 3 ds_read_b128
//   B: W2 split by wprep_w2x6_kernel into [nt][chunk][tap][part][lane][8]
//      bf16, lane (n, h) holding W2[tap][16 chunk + 8h + i][32 nt + n]
// The next chunk is register-staged (16-B global loads issued at the chunk's
// start) and split into the other image after the chunk's MFMAs: one barrier
// per chunk, no LDS-DMA.  Same work split, C layout and epilogue as conv_mfma.
// ---------------------------------------------------------------------------

// One split W2 image [ntile][chunk][tap][part][lane][8] bf16 of W2[tap][CIN][COUT]:
// lane (n, h) holds the weight of contraction channel ch = 16 chunk + 8h + i
// and output channel 32 ntile + n,
//   forward (wl2x6):  W2[tap][ch][n]          (ch in CIN, n in COUT)
//   FLIP (wd1x6):     W2[flip(tap)][n][ch]    (ch in COUT, n in CIN)
template <int CIN, int COUT, int F, bool FLIP>
__device__ __forceinline__ void wprep_x6(const float* __restrict__ W2, uint16_t* __restrict__ Wx) {
  constexpr int NCH = (FLIP ? COUT : CIN) / 16, FF = F * F, NT = (FLIP ? CIN : COUT) / 32;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= NT * NCH * FF * 64 * 8) return;
  const int i = e & 7, L = (e >> 3) & 63, rest = e >> 9;
  const int t = rest % FF, c = (rest / FF) % NCH, nt = rest / (FF * NCH);
  const int dy = t / F, dx = t - dy * F, tf = (F - 1 - dy) * F + (F - 1 - dx);
  const int ch = 16 * c + 8 * (L >> 5) + i, n = 32 * nt + (L & 31);
  __bf16 p[3];
  mfma::split3(FLIP ? W2[((size_t)tf * CIN + n) * COUT + ch] : W2[((size_t)t * CIN + ch) * COUT + n], p[0], p[1], p[2]);
#pragma unroll
  for (int q = 0; q < 3; q++) Wx[((size_t)rest * 3 + q) * 512 + L * 8 + i] = __builtin_bit_cast(uint16_t, p[q]);
}

template <int CIN, int COUT, int F>
__global__ void wprep_w2x6_kernel(const float* __restrict__ W2, uint16_t* __restrict__ Wx) {
  wprep_x6<CIN, COUT, F, false>(W2, Wx);
}
// (delta1's image: contraction over n2 = COUT, outputs the n1 = CIN channels)
template <int N1, int N2, int F>
__global__ void wprep_d1x6_kernel(const float* __restrict__ W2, uint16_t* __restrict__ Wx) {
  wprep_x6<N1, N2, F, true>(W2, Wx);
}

// (wl2x6 and wd1x6 each split and store their staged quads and store their
// tiles by their own copy of the code: through shared forceinline helpers the
// compiler reschedules both one-wave-per-SIMD kernels,
// profiles/r13_wide_split/isa_identity.md)

template <int CIN, int COUT, int F, int MT>
__global__ __launch_bounds__(256, 1) void wl2x6_fwd_kernel(const float* __restrict__ in,
                                                          const uint16_t* __restrict__ Wx,
                                                          const float* __restrict__ bias,
                                                          float* __restrict__ out, CGeom g) {
  using mfma::bf16x8;
  constexpr int NCH = CIN / 16, FF = F * F;
  static_assert(CIN % 16 == 0 && COUT == 64, "one 64-channel part");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int lane = lane_id(), wave = wave_id(), j = lane & 31, h = lane >> 5;
  const int nt = wave & 1, mg = wave >> 1;
  const int ipx = g.img_w * g.img_h, npx = g.npx;
  const SplitImgLds L(g, 2);
  const int pitch = L.pitch;
  uint32_t* const img0 = reinterpret_cast<uint32_t*>(smem);
  uint32_t* const img1 = img0 + L.img;
  // register staging of one chunk: quad i = pixel i / 4, channels 4 (i % 4) ..
  constexpr int kQ = (kW6ImgMax * 4 + 255) / 256;
  f32x4 xr[kQ];
  int soff[kQ];  // quad i's LDS offset in an image (the same every chunk)
#pragma unroll
  for (int k = 0; k < kQ; k++) {
    const int i = threadIdx.x + 256 * k, p = i >> 2, py = p / g.img_w;
    soff[k] = py * pitch + (p - py * g.img_w) * kW6Row + 2 * (i & 3);
  }
  auto load = [&](int s, int c) __attribute__((always_inline)) {
    const float* src = in + (size_t)s * ipx * CIN + 16 * c;
#pragma unroll
    for (int k = 0; k < kQ; k++) {
      const int i = threadIdx.x + 256 * k;
      if (i < ipx * 4) xr[k] = *reinterpret_cast<const f32x4*>(src + (size_t)(i >> 2) * CIN + 4 * (i & 3));
    }
  };
  auto store_split = [&](uint32_t* buf) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < kQ; k++) {
      const int i = threadIdx.x + 256 * k;
      if (i < ipx * 4) {
        float v[8];
#pragma unroll
        for (int e = 0; e < 4; e++) v[e] = v[4 + e] = xr[k][e];
        bf16x8 pp[3];
        mfma::split8(v, pp);
        uint32_t* d = buf + soff[k];
#pragma unroll
        for (int q = 0; q < 3; q++) {
          const mfma::u32x4 w = __builtin_bit_cast(mfma::u32x4, pp[q]);
          *reinterpret_cast<uint2*>(d + 8 * q) = make_uint2(w[0], w[1]);
        }
      }
    }
  };
  const int nitems = g.batch;
  if ((int)blockIdx.x < nitems) {
    load(blockIdx.x, 0);
    store_split(img0);
  }
  __syncthreads();
  int phase = 0;
  for (int it = blockIdx.x; it < nitems; it += gridDim.x) {
    const int s = it;
    int abase[MT];
#pragma unroll
    for (int m = 0; m < MT; m++) {
      const int o = min(32 * (2 * m + mg) + j, npx - 1), oy = o / g.out_w;
      abase[m] = oy * pitch + (o - oy * g.out_w) * kW6Row + 4 * h;
    }
    f32x16 acc[MT];
#pragma unroll
    for (int m = 0; m < MT; m++) acc[m] = zero16();
    const uint16_t* wl = Wx + (size_t)nt * NCH * FF * 3 * 512 + lane * 8;
    for (int c = 0; c < NCH; c++) {
      const uint32_t* cur = phase ? img1 : img0;
      uint32_t* nxt = phase ? img0 : img1;
      const int ns = c + 1 < NCH ? s : s + (int)gridDim.x, nc = c + 1 < NCH ? c + 1 : 0;
      const bool more = ns < nitems;
      if (more) load(ns, nc);
      const uint16_t* wc = wl + (size_t)c * FF * 3 * 512;
      // B operands: this tap's, and the next tap's loaded under its MFMAs
      bf16x8 bq[3], bn[3];
#pragma unroll
      for (int q = 0; q < 3; q++) bq[q] = *reinterpret_cast<const bf16x8*>(wc + q * 512);
#pragma unroll 1
      for (int dy = 0; dy < F; dy++) {
#pragma unroll
        for (int dx = 0; dx < F; dx++) {
          const int t = dy * F + dx, tn = min(t + 1, FF - 1);
#pragma unroll
          for (int q = 0; q < 3; q++) bn[q] = *reinterpret_cast<const bf16x8*>(wc + (tn * 3 + q) * 512);
          const int toff = dy * pitch + dx * kW6Row;
#pragma unroll
          for (int m = 0; m < MT; m++) {
            bf16x8 a[3];
#pragma unroll
            for (int q = 0; q < 3; q++) a[q] = *reinterpret_cast<const bf16x8*>(cur + abase[m] + toff + 8 * q);
            acc[m] = mfma::mma_x6(a, bq, acc[m]);
          }
#pragma unroll
          for (int q = 0; q < 3; q++) bq[q] = bn[q];
        }
      }
      if (more) store_split(nxt);
      __syncthreads();
      phase ^= 1;
    }
    const int n = nt * 32 + j;
    const float bn = bias[n];
    const size_t obase = (size_t)s * npx * COUT + n;
#pragma unroll
    for (int m = 0; m < MT; m++) {
      int hl = h;
      asm volatile("" : "+v"(hl));
      const int p0 = 32 * (2 * m + mg) + 4 * hl;
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int pix = p0 + crow(r, 0);
        if (pix < npx) out[obase + (size_t)pix * COUT] = fmaxf(acc[m][r] + bn, 0.0f);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// wd1x6: delta1 of the step (conv_mfma<.., true>'s contraction) with split-bf16
// products, written to D1 BEFORE its ReLU' factor; gW1 / gB1 then come from
// D1 and A1 (l1_grad_kernel<.., MASK>, which applies [A1 > 0]):
//   delta1[p][n] = [A1[p][n] > 0] sum_{tap, c} delta2pad[p + off(tap)][c] W2[flip(tap)][n][c]
// (layer_deltas.cl; delta2 zero-padded by F - 1).  Work item = (sample, 64
// delta1 channels), the two items of a sample on one XCD (d1g16); waves as in
// wl2x6 (N tile nt of 32 channels, M group mg of the 32-pixel tiles 2m + mg).
// A 16-channel chunk of the padded delta2 image (29 x 29 px for 33x33 tiles)
// is split into ONE LDS image of wl2x6's 112-B rows: the next chunk is
// register-staged under the chunk's MFMAs and split into the image between
// two barriers.  Tap rows whose source rows are all zero border for every
// pixel of a tile are skipped (wave-uniform, conv_mfma).
// ---------------------------------------------------------------------------
// (B: W2 split by wprep_d1x6_kernel above, lane (n, h) holding
// W2[flip(tap)][32 ntile + n][16 chunk + 8h + i])
template <int CIN, int COUT, int F, int MT>
__global__ __launch_bounds__(256, 1) void wd1x6_kernel(const float* __restrict__ in,
                                                      const uint16_t* __restrict__ Wx,
                                                      float* __restrict__ out, CGeom g) {
  using mfma::bf16x8;
  constexpr int NCH = CIN / 16, FF = F * F, NP = COUT / 64;
  static_assert(CIN % 16 == 0 && COUT % 64 == 0 && MT % 2 == 0, "shape");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  uint32_t* const img = reinterpret_cast<uint32_t*>(smem);
  const int lane = lane_id(), wave = wave_id(), j = lane & 31, h = lane >> 5;
  const int nt = wave & 1, mg = wave >> 1;
  const int ipx = g.img_w * g.img_h, npx = g.npx, ow = g.out_w;
  const int pitch = SplitImgLds(g, 1).pitch;
  const int nitems = g.batch * NP;
  const int vb = xcd_item<NP>();  // the NP items of a sample on one XCD (d1g16)
  constexpr int kQ = (kWD6ImgMax * 4 + 255) / 256;
  f32x4 xr[kQ];
  // staged quad i = pixel i / 4 of the padded image, channels 4 (i % 4) ..;
  // -1: zero border or past the image
  auto src_of = [&](int k) __attribute__((always_inline)) {
    const int i = threadIdx.x + 256 * k, p = i >> 2, iy = p / g.img_w, ix = p - iy * g.img_w;
    const int y = iy - g.pad, x = ix - g.pad;
    const bool ok = i < ipx * 4 && (unsigned)y < (unsigned)g.in_h && (unsigned)x < (unsigned)g.in_w;
    return ok ? (y * g.in_w + x) * CIN + 4 * (i & 3) : -1;
  };
  // (every load issued, the unused ones at offset 0: see wgrad2x6)
  auto load = [&](int s, int c) __attribute__((always_inline)) {
    const float* src = in + (size_t)s * g.in_h * g.in_w * CIN + 16 * c;
#pragma unroll
    for (int k = 0; k < kQ; k++) {
      const int o = src_of(k);
      xr[k] = *reinterpret_cast<const f32x4*>(src + (o >= 0 ? o : 0));
    }
  };
  auto store_split = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < kQ; k++) {
      const int i = threadIdx.x + 256 * k;
      if (i < ipx * 4) {
        const bool ok = src_of(k) >= 0;
        float v[8];
#pragma unroll
        for (int e = 0; e < 4; e++) v[e] = v[4 + e] = ok ? xr[k][e] : 0.0f;
        bf16x8 pp[3];
        mfma::split8(v, pp);
        const int p = i >> 2, py = p / g.img_w;
        uint32_t* d = img + py * pitch + (p - py * g.img_w) * kW6Row + 2 * (i & 3);
#pragma unroll
        for (int q = 0; q < 3; q++) {
          const mfma::u32x4 w = __builtin_bit_cast(mfma::u32x4, pp[q]);
          *reinterpret_cast<uint2*>(d + 8 * q) = make_uint2(w[0], w[1]);
        }
      }
    }
  };
  if (vb < nitems) {
    load(vb / NP, 0);
    store_split();
  }
  __syncthreads();
  for (int it = vb; it < nitems; it += gridDim.x) {
    const int s = it / NP, part = it - s * NP;
    int abase[MT], dlo[MT], dhi[MT];
#pragma unroll
    for (int m = 0; m < MT; m++) {
      const int p0 = 32 * (2 * m + mg), p1 = min(p0 + 31, npx - 1);
      const int o = min(p0 + j, npx - 1), oy = o / ow;
      abase[m] = oy * pitch + (o - oy * ow) * kW6Row + 4 * h;
      const int oy0 = p0 / ow, oy1 = p1 / ow;
      dlo[m] = p0 < npx ? max(0, g.pad - oy1) : F;
      dhi[m] = min(F - 1, g.pad + g.in_h - 1 - oy0);
    }
    f32x16 acc[MT];
#pragma unroll
    for (int m = 0; m < MT; m++) acc[m] = zero16();
    const uint16_t* wl = Wx + (size_t)(2 * part + nt) * NCH * FF * 3 * 512 + lane * 8;
    for (int c = 0; c < NCH; c++) {
      const int nit = c + 1 < NCH ? it : it + (int)gridDim.x, nc = c + 1 < NCH ? c + 1 : 0;
      const bool more = nit < nitems;
      load(more ? nit / NP : s, nc);
      const uint16_t* wc = wl + (size_t)c * FF * 3 * 512;
      bf16x8 bq[3], bn[3];
#pragma unroll
      for (int q = 0; q < 3; q++) bq[q] = *reinterpret_cast<const bf16x8*>(wc + q * 512);
      // A operands read one tile ahead, unconditionally (only the MFMAs of a
      // skipped tap row are branched around: with the reads inside the branch
      // each tile waited out its LDS latency, one wave per SIMD)
      bf16x8 a2[2][3];
      auto rd = [&](int m, int toff, bf16x8 (&a)[3]) __attribute__((always_inline)) {
#pragma unroll
        for (int q = 0; q < 3; q++) a[q] = *reinterpret_cast<const bf16x8*>(img + abase[m] + toff + 8 * q);
      };
      rd(0, 0, a2[0]);
#pragma unroll 1
      for (int dy = 0; dy < F; dy++) {
#pragma unroll
        for (int dx = 0; dx < F; dx++) {
          const int t = dy * F + dx, tn = min(t + 1, FF - 1);
#pragma unroll
          for (int q = 0; q < 3; q++) bn[q] = *reinterpret_cast<const bf16x8*>(wc + (tn * 3 + q) * 512);
          const int toff = dy * pitch + dx * kW6Row;
          const int toffn = (tn / F) * pitch + (tn % F) * kW6Row;
#pragma unroll
          for (int m = 0; m < MT; m++) {
            // (MT even: tile m's operands are in a2[m & 1]; the next tap's tile 0 in a2[0])
            if (m + 1 < MT)
              rd(m + 1, toff, a2[(m + 1) & 1]);
            else
              rd(0, toffn, a2[0]);
            if (dy >= dlo[m] && dy <= dhi[m]) acc[m] = mfma::mma_x6(a2[m & 1], bq, acc[m]);
          }
#pragma unroll
          for (int q = 0; q < 3; q++) bq[q] = bn[q];
        }
      }
      __syncthreads();  // the chunk's image is consumed
      if (more) store_split();
      __syncthreads();
    }
    const int n = part * 64 + nt * 32 + j;
    const size_t obase = (size_t)s * npx * COUT + n;
#pragma unroll
    for (int m = 0; m < MT; m++) {
      int hl = h;
      asm volatile("" : "+v"(hl));
      const int p0 = 32 * (2 * m + mg) + 4 * hl;
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int pix = p0 + crow(r, 0);
        if (pix < npx) out[obase + (size_t)pix * COUT] = acc[m][r];  // (ReLU' in l1_grad_kernel)
      }
    }
  }
}
