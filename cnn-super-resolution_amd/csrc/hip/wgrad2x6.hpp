// wgrad2x6.hpp -- wgrad2x6, the split-bf16 gW2 / gB2 of the wide step (LDS
// images: kG6RowP .. kG6Lds, wide_layout.hpp).  Included by train_wide.hip
// inside namespace srcnn::wide.

// ---------------------------------------------------------------------------
// wgrad2x6: wgrad2 with split-bf16 products (split.hpp) on
// v_mfma_f32_16x16x32_bf16: rows = 16 channels, cols = 16 n, K = 32 output
// pixels per k-step as 4 RUNS of 8 consecutive pixels of an output row (lane
// group gq = one run; a row of w2 <= 24 pixels is ceil(w2 / 8) runs, the
// slots past w2 carry zero delta2).  Block = (16-channel slice cq, sample
// group), 8 waves = (n half nh) x (tap group tg: taps 0-6 / 7-12 / 13-18 /
// 19-24), a wave holding 2 n tiles x 7 taps of 16x16 accumulators (tap group
// 3's spare slot sums gB2 with an all-ones A operand in the cq = 0 blocks).
// Per sample, bands of 4 output rows (one k-step = the 4 rows' runs at one
// column, so a read's 64 lanes hit 64 banks; a last band of < 4 rows packs
// its runs row by row):
//   A: A1 rows in a ring of 8, split, as PAIR images: dword x of (channel,
//      part, ring row) holds the parts of pixels x and x + 1, so a run's 8
//      values under any tap are dwords m, m+2, m+4, m+6 (two ds_read2_b32);
//      ring rows 48 dwords apart, channels kG6CP (= 1 mod 64) apart
//   B: the band's delta2 rows split, [part][row][n][24 px] bf16 (n pitch 12
//      dwords: each 16-lane group of a ds_read_b128 conflict-free)
// The next band's rows are register-staged (loads issued at the band's
// start) and split into LDS after its MFMAs, between two barriers.
// ---------------------------------------------------------------------------
template <int CIN, int COUT, int F>
__global__ __launch_bounds__(512, 1) void wgrad2x6_kernel(const float* __restrict__ A1,
                                                         const float* __restrict__ D2,
                                                         float* __restrict__ slab2, G2Geom g) {
  using mfma::bf16x8;
  using mfma::f32x2;
  using mfma::u32x4;
  constexpr int FF = F * F, NCQ = CIN / 16, TG = (FF + 3) / 4;
  static_assert(CIN % 16 == 0 && COUT == 64 && F <= 5 && FF % 4 == 1, "shape");
  constexpr size_t P2 = (size_t)FF * CIN * COUT + COUT;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  uint32_t* const ra = reinterpret_cast<uint32_t*>(smem);
  uint16_t* const dh = reinterpret_cast<uint16_t*>(smem + kG6A);
  const int lane = lane_id(), wave = wave_id(), i16 = lane & 15, gq = lane >> 4;
  const int nh = wave & 1, tg = wave >> 1;
  const int t0 = tg == 0 ? 0 : TG + (tg - 1) * (TG - 1), tcnt = tg == 0 ? TG : TG - 1;
  int cq = blockIdx.x % NCQ, grp = blockIdx.x / NCQ;
  if (gridDim.x % (8 * NCQ) == 0) {  // a group's NCQ slices on one XCD (wgrad2)
    const int j = blockIdx.x / 8;
    cq = j % NCQ;
    grp = blockIdx.x % 8 + 8 * (j / NCQ);
  }
  const bool gbw = cq == 0 && tg == 3;  // (tap group 3 has TG - 1 taps: slot TG - 1 is free)
  const int w1 = g.w1, h1 = g.h1, w2 = g.w2, h2 = g.h2;
  const int nb = (h2 + 3) / 4, nrx = (w2 + 7) / 8;
  for (int e = threadIdx.x; e < kG6A + kG6D; e += 512) ra[e] = 0u;
  f32x4 acc[TG][2];
#pragma unroll
  for (int t = 0; t < TG; t++) acc[t][0] = acc[t][1] = zero4();
  const int nsamp = g.batch > grp ? (g.batch - grp + g.groups - 1) / g.groups : 0;
  const int nunits = nsamp * nb;
  // register staging in runs of 8 pixels (coalesced loads, 16-B LDS writes),
  // by wave role:
  //   waves 0-5, delta2: thread = (band row dr, run dxr, n pair dnp), the
  //     run's 8 pixels x 2 n (a wave's load: two pixels' 64 n, 512 B)
  //   waves 6-7, A1: thread = (ring row, run axr, channel pair acp), the
  //     run's 8 pixels + the next one (the pair image's last dword) x 2
  //     channels; two passes for a band's first 8 rows
  // Each role's loads sit in one wave-uniform branch (loads in per-load
  // branches make the compiler wait for each before issuing the next).
  const int tid = threadIdx.x;
  const bool drole = wave < 3, arole = wave >= 6;
  const int dnq = tid & 15, dru = (tid >> 4) % 12, dr = dru / 3, dxr = dru - 3 * dr;
  const int ta = tid & 127, acp = ta & 7, aru = ta >> 3, ar = aru >> 2, axr = aru & 3;
  f32x2 xa[2][9];
  f32x4 xd[8];
  auto rows_of = [&](int u, int& s, int& b, int& alo, int& ahi) __attribute__((always_inline)) {
    s = grp + (u / nb) * g.groups;
    b = u % nb;
    alo = b == 0 ? 0 : 4 * b + 4;
    ahi = min(4 * b + 8, h1);
  };
  auto load = [&](int u) __attribute__((always_inline)) {
    int s, b, alo, ahi;
    rows_of(u, s, b, alo, ahi);
    if (drole) {
      const int row = 4 * b + dr;
      const bool dok = dxr < nrx && row < h2;
      const size_t dbase = (((size_t)s * h2 + row) * w2 + 8 * dxr) * COUT + 4 * dnq;
#pragma unroll
      for (int j = 0; j < 8; j++)
        xd[j] = *reinterpret_cast<const f32x4*>(D2 + (dok && 8 * dxr + j < w2 ? dbase + (size_t)j * COUT : 0));
    } else if (arole) {
#pragma unroll
      for (int pass = 0; pass < 2; pass++) {
        const int row = alo + ar + 4 * pass;
        const size_t abase = (((size_t)s * h1 + row) * w1 + 8 * axr) * CIN + 16 * cq + 2 * acp;
#pragma unroll
        for (int j = 0; j < 9; j++)
          xa[pass][j] = *reinterpret_cast<const f32x2*>(
              A1 + (row < ahi && 8 * axr + j < w1 ? abase + (size_t)j * CIN : 0));
      }
    }
  };
  auto store = [&](int u) __attribute__((always_inline)) {
    int s, b, alo, ahi;
    rows_of(u, s, b, alo, ahi);
    if (arole) {
#pragma unroll
      for (int pass = 0; pass < 2; pass++) {
        const int row = alo + ar + 4 * pass;
        if (row < ahi) {
          const int slot = row & (kG6Ring - 1);
#pragma unroll
          for (int e = 0; e < 2; e++) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; j++) v[j] = 8 * axr + j < w1 ? xa[pass][j][e] : 0.0f;
            bf16x8 pp[3];
            mfma::split8(v, pp);
            __bf16 p8[3];
            mfma::split3(8 * axr + 8 < w1 ? xa[pass][8][e] : 0.0f, p8[0], p8[1], p8[2]);
            uint32_t* d = ra + (2 * acp + e) * kG6CP + slot * kG6RowP + 8 * axr;
#pragma unroll
            for (int q = 0; q < 3; q++) {
              const u32x4 lo = __builtin_bit_cast(u32x4, pp[q]);  // parts of pixels 2i, 2i + 1 (i < 4)
              uint32_t w[8];
#pragma unroll
              for (int i = 0; i < 4; i++) w[2 * i] = lo[i];
#pragma unroll
              for (int i = 0; i < 3; i++) w[2 * i + 1] = (lo[i] >> 16) | (lo[i + 1] << 16);
              w[7] = (lo[3] >> 16) | ((uint32_t)__builtin_bit_cast(uint16_t, p8[q]) << 16);
#pragma unroll
              for (int i = 0; i < 8; i++) d[q * kG6QP + i] = w[i];
            }
          }
        }
      }
    } else if (drole && dxr < nrx) {
      const bool rok = 4 * b + dr < h2;  // rows past the image: zero delta2
#pragma unroll
      for (int e = 0; e < 4; e++) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; j++) v[j] = rok && 8 * dxr + j < w2 ? xd[j][e] : 0.0f;
        bf16x8 pp[3];
        mfma::split8(v, pp);
#pragma unroll
        for (int q = 0; q < 3; q++)
          *reinterpret_cast<bf16x8*>(dh + ((q * 4 + dr) * 64 + 4 * dnq + e) * (2 * kG6NP) + 8 * dxr) = pp[q];
      }
    }
  };
  if (nunits > 0) {
    load(0);
    __syncthreads();  // (the LDS clear)
    store(0);
  }
  __syncthreads();
  bf16x8 ones;
#pragma unroll
  for (int e = 0; e < 8; e++) ones[e] = (__bf16)1.0f;
  for (int u = 0; u < nunits; u++) {
    if (u + 1 < nunits) load(u + 1);
    const int y0 = 4 * (u % nb), nr = min(4, h2 - y0);
    const bool full = nr == 4;
    const int nks = full ? nrx : (nr * nrx + 3) / 4;
    for (int kk = 0; kk < nks; kk++) {
      // this lane group's run: band row rg, first column x0
      const int j = 4 * kk + gq, rg = full ? gq : j / nrx, x0 = full ? 8 * kk : 8 * (j - rg * nrx);
      bf16x8 bq[2][3];
#pragma unroll
      for (int n2 = 0; n2 < 2; n2++)
#pragma unroll
        for (int q = 0; q < 3; q++)
          bq[n2][q] = *reinterpret_cast<const bf16x8*>(
              dh + ((q * 4 + rg) * 64 + 32 * nh + 16 * n2 + i16) * (2 * kG6NP) + x0);
      const int ab = i16 * kG6CP + x0, yr = y0 + rg;
      // tap slot ti's A operand (slot TG - 1 of tap groups 1-3 reads a valid
      // address and is not used)
      auto rda = [&](int ti, bf16x8 (&a)[3]) __attribute__((always_inline)) {
        const int t = min(t0 + ti, FF - 1), dy = t / F, dx = t - dy * F;
        const uint32_t* pa = ra + ab + ((yr + dy) & (kG6Ring - 1)) * kG6RowP + dx;
#pragma unroll
        for (int q = 0; q < 3; q++) {
          u32x4 w;
          w[0] = pa[q * kG6QP];
          w[1] = pa[q * kG6QP + 2];
          w[2] = pa[q * kG6QP + 4];
          w[3] = pa[q * kG6QP + 6];
          a[q] = __builtin_bit_cast(bf16x8, w);
        }
      };
      // slots 0 .. TG - 2 (every wave's) without branches, each slot's reads
      // issued under the previous slot's MFMAs; then the last slot
      bf16x8 a2[2][3];
      rda(0, a2[0]);
#pragma unroll
      for (int ti = 0; ti < TG - 1; ti++) {
        rda(ti + 1, a2[(ti + 1) & 1]);
        acc[ti][0] = mfma::mma16_x6(a2[ti & 1], bq[0], acc[ti][0]);
        acc[ti][1] = mfma::mma16_x6(a2[ti & 1], bq[1], acc[ti][1]);
      }
      if (tcnt == TG) {
        acc[TG - 1][0] = mfma::mma16_x6(a2[(TG - 1) & 1], bq[0], acc[TG - 1][0]);
        acc[TG - 1][1] = mfma::mma16_x6(a2[(TG - 1) & 1], bq[1], acc[TG - 1][1]);
      } else if (gbw) {
        // gB2[n] += sum_k delta2[k][n]: the three parts against ones
#pragma unroll
        for (int n2 = 0; n2 < 2; n2++)
#pragma unroll
          for (int q = 0; q < 3; q++) acc[TG - 1][n2] = mfma::mma16_bf16(ones, bq[n2][q], acc[TG - 1][n2]);
      }
    }
    __syncthreads();  // the band's operands are consumed
    if (u + 1 < nunits) store(u + 1);
    __syncthreads();
  }
  // slab rows of this block: channels 16 cq + 4 gq + r, n = 32 nh + 16 n2 + i16
  float* out = slab2 + (size_t)grp * P2;
#pragma unroll
  for (int ti = 0; ti < TG; ti++) {
    if (ti < tcnt) {
      const int t = t0 + ti;
#pragma unroll
      for (int n2 = 0; n2 < 2; n2++)
#pragma unroll
        for (int r = 0; r < 4; r++)
          out[((size_t)t * CIN + 16 * cq + 4 * gq + r) * COUT + 32 * nh + 16 * n2 + i16] = acc[ti][n2][r];
    } else if (gbw && gq == 0) {
#pragma unroll
      for (int n2 = 0; n2 < 2; n2++) out[(size_t)FF * CIN * COUT + 32 * nh + 16 * n2 + i16] = acc[ti][n2][0];
    }
  }
}
