// wgrad2.hpp -- wgrad2, the fp32 gW2 / gB2 of the wide middle layer (step and
// op-level call) over LDS-DMA'd row bands (geometry: G2Geom; band buffers:
// kGAS .. kG2Lds, wide_layout.hpp).  Included by train_wide.hip inside
// namespace srcnn::wide.

// ---------------------------------------------------------------------------
// wgrad2: gW2[t][c][n] += sum_{s,p} A1[p + off(t)][c] delta2[p][n]; gB2[n] += sum delta2
// (backpropagate.cl:64-113, summed race-free).  16x16x4 MFMA: rows = 16
// channels, cols = 16 n, K = 4 pixels.  Block = (32-channel chunk cq, sample
// group); 8 waves = (16-channel half ct) x (n tile nt), each holding all F*F
// taps (F*F x 4 accumulators).  Per sample, bands of R output rows: the A1
// rows they read (R + F - 1 rows x 32 channels, 48-float pixels) and their
// delta2 rows (64 channels, 80-float pixels) are DMA'd into LDS, double
// buffered across bands; the compute loop only reads LDS.
// ---------------------------------------------------------------------------
template <int CIN, int COUT, int F>
__global__ __launch_bounds__(512, 1) void wgrad2_kernel(const float* __restrict__ A1,
                                                       const float* __restrict__ D2,
                                                       float* __restrict__ slab2, G2Geom g) {
  static_assert(CIN % 32 == 0 && COUT == 64, "shape");
  constexpr int FF = F * F, NCQ = CIN / 32;
  constexpr size_t P2 = (size_t)FF * CIN * COUT + COUT;
  extern __shared__ float smem[];
  const int lane = lane_id(), wave = wave_id(), i = lane & 15, gq = lane >> 4;
  const int ct = wave & 1, nt = wave >> 1;
  int cq = blockIdx.x % NCQ, grp = blockIdx.x / NCQ;
  if (gridDim.x % (8 * NCQ) == 0) {
    // blocks go round-robin over the 8 XCDs: blocks x, x + 8, ... share an
    // XCD, so a group's NCQ channel quarters are put there and read each
    // delta2 band from that XCD's L2 instead of NCQ times from HBM
    // (xcd_item<NCQ>() taken apart: through it the kernel compiles differently)
    const int j = blockIdx.x / 8;
    cq = j % NCQ;
    grp = blockIdx.x % 8 + 8 * (j / NCQ);
  }
  const bool gbw = cq == 0 && ct == 0;
  f32x4 acc[FF];
#pragma unroll
  for (int t = 0; t < FF; t++) acc[t] = zero4();
  float gb = 0.0f;
  // a band is rows x cols output pixels (row-major, cols = w2 for full-width
  // bands); its A1 image is (rows + F - 1) x aw pixels, aw = cols + F - 1
  const int aw = g.aw;
  int abase[16];
  const int bandpx_full = g.rows * g.cols;
#pragma unroll
  for (int kq = 0; kq < 16; kq++) {
    const int k = min(4 * kq + gq, bandpx_full - 1), ky = k / g.cols, kx = k - ky * g.cols;
    abase[kq] = (ky * aw + kx) * kGAS + 16 * ct + i;
  }
  const int dlane = kGAFl + gq * kGDS + 16 * nt + i;
  for (int e = threadIdx.x; e < 2 * kGBuf; e += 512) smem[e] = 0.0f;
  __syncthreads();
  // units = (sample, band) of this group
  const int nsamp = g.batch > grp ? (g.batch - grp + g.groups - 1) / g.groups : 0;
  const int nunits = nsamp * g.nbands;
  auto stage = [&](int u, float* buf, const float* prev) {
    const int s = grp + (u / g.nbands) * g.groups, b = u % g.nbands, by = b / g.nbx;
    const int y0 = by * g.rows, rb = min(g.rows, g.h2 - y0);
    const int x0 = (b - by * g.nbx) * g.cols, cb = min(g.cols, g.w2 - x0);
    // A1 window rows y0 .. y0 + rb + F - 2, columns x0 .. x0 + aw - 1 (past the
    // image: zero)
    const int aslots = (rb + F - 1) * aw * 12;
    const float* asrc = A1 + ((size_t)s * g.h1 * g.w1 + (size_t)y0 * g.w1 + x0) * CIN + 32 * cq;
    const int dslots = (kBandPx + 4) * 20;
    const float* dsrc = D2 + ((size_t)s * g.h2 * g.w2 + (size_t)y0 * g.w2 + x0) * COUT;
    int k0 = 0;  // first 64-slot DMA group of the A1 image that comes from HBM
    if (g.nbx == 1 && b > 0 && prev) {
      // the band's first F - 1 A1 rows are the previous band's last F - 1 rows
      // (that band is full, rows = g.rows), already in LDS: copied LDS -> LDS in
      // whole 64-slot groups, the rest DMA'd, so each A1 row leaves HBM once
      k0 = (F - 1) * aw * 12 / 64;
      const float4* src = reinterpret_cast<const float4*>(prev + g.rows * aw * kGAS);
      float4* dst = reinterpret_cast<float4*>(buf);
      for (int e = threadIdx.x; e < k0 * 64; e += 512) dst[e] = src[e];
    }
    if (g.nbx == 1) {  // full-width bands: the band's rows are contiguous in HBM
      for (int k = k0 + wave; k * 64 < aslots; k += 8) {
        const int slot = k * 64 + lane, pix = slot / 12, q = slot - 12 * pix;
        const bool ok = q < 8 && slot < aslots;
        dma16(ok ? asrc + (size_t)pix * CIN + 4 * q : g_zero_src, buf + k * 256);
      }
      const int dpx = rb * g.w2;
      for (int k = wave; k * 64 < dslots; k += 8) {
        const int slot = k * 64 + lane, pix = slot / 20, q = slot - 20 * pix;
        const bool ok = q < 16 && pix < dpx;
        dma16(ok ? dsrc + (size_t)pix * COUT + 4 * q : g_zero_src, buf + kGAFl + k * 256);
      }
    } else {
      for (int k = wave; k * 64 < aslots; k += 8) {
        const int slot = k * 64 + lane, pix = slot / 12, q = slot - 12 * pix;
        const int py = pix / aw, px = pix - py * aw;
        const bool ok = q < 8 && slot < aslots && x0 + px < g.w1;
        dma16(ok ? asrc + ((size_t)py * g.w1 + px) * CIN + 4 * q : g_zero_src, buf + k * 256);
      }
      for (int k = wave; k * 64 < dslots; k += 8) {
        const int slot = k * 64 + lane, pix = slot / 20, q = slot - 20 * pix;
        const int py = pix / g.cols, px = pix - py * g.cols;
        const bool ok = q < 16 && py < rb && px < cb;
        dma16(ok ? dsrc + ((size_t)py * g.w2 + px) * COUT + 4 * q : g_zero_src, buf + kGAFl + k * 256);
      }
    }
  };
  int bsel = 0;
  if (nunits > 0) stage(0, smem, nullptr);
  for (int u = 0; u < nunits; u++) {
    wait_vm0();
    __syncthreads();  // unit u landed; everyone is done with the other buffer
    const float* cur = smem + (bsel ? kGBuf : 0);
    if (u + 1 < nunits) stage(u + 1, smem + (bsel ? 0 : kGBuf), cur);
    // k-step kq's operands (delta2 value + the F*F A1 taps) are read one
    // k-step ahead into two named register sets, pinned by sched_barriers:
    // left alone, the scheduler reads two taps at a time right before their
    // MFMA pair and waits out the LDS latency every other MFMA
    float av[2][FF], bv[2];
    auto rd = [&](int kq) {
      bv[kq & 1] = cur[dlane + kq * 4 * kGDS];
#pragma unroll
      for (int t = 0; t < FF; t++) av[kq & 1][t] = cur[abase[kq] + ((t / F) * aw + t % F) * kGAS];
    };
    rd(0);
#pragma unroll
    for (int kq = 0; kq < 16; kq++) {
      if (kq + 1 < 16) rd(kq + 1);
      __builtin_amdgcn_sched_barrier(0);
      const float b = bv[kq & 1];
      if (gbw) gb += b;
#pragma unroll
      for (int t = 0; t < FF; t++) {
        const float a = av[kq & 1][t];
        acc[t] = mma16(a, b, acc[t]);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    bsel ^= 1;
  }
  // slab rows of this block: channels 32 cq + 16 ct + 4 gq + r, n = 16 nt + i
  float* out = slab2 + (size_t)grp * P2;
#pragma unroll
  for (int t = 0; t < FF; t++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int c = 32 * cq + 16 * ct + 4 * gq + r;
      out[((size_t)t * CIN + c) * COUT + 16 * nt + i] = acc[t][r];
    }
  if (gbw) {
    gb += __shfl_down(gb, 32, 64);
    gb += __shfl_down(gb, 16, 64);
    if (gq == 0) out[(size_t)FF * CIN * COUT + 16 * nt + i] = gb;
  }
}
