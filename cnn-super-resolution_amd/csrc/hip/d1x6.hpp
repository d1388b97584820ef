// d1x6.hpp -- kernel 3 of the fused step (delta1 + gW1/gB1 + gW2/gB2) for
// the reference default net (n1 = 64, n2 = 32, f1 = 9) in split-bf16
// products (split.hpp), paired with l12x6 (its A1 layout and pixel order,
// runs.hpp).  Included by train_fused.hip inside namespace srcnn::fused, after
// d3taps.hpp, fused_layout.hpp (its LDS layout D6Lds, Geom, RunGeom, D3Geom,
// d6tr.hpp's address maps) and l12x6.hpp (the mfma:: names it imports); uses
// train_fused.hip's g_clk.
// Same mathematics as d1c_grad12_kernel (layer_deltas.cl:42-127 with f = 1,
// backpropagate.cl:56-114 for layers 1 and 2).
//
// One wave per chunk of 32 slots (8 runs of 4 pixels), all 64 channels, on
// v_mfma_f32_32x32x16_bf16 (x6: six part products per 16-slot k-step):
//   delta1[p][c] = sum_n delta2[p][n] W2[c][n]       M = slots, N = channels
//                  (2 tiles), K = n2 (2 k-steps); delta2 rows straight from
//                  HBM (lane = slot), W2 a split image in LDS.  The result
//                  has the CHANNEL on the lane and the slots in registers
//                  (register r of half h = slot crow(r, h)), the layout of
//                  l12x6's transposed A1 loads, so relu'(A1) is elementwise
//   gW2[c][n] += sum_p A1[p][c] delta2[p][n]         K = slots: A = A1^T as
//                  loaded, B = delta2^T through a per-wave LDS transpose (of
//                  the fp32 values, split again; kTr: of delta1's split parts,
//                  a bf16 image read back with transposed reads, d6tr.hpp)
//   gW1[t][c] += sum_p X[p + off(t)] delta1[p][c]    written as gW1^T: M =
//                  channels, N = taps (3 tiles: 81 taps, the ones column of
//                  gB1, zeros), K = slots; A = delta1 as it stands, B = X
//                  windows: the slots of k-step m, half h are runs 4m + h and
//                  4m + 2 + h, each 4 consecutive X values under any tap --
//                  one ds_read2_b32 per run and part from part-interleaved
//                  pair images (row runs: R; column runs: T, column-major)
//                  kD3: in two fp16 parts per operand instead (split.hpp),
//                  three v_mfma_f32_32x32x16_f16 per k-step where the bf16
//                  form takes six: delta1 2^e1 and X 2^ex with one pair of
//                  exponents for the launch, from bounds over all its samples
//                  (max |delta3| times the two weight norms; max |X|: the
//                  per-block maxima that l3r and l12x6 leave behind the mask,
//                  reduced in the prologue), the accumulators 2^(e1 + ex) x
//                  the sum (the bias column 2^e1 x), unscaled in the block
//                  reduction; a sample's top is its image builds and one
//                  barrier.  The X images keep their layout and use dwords 0
//                  and 1 of a position's three
//   gB2[n] += sum_p delta2[p][n]                     VALU over delta2^T (kTr:
//                  per lane over the rows, crossed over lanes in the epilogue)
// Each wave accumulates over its chunks; at the end the four waves' sums are
// added in wave order through LDS and the block writes one slab (summed by
// slab_reduce in block order).  (One slab per wave was 4x the slab traffic:
// 30 MB written and read back per step.)
// One wave per SIMD (512 registers: 128 accumulators + operands).

// kD3: the waves' launch maxima in the constant region (dword offsets).
// (gW1's accumulators cannot overflow under the launch's scales: 2^30 per
// product, < 2^20 slots per wave)
constexpr int kD6Mxx = 12, kD6Mx3 = 25;

// the all-zero delta2 row that dummy slots load (runs.hpp: slots past the
// tile), with the lane-half offset and the four 16-B quads of a real row
constexpr int kD6Zero = 32;
__device__ __attribute__((aligned(16))) float g_d6_zero[kD6Zero] = {};
// ld_d2's addressing: a row's lane-half offset (kD3: A2 rows in crow order,
// n = 4h + 8k ..; else delta2 rows, n = 8h + 16 (k >> 1) + 4 (k & 1) ..) and
// its 16-B quad k.  The zero row takes the same offsets as a real row.
constexpr int d6_row_half(bool d3, int h) { return (d3 ? 4 : 8) * h; }
constexpr int d6_zero_half(bool d3, int h) { return d6_row_half(d3, h); }
constexpr int d6_row_quad(bool d3, int k) { return d3 ? 8 * k : 16 * (k >> 1) + 4 * (k & 1); }
constexpr bool d6_zero_row_covers(bool d3) {
  for (int h = 0; h < 2; h++)
    for (int k = 0; k < 4; k++)
      if (d6_zero_half(d3, h) + d6_row_quad(d3, k) + 4 > kD6Zero) return false;
  return true;
}

// c0 += a0 . b0 and c1 += a1 . b1 (two x6 chains interleaved, so no MFMA
// waits on its predecessor's result)
__device__ __forceinline__ void mma_x6_2(const bf16x8 (&a0)[3], const bf16x8 (&b0)[3], f32x16& c0,
                                         const bf16x8 (&a1)[3], const bf16x8 (&b1)[3], f32x16& c1) {
  using mfma::mma_bf16;
  c0 = mma_bf16(a0[2], b0[0], c0);
  c1 = mma_bf16(a1[2], b1[0], c1);
  c0 = mma_bf16(a0[1], b0[1], c0);
  c1 = mma_bf16(a1[1], b1[1], c1);
  c0 = mma_bf16(a0[0], b0[2], c0);
  c1 = mma_bf16(a1[0], b1[2], c1);
  c0 = mma_bf16(a0[1], b0[0], c0);
  c1 = mma_bf16(a1[1], b1[0], c1);
  c0 = mma_bf16(a0[0], b0[1], c0);
  c1 = mma_bf16(a1[0], b1[1], c1);
  c0 = mma_bf16(a0[0], b0[0], c0);
  c1 = mma_bf16(a1[0], b1[0], c1);
}

// the split of one 8-value fragment (the scalar-subtraction form: packed
// v_pk_add_f32 costs more issue time beside MFMAs, MI355X_MICROARCH.md)
__device__ __forceinline__ void d6_split(const float (&v)[8], bf16x8 (&o)[3]) { mfma::split8(v, o); }

// kD3 (with l3r_delta_kernel<F3, true>): D2 holds delta3 (w3 x h3 per
// sample) and each item forms its delta2 rows itself,
//   delta2T[n][slot] = [A2 > 0] sum_tap W3[tap][n] delta3(slot - off(tap))
// (layer_deltas.cl:79-123 for layer 2) as one more split-bf16 GEMM: M = n2,
// N = the 32 slots, K = 2 k-steps of 16 tap slots (k-step s, lane half h,
// element j: pair slot 8s + 4h + (j >> 1) of d3taps.hpp, ceil(f3 / 2) pairs
// per tap row; zero weights on the unused elements), B = delta3 from a
// per-sample pair image (the 2 values of a pair are consecutive, each pair
// dword has its own offset), the relu' mask one dword per slot that l3r wrote
// after delta3 in the D2 region (M2: bit n = A2[pixel][n] > 0; the A2 rows
// themselves, 328 MB per 4096-tile step, were read here for that one bit per
// value).  12 MFMAs per item instead of delta2's HBM round trip (328 MB more).
//
// kTr (kD3 with D6Lds::tr): gW2's delta2 operand db holds the very parts of
// delta1's operand da, only on other lanes, so da's parts go through a
// per-wave bf16 image [slot][part][n] (d6tr.hpp: one ds_write2_b64 per part
// and k-step) and come back as db through transposed reads
// (ds_read_b64_tr_b16, two per part and k-step) instead of delta2's fp32
// transpose and a second split; gB2 sums delta2 per lane in the row layout
// and crosses lanes once, after the loop.  Without kTr the fp32 scratch form.
template <bool kD3, bool kTr = false>
__global__ __launch_bounds__(256, 1) void d1x6_grad12_kernel(const float* __restrict__ X,
                                                              const float* __restrict__ A1T,
                                                              const float* __restrict__ D2,
                                                              const float* __restrict__ A2,
                                                              const uint32_t* __restrict__ M2,
                                                              const float* __restrict__ xmaxs,
                                                              const float* __restrict__ d3maxs, D6MaxGeom mg,
                                                              const float* __restrict__ W2,
                                                              const float* __restrict__ W3,
                                                              float* __restrict__ slab, Geom g, RunGeom rg,
                                                              D3Geom dg) {
  constexpr int N1 = 64, N2 = 32, F1 = 9, K1 = F1 * F1;
  constexpr int NW1 = K1 * N1, NW2 = N1 * N2, P12 = NW1 + N1 + NW2 + N2;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  static_assert(kD3 || !kTr, "the part images belong to the delta3 form");
  const D6Lds L(g.W, g.H, rg, kD3);
  char* const base = reinterpret_cast<char*>(smem);
  __bf16* const w2i = reinterpret_cast<__bf16*>(base + L.w2);
  uint32_t* const u32 = reinterpret_cast<uint32_t*>(smem);
  uint32_t* const xbuf = u32 + L.xb / 4;
  int* const slots = reinterpret_cast<int*>(base + L.slots);
  int* const runs = reinterpret_cast<int*>(base + L.runs);

  SRCNN_CLOCK_BEGIN();
  const int lane = mfma::lane_id(), wave = mfma::wave_id();
  const int h = lane >> 5, li = lane & 31;
  const int W = g.W, xn = g.W * g.H, npx = g.ow * g.oh, nch = rg.nch;
  const int x0col = 4 * rg.a;  // first column of the column runs

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
  // kD3: the launch's maxima of |X| (one slot per l12x6 block with a sample)
  // and of |delta3| (per l3r block), two slots of each per thread, in flight
  // with the W2 / W3 loads below.  Only the written slots are read.
  float lmx = 0.0f, lm3 = 0.0f;
  if constexpr (kD3) {
    static_assert(kL12Grid <= 512 && kL3RGrid <= 512, "two slots per thread");
#pragma unroll
    for (int k = 0; k < 2; k++) {
      const int i = threadIdx.x + 256 * k;
      const float a = i < mg.n12 ? xmaxs[i] : 0.0f, b = i < mg.n3 ? d3maxs[i] : 0.0f;
      lmx = fmaxf(lmx, a);
      lm3 = fmaxf(lm3, b);
    }
  }

  // ---- per-block tables and images ----
  if constexpr (!kTr)
    for (int i = threadIdx.x; i < nch * 32; i += 256) slots[i] = slot_pixel(rg, i >> 5, i & 31);
  for (int k = threadIdx.x; k < nch * 8; k += 256) {
    int iy, ix;
    bool col;
    run_origin(rg, k < rg.nrun ? k : 0, iy, ix, col);
    // (a chunk's codes by lane half: k-step m of half h takes runs 4m + h
    // and 4m + 2 + h, the four of a half one 16-B read)
    runs[(k & ~7) + 4 * (k & 1) + 2 * ((k >> 2) & 1) + ((k >> 1) & 1)] =
        col ? ~(L.rdw + 3 * ((ix - x0col) * L.st + iy)) : 3 * (iy * L.rs + ix);
  }
  // T rows past the tile (and the pair partner of the last row), and the R
  // rows' pad columns, stay zero (16-B stores: the region ends on the 16-B
  // aligned scratch)
  for (int i = threadIdx.x; i < (2 * L.xbuf + 3) / 4; i += 256) reinterpret_cast<uint4*>(xbuf)[i] = uint4{0u, 0u, 0u, 0u};
  // gW1's third tap tile past tap 80: the ones column (gB1) and zero columns
  // read these constant pair images instead of X (dwords q and q + 6 of part q)
  // kD3 (gW1 in two fp16 parts, below): two ones images, at dwords 0 and 3
  // (sample parity; dwords q, q + 6 of part q < 2), both the fp16 pair 1.0
  // (the bias column carries delta1's scale alone); the zero image from dword
  // 16; dwords 12-15 and 25-28 hold the waves' maxima of |X| and |delta3|
  // (kD6Mxx, kD6Mx3: written before this store may land, so it leaves them out)
  if (threadIdx.x < 32 && (!kD3 || threadIdx.x < kD6Mxx || (threadIdx.x >= 16 && threadIdx.x < kD6Mx3))) {
    const bool one = threadIdx.x == 0 || threadIdx.x == 6 || (kD3 && (threadIdx.x == 3 || threadIdx.x == 9));
    u32[L.cst / 4 + threadIdx.x] = one ? (kD3 ? 0x3C003C00u : 0x3F803F80u) : 0u;
  }
  {
    // delta1's B operand W2^T: tile t, k-step k, lane (c, h), element j <->
    // W2[32 t + c][n] with n = 16 k + 8 h + j (delta2 rows as loaded), or for
    // kD3 n = crow(8 k + j, h) (delta2 as the GEMM leaves it)
    constexpr int kIt = 2 * 2 * 64 * 8 / 256;
    float v[kIt];
#pragma unroll
    for (int k = 0; k < kIt; k++) {
      const int e = threadIdx.x + 256 * k;
      const int j = e & 7, L_ = (e >> 3) & 63, kk = (e >> 9) & 1, t = e >> 10;
      const int n = kD3 ? crow(8 * kk + j, L_ >> 5) : 16 * kk + 8 * (L_ >> 5) + j;
      v[k] = W2[(32 * t + (L_ & 31)) * N2 + n];
    }
#pragma unroll
    for (int k = 0; k < kIt; k++) {
      const int e = threadIdx.x + 256 * k;
      const int j = e & 7, L_ = (e >> 3) & 63, kk = (e >> 9) & 1, t = e >> 10;
      __bf16 p[3];
      split3(v[k], p[0], p[1], p[2]);
#pragma unroll
      for (int q = 0; q < 3; q++) w2i[((t * 2 + kk) * 3 + q) * 512 + L_ * 8 + j] = p[q];
    }
  }

  uint32_t* const d3u = u32 + L.d3img / 4;  // kD3: the three delta3 buffers
  const int nout3 = dg.w3 * dg.h3;
  float d3n[2] = {0.0f, 0.0f};  // kD3: this thread's delta3 values of a later sample
  auto d3load = [&](int smp) {
#pragma unroll
    for (int k = 0; k < 2; k++) {
      const int t = threadIdx.x + 256 * k;
      d3n[k] = t < nout3 ? D2[(size_t)smp * nout3 + t] : 0.0f;
    }
  };
  // delta3 (y3, x3) -> image (y3 + 5, x3 + 7): pair dwords x3 + 7 (low half)
  // and x3 + 6 (high half) of each part row
  auto d3build = [&](int buf) {
    uint16_t* const b16 = reinterpret_cast<uint16_t*>(d3u + buf * L.d3buf);
#pragma unroll
    for (int k = 0; k < 2; k++) {
      const int t = threadIdx.x + 256 * k;
      if (t < nout3) {
        const int y = t / dg.w3, x = t - y * dg.w3, d = (y + 5) * L.gs + x + 7;
        __bf16 p[3];
        split3(d3n[k], p[0], p[1], p[2]);
#pragma unroll
        for (int q = 0; q < 3; q++) {
          const uint16_t b = __builtin_bit_cast(uint16_t, p[q]);
          b16[2 * (d + L.gw * q)] = b;
          b16[2 * (d + L.gw * q) - 1] = b;
        }
      }
    }
  };
  // kD3: gW1 / gB1 in two fp16 parts per operand (split.hpp: three MFMAs per
  // k-step where the bf16 form takes six).  delta1 is scaled by 2^e1 from the
  // bound |delta1| <= max |delta3| . max_n sum_tap |W3[tap][n]| . max_c sum_n
  // |W2[c][n]| and X by 2^ex from max |X|, both maxima over the whole launch
  // (l3r's and l12x6's per-block maxima, reduced here through the constant
  // region behind the prologue's barrier): gW1 and gB1 are sums over the
  // launch, a power of two leaves an operand's parts as they are while none is
  // subnormal, and a sample more than 2^17 below the largest loses low bits
  // at 2^-39 of the largest one's terms.  The accumulators hold 2^EW x the sum
  // (EW = e1 + ex; the bias column 2^EB x, EB = e1), unscaled in the block
  // reduction.
  float* const mxx = smem + L.cst / 4 + kD6Mxx;
  float* const mx3 = smem + L.cst / 4 + kD6Mx3;
  auto wave_max = [&](float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
  };
  auto put_max = [&](float* slot, float v) {
    v = wave_max(v);
    if (lane == 0) slot[wave] = v;
  };
  // (the same four values in the same order on every thread; scalar)
  auto take_max_reg = [&](float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
  };
  auto take_max = [&](const float* slot) {
    const float v = fmaxf(fmaxf(slot[0], slot[1]), fmaxf(slot[2], slot[3]));
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
  };
  float wnorm = 0.0f;  // the two norms' product
  int EW = 0, EB = 0;
  float s1 = 1.0f, sX = 1.0f;  // kD3: 2^e1 for delta1, 2^ex for X
  if constexpr (kD3) {
    {
      // (every wave forms both norms itself: lane = W2's channel, lane & 31 = W3's)
      float n2 = 0.0f, n3 = 0.0f;
      for (int n = 0; n < N2; n++) n2 += fabsf(W2[lane * N2 + n]);
      for (int t = 0; t < dg.f3 * dg.f3; t++) n3 += fabsf(W3[t * N2 + li]);
      wnorm = take_max_reg(wave_max(n2)) * take_max_reg(wave_max(n3));
    }
    // delta2's A operand W3^T: k-step s, part q, lane (n, h), element j <->
    // W3[tap of pair slot 8 s + 4 h + (j >> 1), element j & 1][n], zero on
    // the unused elements (d3taps.hpp)
    // (all four loads in flight at once: one per loop trip, each waited
    // for, they were 6% of a 512-tile launch)
    __bf16* const w3i = reinterpret_cast<__bf16*>(base + L.w3i);
    constexpr int kW3It = 2 * 64 * 8 / 256;
    static_assert(kW3It * 256 * 3 == kD6W3, "the W3 image: 2 k-steps x 3 parts");
    float w3v[kW3It];
#pragma unroll
    for (int k = 0; k < kW3It; k++) {
      const int e = threadIdx.x + 256 * k;
      const int j = e & 7, L_ = (e >> 3) & 63, s_ = e >> 9;
      const D3Pair tp = d3_pair_slot(8 * s_ + 4 * (L_ >> 5) + (j >> 1), dg.f3);
      const int dx = d3_pair_dx(tp, j & 1, dg.f3), n = L_ & 31;
      const bool in = dx >= 0;
      w3v[k] = W3[in ? (tp.dy * dg.f3 + dx) * N2 + n : 0];
      if (!in) w3v[k] = 0.0f;
    }
#pragma unroll
    for (int k = 0; k < kW3It; k++) {
      const int e = threadIdx.x + 256 * k;
      const int j = e & 7, L_ = (e >> 3) & 63, s_ = e >> 9;
      __bf16 p[3];
      split3(w3v[k], p[0], p[1], p[2]);
#pragma unroll
      for (int q = 0; q < 3; q++) w3i[((s_ * 3 + q) * 64 + L_) * 8 + j] = p[q];
    }
    // slot -> its delta3 image offset py gs + px (dummy slots: pixel (0, 0))
    // (kTr: in one dword with the slot's pixel, d6_slot_pack)
    int* const d3tab = reinterpret_cast<int*>(base + L.d3tab);
    for (int i = threadIdx.x; i < nch * 32; i += 256) {
      int iy, ix;
      slot_coord(rg, i >> 5, i & 31, iy, ix);
      d3tab[i] = kTr ? d6_slot_pack(slot_pixel(rg, i >> 5, i & 31), iy * L.gs + ix) : iy * L.gs + ix;
    }
    for (int i = threadIdx.x; i < (3 * L.d3buf + 3) / 4; i += 256)  // borders stay zero
      reinterpret_cast<uint4*>(d3u)[i] = uint4{0u, 0u, 0u, 0u};
    if ((int)blockIdx.x < g.batch) d3load(blockIdx.x);
    put_max(mxx, lmx);
    put_max(mx3, lm3);
    __syncthreads();  // zeroed before the first build
    {
      // the launch's scales (the same scalars on every thread)
      const float xmax = take_max(mxx), bound = take_max(mx3) * wnorm;
      // (a zero bound: delta1 = 0 throughout, any finite scale does; zero X alike)
      const int e1 = bound > 0.0f ? mfma::scale_exp_h(bound) : 0, ex = xmax > 0.0f ? mfma::scale_exp_h(xmax) : 0;
      EW = e1 + ex;
      EB = e1;
      s1 = mfma::pow2_h(e1);
      sX = mfma::pow2_h(ex);
    }
    d3build(0);       // sample 0 (buffer j % 3 holds sample j)
    if ((int)blockIdx.x + (int)gridDim.x < g.batch) d3load(blockIdx.x + gridDim.x);
  }

  // gW1 operand offsets of this lane's tap 32u + li (3 dwords per pair
  // position); tile 2's lanes past tap 80 read the constant images
  // (byte offsets, as the run bases of an item are: an address is one select
  // and one addition)
  int offR3[3], offT3[3];
#pragma unroll
  for (int u = 0; u < 3; u++) {
    const int tap = 32 * u + li;
    const int dy = tap < K1 ? tap / F1 : 0, dx = tap < K1 ? tap - dy * F1 : 0;
    offR3[u] = 12 * (dy * L.rs + dx);
    offT3[u] = 12 * (dx * L.st + dy);
  }
  // (these addresses are LDS addresses, the region's own included, so that
  // nothing is left to add after the per-part addresses below)
  typedef __attribute__((address_space(3))) const uint32_t lds_u32;
  const int lds0 = (int)(uintptr_t)(__attribute__((address_space(3))) char*)base;
  const int spec = li == K1 - 64 ? lds0 + L.cst : li > K1 - 64 ? lds0 + L.cst + 64 : -1;

  f32x16 g1[2][3], g2[2];
#pragma unroll
  for (int t = 0; t < 2; t++) {
    g2[t] = zero16();
#pragma unroll
    for (int u = 0; u < 3; u++) g1[t][u] = zero16();
  }
  float gb2 = 0.0f;
  // kTr: delta2's running sums in the row layout (register r <-> channel
  // crow(r, h), this lane's slot over the wave's items)
  float gbr[16];
#pragma unroll
  for (int r = 0; r < 16; r++) gbr[r] = 0.0f;

  float* const sc = smem + L.sc / 4 + wave * kD6Sc;
  // kTr: this wave's part image in the sc region: the lane's write address of
  // either k-step and its transposed-read address (d6tr.hpp)
  char* const trw = base + L.sc + d6tr_wave_off(wave);
  char* const trw0 = trw + d6tr_write_off(li, h, 0, 0, 0);
  char* const trw1 = trw + d6tr_write_off(li, h, 1, 0, 0);
  const char* const trr = trw + d6tr_read_off(lane, 0, 0, 0);
  const uint16_t* const wl2 = reinterpret_cast<const uint16_t*>(w2i) + lane * 8;

  // The block's chunks form one stream (sample j of the block = blockIdx.x +
  // j * gridDim.x, chunks 0 .. nch-1 each); wave w takes stream items w,
  // w + 4, ...  Items past the batch load a valid sample and are never run.
  const float inv_nch = 1.0f / (float)nch;
  auto item = [&](int i, int& j, int& c) {
    j = run_div(i, inv_nch);
    c = i - j * nch;
  };
  auto item_sample = [&](int j) {
    const int smp = (int)blockIdx.x + j * (int)gridDim.x;
    return smp < g.batch ? smp : (int)blockIdx.x;
  };
  // operand registers from HBM: delta2 rows of this lane's slot (n = 8h ..
  // 8h+7 and 16 + 8h ..), A1^T runs of this lane's channel.  kD3: instead of
  // the rows, the slot's layer-2 relu' mask (l3r's M2: bit n = A2[pixel][n] >
  // 0; 0 for a dummy slot), shifted by 4h so that bit 8 (r >> 2) + (r & 3) is
  // channel crow(r, h), register r of the delta2 GEMM's result
  f32x4 d2r[4], a1r[2][4];
  uint32_t d2m = 0, d2raw = 0;
  int d2pix = 0;
  // (sv: kTr, the slot's table dword, read by the caller for its delta3 offset too)
  auto ld_d2 = [&](int j, int c, int sv) {
    const int pix = kTr ? d6_slot_pix(sv) : slots[c * 32 + li];
    if constexpr (kD3) {
      // (only the load here; the select and shift wait for it at the use)
      d2pix = pix;
      d2raw = M2[(size_t)item_sample(j) * npx + (pix >= 0 ? pix : 0)];
    } else {
      // every 16-B load of a dummy slot lies inside the zero row
      static_assert(d6_zero_row_covers(false), "dummy-slot loads past g_d6_zero");
      const float* d2 = pix >= 0 ? D2 + ((size_t)item_sample(j) * npx + pix) * N2 + d6_row_half(false, h)
                                 : g_d6_zero + d6_zero_half(false, h);
#pragma unroll
      for (int k = 0; k < 4; k++) d2r[k] = *reinterpret_cast<const f32x4*>(d2 + d6_row_quad(false, k));
    }
  };
  // kD3: register r of the delta2 GEMM's result under the mask (a sign-extended
  // bit field and an AND: the two VALU ops of a compare and select)
  auto mask_take = [&]() __attribute__((always_inline)) { d2m = (d2pix >= 0 ? d2raw : 0u) >> (4 * h); };
  auto mask_d2 = [&](int r, float v) __attribute__((always_inline)) {
    // (the instruction itself: from shifts or the sbfe builtin the compiler
    // made and + compare + select; r is a constant once the loops are unrolled)
    int keep;
    asm("v_bfe_i32 %0, %1, %2, 1" : "=v"(keep) : "v"(d2m), "i"(8 * (r >> 2) + (r & 3)));
    return __builtin_bit_cast(float, __builtin_bit_cast(int, v) & keep);
  };
  auto ld_a1 = [&](int j, int c, int k0 = 0, int k1 = 8) __attribute__((always_inline)) {
    const float* a1 = A1T + ((size_t)item_sample(j) * nch + c) * (64 * 32) + li * 32 + 4 * h;
#pragma unroll
    for (int k = k0; k < k1; k++) a1r[k >> 2][k & 3] = *reinterpret_cast<const f32x4*>(a1 + (k >> 2) * 32 * 32 + 8 * (k & 3));
  };
  // delta2 split for delta1 (row layout, da) and, through the per-wave
  // transpose scratch, for gW2 (db); gbs = the item's delta2 sum for gB2
  bf16x8 da[2][3], db[2][3];
  float gbs;
  // the item's delta2 row values, register r <-> n = 16 (r >> 3) + 8 h + (r & 7)
  // (rows as loaded) or crow(r, h) (kD3)
  f32x16 d2v;
  auto stage_d2 = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < 4; k++) {
      f32x4 v;
#pragma unroll
      for (int i = 0; i < 4; i++) v[i] = d2v[4 * k + i];
      *reinterpret_cast<f32x4*>(sc + li * 36 + (kD3 ? 8 * k + 4 * h : 16 * (k >> 1) + 8 * h + 4 * (k & 1))) = v;
    }
    __builtin_amdgcn_wave_barrier();
  };
  auto take_rows = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int r = 0; r < 16; r++) d2v[r] = d2r[r >> 2][r & 3];
  };
  // kD3: delta2 of item (j, c) as split-bf16 GEMM operands -- delta3 window
  // parts (B) of k-step s from buffer j % 3, W3 parts (A) -- and the GEMM
  const __bf16* const w3l = reinterpret_cast<const __bf16*>(base + L.w3i) + lane * 8;
  const int* const d3tab_ = reinterpret_cast<const int*>(base + L.d3tab);
  // the image offsets of this lane half's pair dwords of k-step s (row 5 -
  // dy, column col of pair slot 8 s + 4 h + e, d3taps.hpp): d3a for pairs e =
  // 0 .. 2 (one row, columns 2 apart), d3b for pair 3.  They depend on the
  // lane half alone, so they are formed once.  Unused pairs (zero weights)
  // read inside the image as well
  int d3a[2] = {}, d3b[2] = {};
  if constexpr (kD3) {
#pragma unroll
    for (int s_ = 0; s_ < 2; s_++) {
      const D3Pair ta = d3_pair_slot(8 * s_ + 4 * h, dg.f3), tb = d3_pair_slot(8 * s_ + 4 * h + 3, dg.f3);
      d3a[s_] = (5 - ta.dy) * L.gs + ta.col;
      d3b[s_] = (5 - tb.dy) * L.gs + tb.col;
    }
  }
  // (t = the item's d3tab entry, read once per item: read here, each k-step's
  // reads waited for it)
  auto d3read = [&](int j, int t, int s_, bf16x8 (&a)[3], bf16x8 (&b)[3]) __attribute__((always_inline)) {
    const int buf = j - 3 * (j / 3);
    const int o = L.d3img / 4 + buf * L.d3buf + t;
    const int oa = o + d3a[s_], ob = o + d3b[s_];
#pragma unroll
    for (int q = 0; q < 3; q++) {
      u32x4 d;
      d[0] = u32[oa + L.gw * q];
      d[1] = u32[oa + L.gw * q + 2];
      d[2] = u32[oa + L.gw * q + 4];
      d[3] = u32[ob + L.gw * q];
      b[q] = __builtin_bit_cast(bf16x8, d);
      a[q] = *reinterpret_cast<const bf16x8*>(w3l + (s_ * 3 + q) * 512);
    }
  };
  // kTr: da[k]'s parts into the wave's image, then db[m] out of it
  auto tr_write = [&](int k) __attribute__((always_inline)) {
    char* const p = k ? trw1 : trw0;
#pragma unroll
    for (int q = 0; q < 3; q++) {
      const u32x4 d = __builtin_bit_cast(u32x4, da[k][q]);
      *reinterpret_cast<uint2*>(p + q * kD6TrPartRow) = uint2{d[0], d[1]};
      *reinterpret_cast<uint2*>(p + q * kD6TrPartRow + 16) = uint2{d[2], d[3]};
    }
  };
  auto tr_read = [&](int m) __attribute__((always_inline)) {
    typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
#pragma unroll
    for (int q = 0; q < 3; q++) {
      const char* const p = trr + 16 * m * kD6TrRow + q * kD6TrPartRow;
      const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(p));
      const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(p + 8 * kD6TrRow));
      db[m][q] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    }
  };
  // (f = 1 for an item that will run, 0 for the one past the block's last:
  // its delta2 is formed like any other, from a stale delta3 image; x * 1 + s
  // rounds once, as the addition)
  auto sum_d2 = [&](float f) __attribute__((always_inline)) {
#pragma unroll
    for (int r = 0; r < 16; r++) gbr[r] = __builtin_fmaf(d2v[r], f, gbr[r]);
  };
  // in pieces, so phase C can spread them over its MFMA groups: 0 the
  // transposed reads, 1-2 da, 3-4 db (+ gbs)
  float d2t[16];
  auto split_d2 = [&](int piece) __attribute__((always_inline)) {
    if (piece == 0) {
#pragma unroll
      for (int r = 0; r < 16; r++) d2t[r] = sc[crow(r, h) * 36 + li];
    } else if (piece <= 2) {
      const int k = piece - 1;
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; j++) v[j] = d2v[8 * k + j];
      d6_split(v, da[k]);
    } else {
      const int m = piece - 3;
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; j++) v[j] = d2t[8 * m + j];
      d6_split(v, db[m]);
      if (m == 1) {
        float s0 = 0.0f, s1 = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
          s0 += d2t[r];
          s1 += d2t[r + 1];
        }
        gbs = s0 + s1;
      }
    }
  };

  // kD3: the delta2 GEMM of an item (the operands of k-step 0 read ahead
  // into ga / gb), masked by its relu' bits in d2m
  auto d2gemm = [&](int j, int t, bf16x8 (&ga)[3], bf16x8 (&gb)[3]) __attribute__((always_inline)) {
    f32x16 acc[2] = {zero16(), zero16()};
    bf16x8 a1_[3], b1_[3];
    d3read(j, t, 1, a1_, b1_);
    mma_x6_2(ga, gb, acc[0], a1_, b1_, acc[1]);
    mask_take();
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const float v = acc[0][r] + acc[1][r];
      d2v[r] = mask_d2(r, v);
    }
  };

  // delta1's k-step-0 B operands (W2 parts of both tiles), read under the
  // previous item's last gW1 step: read at the top of phase A, each of its
  // first six MFMAs waited out one ds_read_b128
  bf16x8 w2k0[2][3];
  auto w2read0 = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int q = 0; q < 3; q++) {
      w2k0[0][q] = *reinterpret_cast<const bf16x8*>(wl2 + ((0 * 2 + 0) * 3 + q) * 512);
      w2k0[1][q] = *reinterpret_cast<const bf16x8*>(wl2 + ((1 * 2 + 0) * 3 + q) * 512);
    }
  };

  int ki = wave, kj, kc;  // this wave's current item: stream index, sample, chunk
  item(ki, kj, kc);
  __syncthreads();  // tables (kD3: and the first delta3 image)
  w2read0();
  {
    const int sv = kD3 ? d3tab_[kc * 32 + li] : 0;
    ld_d2(kj, kc, sv);
    ld_a1(kj, kc);
    if constexpr (kD3) {
      bf16x8 ga[3], gb[3];
      const int t = kTr ? d6_slot_off(sv) : sv;
      d3read(kj, t, 0, ga, gb);
      d2gemm(kj, t, ga, gb);
    } else {
      take_rows();
    }
  }
  if constexpr (kTr) {
    sum_d2(1.0f);
#pragma unroll
    for (int k = 0; k < 2; k++) {
      split_d2(1 + k);
      tr_write(k);
    }
    __builtin_amdgcn_wave_barrier();
    tr_read(0);
    tr_read(1);
  } else {
    stage_d2();
#pragma unroll
    for (int piece = 0; piece < 5; piece++) split_d2(piece);
  }

  // Each item runs as three phases whose MFMAs carry the VALU work of the
  // next phase or item (one wave per SIMD: nothing else covers it):
  //   A  delta1 = delta2 . W2^T (24 MFMAs)      | A1 split for gW2; next delta2 loads
  //   B  gW2 += A1^T . delta2 (24)              | relu'(A1) mask, delta1 split; next A1 loads
  //   C  gW1^T += delta1^T . Xwin (72)          | next item's delta2 splits (da, db)
  for (int it = 0; (int)blockIdx.x + it * (int)gridDim.x < g.batch; it++) {
    const int smp = blockIdx.x + it * gridDim.x;
    uint32_t* const xi = xbuf + (it & 1) * L.xbuf;
    // kD3: sample it + 1's delta3 image into buffer (it + 1) % 3, last read for
    // sample it - 2 (every wave is past that sample: the barrier at the top of
    // sample it - 1); read from the first delta2 of sample it + 1 on, after
    // the barrier below
    if constexpr (kD3) {
      if (smp + (int)gridDim.x < g.batch) d3build((it + 1) - 3 * ((it + 1) / 3));
    }
    // ---- this sample's X pair images (buffer it & 1) ----
    if constexpr (kD3) {
      // (two fp16 parts of X 2^ex in dwords 0 and 1 of a position's three;
      // buffer it & 1 was last read for sample it - 2, as the delta3 buffer)
      uint16_t* const x16 = reinterpret_cast<uint16_t*>(xi);
#pragma unroll
      for (int k = 0; k < kL12Regs; k++) {
        const int i = threadIdx.x + 256 * k;
        if (i < xn) {
          const float xs = xr[k] * sX;
          const _Float16 p0 = (_Float16)xs;
          const _Float16 p[2] = {p0, (_Float16)(xs - (float)p0)};
          const int y = i / W, x = i - y * W, ri = y * L.rs + x;
          const int ti = L.rdw + 3 * ((x - x0col) * L.st + y);
#pragma unroll
          for (int q = 0; q < 2; q++) {
            const uint16_t b = __builtin_bit_cast(uint16_t, p[q]);
            x16[2 * (3 * ri + q)] = b;
            if (ri > 0) x16[2 * (3 * (ri - 1) + q) + 1] = b;
            if (L.tcols && x >= x0col) {
              x16[2 * (ti + q)] = b;
              if (y > 0) x16[2 * (ti - 3 + q) + 1] = b;
            }
          }
        }
      }
    } else {
      uint16_t* const x16 = reinterpret_cast<uint16_t*>(xi);
#pragma unroll
      for (int k = 0; k < kL12Regs; k++) {
        const int i = threadIdx.x + 256 * k;
        if (i < xn) {
          __bf16 p[3];
          split3(xr[k], p[0], p[1], p[2]);
          const int y = i / W, x = i - y * W, ri = y * L.rs + x;
          const int ti = L.rdw + 3 * ((x - x0col) * L.st + y);
#pragma unroll
          for (int q = 0; q < 3; q++) {
            const uint16_t b = __builtin_bit_cast(uint16_t, p[q]);
            x16[2 * (3 * ri + q)] = b;
            if (ri > 0) x16[2 * (3 * (ri - 1) + q) + 1] = b;
            if (L.tcols && x >= x0col) {
              x16[2 * (ti + q)] = b;
              if (y > 0) x16[2 * (ti - 3 + q) + 1] = b;
            }
          }
        }
      }
    }
    // images (and at it == 0 the tables) complete; every wave is past sample
    // it - 1: X buffer (it+1)&1 and delta3 buffer (it+2)%3 are free
    __syncthreads();
    const int nsmp = smp + (int)gridDim.x;
    if (nsmp < g.batch) xload(nsmp);
    if constexpr (kD3) {
      if (nsmp + (int)gridDim.x < g.batch) d3load(nsmp + gridDim.x);
    }
    const int xo = L.xb / 4 + (it & 1) * L.xbuf;  // this sample's X images (dwords into smem)

    while (kj == it) {
      const int c = kc;
      int nj, nc;  // the next item
      item(ki + 4, nj, nc);

      // ---------------- phase A ----------------
      // (the next item's loads go out in VMEM slots of the MFMA patterns:
      // left alone, the scheduler sank them to just before their first use;
      // issued between the phases they cost ~10% of an item)
      if constexpr (!kTr) gb2 += gbs;
      if constexpr (!kD3) ld_d2(nj, nc, 0);
      // run codes of this lane's half (k-step m takes runs 4m + h, 4m + 2 +
      // h) as the runs' base byte addresses in this sample's X images and
      // their orientation, once per item: the R / T choice and the ~code were
      // redone for each of gW1's six steps
      const u32x4 rc4 = *reinterpret_cast<const u32x4*>(runs + 8 * c + 4 * h);
      int xrb[2][2];
      bool xrt[2][2];
#pragma unroll
      for (int m = 0; m < 2; m++)
#pragma unroll
        for (int e = 0; e < 2; e++) {
          const int code = (int)rc4[2 * m + e];
          xrt[m][e] = code < 0;
          xrb[m][e] = lds0 + 4 * (xo + (code < 0 ? ~code : code));
        }
      const int d3s = kD3 ? d3tab_[nc * 32 + li] : 0;  // the next item's
      const int d3t = kTr ? d6_slot_off(d3s) : d3s;
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (kD3) ld_d2(nj, nc, d3s);
      f32x16 d1[2] = {zero16(), zero16()};
      {
        bf16x8 b0[3], b1[3];
#pragma unroll
        for (int q = 0; q < 3; q++) {
          b0[q] = *reinterpret_cast<const bf16x8*>(wl2 + ((0 * 2 + 1) * 3 + q) * 512);
          b1[q] = *reinterpret_cast<const bf16x8*>(wl2 + ((1 * 2 + 1) * 3 + q) * 512);
        }
        mma_x6_2(da[0], w2k0[0], d1[0], da[0], w2k0[1], d1[1]);
        mma_x6_2(da[1], b0, d1[0], da[1], b1, d1[1]);
      }
      bf16x8 aa[2][2][3];  // A1^T parts [t][m]
#pragma unroll
      for (int t = 0; t < 2; t++)
#pragma unroll
        for (int m = 0; m < 2; m++) {
          float v[8];
#pragma unroll
          for (int j = 0; j < 8; j++) v[j] = a1r[t][2 * m + (j >> 2)][j & 3];
          d6_split(v, aa[t][m]);
        }
#pragma unroll
      for (int i = 0; i < 24; i++) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // MFMA
        __builtin_amdgcn_sched_group_barrier(0x002, 7, 0);  // VALU
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);  // DS read
        if (kD3 && i == 1) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);  // VMEM read (the mask dword)
      }

      // ---------------- phase B ----------------
#pragma unroll
      for (int m = 0; m < 2; m++) mma_x6_2(aa[0][m], db[m], g2[0], aa[1][m], db[m], g2[1]);
      // relu' of layer 1 (register r of d1[t] and a1r[t] is the same slot)
#pragma unroll
      for (int t = 0; t < 2; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) d1[t][r] = a1r[t][r >> 2][r & 3] > 0.0f ? d1[t][r] : 0.0f;
      bf16x8 dx[2][2][3];  // delta1 parts [m][t]: m = 0 here, m = 1 under gW1's first half
      mfma::f16x8 dxh[2][2][2];  // kD3: the two fp16 parts of delta1 2^e1
      auto split_d1 = [&](int m, int t) __attribute__((always_inline)) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; j++) v[j] = kD3 ? d1[t][8 * m + j] * s1 : d1[t][8 * m + j];  // (kD3: 2^e1, exact)
        if constexpr (kD3)
          mfma::split8_h(v, dxh[m][t]);
        else
          d6_split(v, dx[m][t]);
      };
      split_d1(0, 0);
      split_d1(0, 1);
      // kD3: the next item's delta2 GEMM, k-step 0 operands, read under gW2
      // (at the phase boundary the first GEMM MFMA waited out their latency)
      bf16x8 ga[3], gb[3];
      if constexpr (kD3) d3read(nj, d3t, 0, ga, gb);
#pragma unroll
      for (int i = 0; i < 24; i++) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 7, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (!kD3) ld_a1(nj, nc);  // (a1r consumed: A1 split in phase A, the mask above)
      if constexpr (!kD3) {
        take_rows();
        stage_d2();  // the next item's delta2 (loaded in phase A) into the transpose scratch
      }
      __builtin_amdgcn_sched_barrier(0);

      // ---------------- phase C ----------------
      // six steps (m, u) of 12 MFMAs; step s reads the X operands of step
      // s + 1 and carries one piece of VALU work: the m = 1 delta1 split
      // (steps 0-1; needed from step 3), then the next item's delta2 splits
      // (transposed reads in step 1, the splits in steps 2-5).
      // sched_barriers between the steps keep each piece under its MFMAs
      auto xread = [&](int m, int u, bf16x8 (&b)[3]) __attribute__((always_inline)) {
        u32x4 d[3];
#pragma unroll
        for (int e = 0; e < 2; e++) {
          int a = xrb[m][e] + (xrt[m][e] ? offT3[u] : offR3[u]);
          if (u == 2) a = spec >= 0 ? spec : a;
          // (a part's two dwords are one ds_read2_b32 into its operand's
          // register pair only with an address of the part's own: from one
          // address the six were paired by offset, across the parts, and each
          // operand then took two moves to assemble, 36 per item)
          int aq[3] = {a, a + 4, a + 8};
          asm("" : "+v"(aq[1]), "+v"(aq[2]));
#pragma unroll
          for (int q = 0; q < 3; q++) {
            d[q][2 * e] = *(lds_u32*)(uintptr_t)(unsigned)aq[q];
            d[q][2 * e + 1] = *(lds_u32*)(uintptr_t)(unsigned)(aq[q] + 24);
          }
        }
#pragma unroll
        for (int q = 0; q < 3; q++) b[q] = __builtin_bit_cast(bf16x8, d[q]);
      };
      // kD3: the two fp16 parts of X 2^ex (dwords 0 and 1 of a position's three)
      const int spech = kD3 && li == K1 - 64 ? spec + 12 * (it & 1) : spec;
      auto xread_h = [&](int m, int u, mfma::f16x8 (&b)[2]) __attribute__((always_inline)) {
        u32x4 d[2];
#pragma unroll
        for (int e = 0; e < 2; e++) {
          int a = xrb[m][e] + (xrt[m][e] ? offT3[u] : offR3[u]);
          if (u == 2) a = spech >= 0 ? spech : a;
          int aq[2] = {a, a + 4};
          asm("" : "+v"(aq[1]));
#pragma unroll
          for (int q = 0; q < 2; q++) {
            d[q][2 * e] = *(lds_u32*)(uintptr_t)(unsigned)aq[q];
            d[q][2 * e + 1] = *(lds_u32*)(uintptr_t)(unsigned)(aq[q] + 24);
          }
        }
#pragma unroll
        for (int q = 0; q < 2; q++) b[q] = __builtin_bit_cast(mfma::f16x8, d[q]);
      };
      bf16x8 bx[2][3];
      mfma::f16x8 bxh[2][2];
      if constexpr (kD3)
        xread_h(0, 0, bxh[0]);
      else
        xread(0, 0, bx[0]);
      f32x16 gacc[2];  // kD3: the next item's delta2 GEMM, two chains
      if constexpr (kD3) {
        // the next item's delta2 GEMM (12 MFMAs) as two fenced groups of 6,
        // one per k-step and accumulator chain: the first reads the second
        // k-step's operands, each carries half of the m = 1 delta1 split and
        // half of the next item's A1 loads; the sum and mask go under gW1's
        // first step
        gacc[0] = zero16();
        gacc[1] = zero16();
#pragma unroll
        for (int s_ = 0; s_ < 2; s_++) {
          bf16x8 na[3], nb[3];
          if (s_ < 1) d3read(nj, d3t, s_ + 1, na, nb);
          ld_a1(nj, nc, 4 * s_, 4 * s_ + 4);  // (a1r consumed: phase A's split, B's mask)
          gacc[s_] = mma_x6(ga, gb, gacc[s_]);
          split_d1(1, s_);
          // (the reads first: placed one per MFMA, the last ones trailed the
          // group and the next group's first MFMA waited for all of them)
          if (s_ < 1) __builtin_amdgcn_sched_group_barrier(0x100, 9, 0);
#pragma unroll
          for (int i = 0; i < 6; i++) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, 7, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            if (i < 4) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
          }
          __builtin_amdgcn_sched_barrier(0);
          if (s_ < 1) {
#pragma unroll
            for (int q = 0; q < 3; q++) {
              ga[q] = na[q];
              gb[q] = nb[q];
            }
          }
        }
      }
#pragma unroll
      for (int st = 0; st < 6; st++) {
        const int m = st / 3, u = st % 3;
        if (st == 5)
          w2read0();  // the next item's phase A
        else if constexpr (kD3)
          xread_h((st + 1) / 3, (st + 1) % 3, bxh[(st + 1) & 1]);
        else
          xread((st + 1) / 3, (st + 1) % 3, bx[(st + 1) & 1]);
        if constexpr (kD3)
          mfma::mma_x3_h_2(dxh[m][0], bxh[st & 1], g1[0][u], dxh[m][1], bxh[st & 1], g1[1][u]);
        else
          mma_x6_2(dx[m][0], bx[st & 1], g1[0][u], dx[m][1], bx[st & 1], g1[1][u]);
        if (kTr) {
          // step 0: the delta2 sum and relu' mask, 1-2: da and its parts into
          // the image, 3: gB2's sums and the transposed reads of db
          if (st == 0) {
            mask_take();
#pragma unroll
            for (int r = 0; r < 16; r++) {
              const float v = gacc[0][r] + gacc[1][r];
              d2v[r] = mask_d2(r, v);
            }
          }
          if (st == 1 || st == 2) {
            split_d2(st);
            tr_write(st - 1);
          }
          if (st == 3) {
            sum_d2((int)blockIdx.x + nj * (int)gridDim.x < g.batch ? 1.0f : 0.0f);
            __builtin_amdgcn_wave_barrier();
            tr_read(0);
            tr_read(1);
          }
        } else if (kD3) {
          // step 0: the delta2 sum, relu' mask and rows into the transpose
          // scratch, 1: the transposed reads and da, 2: da, 3-4: db (+ gbs)
          if (st == 0) {
            mask_take();
#pragma unroll
            for (int r = 0; r < 16; r++) {
              const float v = gacc[0][r] + gacc[1][r];
              d2v[r] = mask_d2(r, v);
            }
            stage_d2();
          }
          if (st == 1) split_d2(0);
          if (st >= 1 && st <= 4) split_d2(st);
        } else if (st < 2) {
          split_d1(1, st);
          if (st == 1) split_d2(0);
        } else {
          split_d2(st - 1);  // 1-2 da, 3-4 db (+ gbs)
        }
#pragma unroll
        // (kD3: the same VALU and LDS work under half the MFMAs)
        for (int i = 0; i < (kD3 ? 6 : 12); i++) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x002, kD3 ? 12 : 6, 0);
          __builtin_amdgcn_sched_group_barrier(0x100, kD3 ? 2 : 1, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      ki += 4;
      kj = nj;
      kc = nc;
    }
  }
  SRCNN_CLOCK_END(g_clk, 2);

  // ---- block reduction and slab, in two rounds of four 16-register tiles:
  // every wave parks its four tiles in LDS, then wave w adds tile 4k + w of
  // the four waves in wave order (fixed, deterministic: the same sums as
  // waves 1-3 handing each tile to wave 0) and writes it to the block's slab
  // [gW1 | gB1 | gW2 | gB2].  (Wave 0 alone, one tile per barrier pair, took
  // 16 barriers and wrote the whole slab.) ----
  __syncthreads();  // every wave is done with the LDS images
  float* const red = smem;  // [4 tiles][4 waves][16 registers][64 lanes] (64 KB)
  float* out = slab + (size_t)blockIdx.x * P12;
  // the block's slab is assembled in LDS after the scratch and leaves as
  // coalesced 16-B stores (each wave storing its tiles straight from the
  // accumulator layout wrote 64 scattered dwords per store instruction: 8% of
  // a 512-tile launch); rows 0-81 (gW1 taps | gB1) with their 16-B quads
  // XOR-swizzled by the row, so a half-wave's 32 taps of one channel hit 16
  // banks
  float* const stg = smem + 4 * 4 * 16 * 64;
  auto stg_w1 = [&](int row, int ch) -> float& { return stg[row * N1 + (ch ^ ((row & 15) << 2))]; };
  // tiles 0-5: g1[t][u] (t = tile / 3, u = tile % 3), 6-7: g2[t]
  auto tile_ref = [&](int k) -> f32x16& { return k < 6 ? g1[k / 3][k % 3] : g2[k - 6]; };
#pragma unroll
  for (int rd = 0; rd < 2; rd++) {
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const f32x16& a = tile_ref(4 * rd + k);
#pragma unroll
      for (int r = 0; r < 16; r++) red[((k * 4 + wave) * 16 + r) * 64 + lane] = a[r];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; k++) {
      if (wave != k) continue;  // (wave-uniform)
      const int tile = 4 * rd + k;
      f32x16 sum;
#pragma unroll
      for (int r = 0; r < 16; r++) {
        float v = red[((k * 4 + 0) * 16 + r) * 64 + lane];
#pragma unroll
        for (int w = 1; w < 4; w++) v += red[((k * 4 + w) * 16 + r) * 64 + lane];
        sum[r] = v;
      }
      if (tile < 6) {
        const int t = tile / 3, u = tile % 3, tap = 32 * u + li;
        if constexpr (kD3) {
          // the sums leave their scale 2^EW (the bias column 2^EB), in three
          // exact steps (|EW| <= 378); every wave holds the same exponents
          int e = -(tap == K1 ? EB : EW);
#pragma unroll
          for (int k = 0; k < 3; k++) {
            const int a = e < -126 ? -126 : e > 126 ? 126 : e;
            const float f = mfma::pow2_h(a);
#pragma unroll
            for (int r = 0; r < 16; r++) sum[r] *= f;
            e -= a;
          }
        }
#pragma unroll
        for (int r = 0; r < 16; r++)
          if (tap <= K1) stg_w1(tap, 32 * t + crow(r, h)) = sum[r];  // (tap K1: gB1, row 81 at NW1)
      } else {
        const int t = tile - 6;
#pragma unroll
        for (int r = 0; r < 16; r++) stg[NW1 + N1 + (32 * t + crow(r, h)) * N2 + li] = sum[r];
      }
    }
    __syncthreads();
  }
  if constexpr (kTr) {
    // gB2[n]: the lanes' sums of channel n = crow(r, h) over the four waves
    // and 32 slots, in one fixed order per channel (slots from n on, so the 32
    // channels' reads fall on 32 banks)
#pragma unroll
    for (int r = 0; r < 16; r++) red[(wave * 16 + r) * 64 + lane] = gbr[r];
    __syncthreads();
    if (threadIdx.x < N2) {
      const int n = threadIdx.x, r = (n & 3) + 4 * (n >> 3), hn = (n >> 2) & 1;
      float v = 0.0f;
      for (int w = 0; w < 4; w++)
        for (int i = 0; i < 32; i++) v += red[(w * 16 + r) * 64 + 32 * hn + ((i + n) & 31)];
      stg[NW1 + N1 + NW2 + n] = v;
    }
  } else {
    red[wave * 64 + lane] = gb2;
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int w = 1; w < 4; w++) gb2 += red[w * 64 + lane];
      gb2 += __shfl_xor(gb2, 32, 64);
      if (h == 0) stg[NW1 + N1 + NW2 + li] = gb2;
    }
  }
  __syncthreads();
  static_assert(N1 == 64 && P12 % 4 == 0, "16 quads per slab row");
  const f32x4* const s4 = reinterpret_cast<const f32x4*>(stg);
  f32x4* const o4 = reinterpret_cast<f32x4*>(out);
  for (int i = threadIdx.x; i < P12 / 4; i += 256) {
    const int row = i >> 4;
    o4[i] = s4[i < (K1 + 1) * 16 ? (row << 4) + ((i & 15) ^ (row & 15)) : i];
  }
}
