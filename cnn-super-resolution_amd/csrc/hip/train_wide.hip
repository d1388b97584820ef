// train_wide.hip -- gfx950 training step for SRCNN nets whose middle layer is
// spatial (f2 > 1): BASELINE.json configs[3], n1=128, n2=64, f1=9, f2=5, f3=5.
//
// The reference runs the same nine OpenCL kernels as for the default net
// (ConfigBasedDataPipeline.cpp:200-323); for this net 95% of the step's FLOPs
// are the three f2 x f2 x n1 x n2 contractions of layer 2 (forward, delta1 and
// gW2: 180.6 MFLOP each per 33x33 tile).  Here every stage is
// an fp32 MFMA implicit GEMM over the reference-layout (HWC) buffers:
//
//   prepack_w2   W2 -> two operand-ordered images (forward / flipped-transposed
//                for delta1), one 1 KB coalesced load per wave per k-step
//   wl1_fwd      L1 9x9x1 -> n1 + bias + ReLU (K = 81 taps, X tile in LDS)
//   conv_mfma    L2 forward (+bias, ReLU) and delta1 = relu'(A1) * full-conv
//                (delta2, W2^T): input channel chunks staged HBM -> LDS by
//                LDS-DMA (double-buffered, 80-B pixel rows: conflict-free
//                ds_read_b128), accumulators for the whole sample in registers;
//                the delta1 variant feeds its masked tiles straight into
//                gW1 / gB1 (ones row) MFMAs, so delta1 never reaches HBM
//   wl3          L3 (Q trick) + last delta (reference relu' quirk) + squared
//                error + delta2 (MFMA over taps) + gW3 / gB3 (MFMA over pixels)
//   wgrad2       gW2 / gB2: 16x16x4 MFMA, K = pixels, per row band of a sample
//                (A1 rows + delta2 rows in LDS), per-block slabs
//   slab_reduce  fixed-order sum of the slabs into the gradient buffer
//
// Deterministic: static work assignment, fixed summation order, no atomics.
#include <map>
#include <mutex>
#include <utility>

#include "common.hpp"
#include "mfma.hpp"
#include "ops.hpp"
#include "split.hpp"

// M0 is written only by the LDS-DMA asm below (nothing else in this file uses it)
#pragma clang diagnostic ignored "-Winline-asm"

namespace srcnn {
namespace wide {

using mfma::crow;
using mfma::f32x16;
using mfma::f32x4;
using mfma::lane_id;
using mfma::mma;
using mfma::mma16;
using mfma::wave_id;
using mfma::zero16;
using mfma::zero4;

typedef __attribute__((address_space(3))) void lds_void;

// 16-B zero source for the LDS-DMA of padding / out-of-image slots
__device__ float g_zero_src[64] = {0.0f};

// LDS-DMA (global_load_lds, 16 or 4 B per lane into M0 + 16 / 4 * lane) as
// inline asm: issued through the builtin, the compiler cannot tell the
// in-flight DMA into the NEXT buffer from reads of the current one and puts
// an s_waitcnt vmcnt(0) before every later LDS read, which drains the whole
// prefetch each k-step.  Hidden from it, its own vmcnt waits only under-count
// (stay safe); every consumer reaches the data through an explicit
// s_waitcnt vmcnt(0) + barrier.
__device__ __forceinline__ uint32_t lds_addr(const float* p) {
  return (uint32_t)reinterpret_cast<uintptr_t>((lds_void*)p);
}
__device__ __forceinline__ void dma16(const float* src, float* lds_dst) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off"
               :
               : "s"(__builtin_amdgcn_readfirstlane(lds_addr(lds_dst))), "v"(src)
               : "m0");
}
// (conv_mfma / d1g16 stage their input images with the default cache policy:
// with the nontemporal hint the L2 forward's HBM bytes went 2.21 -> 3.09 GB
// per launch and delta1's 2.23 -> 2.78 GB, profiles/r04_ab_widedmant)
__device__ __forceinline__ void dma4(const float* src, float* lds_dst) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dword %1, off"
               :
               : "s"(__builtin_amdgcn_readfirstlane(lds_addr(lds_dst))), "v"(src)
               : "m0");
}

struct WGeom {
  int w, h;    // X / T tile
  int w1, h1;  // A1 / D1
  int w2, h2;  // A2 / D2
  int w3, h3;  // A3
  int batch;
};

// ---------------------------------------------------------------------------
// L1 forward: A1 = relu(B1 + conv9x9(X, W1))   (layer_uber_kernel.cl:36-96)
// GEMM M = pixels (32-row tiles), N = 4 x 32 channels (one tile per wave),
// K = 81 taps (+1 zero tap).  The k-slot pairing gives half h the taps
// [KP*h, KP*h + KP), so every A operand is one ds_read_b32 at a per-half base
// plus an immediate.  Four blocks per CU (launch bound: 120 VGPRs), so the
// 1024-block grid is resident at once and every block gets the same number
// of samples (at three blocks per CU, 256 of the 1024 ran after the rest:
// 0.509 -> 0.486 ms, profiles/r03_ab_wl1).
// ---------------------------------------------------------------------------
constexpr int kXS = 40;                // LDS row stride of an X tile (w, h <= kXS)
constexpr int kXTile = kXS * (kXS + 1);  // + one zero row read by the padded tap

template <int N1, int F1>
__global__ __launch_bounds__(256, 4) void wl1_fwd_kernel(const float* __restrict__ X,
                                                      const float* __restrict__ W1,
                                                      const float* __restrict__ B1,
                                                      float* __restrict__ A1, WGeom g) {
  static_assert(N1 == 128, "four waves x 32 output channels");
  constexpr int NT = F1 * F1, KP = (NT + 1) / 2;
  constexpr int Q = KP / F1, R = KP % F1;
  __shared__ float xs[kXTile];
  const int lane = lane_id(), wave = wave_id(), j = lane & 31, h = lane >> 5;
  const int n = 32 * wave + j;
  float wb[KP];
#pragma unroll
  for (int kp = 0; kp < KP; kp++) {
    const int t = kp + KP * h;
    wb[kp] = t < NT ? W1[t * N1 + n] : 0.0f;
  }
  const float bias = B1[n];
  for (int i = threadIdx.x; i < kXTile; i += 256) xs[i] = 0.0f;
  const int npx = g.w1 * g.h1, mtiles = (npx + 31) / 32;
  // tap kp + KP (half 1) sits at one of two fixed offsets from tap kp
  const int dA = h * (Q * kXS + R), dB = h * ((Q + 1) * kXS + R - F1);
  for (int s = blockIdx.x; s < g.batch; s += gridDim.x) {
    __syncthreads();
    const float* xsrc = X + (size_t)s * g.w * g.h;
    for (int i = threadIdx.x; i < g.w * g.h; i += 256) {
      const int y = i / g.w;
      xs[y * kXS + i - y * g.w] = xsrc[i];
    }
    __syncthreads();
    float* dst = A1 + (size_t)s * npx * N1 + n;
    for (int m = 0; m < mtiles; m += 2) {
      int base[2];
#pragma unroll
      for (int u = 0; u < 2; u++) {
        const int o = min(32 * (m + u) + j, npx - 1), oy = o / g.w1;
        base[u] = oy * kXS + o - oy * g.w1;
      }
      f32x16 acc0 = zero16(), acc1 = zero16();
#pragma unroll
      for (int kp = 0; kp < KP; kp++) {
        const int toff = (kp / F1) * kXS + kp % F1;
        const int d = (kp % F1 + R < F1) ? dA : dB;
        acc0 = mma(xs[base[0] + d + toff], wb[kp], acc0);
        acc1 = mma(xs[base[1] + d + toff], wb[kp], acc1);
      }
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int p0 = 32 * m + crow(r, h), p1 = p0 + 32;
        if (p0 < npx) dst[(size_t)p0 * N1] = fmaxf(acc0[r] + bias, 0.0f);
        if (p1 < npx) dst[(size_t)p1 * N1] = fmaxf(acc1[r] + bias, 0.0f);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// wl1x6: the L1 forward of the step with split-bf16 products (split.hpp),
// l12x6's layer 1 (fused, l12x6.hpp) with the operands swapped so the
// accumulator holds [pixel][channel] and A1 leaves as HWC rows:
//   A1[p][n] = relu(B1[n] + sum_tap X[p + off(tap)] W1[tap][n])   (layer_uber_kernel.cl:36-96)
// GEMM M = the 32 pixel slots of a chunk (runs.hpp order), N = 32 channels
// per wave (four waves: n1 = 128), K = taps: taps 0-79 in 5 bf16 k-steps of
// 16 (slot 8h + j of k-step s: group g = 2s + h <= 8 is tap (g, j), g = 9 is
// tap (j, 8)), tap 80 and the bias in one fp32 32x32x2 MFMA that starts the
// accumulator.  A: X windows -- k-steps 0-3 one row of 8 pixels = 4 pair
// dwords per part of the pair image (l12x6's X6Lds layout: the three part
// rows side by side, row stride rs3 = 4 (ow / 4) (mod 32), so a half-wave's
// 32 slots hit 32 banks), k-step 4 the fp32 tile split in registers.  B: the
// wave's W1 parts, register-resident (5 k-steps x 3 parts).  Per chunk 30
// bf16 MFMAs + 1 fp32 where wl1_fwd_kernel issues 82 fp32 32x32x2 (two
// 16-pixel halves of 41 k-pairs); four blocks per CU.
// ---------------------------------------------------------------------------
#include "runs.hpp"

constexpr int kW1x6Regs = 6;  // X tile values per thread (w * h <= 1536)

struct W1x6Lds {
  int rs3, xs, rb, px, bytes;  // pair-image row stride (dwords); byte offsets
  __host__ __device__ W1x6Lds(int w, int h, const RunGeom& rg) {
    const int a4 = (4 * rg.a) % 32;
    rs3 = 3 * w + ((a4 - 3 * w) % 32 + 32) % 32;
    xs = ((rs3 * h + 1) * 4 + 15) & ~15;  // fp32 tile (tap 80, k-step 4)
    rb = (xs + w * h * 4 + 15) & ~15;     // slot -> pair-image row base iy rs3 + ix, and iy w + ix
    px = rb + rg.nch * 32 * 2 * 4;        // [chunk][half][register] -> output pixel (-1: dummy)
    bytes = px + rg.nch * 32 * 4;
  }
};

inline bool wl1x6_fits(int w, int h, int n1, int f1) {
  if (n1 != 128 || f1 != 9 || w * h > 256 * kW1x6Regs) return false;
  const RunGeom rg = run_geom(w - 8, h - 8);
  return W1x6Lds(w, h, rg).bytes <= 36 * 1024;
}

__global__ __launch_bounds__(256, 4) void wl1x6_fwd_kernel(const float* __restrict__ X,
                                                          const float* __restrict__ W1,
                                                          const float* __restrict__ B1,
                                                          float* __restrict__ A1, WGeom g, RunGeom rg) {
  using mfma::bf16x8;
  using mfma::mma_x6;
  using mfma::split3;
  using mfma::split8;
  using mfma::u32x4;
  constexpr int N1 = 128, F1 = 9, K1 = F1 * F1;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const W1x6Lds L(g.w, g.h, rg);
  char* const base = reinterpret_cast<char*>(smem);
  uint32_t* const rimg = reinterpret_cast<uint32_t*>(smem);
  float* const xs = reinterpret_cast<float*>(base + L.xs);
  int* const rbt = reinterpret_cast<int*>(base + L.rb);
  int* const pxt = reinterpret_cast<int*>(base + L.px);
  const int lane = lane_id(), wave = wave_id(), h = lane >> 5, li = lane & 31;
  const int W = g.w, xn = g.w * g.h, npx = g.w1 * g.h1, nch = rg.nch, rs3 = L.rs3;
  const int n = 32 * wave + li;  // this lane's channel (B operand column, output column)

  float xr[kW1x6Regs];
  auto xload = [&](int smp) {
    const float* src = X + (size_t)smp * xn;
#pragma unroll
    for (int k = 0; k < kW1x6Regs; k++) {
      const int i = threadIdx.x + 256 * k;
      xr[k] = i < xn ? src[i] : 0.0f;
    }
  };
  if ((int)blockIdx.x < g.batch) xload(blockIdx.x);

  // W1 parts: k-step s, lane (n, h), element j <-> tap of group g = 2s + h
  bf16x8 wb[5][3];
#pragma unroll
  for (int s_ = 0; s_ < 5; s_++) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const int gg = 2 * s_ + h, tap = gg <= 8 ? gg * F1 + j : j * F1 + 8;
      v[j] = W1[tap * N1 + n];
    }
    split8(v, wb[s_]);
  }
  // tap 80 (half 0) and the bias (half 1): the fp32 MFMA's B operand
  const float b88 = h ? B1[n] : W1[(K1 - 1) * N1 + n];

  for (int i = threadIdx.x; i < nch * 32; i += 256) {
    int iy, ix;
    slot_coord(rg, i >> 5, i & 31, iy, ix);
    rbt[2 * i] = iy * rs3 + ix;
    rbt[2 * i + 1] = iy * W + ix;
    // [chunk][half][register]: register r of half hh is slot crow(r, hh)
    const int c = i >> 5, hh = (i >> 4) & 1, r = i & 15;
    pxt[i] = slot_pixel(rg, c, crow(r, hh));
  }

  for (int sample = blockIdx.x; sample < g.batch; sample += gridDim.x) {
    __syncthreads();  // the previous sample's readers are done with the images
    {
      uint16_t* const r16 = reinterpret_cast<uint16_t*>(rimg);
#pragma unroll
      for (int k = 0; k < kW1x6Regs; k++) {
        const int i = threadIdx.x + 256 * k;
        if (i < xn) {
          xs[i] = xr[k];
          const int y = i / W, x = i - y * W, d = y * rs3 + x;
          __bf16 p[3];
          split3(xr[k], p[0], p[1], p[2]);
#pragma unroll
          for (int q = 0; q < 3; q++) {
            const uint16_t b = __builtin_bit_cast(uint16_t, p[q]);
            r16[2 * (d + W * q)] = b;                 // low half of pair x
            if (x > 0) r16[2 * (d + W * q) - 1] = b;  // high half of pair x - 1
          }
        }
      }
    }
    __syncthreads();
    if (sample + (int)gridDim.x < g.batch) xload(sample + gridDim.x);
    // A1 rows of this sample through a range-checked buffer: a dummy slot's
    // offset (pixel -1) lies outside it and its store is dropped, no branch
    const auto a1rs = __builtin_amdgcn_make_buffer_rsrc(A1 + (size_t)sample * npx * N1, 0, npx * N1 * 4, 0x00020000);

    for (int c = 0; c < nch; c++) {
      const int rb = rbt[2 * (32 * c + li)] + h * rs3, xy = rbt[2 * (32 * c + li) + 1];
      f32x16 acc = mma(h ? 1.0f : xs[xy + 8 * W + 8], b88, zero16());
      auto xop = [&](int s_, bf16x8 (&a)[3]) {
#pragma unroll
        for (int q = 0; q < 3; q++) {
          const uint32_t* r = rimg + W * q + rb + 2 * s_ * rs3;
          u32x4 d;
          d[0] = r[0];
          d[1] = r[2];
          d[2] = r[4];
          d[3] = r[6];
          a[q] = __builtin_bit_cast(bf16x8, d);
        }
      };
#pragma unroll
      for (int s_ = 0; s_ < 4; s_++) {
        bf16x8 a[3];
        xop(s_, a);
        acc = mma_x6(a, wb[s_], acc);
      }
      {
        // k-step 4: half 0 row 8 (dx 0..7), half 1 column 8 (dy 0..7)
        const int b4 = h ? xy + 8 : xy + 8 * W, st4 = h ? W : 1;
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; j++) v[j] = xs[b4 + j * st4];
        bf16x8 a[3];
        split8(v, a);
        acc = mma_x6(a, wb[4], acc);
      }
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int4 t = *reinterpret_cast<const int4*>(pxt + 32 * c + 16 * h + 4 * k);
        const int pr[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
        for (int e = 0; e < 4; e++)
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, mfma::relu1(acc[4 * k + e])), a1rs,
                                                pr[e] * (N1 * 4) + 4 * n, 0, 0);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// wg1x6: gW1 / gB1 of the step with split-bf16 products -- d1x6's gW1
// contraction (fused, d1x6.hpp) with delta1 read from HBM (D1, written by
// wd1x6 before its ReLU' factor) and the factor from A1:
//   gW1[t][n] += sum_p X[p + off(t)] [A1[p][n] > 0] D1[p][n],   gB1[n] += sum_p ...
// (backpropagate.cl:56-114 for layer 1).  Written as gW1^T: M = channels
// (one tile of 32 per wave, four waves = n1 128), N = taps (three tiles: 81
// taps, the ones column of gB1, zeros), K = the 32 slots of a chunk
// (runs.hpp order) in 2 k-steps; A = the wave's masked delta1 (lane =
// channel, 8 slots per lane half: runs 4m + h and 4m + 2 + h), split in
// registers; B = X windows from d1x6's part-interleaved pair images (row
// runs: R, rows padded to rs = 9 (mod 64); column runs: T, column-major),
// double-buffered per sample.  The next item's 32 delta1 / A1 loads (range-
// checked buffer loads: a dummy slot's offset lies outside and reads 0) are
// in flight under the current item's 36 MFMAs.  Every wave owns its channel
// tile, so the block writes its slab with no cross-wave reduction; two
// blocks per CU.  (l1_grad_kernel<MASK> did this on fp32 16x16x4 MFMAs.)
// ---------------------------------------------------------------------------
struct G1x6Lds {
  int st, tcols, rs, rdw, tdw, xbuf, offs, runs, cst, bytes;  // (as fused::D6Lds)
  __host__ __device__ G1x6Lds(int w, int h, const RunGeom& rg) {
    st = 4 * rg.cr + 9;
    if (st < h + 1) st = h + 1;
    tcols = rg.b ? rg.b + 8 : 0;
    rs = w + ((9 - w) % 64 + 64) % 64;
    rdw = 3 * (rs * h + 1);
    tdw = 3 * tcols * st;
    xbuf = rdw + tdw;
    offs = (2 * xbuf * 4 + 15) & ~15;   // [chunk][half][16]: byte offsets of the lane half's slots' rows
    runs = offs + rg.nch * 32 * 4;
    cst = runs + rg.nch * 8 * 4;
    bytes = cst + 32 * 4;
  }
};

inline bool wg1x6_fits(int w, int h, int n1, int f1) {
  if (n1 != 128 || f1 != 9 || w * h > 256 * kW1x6Regs || w > 57) return false;
  const RunGeom rg = run_geom(w - 8, h - 8);
  return G1x6Lds(w, h, rg).bytes <= 80 * 1024;
}

__global__ __launch_bounds__(256, 2) void wg1x6_kernel(const float* __restrict__ X,
                                                      const float* __restrict__ D1,
                                                      const float* __restrict__ A1,
                                                      float* __restrict__ slab, WGeom g, RunGeom rg) {
  using mfma::bf16x8;
  using mfma::mma_x6;
  using mfma::split3;
  using mfma::split8;
  using mfma::u32x4;
  constexpr int N1 = 128, F1 = 9, K1 = F1 * F1, P1 = K1 * N1 + N1;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const G1x6Lds L(g.w, g.h, rg);
  char* const base = reinterpret_cast<char*>(smem);
  uint32_t* const u32 = reinterpret_cast<uint32_t*>(smem);
  int* const offs = reinterpret_cast<int*>(base + L.offs);
  int* const runs = reinterpret_cast<int*>(base + L.runs);
  const int lane = lane_id(), wave = wave_id(), h = lane >> 5, li = lane & 31;
  const int W = g.w, xn = g.w * g.h, npx = g.w1 * g.h1, nch = rg.nch;
  const int x0col = 4 * rg.a;
  const int n = 32 * wave + li;  // this lane's channel (A operand row)

  float xr[kW1x6Regs];
  auto xload = [&](int smp) {
    const float* src = X + (size_t)smp * xn;
#pragma unroll
    for (int k = 0; k < kW1x6Regs; k++) {
      const int i = threadIdx.x + 256 * k;
      xr[k] = i < xn ? src[i] : 0.0f;
    }
  };
  if ((int)blockIdx.x < g.batch) xload(blockIdx.x);

  // per-block tables: element e = 8m + j of lane half hh of chunk c is slot
  // 16m + 8 (j >> 2) + 4 hh + (j & 3) (runs 4m + hh, 4m + 2 + hh)
  for (int i = threadIdx.x; i < nch * 32; i += 256) {
    const int c = i >> 5, hh = (i >> 4) & 1, e = i & 15, m = e >> 3, j = e & 7;
    const int pix = slot_pixel(rg, c, 16 * m + 8 * (j >> 2) + 4 * hh + (j & 3));
    offs[i] = pix >= 0 ? pix * (N1 * 4) : (int)0x80000000;
  }
  for (int k = threadIdx.x; k < nch * 8; k += 256) {
    int iy, ix;
    bool col;
    run_origin(rg, k < rg.nrun ? k : 0, iy, ix, col);
    runs[k] = col ? ~(L.rdw + 3 * ((ix - x0col) * L.st + iy)) : 3 * (iy * L.rs + ix);
  }
  for (int i = threadIdx.x; i < 2 * L.xbuf; i += 256) u32[i] = 0u;
  if (threadIdx.x < 32) u32[L.cst / 4 + threadIdx.x] = threadIdx.x == 0 || threadIdx.x == 6 ? 0x3F803F80u : 0u;

  int offR3[3], offT3[3];
#pragma unroll
  for (int u = 0; u < 3; u++) {
    const int tap = 32 * u + li;
    const int dy = tap < K1 ? tap / F1 : 0, dx = tap < K1 ? tap - dy * F1 : 0;
    offR3[u] = 3 * (dy * L.rs + dx);
    offT3[u] = 3 * (dx * L.st + dy);
  }
  const int spec = li == K1 - 64 ? L.cst / 4 : li > K1 - 64 ? L.cst / 4 + 16 : -1;

  f32x16 g1[3] = {zero16(), zero16(), zero16()};
  // items k = (sample it, chunk c) of the block, it = k / nch; their delta1
  // and A1 values (element e = 8m + j) are loaded two items ahead into two
  // register buffers (one item of MFMAs did not cover the HBM latency)
  float dv[2][16], mv[2][16];
  const int nsmp = (g.batch - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x, nit = nsmp * nch;
  const float inv_nch = 1.0f / (float)nch;
  auto ldi = [&](int k, float (&dd)[16], float (&mm)[16]) __attribute__((always_inline)) {
    if (k >= nit) return;
    const int it = run_div(k, inv_nch), c = k - it * nch, smp = blockIdx.x + it * gridDim.x;
    const auto rd = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(D1) + (size_t)smp * npx * N1, 0,
                                                      npx * N1 * 4, 0x00020000);
    const auto ra = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(A1) + (size_t)smp * npx * N1, 0,
                                                      npx * N1 * 4, 0x00020000);
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int4 o = *reinterpret_cast<const int4*>(offs + 32 * c + 16 * h + 4 * q);
      const int oo[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
      for (int e = 0; e < 4; e++) {
        dd[4 * q + e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rd, oo[e] + 4 * n, 0, 0));
        mm[4 * q + e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ra, oo[e] + 4 * n, 0, 0));
      }
    }
  };
  bf16x8 da[2][3];  // the current item's masked delta1 parts [m]
  auto mask_split = [&](const float (&dd)[16], const float (&mm)[16]) __attribute__((always_inline)) {
#pragma unroll
    for (int m = 0; m < 2; m++) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; j++) v[j] = mm[8 * m + j] > 0.0f ? dd[8 * m + j] : 0.0f;
      split8(v, da[m]);
    }
  };
  // item k: at a sample's first chunk its X pair images (buffer it & 1) and
  // the barrier; then the loads of item k + 2 into the buffer item k came
  // from, the MFMAs, and the split of item k + 1
  auto step = [&](int k, float (&ld)[16], float (&lm)[16], const float (&sd)[16], const float (&sm)[16])
      __attribute__((always_inline)) {
    const int it = run_div(k, inv_nch), c = k - it * nch, smp = blockIdx.x + it * gridDim.x;
    if (c == 0) {
      uint32_t* const xi = u32 + (it & 1) * L.xbuf;
      uint16_t* const x16 = reinterpret_cast<uint16_t*>(xi);
#pragma unroll
      for (int q = 0; q < kW1x6Regs; q++) {
        const int i = threadIdx.x + 256 * q;
        if (i < xn) {
          __bf16 p[3];
          split3(xr[q], p[0], p[1], p[2]);
          const int y = i / W, x = i - y * W, ri = y * L.rs + x;
          const int ti = L.rdw + 3 * ((x - x0col) * L.st + y);
#pragma unroll
          for (int pq = 0; pq < 3; pq++) {
            const uint16_t b = __builtin_bit_cast(uint16_t, p[pq]);
            x16[2 * (3 * ri + pq)] = b;
            if (ri > 0) x16[2 * (3 * (ri - 1) + pq) + 1] = b;
            if (L.tcols && x >= x0col) {
              x16[2 * (ti + pq)] = b;
              if (y > 0) x16[2 * (ti - 3 + pq) + 1] = b;
            }
          }
        }
      }
      __syncthreads();  // images of buffer it & 1 complete; every wave is past sample it - 1
      if (it + 1 < nsmp) xload(smp + gridDim.x);
    }
    ldi(k + 2, ld, lm);
    const int xo = (it & 1) * L.xbuf;
    int rc4[2][2];
#pragma unroll
    for (int m = 0; m < 2; m++)
#pragma unroll
      for (int e = 0; e < 2; e++) rc4[m][e] = runs[8 * c + 4 * m + 2 * e + h];
#pragma unroll
    for (int m = 0; m < 2; m++)
#pragma unroll
      for (int u = 0; u < 3; u++) {
        u32x4 d[3];
#pragma unroll
        for (int e = 0; e < 2; e++) {
          const int code = rc4[m][e];
          int a = xo + (code >= 0 ? code + offR3[u] : ~code + offT3[u]);
          if (u == 2) a = spec >= 0 ? spec : a;
#pragma unroll
          for (int q = 0; q < 3; q++) {
            d[q][2 * e] = u32[a + q];
            d[q][2 * e + 1] = u32[a + q + 6];
          }
        }
        bf16x8 bx[3];
#pragma unroll
        for (int q = 0; q < 3; q++) bx[q] = __builtin_bit_cast(bf16x8, d[q]);
        g1[u] = mma_x6(da[m], bx, g1[u]);
      }
    if (k + 1 < nit) mask_split(sd, sm);
  };

  __syncthreads();  // tables
  ldi(0, dv[0], mv[0]);
  ldi(1, dv[1], mv[1]);
  if (nit > 0) mask_split(dv[0], mv[0]);
  for (int k = 0; k < nit; k += 2) {
    step(k, dv[0], mv[0], dv[1], mv[1]);
    if (k + 1 < nit) step(k + 1, dv[1], mv[1], dv[0], mv[0]);
  }

  // the block's slab [gW1 | gB1]: wave w's channels 32 w .. 32 w + 31
  float* const out = slab + (size_t)blockIdx.x * P1;
#pragma unroll
  for (int u = 0; u < 3; u++) {
    const int tap = 32 * u + li;
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int ch = 32 * wave + crow(r, h);
      if (tap < K1)
        out[tap * N1 + ch] = g1[u][r];
      else if (tap == K1)
        out[K1 * N1 + ch] = g1[u][r];
    }
  }
}

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
constexpr int kCC = 16;       // input channels per LDS chunk
constexpr int kPS = kCC + 4;  // LDS floats per staged pixel (80 B rows)

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
constexpr int kImgMax = 960;                  // pixels of one chunk image (<= 31 x 31)
constexpr int kImgSlack = 256;                // floats: one DMA instruction past the image

struct CGeom {
  int in_w, in_h, pad;    // unpadded input, zero border
  int img_w, img_h;       // largest staged image (window output + F - 1 per side)
  int out_w, out_h, npx;  // output
  int batch;
  int xw, xh;             // delta1 + gW1: the X tile (layer-1 input)
  int wo;                 // > 0: windows of wo x wo outputs (op-level calls on large
                          // images); 0: the whole image is one window
};

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
inline int conv_windows(const CGeom& g) {
  return g.wo == 0 ? 1 : ((g.out_w + g.wo - 1) / g.wo) * ((g.out_h + g.wo - 1) / g.wo);
}

constexpr int kXBuf = kXTile + 64;  // X tile buffer of the fused gW1 epilogue (d1g16)

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
  const int buf_floats = g.img_w * g.img_h * kPS + kImgSlack;  // the largest window image
  const int nitems = g.batch * NP * (g.wo == 0 ? 1 : ((g.out_w + g.wo - 1) / g.wo) * ((g.out_h + g.wo - 1) / g.wo));
  int abase[MT];
  // delta1: a tap row dy whose image rows are zero border for every pixel of
  // tile m (dy outside [dlo, dhi]) is skipped for that tile (wave-uniform
  // branches around MFMA groups that hold no memory operations)
  int dlo[MT], dhi[MT];
  // the image pixel of M-tile slot `slot` (raster order)
  auto pix_of = [&](int slot, int npxw_) { return min(slot, npxw_ - 1); };
  // one LDS-DMA instruction k (64 slots of 16 B) of chunk c of window wn
  // (every window's image is img_w wide: pix / img_w as a multiply, exact for
  // pix < 4096; the predicate is formed without short-circuit branches)
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
constexpr int kW6Row = 28;  // dwords per staged pixel: 3 parts x 16 bf16 + 16 B pad
// pixels of one chunk image: two images in the 160 KiB LDS
constexpr int kW6ImgMax = 160 * 1024 / (2 * kW6Row * 4);
// Image row pitch (dwords).  Lane j of an M tile reads output pixel 32 T + j,
// i.e. image pixel (oy, ox) at quad 7 ox + (pitch / 4) oy; its 16-lane
// ds_read_b128 groups hit 16 distinct quads mod 16 when that quad index is
// 7 (oy out_w + ox) mod 16 -- consecutive outputs, 7 odd -- also across the
// output-row wrap inside a tile.  So pitch / 4 = 7 out_w (mod 16): img_w
// pixels plus (7 (out_w - img_w)) mod 16 pad quads per row (4 for f = 5).
// At pitch = img_w pixels every wrapping tile read was conflicted: 56% / 49%
// of wl2x6 / wd1x6's LDS cycles were bank conflicts (profiles/pmc_r06.json).
__host__ __device__ inline int w6_pitch(int img_w, int out_w) {
  return kW6Row * img_w + 4 * (((7 * (out_w - img_w)) % 16 + 16) % 16);
}

template <int CIN, int COUT, int F>
__global__ void wprep_w2x6_kernel(const float* __restrict__ W2, uint16_t* __restrict__ Wx) {
  constexpr int NCH = CIN / 16, FF = F * F, NT = COUT / 32;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= NT * NCH * FF * 64 * 8) return;
  const int i = e & 7, L = (e >> 3) & 63, rest = e >> 9;
  const int t = rest % FF, c = (rest / FF) % NCH, nt = rest / (FF * NCH);
  const int ch = 16 * c + 8 * (L >> 5) + i, n = 32 * nt + (L & 31);
  __bf16 p[3];
  mfma::split3(W2[((size_t)t * CIN + ch) * COUT + n], p[0], p[1], p[2]);
#pragma unroll
  for (int q = 0; q < 3; q++) Wx[((size_t)rest * 3 + q) * 512 + L * 8 + i] = __builtin_bit_cast(uint16_t, p[q]);
}

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
  const int pitch = w6_pitch(g.img_w, g.out_w);
  uint32_t* const img0 = reinterpret_cast<uint32_t*>(smem);
  uint32_t* const img1 = img0 + g.img_h * pitch;
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
constexpr int kWD6ImgMax = 900;  // staged pixels (30 x 30; one 100.8 KB image)

template <int N1, int N2, int F>
__global__ void wprep_d1x6_kernel(const float* __restrict__ W2, uint16_t* __restrict__ Wx) {
  // [ntile][chunk][tap][part][lane][8] bf16: lane (n, h) holds
  // W2[flip(tap)][32 ntile + n][16 chunk + 8h + i]
  constexpr int NCH = N2 / 16, FF = F * F, NT = N1 / 32;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= NT * NCH * FF * 64 * 8) return;
  const int i = e & 7, L = (e >> 3) & 63, rest = e >> 9;
  const int t = rest % FF, c = (rest / FF) % NCH, nt = rest / (FF * NCH);
  const int dy = t / F, dx = t - dy * F, tf = (F - 1 - dy) * F + (F - 1 - dx);
  const int ch = 16 * c + 8 * (L >> 5) + i, n = 32 * nt + (L & 31);
  __bf16 p[3];
  mfma::split3(W2[((size_t)tf * N1 + n) * N2 + ch], p[0], p[1], p[2]);
#pragma unroll
  for (int q = 0; q < 3; q++) Wx[((size_t)rest * 3 + q) * 512 + L * 8 + i] = __builtin_bit_cast(uint16_t, p[q]);
}

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
  const int pitch = w6_pitch(g.img_w, g.out_w);
  const int nitems = g.batch * NP;
  int vb = blockIdx.x;  // the NP items of a sample on one XCD (d1g16)
  if (gridDim.x % (8 * NP) == 0) {
    const int jb = blockIdx.x / 8;
    vb = (blockIdx.x % 8 + 8 * (jb / NP)) * NP + jb % NP;
  }
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

// ---------------------------------------------------------------------------
// d1g16: delta1 + gW1 of the wide training step on 16-pixel M tiles (round 3).
// The same contraction as conv_mfma<DELTA> (delta1 = relu'(A1) * (delta2
// padded by F-1 (*) W2 flipped / transposed), then gW1 += Xwin^T delta1 and
// gB1 from a ones row), on v_mfma_f32_16x16x4_f32 instead of 32x32x2: the
// same FLOPs per cycle and the same operand reads per MAC, but the border
// taps are skipped per 16-pixel tile instead of per 32-pixel tile.  The 625
// output pixels sit in 40 tiles in the class-grouped order of conv_mfma
// (12,768 -> 11,968 issued pixel-taps for 11,025 useful ones).
//   work item = (sample, 64 output channels); wave = (nt: 32 of them as two
//   16-wide N tiles, mg: the M tiles 2m + mg, m < 20)
//   k-step (tap, 16-channel chunk): A = one ds_read_b128 per lane and tile
//   (lane (i, g): pixel i of the tile, channels 4g .. 4g + 3 of the chunk),
//   feeding 4 MFMAs per N tile; B = one float4 per lane and N tile from the
//   D16 image (prepack_w2_kernel), in a 5-tap ring 4 taps ahead
//   the tiles run in two halves of 10: one half's MFMAs while the other
//   half's A operands load
//   epilogue per tile: C register r of lane (n, g) is pixel slot 4g + r of
//   channel n, i.e. directly gW1's B operand (K = the 4 pixel slots); A = the
//   X windows of 16-tap tiles (81 taps + the ones row: 6 tiles)
// ---------------------------------------------------------------------------
constexpr int kD16MT = 20;                   // 16-pixel tiles per wave group
constexpr int kD16Slots = 2 * kD16MT * 16;  // pixel slots of the tile table
template <int CIN, int COUT, int F, int F1>
__global__ __launch_bounds__(256, 1) void d1g16_kernel(const float* __restrict__ in,
                                                      const float* __restrict__ Wimg,
                                                      const float* __restrict__ ycur,
                                                      const float* __restrict__ X,
                                                      float* __restrict__ slab1, CGeom g) {
  constexpr int NCH = CIN / kCC, FF = F * F, NP = COUT / 64, MT = kD16MT, MH = MT / 2;
  // gW1: taps 0 .. 16 TT - 1 on the matrix core, the last tap and gB1 by VALU
  constexpr int NT1 = F1 * F1, TT = (NT1 - 1) / 16, P1 = NT1 * COUT + COUT;
  static_assert(CIN % kCC == 0 && COUT % 64 == 0 && F == 5 && MT % 2 == 0 && NT1 == 16 * TT + 1, "shape");
  extern __shared__ float smem[];
  const int lane = lane_id(), wave = wave_id(), i16 = lane & 15, g4 = lane >> 4;
  const int nt = wave & 1, mg = wave >> 1;
  const int buf_floats = g.img_w * g.img_h * kPS + kImgSlack;
  const int nitems = g.batch * NP;
  // the NP parts of a sample (the same delta2 image) on one XCD: blocks go
  // round-robin over the 8 XCDs, so parts of pair k run as blocks x, x + 8
  int vb = blockIdx.x;
  if (gridDim.x % (8 * NP) == 0) {
    const int j = blockIdx.x / 8;
    vb = (blockIdx.x % 8 + 8 * (j / NP)) * NP + j % NP;
  }
  float* const xsm = smem + 2 * buf_floats;  // 2 X tile buffers (item parity)
  int* const ptab = reinterpret_cast<int*>(xsm + 2 * kXBuf);
  // gW1 A operand: tap 16 tt + i16; tap NT1 - 1 (offset toffl) and gB1 by VALU
  int toffx[TT];
#pragma unroll
  for (int tt = 0; tt < TT; tt++) {
    const int tap = 16 * tt + i16;
    toffx[tt] = (tap / F1) * kXS + tap % F1;
  }
  constexpr int toffl = ((NT1 - 1) / F1) * kXS + (NT1 - 1) % F1;
  f32x4 gacc[TT][2];
#pragma unroll
  for (int tt = 0; tt < TT; tt++) gacc[tt][0] = gacc[tt][1] = zero4();
  float gv[2] = {0.0f, 0.0f}, gvb[2] = {0.0f, 0.0f};
  auto xdma = [&](int it, int par) {
    const int s = it / NP;
    float* dst = xsm + par * kXBuf;
    for (int k = wave; k * 64 < kXTile; k += 4) {
      const int f = k * 64 + lane, row = f / kXS, col = f - row * kXS;
      const bool ok = row < g.xh && col < g.xw;
      dma4(ok ? X + (size_t)s * g.xw * g.xh + row * g.xw + col : g_zero_src, dst + k * 64);
    }
  };
  // slot -> pixel table in the class-grouped order (conv_mfma), then each
  // 16-slot tile's mask of the taps any of its pixels can use
  const int ow = g.out_w, oh = g.out_h;
  if (threadIdx.x == 0) {
    constexpr int B = F - 1;
    int n = 0;
    if (ow < 2 * B + 1 || oh < 2 * B + 1 || ow * oh > kD16Slots) {  // (the host keeps ow * oh <= kD16Slots)
      for (; n < ow * oh && n < kD16Slots; n++) ptab[n] = n;  // raster order
    } else {
      auto lo = [&](int c, int e) { return c < B ? c : (c == B ? B : e - 2 * B - 1 + c); };
      auto hi = [&](int c, int e) { return c < B ? c + 1 : (c == B ? e - B : e - 2 * B + c); };
      for (int yo = 0; yo <= 2 * B; yo++) {
        const int yc = yo == 0 ? B : (yo <= B ? yo - 1 : yo);
        for (int xc = 0; xc <= 2 * B; xc++)
          for (int x = lo(xc, ow); x < hi(xc, ow); x++)
            for (int y = lo(yc, oh); y < hi(yc, oh); y++) ptab[n++] = y * ow + x;
      }
    }
    for (; n < kD16Slots; n++) ptab[n] = ow * oh - 1;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kD16Slots; i += 256) {
    const int pix = ptab[i], y = pix / ow, x = pix - y * ow;
    uint32_t mb = 0;
#pragma unroll
    for (int dy = 0; dy < F; dy++)
#pragma unroll
      for (int dx = 0; dx < F; dx++) {
        const bool ok = y + dy >= g.pad && y + dy < g.pad + g.in_h && x + dx >= g.pad && x + dx < g.pad + g.in_w;
        mb |= ok ? 1u << (dy * F + dx) : 0u;
      }
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) mb |= __shfl_xor(mb, o, 64);
    if ((i & 15) == 0) ptab[kD16Slots + i / 16] = (int)mb;
  }
  __syncthreads();
  // tile order: position 2m + mg <- class-order tile perm[2m + mg], dealt by
  // tap count (most first) to the wave group with fewer taps so far and room
  // left, so the two groups issue equally many MFMAs (25x25: 375 / 373 tile-taps
  // instead of 377 / 371 for alternate tiles)
  int* const perm = ptab + kD16Slots + 2 * MT;
  if (threadIdx.x == 0) {
    int cnt[2] = {0, 0}, sum[2] = {0, 0};
    for (int pc = FF; pc >= 0; pc--)
      for (int t = 0; t < 2 * MT; t++)
        if (__popc((uint32_t)ptab[kD16Slots + t]) == pc) {
          const int k = (cnt[1] >= MT || (cnt[0] < MT && sum[0] <= sum[1])) ? 0 : 1;
          perm[2 * cnt[k] + k] = t;
          cnt[k]++;
          sum[k] += pc;
        }
  }
  __syncthreads();
  uint32_t tmask[MT];
  int abase[MT], tbase[MT];  // tbase: first slot of the tile at position 2m + mg
#pragma unroll
  for (int m = 0; m < MT; m++) {
    const int T = __builtin_amdgcn_readfirstlane(perm[2 * m + mg]);
    tbase[m] = 16 * T;
    tmask[m] = __builtin_amdgcn_readfirstlane(ptab[kD16Slots + T]);
    const int o = ptab[16 * T + i16], oy = o / ow;
    abase[m] = (oy * g.img_w + o - oy * ow) * kPS + 4 * g4;
  }
  // pix / img_w as a multiply (exact for pix < 4096), predicate without branches
  const uint32_t iw_mag = (1u << 20) / (uint32_t)g.img_w + 1u;
  auto dma = [&](int s, int c, float* buf, int k) {
    const int slot = k * 64 + lane;
    const int pix = slot / 5, q = slot - 5 * pix;
    const int iy = (int)(((uint32_t)pix * iw_mag) >> 20), ix = pix - iy * g.img_w;
    const int y = iy - g.pad, x = ix - g.pad;
    const bool ok = (q < 4) & (slot < g.img_w * g.img_h * 5) & ((unsigned)y < (unsigned)g.in_h) &
                    ((unsigned)x < (unsigned)g.in_w);
    const float* base = in + ((size_t)s * g.in_h * g.in_w) * CIN + c * kCC;
    const float* src = ok ? base + (y * g.in_w + x) * CIN + 4 * q : g_zero_src;
    dma16(src, buf + k * 256);
  };
  const int kdma = (g.img_w * g.img_h * 5 + 63) / 64;
  float* const buf0 = smem;
  float* const buf1 = smem + buf_floats;
  if (vb < nitems)
    for (int k = wave; k < kdma; k += 4) dma(vb / NP, 0, buf0, k);
  wait_vm0();
  __syncthreads();
  int bsel = 0, ipar = 0;
  for (int it = vb; it < nitems; it += gridDim.x, ipar ^= 1) {
    const int s = it / NP, part = it - s * NP;
    xdma(it, ipar);  // lands before the first chunk barrier
    // B: N tile q of this wave is n16 = 4 part + 2 nt + q
    const float4* wp = reinterpret_cast<const float4*>(Wimg) + (size_t)(4 * part + 2 * nt) * NCH * FF * 64 + lane;
    constexpr int WQ = NCH * FF * 64;  // float4s between the two N tiles
    f32x4 acc[MT][2];
#pragma unroll
    for (int m = 0; m < MT; m++) acc[m][0] = acc[m][1] = zero4();
    float4 bq[F][2];
#pragma unroll
    for (int d = 0; d < F - 1; d++)
#pragma unroll
      for (int q = 0; q < 2; q++) bq[d][q] = wp[(size_t)q * WQ + d * 64];
    for (int c = 0; c < NCH; c++) {
      const float* cur = bsel ? buf1 : buf0;
      float* nxt = bsel ? buf0 : buf1;
      int nit = it, nc = c + 1;
      if (nc == NCH) {
        nit = it + gridDim.x;
        nc = 0;
      }
      const bool stage = nit < nitems;
      float4 a[MH], an[MH];
#pragma unroll
      for (int m = 0; m < MH; m++) a[m] = *reinterpret_cast<const float4*>(cur + abase[m]);
#pragma unroll 1
      for (int dy = 0; dy < F; dy++) {
#pragma unroll
        for (int dx = 0; dx < F; dx++) {
          const int t = dy * F + dx;
          const int toff = (dy * g.img_w + dx) * kPS;
          const int tn = dx + 1 < F ? t + 1 : (dy + 1 < F ? t + 1 : t);
          const int toffn = ((tn / F) * g.img_w + (tn % F)) * kPS;
          // B of tap t + 4 (this chunk or the next) into the slot tap t - 1 used
          const int kb = min(c * FF + t + F - 1, NCH * FF - 1);
#pragma unroll
          for (int q = 0; q < 2; q++) bq[(dx + F - 1) % F][q] = wp[(size_t)q * WQ + kb * 64];
          // the next chunk's whole DMA in the first tap, after its B loads (conv_mfma)
          if (stage && t == 0)
            for (int k = wave; k < kdma; k += 4) dma(nit / NP, nc, nxt, k);
          // tiles MH.. of tap t load while tiles ..MH of tap t run
#pragma unroll
          for (int m = 0; m < MH; m++) an[m] = *reinterpret_cast<const float4*>(cur + abase[MH + m] + toff);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int m = 0; m < MH; m++)
            if ((tmask[m] >> t) & 1u) {
#pragma unroll
              for (int jj = 0; jj < 4; jj++)
#pragma unroll
                for (int q = 0; q < 2; q++) acc[m][q] = mma16(a[m][jj], bq[dx][q][jj], acc[m][q]);
            }
          __builtin_amdgcn_sched_barrier(0);
          // tiles ..MH of tap t + 1 load while tiles MH.. of tap t run
#pragma unroll
          for (int m = 0; m < MH; m++) a[m] = *reinterpret_cast<const float4*>(cur + abase[m] + toffn);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int m = 0; m < MH; m++)
            if ((tmask[MH + m] >> t) & 1u) {
#pragma unroll
              for (int jj = 0; jj < 4; jj++)
#pragma unroll
                for (int q = 0; q < 2; q++) acc[MH + m][q] = mma16(an[m][jj], bq[dx][q][jj], acc[MH + m][q]);
            }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      wait_vm0();
      __syncthreads();
      bsel ^= 1;
    }
    // epilogue: delta1 = relu'(A1) * acc, then gW1 += Xwin^T delta1
    const float* xs = xsm + ipar * kXBuf;
    const uint32_t ow_mag = (1u << 20) / (uint32_t)ow + 1u;  // pix / ow as a multiply (pix < 4096)
    const size_t obase = (size_t)s * g.npx * COUT + part * 64 + nt * 32 + i16;
    // relu' operands (A1, from HBM) kEpD tiles ahead in a ring of named sets:
    // a tile's gW1 work (48 MFMAs) is shorter than one HBM round trip
    constexpr int kEpD = 3;  // epilogue relu' loads this many tiles ahead
    float mk[kEpD + 1][2][4];
    auto ldmask = [&](int m, float (&d)[2][4]) {
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int pix = ptab[tbase[m] + 4 * g4 + r];
#pragma unroll
        for (int q = 0; q < 2; q++) d[q][r] = ycur[obase + (size_t)pix * COUT + 16 * q];
      }
    };
#pragma unroll
    for (int m = 0; m < kEpD; m++) ldmask(m, mk[m]);
#pragma unroll
    for (int m = 0; m < MT; m++) {
      if (m + kEpD < MT) ldmask(m + kEpD, mk[(m + kEpD) % (kEpD + 1)]);
      const int s0 = tbase[m] + 4 * g4;
#pragma unroll
      for (int r = 0; r < 4; r++)
#pragma unroll
        for (int q = 0; q < 2; q++)
          acc[m][q][r] = (s0 + r < g.npx && mk[m % (kEpD + 1)][q][r] > 0.0f) ? acc[m][q][r] : 0.0f;
      // X windows of k-step r (pixel slot s0 + r), one k-step ahead, two named sets
      float xq[2][TT + 1];
      auto xrd = [&](int r) {
        const int pix = ptab[s0 + r], py = (int)(((uint32_t)pix * ow_mag) >> 20);
        const int xb = py * kXS + pix - py * ow;
#pragma unroll
        for (int tt = 0; tt < TT; tt++) xq[r & 1][tt] = xs[xb + toffx[tt]];
        xq[r & 1][TT] = xs[xb + toffl];
      };
      xrd(0);
#pragma unroll
      for (int r = 0; r < 4; r++) {
        if (r + 1 < 4) xrd(r + 1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int tt = 0; tt < TT; tt++)
#pragma unroll
          for (int q = 0; q < 2; q++) gacc[tt][q] = mma16(xq[r & 1][tt], acc[m][q][r], gacc[tt][q]);
#pragma unroll
        for (int q = 0; q < 2; q++) {
          gv[q] = fmaf(xq[r & 1][TT], acc[m][q][r], gv[q]);
          gvb[q] += acc[m][q][r];
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
  // the VALU rows summed over the four pixel-slot groups (fixed order)
#pragma unroll
  for (int q = 0; q < 2; q++) {
    gv[q] += __shfl_xor(gv[q], 16, 64);
    gv[q] += __shfl_xor(gv[q], 32, 64);
    gvb[q] += __shfl_xor(gvb[q], 16, 64);
    gvb[q] += __shfl_xor(gvb[q], 32, 64);
  }
  // gW1 slab of this block pair: waves mg = 1 park their partials in LDS,
  // waves mg = 0 add them (fixed order) and store rows tap < NT1 and gB1
  __syncthreads();
  float* red = smem;
  constexpr int RV = 2 * TT * 2 * 4 * 64;  // the VALU rows' parking place
  if (mg == 1) {
#pragma unroll
    for (int tt = 0; tt < TT; tt++)
#pragma unroll
      for (int q = 0; q < 2; q++)
#pragma unroll
        for (int r = 0; r < 4; r++) red[(((nt * TT + tt) * 2 + q) * 4 + r) * 64 + lane] = gacc[tt][q][r];
#pragma unroll
    for (int q = 0; q < 2; q++) {
      red[RV + ((nt * 2 + q) * 2 + 0) * 64 + lane] = gv[q];
      red[RV + ((nt * 2 + q) * 2 + 1) * 64 + lane] = gvb[q];
    }
  }
  __syncthreads();
  if (mg == 0) {
    float* o1 = slab1 + (size_t)(vb / NP) * P1;
#pragma unroll
    for (int q = 0; q < 2; q++) {
      const int ch = (vb % NP) * 64 + 32 * nt + 16 * q + i16;
#pragma unroll
      for (int tt = 0; tt < TT; tt++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int tap = 16 * tt + 4 * g4 + r;
          o1[tap * COUT + ch] = gacc[tt][q][r] + red[(((nt * TT + tt) * 2 + q) * 4 + r) * 64 + lane];
        }
      if (g4 == 0) {
        o1[(NT1 - 1) * COUT + ch] = gv[q] + red[RV + ((nt * 2 + q) * 2 + 0) * 64 + lane];
        o1[NT1 * COUT + ch] = gvb[q] + red[RV + ((nt * 2 + q) * 2 + 1) * 64 + lane];
      }
    }
  }
}

// ---------------------------------------------------------------------------
// wl3: per sample
//   1. Q[p][t] = sum_c A2[p][c] W3[t][c]      (MFMA: M = pixels, N = taps, K = n2)
//   2. A3[o] = B3 + sum_t Q[o + off(t)][t]; delta3 = (A3 - T[o + pad]) [A3 > 0]
//      (last_layer_delta.cl:34-48, relu' quirk kept); squared error
//      (squared_error.cl); delta3 written into a zero-bordered grid Gd
//   3. delta2[p][c] = [A2 > 0] sum_t Gd[p - off(t)] W3[t][c]   (MFMA, K = taps)
//   4. gW3[t][c] += sum_p Gd[p - off(t)] A2[p][c]              (MFMA, K = pixels)
// gW3 / gB3 / squared error accumulate in registers across the block's
// samples and leave as one slab per block.
// ---------------------------------------------------------------------------
// Operands run ahead of their use (round 3, -18% wl3): each wave's next Q
// tile (across samples: the next sample's first tile) is in flight under the
// current tile's MFMAs, and gW3's A2 pixel pairs come in batches of kWl3B, the
// next batch in flight under the current one.  Two blocks per CU, every
// accumulator in VGPRs (launch bound).
constexpr int kWl3B = 4;  // gW3 pixel pairs per prefetch batch
template <int N2, int F3>
__global__ __launch_bounds__(256, 2) void wl3_kernel(const float* __restrict__ A2,
                                                  const float* __restrict__ T,
                                                  const float* __restrict__ W3,
                                                  const float* __restrict__ B3,
                                                  float* __restrict__ D2, float* __restrict__ slab3,
                                                  float* __restrict__ sqs, float* __restrict__ A3out,
                                                  WGeom g, int qfloats) {
  static_assert(N2 == 64 && F3 * F3 <= 32, "shape");
  constexpr int FF = F3 * F3, KP3 = (FF + 1) / 2, P3 = FF * N2 + 1;
  extern __shared__ float smem[];
  float* Qs = smem;             // [npx2][FF], later the cross-wave reduction
  float* Gd = smem + qfloats;   // [(h3 + 2(F3-1))][(w3 + 2(F3-1))]
  // relu' mask of A2 as bits, built from the step-1 operand registers so step
  // 3 does not re-read A2 from HBM: word [p][h] bit 4kk + jj <-> channel 8kk + 4h + jj
  unsigned* mbits = reinterpret_cast<unsigned*>(Gd + (g.w3 + 2 * (F3 - 1)) * (g.h3 + 2 * (F3 - 1)));
  __shared__ float red_s[2][4];
  const int lane = lane_id(), wave = wave_id(), j = lane & 31, h = lane >> 5;
  const int npx2 = g.w2 * g.h2, mt2 = (npx2 + 31) / 32, npx3 = g.w3 * g.h3;
  const int GW = g.w3 + 2 * (F3 - 1), GH = g.h3 + 2 * (F3 - 1);
  const int padT = (g.w - g.w3) / 2;  // last_layer_delta.cl:25 (from the width)
  const uint32_t w2_mag = (1u << 20) / (uint32_t)g.w2 + 1u;  // p / w2 as a multiply (p < 4096)
  auto row_of = [&](int p) { return (int)(((uint32_t)p * w2_mag) >> 20); };
  for (int i = threadIdx.x; i < GW * GH; i += 256) Gd[i] = 0.0f;
  // step 1 B operand: W3[t = j][c = 8kk + 4h + jj]
  float wq[8][4];
#pragma unroll
  for (int kk = 0; kk < 8; kk++)
#pragma unroll
    for (int jj = 0; jj < 4; jj++) wq[kk][jj] = j < FF ? W3[j * N2 + 8 * kk + 4 * h + jj] : 0.0f;
  // step 3: wave = (N tile nt, M group mg); taps kp + KP3*h
  const int nt = wave & 1, mg = wave >> 1;
  float wd[KP3];
  int goff[KP3];
#pragma unroll
  for (int kp = 0; kp < KP3; kp++) {
    const int t = kp + KP3 * h, tc = min(t, FF - 1);
    wd[kp] = t < FF ? W3[t * N2 + 32 * nt + j] : 0.0f;
    goff[kp] = -((tc / F3) * GW + tc % F3);
  }
  // step 4: row = tap j
  const int tA = min(j, FF - 1);
  const int goffA = -((tA / F3) * GW + tA % F3);
  const bool tapA = j < FF;
  f32x16 gacc0 = zero16(), gacc1 = zero16();
  float sq = 0.0f, gb3 = 0.0f;
  const float b3 = B3[0];
  // step 1 operands of tile mt: lane (j, h) reads pixel 32 mt + j, channels
  // 8 kk + 4 h + jj.  The next tile's (across samples: the next sample's first
  // tile's) loads are in flight under the current tile's MFMAs.
  float4 vn[8];
  auto ldq = [&](const float* a2s_, int mt_) {
    const int p = min(32 * mt_ + j, npx2 - 1);
    const float4* src = reinterpret_cast<const float4*>(a2s_ + (size_t)p * N2) + h;
#pragma unroll
    for (int kk = 0; kk < 8; kk++) vn[kk] = src[2 * kk];
  };
  if ((int)blockIdx.x < g.batch && wave < mt2) ldq(A2 + (size_t)blockIdx.x * npx2 * N2, wave);
  for (int s = blockIdx.x; s < g.batch; s += gridDim.x) {
    const float* a2s = A2 + (size_t)s * npx2 * N2;
    __syncthreads();  // previous sample's Gd / Qs readers are done
    // 1. Q
    for (int mt = wave; mt < mt2; mt += 4) {
      float4 v[8];
#pragma unroll
      for (int kk = 0; kk < 8; kk++) v[kk] = vn[kk];
      if (mt + 4 < mt2) ldq(a2s, mt + 4);
      f32x16 acc = zero16();
#pragma unroll
      for (int kk = 0; kk < 8; kk++)
#pragma unroll
        for (int jj = 0; jj < 4; jj++) acc = mma(v[kk][jj], wq[kk][jj], acc);
      {
        unsigned m = 0;
#pragma unroll
        for (int kk = 0; kk < 8; kk++)
#pragma unroll
          for (int jj = 0; jj < 4; jj++) m |= (v[kk][jj] > 0.0f ? 1u : 0u) << (4 * kk + jj);
        if (32 * mt + j < npx2) mbits[2 * (32 * mt + j) + h] = m;
      }
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int pix = 32 * mt + crow(r, h);
        if (pix < npx2 && j < FF) Qs[pix * FF + j] = acc[r];
      }
    }
    __syncthreads();
    // 2. A3, last delta, squared error
    const float* ts = T + (size_t)s * g.w * g.h;
    for (int o = threadIdx.x; o < npx3; o += 256) {
      const int oy = o / g.w3, ox = o - oy * g.w3;
      const float* q0 = Qs + (oy * g.w2 + ox) * FF;
      float v = 0.0f;
#pragma unroll
      for (int t = 0; t < FF; t++) v += q0[((t / F3) * g.w2 + t % F3) * FF + t];
      const float a3 = v + b3;
      A3out[(size_t)s * npx3 + o] = a3;  // to the workspace (srcnn_train_activations)
      const float diff = a3 - ts[(oy + padT) * g.w + ox + padT];
      const float d = a3 > 0.0f ? diff : 0.0f;
      sq += diff * diff;
      gb3 += d;
      Gd[(oy + F3 - 1) * GW + ox + F3 - 1] = d;
    }
    __syncthreads();
    // 3. delta2 (channel 32nt + j: mask word half mh, bit mbit)
    const int mc = 32 * nt + j, mh = (mc >> 2) & 1, mbit = 4 * (mc >> 3) + (mc & 3);
    for (int mt = mg; mt < mt2; mt += 2) {
      const int p = min(32 * mt + j, npx2 - 1), py = row_of(p), px = p - py * g.w2;
      const int gb = (py + F3 - 1) * GW + px + F3 - 1;
      f32x16 acc = zero16();
#pragma unroll
      for (int kp = 0; kp < KP3; kp++) acc = mma(Gd[gb + goff[kp]], wd[kp], acc);
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int pix = 32 * mt + crow(r, h);
        if (pix < npx2) {
          const size_t idx = ((size_t)s * npx2 + pix) * N2 + 32 * nt + j;
          D2[idx] = (mbits[2 * pix + mh] >> mbit) & 1u ? acc[r] : 0.0f;
        }
      }
    }
    // the next sample's first Q tile, in flight under delta2 / gW3
    if (s + (int)gridDim.x < g.batch && wave < mt2) ldq(a2s + (size_t)gridDim.x * npx2 * N2, wave);
    // 4. gW3 (K = pixel pairs kp = wave + 4 i split over the waves; B columns:
    // channel 2j + tile), in batches of kWl3B pairs: the next batch's A2 loads
    // and delta3-window reads are issued before the current batch's MFMAs
    // (two named register sets); pairs past the wave's count are not issued
    const int niter = (npx2 + 1) / 2 > wave ? ((npx2 + 1) / 2 - wave + 3) / 4 : 0;
    float2 bb[2][kWl3B];
    float ab[2][kWl3B];
    auto ldb = [&](int i0, float2 (&b_)[kWl3B], float (&a_)[kWl3B]) {
#pragma unroll
      for (int u = 0; u < kWl3B; u++) {
        const int pk = 2 * (wave + 4 * (i0 + u)) + h;
        const bool pok = pk < npx2;
        const int p = pok ? pk : npx2 - 1, py = row_of(p), px = p - py * g.w2;
        const float av = Gd[(py + F3 - 1) * GW + px + F3 - 1 + goffA];
        a_[u] = (tapA && pok) ? av : 0.0f;
        b_[u] = *reinterpret_cast<const float2*>(a2s + (size_t)p * N2 + 2 * j);
      }
    };
    auto mmb = [&](int i0, const float2 (&b_)[kWl3B], const float (&a_)[kWl3B]) {
#pragma unroll
      for (int u = 0; u < kWl3B; u++)
        if (i0 + u < niter) {
          gacc0 = mma(a_[u], b_[u].x, gacc0);
          gacc1 = mma(a_[u], b_[u].y, gacc1);
        }
    };
    if (niter > 0) ldb(0, bb[0], ab[0]);
    for (int i0 = 0; i0 < niter; i0 += 2 * kWl3B) {
      if (i0 + kWl3B < niter) ldb(i0 + kWl3B, bb[1], ab[1]);
      mmb(i0, bb[0], ab[0]);
      if (i0 + kWl3B >= niter) break;
      if (i0 + 2 * kWl3B < niter) ldb(i0 + 2 * kWl3B, bb[0], ab[0]);
      mmb(i0 + kWl3B, bb[1], ab[1]);
    }
  }
  // cross-wave reduction of gW3 (fixed order), gB3, squared error
  __syncthreads();
  float* red = Qs;  // 4 waves x 2 tiles x 16 regs x 64 lanes
#pragma unroll
  for (int r = 0; r < 16; r++) {
    red[((wave * 2 + 0) * 16 + r) * 64 + lane] = gacc0[r];
    red[((wave * 2 + 1) * 16 + r) * 64 + lane] = gacc1[r];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sq += __shfl_down(sq, o, 64);
    gb3 += __shfl_down(gb3, o, 64);
  }
  if (lane == 0) {
    red_s[0][wave] = sq;
    red_s[1][wave] = gb3;
  }
  __syncthreads();
  float* out = slab3 + (size_t)blockIdx.x * P3;
  for (int e = threadIdx.x; e < 2 * 16 * 64; e += 256) {
    const int tile = e / (16 * 64), r = (e / 64) % 16, l = e & 63;
    const int tap = crow(r, l >> 5), c = 2 * (l & 31) + tile;
    float v = 0.0f;
    for (int w = 0; w < 4; w++) v += red[((w * 2 + tile) * 16 + r) * 64 + l];
    if (tap < FF) out[tap * N2 + c] = v;
  }
  if (threadIdx.x == 0) {
    out[FF * N2] = red_s[1][0] + red_s[1][1] + red_s[1][2] + red_s[1][3];
    sqs[blockIdx.x] = red_s[0][0] + red_s[0][1] + red_s[0][2] + red_s[0][3];
  }
}

// ---------------------------------------------------------------------------
// wl3l: wl3 with the sample's A2 resident in LDS (round 3).  The Q phase
// writes the A2 operands it loaded into a quad-swizzled LDS image, so the
// delta2 mask and gW3's operand come from LDS and A2 is read from HBM once
// (wl3 read it twice: 1.51x the fused-minimum bytes).  A2 (441 x 64 floats,
// 112.9 KB) + Q (44.1 KB) + the delta3 grid fill the LDS, so one block of 8
// waves per CU; the next sample's first Q tile is loaded before the delta2
// stores (a store counts in vmcnt too) and lands under delta2 / gW3.
// ---------------------------------------------------------------------------
template <int N2>
__device__ __forceinline__ int wl3l_at(int p, int c) {  // A2 image float index, quads XOR-swizzled by pixel
  return p * N2 + 4 * ((c >> 2) ^ (p & (N2 / 4 - 1))) + (c & 3);
}
template <int N2, int F3>
__global__ __launch_bounds__(512, 1) void wl3l_kernel(const float* __restrict__ A2,
                                                     const float* __restrict__ T,
                                                     const float* __restrict__ W3,
                                                     const float* __restrict__ B3,
                                                     float* __restrict__ D2, float* __restrict__ slab3,
                                                     float* __restrict__ sqs, float* __restrict__ A3out,
                                                     WGeom g) {
  static_assert(N2 == 64 && F3 * F3 <= 32, "shape");
  constexpr int FF = F3 * F3, KP3 = (FF + 1) / 2, P3 = FF * N2 + 1, NW = 8;
  extern __shared__ float smem[];
  const int npx2 = g.w2 * g.h2, mt2 = (npx2 + 31) / 32, npx3 = g.w3 * g.h3;
  const int GW = g.w3 + 2 * (F3 - 1), GH = g.h3 + 2 * (F3 - 1);
  float* a2i = smem;                  // [npx2][N2], swizzled; the end-of-kernel reduction
  float* Qs = smem + npx2 * N2;       // [npx2][FF]
  float* Gd = Qs + npx2 * FF;         // [GH][GW]
  __shared__ float red_s[2][NW];
  const int lane = lane_id(), wave = wave_id(), j = lane & 31, h = lane >> 5;
  const int padT = (g.w - g.w3) / 2;  // last_layer_delta.cl:25 (from the width)
  // p / w2 as a multiply by a 20-bit reciprocal (exact for p < 4096; a runtime
  // division costs ~15 VALU per pixel pair in the gW3 loop)
  const uint32_t w2_mag = (1u << 20) / (uint32_t)g.w2 + 1u;
  auto row_of = [&](int p) { return (int)(((uint32_t)p * w2_mag) >> 20); };
  for (int i = threadIdx.x; i < GW * GH; i += 512) Gd[i] = 0.0f;
  float wq[8][4];
#pragma unroll
  for (int kk = 0; kk < 8; kk++)
#pragma unroll
    for (int jj = 0; jj < 4; jj++) wq[kk][jj] = j < FF ? W3[j * N2 + 8 * kk + 4 * h + jj] : 0.0f;
  const int nt = wave & 1, mg = wave >> 1;  // delta2: N tile, M group (4)
  float wd[KP3];
  int goff[KP3];
#pragma unroll
  for (int kp = 0; kp < KP3; kp++) {
    const int t = kp + KP3 * h, tc = min(t, FF - 1);
    wd[kp] = t < FF ? W3[t * N2 + 32 * nt + j] : 0.0f;
    goff[kp] = -((tc / F3) * GW + tc % F3);
  }
  const int tA = min(j, FF - 1);
  const int goffA = -((tA / F3) * GW + tA % F3);
  const bool tapA = j < FF;
  f32x16 gacc0 = zero16(), gacc1 = zero16();
  float sq = 0.0f, gb3 = 0.0f;
  const float b3 = B3[0];
  float4 vn[8];
  auto ldq = [&](const float* a2s_, int mt_) {
    const int p = min(32 * mt_ + j, npx2 - 1);
    const float4* src = reinterpret_cast<const float4*>(a2s_ + (size_t)p * N2) + h;
#pragma unroll
    for (int kk = 0; kk < 8; kk++) vn[kk] = src[2 * kk];
  };
  if ((int)blockIdx.x < g.batch && wave < mt2) ldq(A2 + (size_t)blockIdx.x * npx2 * N2, wave);
  for (int s = blockIdx.x; s < g.batch; s += gridDim.x) {
    const float* a2s = A2 + (size_t)s * npx2 * N2;
    const float* ts = T + (size_t)s * g.w * g.h;
    __syncthreads();  // the previous sample's readers of every LDS region are done
    float tv = 0.0f;  // this thread's target pixel (outputs past 512: loaded in place)
    {
      const int o = min((int)threadIdx.x, npx3 - 1), oy = o / g.w3, ox = o - oy * g.w3;
      tv = ts[(oy + padT) * g.w + ox + padT];
    }
    // 1. Q, and the A2 image
    for (int mt = wave; mt < mt2; mt += NW) {
      float4 v[8];
#pragma unroll
      for (int kk = 0; kk < 8; kk++) v[kk] = vn[kk];
      if (mt + NW < mt2) ldq(a2s, mt + NW);
      f32x16 acc = zero16();
#pragma unroll
      for (int kk = 0; kk < 8; kk++)
#pragma unroll
        for (int jj = 0; jj < 4; jj++) acc = mma(v[kk][jj], wq[kk][jj], acc);
      const int p = 32 * mt + j;
      if (p < npx2)
#pragma unroll
        for (int kk = 0; kk < 8; kk++) *reinterpret_cast<float4*>(a2i + wl3l_at<N2>(p, 8 * kk + 4 * h)) = v[kk];
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int pix = 32 * mt + crow(r, h);
        if (pix < npx2 && j < FF) Qs[pix * FF + j] = acc[r];
      }
    }
    __syncthreads();
    // 2. A3, last delta, squared error
    for (int o = threadIdx.x; o < npx3; o += 512) {
      const int oy = o / g.w3, ox = o - oy * g.w3;
      const float* q0 = Qs + (oy * g.w2 + ox) * FF;
      float v = 0.0f;
#pragma unroll
      for (int t = 0; t < FF; t++) v += q0[((t / F3) * g.w2 + t % F3) * FF + t];
      const float a3 = v + b3;
      A3out[(size_t)s * npx3 + o] = a3;  // to the workspace (srcnn_train_activations)
      const float tgt = o == (int)threadIdx.x ? tv : ts[(oy + padT) * g.w + ox + padT];
      const float diff = a3 - tgt;
      const float d = a3 > 0.0f ? diff : 0.0f;
      sq += diff * diff;
      gb3 += d;
      Gd[(oy + F3 - 1) * GW + ox + F3 - 1] = d;
    }
    __syncthreads();
    // the next sample's first Q tile, issued before the delta2 stores
    if (s + (int)gridDim.x < g.batch && wave < mt2) ldq(a2s + (size_t)gridDim.x * npx2 * N2, wave);
    // 3. delta2 = [A2 > 0] sum_t Gd W3 (channel 32 nt + j)
    const int mc = 32 * nt + j;
    for (int mt = mg; mt < mt2; mt += NW / 2) {
      const int p = min(32 * mt + j, npx2 - 1), py = row_of(p), px = p - py * g.w2;
      const int gb = (py + F3 - 1) * GW + px + F3 - 1;
      f32x16 acc = zero16();
#pragma unroll
      for (int kp = 0; kp < KP3; kp++) acc = mma(Gd[gb + goff[kp]], wd[kp], acc);
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int pix = 32 * mt + crow(r, h);
        if (pix < npx2) {
          const size_t idx = ((size_t)s * npx2 + pix) * N2 + mc;
          D2[idx] = a2i[wl3l_at<N2>(pix, mc)] > 0.0f ? acc[r] : 0.0f;
        }
      }
    }
    // 4. gW3 (K = pixel pairs kp = wave + NW i; B columns: channel 2j + tile);
    // batching the LDS reads of 4 or 8 pairs ahead of their MFMAs measured
    // slower (0.349 / 0.356 vs 0.341 ms)
    for (int kp = wave; 2 * kp < npx2; kp += NW) {
      const int pk = 2 * kp + h;
      const bool pok = pk < npx2;
      const int p = pok ? pk : npx2 - 1, py = row_of(p), px = p - py * g.w2;
      const float av = Gd[(py + F3 - 1) * GW + px + F3 - 1 + goffA];
      const float a = (tapA && pok) ? av : 0.0f;
      const float2 bv = *reinterpret_cast<const float2*>(a2i + wl3l_at<N2>(p, 2 * j));
      gacc0 = mma(a, bv.x, gacc0);
      gacc1 = mma(a, bv.y, gacc1);
    }
  }
  // cross-wave reduction of gW3 (fixed wave order), gB3, squared error
  __syncthreads();
  float* red = a2i;  // NW waves x 2 tiles x 16 regs x 64 lanes
#pragma unroll
  for (int r = 0; r < 16; r++) {
    red[((wave * 2 + 0) * 16 + r) * 64 + lane] = gacc0[r];
    red[((wave * 2 + 1) * 16 + r) * 64 + lane] = gacc1[r];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sq += __shfl_down(sq, o, 64);
    gb3 += __shfl_down(gb3, o, 64);
  }
  if (lane == 0) {
    red_s[0][wave] = sq;
    red_s[1][wave] = gb3;
  }
  __syncthreads();
  float* out = slab3 + (size_t)blockIdx.x * P3;
  for (int e = threadIdx.x; e < 2 * 16 * 64; e += 512) {
    const int tile = e / (16 * 64), r = (e / 64) % 16, l = e & 63;
    const int tap = crow(r, l >> 5), c = 2 * (l & 31) + tile;
    float v = 0.0f;
    for (int w = 0; w < NW; w++) v += red[((w * 2 + tile) * 16 + r) * 64 + l];
    if (tap < FF) out[tap * N2 + c] = v;
  }
  if (threadIdx.x == 0) {
    float b = 0.0f, q = 0.0f;
    for (int w = 0; w < NW; w++) {
      b += red_s[1][w];
      q += red_s[0][w];
    }
    out[FF * N2] = b;
    sqs[blockIdx.x] = q;
  }
}

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
constexpr int kGAS = 48;      // LDS floats per A1 pixel (32 channels + pad)
constexpr int kGDS = 80;      // LDS floats per delta2 pixel (64 channels + pad)
constexpr int kBandPx = 64;   // output pixels per band (16 quads)
constexpr int kGAPx = 192;    // A1 pixels per band image (max)
constexpr int kGAFl = kGAPx * kGAS;
constexpr int kGBuf = kGAFl + (kBandPx + 4) * kGDS + 256;

struct G2Geom {
  int w1, h1, w2, h2;
  int rows, nbands;  // output rows per band, bands per sample (nbx * band rows)
  int batch, groups;
  int cols, nbx;     // output columns per band (w2: full rows), bands per band row
  int aw;            // A1 band image width cols + F - 1 (a kernel argument, so the
                     // tap offsets stay scalar: 4 adds per k-step, not 7)
};

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
constexpr int kG6RowP = 48;                              // dwords per ring row (pair image)
constexpr int kG6Ring = 8;                               // ring rows: a band of 4 + F - 1
constexpr int kG6QP = kG6Ring * kG6RowP;                 // dwords per (channel, part)
constexpr int kG6CP = 3 * kG6QP + 1;                     // dwords per channel (= 1 mod 64)
constexpr int kG6A = 16 * kG6CP;                         // A ring dwords
constexpr int kG6NP = 12;                                // dwords per delta2 (part, row, n): 24 px
constexpr int kG6D = 3 * 4 * 64 * kG6NP;                 // delta2 image dwords
constexpr size_t kG6Lds = (size_t)(kG6A + kG6D) * 4;     // 110.7 KB: one block per CU
constexpr int kG6MaxW2 = 24, kG6Groups = 32;

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

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
template <int N1, int N2, int F1, int F2, int F3>
struct Net {
  static constexpr int W1 = F1 * F1 * N1, P1 = W1 + N1;
  static constexpr int W2 = F2 * F2 * N1 * N2, P2 = W2 + N2;
  static constexpr int W3 = F3 * F3 * N2, P3 = W3 + 1;
  static constexpr int MT2 = 7;   // L2 forward: up to 2 x 7 x 32 = 448 output pixels
  static constexpr int MT4 = 10;  // delta1: up to 640 pixels
};

static size_t align_f(size_t n) { return (n + 63) & ~(size_t)63; }

// Everything the step decides before its first launch.  plan_step fills it
// from the shape and the arithmetic alone: no buffer, no HIP call.
struct WidePlan {
  WGeom g;
  CGeom cf, cd;  // L2 forward, delta1
  G2Geom g2;     // wgrad2 bands; groups = the launched kernel's sample groups
  // split-bf16 kernels: x6 wl2x6 (L2 forward), x6d wd1x6 (delta1 into D1,
  // then gW1 apart), x6f wl1x6 (L1 forward), x6g1 wg1x6 (gW1 after wd1x6, else
  // l1_grad_kernel), x6g wgrad2x6.  wl3l: layer 3 with the A2 image in LDS.
  bool x6, x6d, x6f, x6g1, x6g, wl3l;
  int qfloats;                                 // wl3's Q image
  RunGeom rg1;                                 // layer 1's runs (wl1x6, wg1x6)
  int GL1, GL2, G3, GD, GW1, GG1, GG2, nslab1;  // grids: L1, L2, layer 3, delta1, l1_grad, wg1x6, grad2; gW1 slabs
  size_t lds1, lds2, lds3, ldsd, ldsg1, ldsg2;  // dynamic LDS bytes of the launched variants
  // workspace in floats: Wf | Wd | Wx (split W2 image, wl2x6) | Wx1 (split flipped W2, wd1x6) | slab1 | slab2 | slab3 | sqs
  size_t nWf, nWd, nWx, n1, n2, n3, nsq, bytes;
};

template <int N1, int N2, int F1, int F2, int F3>
static bool plan_step(uint32_t w, uint32_t h, uint32_t batch, int arith, WidePlan* out) {
  using NetT = Net<N1, N2, F1, F2, F3>;
  WidePlan& p = *out = {};
  WGeom& g = p.g;
  g.w = (int)w;
  g.h = (int)h;
  g.w1 = g.w - F1 + 1;
  g.h1 = g.h - F1 + 1;
  g.w2 = g.w1 - F2 + 1;
  g.h2 = g.h1 - F2 + 1;
  g.w3 = g.w2 - F3 + 1;
  g.h3 = g.h2 - F3 + 1;
  g.batch = (int)batch;
  if (g.w > kXS || g.h > kXS || g.w3 <= 0 || g.h3 <= 0) return false;
  const int npx1 = g.w1 * g.h1, npx2 = g.w2 * g.h2;
  // L2 forward / delta1 geometry limits (register tiles, LDS images)
  const CGeom cf = p.cf = {g.w1, g.h1, 0, g.w1, g.h1, g.w2, g.h2, npx2, g.batch, 0, 0, 0};
  const CGeom cd = p.cd = {g.w2, g.h2, F2 - 1, g.w2 + 2 * (F2 - 1), g.h2 + 2 * (F2 - 1), g.w1, g.h1, npx1, g.batch,
                           g.w, g.h, 0};
  if ((npx2 + 31) / 32 > 2 * NetT::MT2 || (npx1 + 31) / 32 > 2 * NetT::MT4) return false;
  if (cf.img_w * cf.img_h > kImgMax || cd.img_w * cd.img_h > kImgMax) return false;
  // wgrad2 bands
  G2Geom& g2 = p.g2;
  g2.w1 = g.w1;
  g2.h1 = g.h1;
  g2.w2 = g.w2;
  g2.h2 = g.h2;
  g2.rows = std::min(8, kBandPx / g.w2);
  if (g2.rows < 1 || (g2.rows + F2 - 1) * g.w1 > kGAPx) return false;
  g2.cols = g.w2;  // full-width bands
  g2.nbx = 1;
  g2.aw = g.w1;
  g2.nbands = (g.h2 + g2.rows - 1) / g2.rows;
  g2.batch = g.batch;
  // the split-bf16 wgrad2 (wgrad2x6) takes fewer sample groups (one block per
  // CU); slab2 is sized for wgrad2's, so it holds either arithmetic's
  const int groups2 = (int)std::min<uint32_t>(batch, 64);
  p.x6g = arith == 0 && F2 == 5 && N2 == 64 && N1 % 16 == 0 && g.w2 <= kG6MaxW2;
  g2.groups = p.x6g ? (int)std::min<uint32_t>(batch, kG6Groups) : groups2;
  p.GG2 = p.x6g ? g2.groups * (N1 / 16) : groups2 * (N1 / 32);
  p.ldsg2 = p.x6g ? kG6Lds : 2 * (size_t)kGBuf * sizeof(float);
  // layer 3.  wl3: Q + the delta3 grid + 2 A2 pixels' worth; wl3l: A2 image
  // + Q + delta3 grid (the reduction reuses the A2 image), and the 160 KiB
  // LDS also holds wl3l's static red_s[2][8] (64 B)
  p.qfloats = std::max(npx2 * F3 * F3, 2 * 16 * 64 * 4);
  const int d3grid = (g.w3 + 2 * (F3 - 1)) * (g.h3 + 2 * (F3 - 1));
  const size_t lds3 = (size_t)(p.qfloats + d3grid + 2 * npx2) * 4;
  if (lds3 > 64 * 1024) return false;
  const size_t lds3l = (size_t)(npx2 * N2 + npx2 * F3 * F3 + d3grid) * 4;
  constexpr size_t kWl3lStaticLds = 2 * 8 * sizeof(float);
  p.wl3l = lds3l + kWl3lStaticLds <= 160 * 1024 && npx2 * N2 >= 2 * 16 * 64 * 8 && g.w3 * g.h3 <= 512;
  p.lds3 = p.wl3l ? lds3l : lds3;
  p.G3 = (int)std::min<uint32_t>(batch, p.wl3l ? 256 : 512);  // all blocks resident
  // L1 forward: split-bf16 wl1x6, else wl1_fwd
  p.rg1 = run_geom(g.w1, g.h1);
  p.x6f = arith == 0 && wl1x6_fits(g.w, g.h, N1, F1);
  p.GL1 = (int)std::min<uint32_t>(batch, 1024);
  p.lds1 = p.x6f ? W1x6Lds(g.w, g.h, p.rg1).bytes : 0;
  // L2 forward: split-bf16 wl2x6 (two split chunk images in LDS), else conv_mfma
  const size_t lds6 = 2 * (size_t)cf.img_h * w6_pitch(cf.img_w, cf.out_w) * sizeof(float);
  p.x6 = arith == 0 && N2 == 64 && N1 % 16 == 0 && cf.img_w * cf.img_h <= kW6ImgMax && lds6 <= 160 * 1024;
  p.GL2 = std::min(p.x6 ? g.batch : g.batch * (N2 / 64), 256);
  p.lds2 = p.x6 ? lds6 : 2 * ((size_t)cf.img_w * cf.img_h * kPS + kImgSlack) * sizeof(float);
  // delta1: split-bf16 wd1x6 into D1, then gW1 by wg1x6 (two blocks per CU)
  // or l1_grad_kernel (4 per CU) over their own slabs; else d1g16 does both
  const size_t lds_d6 = (size_t)cd.img_h * w6_pitch(cd.img_w, cd.out_w) * sizeof(float);
  p.x6d = arith == 0 && N1 % 64 == 0 && N2 % 16 == 0 && cd.img_w * cd.img_h <= kWD6ImgMax &&
          (npx1 + 31) / 32 <= 2 * NetT::MT4 && lds_d6 <= 160 * 1024;
  p.x6g1 = arith == 0 && wg1x6_fits(g.w, g.h, N1, F1);
  constexpr int NPD = N1 / 64;                // delta1 items per sample (64-channel parts)
  p.GD = std::min(g.batch * NPD, 256);        // a multiple of NPD: block parity = part
  const int G1 = p.GD / NPD;                  // d1g16's gW1 slabs: one per block pair
  p.GW1 = (int)std::min<uint32_t>(batch, 1024);
  p.GG1 = (int)std::min<uint32_t>(batch, 512);
  p.nslab1 = p.x6d ? (p.x6g1 ? p.GG1 : p.GW1) : G1;
  // d1g16: + the slot -> pixel table, tile masks, tile order
  p.ldsd = p.x6d ? lds_d6
                 : (2 * ((size_t)cd.img_w * cd.img_h * kPS + kImgSlack) + 2 * kXBuf + kD16Slots + 4 * kD16MT) * sizeof(float);
  p.ldsg1 = p.x6d && p.x6g1 ? G1x6Lds(g.w, g.h, p.rg1).bytes : 0;
  p.nWf = p.nWd = align_f(NetT::W2);
  p.nWx = align_f((size_t)NetT::W2 * 3 / 2);
  p.n1 = align_f((size_t)std::max(G1, p.GW1) * NetT::P1);
  p.n2 = align_f((size_t)groups2 * NetT::P2);
  p.n3 = align_f((size_t)p.G3 * NetT::P3);
  p.nsq = align_f(p.G3);
  p.bytes = (p.nWf + p.nWd + 2 * p.nWx + p.n1 + p.n2 + p.n3 + p.nsq) * sizeof(float);
  return true;
}

// Carves the workspace and launches in order; every decision comes from the
// plan.  Each kernel has one profile scope, under either arithmetic.
template <int N1, int N2, int F1, int F2, int F3>
static int run(const WidePlan& p, const srcnn_net* net, const StepBuffers& b, hipStream_t s,
               const fused::SlabUpdate* up) {
  using NetT = Net<N1, N2, F1, F2, F3>;
  if (b.slab_bytes < p.bytes)
    return fail(SRCNN_ERR_WORKSPACE, "wide train step: workspace %zu B < %zu B", b.slab_bytes, p.bytes);
  float* Wf = b.slab;
  float* Wd = Wf + p.nWf;
  uint16_t* Wx = reinterpret_cast<uint16_t*>(Wd + p.nWd);
  uint16_t* Wx1 = reinterpret_cast<uint16_t*>(Wd + p.nWd + p.nWx);
  float* slab1 = Wd + p.nWd + 2 * p.nWx;
  float* slab2 = slab1 + p.n1;
  float* slab3 = slab2 + p.n2;
  float* sqs = slab3 + p.n3;
  const auto P = split_params(b.params, net);
  const float *X = b.X, *T = b.T;
  float *A1 = b.A1, *D1 = b.D1, *A2 = b.A2, *D2 = b.D2, *A3 = b.A3;
  const WGeom& g = p.g;
  const dim3 blk(256);
  {
    SRCNN_PROFILE("wide_prepack_w2", s);
    auto blocks = [](int tot) { return dim3((tot + 255) / 256); };
    if (int rc = launch(prepack_w2_kernel<N1, N2, F2, true>, blocks(2 * NetT::W2), blk, 0, s, P.W2, Wf, Wd)) return rc;
    if (p.x6)
      if (int rc = launch(wprep_w2x6_kernel<N1, N2, F2>, blocks((N2 / 32) * (N1 / 16) * F2 * F2 * 512), blk, 0, s, P.W2, Wx))
        return rc;
    if (p.x6d)
      if (int rc = launch(wprep_d1x6_kernel<N1, N2, F2>, blocks((N1 / 32) * (N2 / 16) * F2 * F2 * 512), blk, 0, s, P.W2, Wx1))
        return rc;
  }
  {
    SRCNN_PROFILE("wide_l1_fwd", s);
    kernels_note(p.x6f ? "wl1x6_fwd" : "wide_l1_fwd");
    if (int rc = p.x6f ? launch(wl1x6_fwd_kernel, dim3(p.GL1), blk, p.lds1, s, X, P.W1, P.B1, A1, g, p.rg1)
                       : launch(wl1_fwd_kernel<N1, F1>, dim3(p.GL1), blk, 0, s, X, P.W1, P.B1, A1, g))
      return rc;
  }
  {
    SRCNN_PROFILE("wide_l2_fwd", s);
    kernels_note(p.x6 ? "wl2x6_fwd" : "wide_l2_fwd");
    if (int rc = p.x6 ? launch(wl2x6_fwd_kernel<N1, N2, F2, NetT::MT2>, dim3(p.GL2), blk, p.lds2, s, A1, Wx, P.B2, A2, p.cf)
                      : launch(conv_mfma_kernel<N1, N2, F2, NetT::MT2, false>, dim3(p.GL2), blk, p.lds2, s, A1, Wf, P.B2,
                               (const float*)nullptr, A2, p.cf))
      return rc;
  }
  {
    SRCNN_PROFILE("wide_l3_delta", s);
    if (int rc = p.wl3l ? launch(wl3l_kernel<N2, F3>, dim3(p.G3), dim3(512), p.lds3, s, A2, T, P.W3, P.B3, D2, slab3, sqs, A3, g)
                        : launch(wl3_kernel<N2, F3>, dim3(p.G3), blk, p.lds3, s, A2, T, P.W3, P.B3, D2, slab3, sqs, A3, g,
                                 p.qfloats))
      return rc;
  }
  {
    SRCNN_PROFILE(p.x6d ? "wide_delta1" : "wide_delta1_grad1", s);
    kernels_note(p.x6d ? "wd1x6" : "d1g16");
    if (int rc = p.x6d ? launch(wd1x6_kernel<N2, N1, F2, NetT::MT4>, dim3(p.GD), blk, p.ldsd, s, D2, Wx1, D1, p.cd)
                       : launch(d1g16_kernel<N2, N1, F2, F1>, dim3(p.GD), blk, p.ldsd, s, D2, Wd, A1, X, slab1, p.cd))
      return rc;
  }
  if (p.x6d) {
    SRCNN_PROFILE("wide_grad1", s);
    if (p.x6g1) {
      kernels_note("wg1x6");
      if (int rc = launch(wg1x6_kernel, dim3(p.GG1), blk, p.ldsg1, s, X, D1, A1, slab1, g, p.rg1)) return rc;
    } else if (int rc = fast::l1_grad_slabs(X, D1, A1, slab1, N1, F1, g.w, g.h, g.batch, p.GW1, s); rc != 1) {
      return rc ? rc : fail(SRCNN_ERR_INVALID, "wide step: no layer-1 gradient kernel for n1 %d f1 %d", N1, F1);
    }
  }
  {
    SRCNN_PROFILE("wide_grad2", s);
    kernels_note(p.x6g ? "wgrad2x6" : "wgrad2");
    if (int rc = p.x6g ? launch(wgrad2x6_kernel<N1, N2, F2>, dim3(p.GG2), dim3(512), p.ldsg2, s, A1, D2, slab2, p.g2)
                       : launch(wgrad2_kernel<N1, N2, F2>, dim3(p.GG2), dim3(512), p.ldsg2, s, A1, D2, slab2, p.g2))
      return rc;
  }
  SRCNN_PROFILE("slab_reduce", s);
  const fused::SlabSeg segs[4] = {{slab1, b.grads, p.nslab1, NetT::P1},
                                  {slab2, b.grads + NetT::P1, p.g2.groups, NetT::P2},
                                  {slab3, b.grads + NetT::P1 + NetT::P2, p.G3, NetT::P3},
                                  {sqs, b.sq_err, p.G3, 1}};
  // with `up` (srcnn_train_step), segments 0-2 are every parameter
  fused::SlabUpdate u{};
  if (up) {
    u = *up;
    u.nseg = 3;
  }
  if (int rc = fused::reduce_slabs(segs, b.sq_err ? 4 : 3, s, &u)) return rc;
  return up ? 2 : 1;
}

// the one instantiated net: plan, run and preload all ask here
using WideNet = Net<128, 64, 9, 5, 5>;
static const auto plan_wide = plan_step<128, 64, 9, 5, 5>;
static const auto run_wide = run<128, 64, 9, 5, 5>;
static bool is_wide_net(const srcnn_net* net) {
  return net->n1 == 128 && net->n2 == 64 && net->f1 == 9 && net->f2 == 5 && net->f3 == 5;
}

bool train_plan(const srcnn_net* net, uint32_t w, uint32_t h, uint32_t batch, StepNeed* need) {
  WidePlan p;
  if (!is_wide_net(net) || !plan_wide(w, h, batch, g_arith, &p)) return false;
  *need = {p.bytes, fused::kA1Hwc};
  return true;
}

int train_fwd_bwd(const srcnn_net* net, uint32_t w, uint32_t h, uint32_t batch, const StepBuffers& b,
                  hipStream_t s, const fused::SlabUpdate* up) {
  WidePlan p;
  if (!is_wide_net(net) || !plan_wide(w, h, batch, g_arith, &p)) return 0;
  return run_wide(p, net, b, s, up);
}

// ---------------------------------------------------------------------------
// op-level entry points (srcnn_conv_fwd / _delta / _grad_acc through
// ops_fast.hip) for the wide middle layer: 5x5, n1 = 128 <-> n2 = 64, the
// same kernels as the net-level step, over the caller's reference-layout
// buffers.  The operand images of W2 live in a per-(device, stream) buffer
// of the library.  1 = handled,
// 0 = shape not served here, < 0 = error.
// ---------------------------------------------------------------------------
namespace {
constexpr int kWN1 = 128, kWN2 = 64, kWF = 5;

// W2 operand images of the op-level calls: ONE device buffer per device
// (2 x 819 KB), reused in stream order.  A W2Image lease holds the device's
// lock from the prepack launch to the consumer launch; a call on another
// stream than the previous user first waits (hipStreamWaitEvent) for the
// event recorded after that user's consumer kernel, so no two streams ever
// share the image at once and nothing grows with the number of streams.
struct ImgSlot {
  float* buf = nullptr;
  hipEvent_t done = nullptr;  // recorded after the last consumer kernel
  hipStream_t last = nullptr;
  bool used = false;
  std::mutex mu;
};
std::mutex g_img_mu;
std::map<int, ImgSlot> g_img;

class W2Image {
 public:
  // prepacks W2 into the device's image on stream s; rc() < 0 on error
  W2Image(const float* W2, hipStream_t s) : s_(s) { rc_ = acquire(W2); }
  ~W2Image() {
    if (slot_) {
      if (rc_ == SRCNN_OK) {
        (void)hipEventRecord(slot_->done, s_);
        slot_->last = s_;
        slot_->used = true;
      }
      slot_->mu.unlock();
    }
  }
  int rc() const { return rc_; }
  float* img() const { return slot_ ? slot_->buf : nullptr; }

 private:
  int acquire(const float* W2) {
    int dev = 0;
    SRCNN_HIP_TRY(hipGetDevice(&dev));
    {
      std::lock_guard<std::mutex> lk(g_img_mu);
      slot_ = &g_img[dev];  // std::map nodes never move
    }
    slot_->mu.lock();
    if (!slot_->buf) {
      SRCNN_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&slot_->buf),
                              2 * align_f(WideNet::W2) * sizeof(float)));
      SRCNN_HIP_TRY(hipEventCreateWithFlags(&slot_->done, hipEventDisableTiming));
    }
    if (slot_->used && slot_->last != s_) SRCNN_HIP_TRY(hipStreamWaitEvent(s_, slot_->done, 0));
    SRCNN_PROFILE("wide_prepack_w2", s_);
    const int tot = 2 * WideNet::W2;
    hipLaunchKernelGGL((prepack_w2_kernel<kWN1, kWN2, kWF>), dim3((tot + 255) / 256), dim3(256), 0,
                       s_, W2, slot_->buf, slot_->buf + align_f(WideNet::W2));
    SRCNN_LAUNCH_TRY();
    return SRCNN_OK;
  }
  hipStream_t s_;
  ImgSlot* slot_ = nullptr;
  int rc_ = SRCNN_OK;
};
}  // namespace

int op_conv_fwd(const float* in, float* out, const float* W, const float* B, uint32_t in_w,
                uint32_t in_h, uint32_t n_prev, uint32_t n_cur, uint32_t f, int relu,
                uint32_t batch, hipStream_t s) {
  if (n_prev != kWN1 || n_cur != kWN2 || f != kWF || !relu) return 0;
  const int ow = (int)in_w - kWF + 1, oh = (int)in_h - kWF + 1;
  CGeom cf{(int)in_w, (int)in_h, 0, (int)in_w, (int)in_h, ow, oh, ow * oh, (int)batch, 0, 0, 0};
  if ((cf.npx + 31) / 32 > 2 * WideNet::MT2 || cf.img_w * cf.img_h > kImgMax) {
    // larger images: 21x21 output windows (441 pixels of the 448 the register
    // tiles hold; 25x25 = 625 staged pixels)
    cf.wo = 21;
    cf.img_w = std::min(ow, cf.wo) + kWF - 1;
    cf.img_h = std::min(oh, cf.wo) + kWF - 1;
  }
  W2Image w2i(W, s);
  if (w2i.rc()) return w2i.rc();
  float* img = w2i.img();
  const size_t lds = 2 * ((size_t)cf.img_w * cf.img_h * kPS + kImgSlack) * sizeof(float);
  SRCNN_PROFILE("conv_fwd_wide_mfma", s);
  const int items = (int)batch * (kWN2 / 64) * conv_windows(cf);
  if (int rc = launch(conv_mfma_kernel<kWN1, kWN2, kWF, WideNet::MT2, false>, dim3(std::min(items, 256)), dim3(256),
                      lds, s, in, img, B, (const float*)nullptr, out, cf))
    return rc;
  return 1;
}

int op_conv_delta(const float* d_next, const float* y_curr, float* d_curr, const float* W_next,
                  uint32_t f_next, uint32_t n_curr, uint32_t n_next, uint32_t curr_w,
                  uint32_t curr_h, uint32_t batch, hipStream_t s) {
  if (n_curr != kWN1 || n_next != kWN2 || f_next != kWF) return 0;
  const int nw = (int)curr_w - kWF + 1, nh = (int)curr_h - kWF + 1;
  CGeom cd{nw, nh, kWF - 1, nw + 2 * (kWF - 1), nh + 2 * (kWF - 1), (int)curr_w, (int)curr_h,
           (int)(curr_w * curr_h), (int)batch, 0, 0, 0};
  if ((cd.npx + 31) / 32 > 2 * WideNet::MT4 || cd.img_w * cd.img_h > kImgMax) {
    // larger images: 25x25 output windows (625 of the 640 pixels the register
    // tiles hold; 29x29 = 841 staged pixels)
    cd.wo = 25;
    cd.img_w = std::min((int)curr_w, cd.wo) + kWF - 1;
    cd.img_h = std::min((int)curr_h, cd.wo) + kWF - 1;
  }
  W2Image w2i(W_next, s);
  if (w2i.rc()) return w2i.rc();
  float* img = w2i.img();
  const size_t lds = 2 * ((size_t)cd.img_w * cd.img_h * kPS + kImgSlack) * sizeof(float);
  SRCNN_PROFILE("conv_delta_wide_mfma", s);
  const int items = (int)batch * (kWN1 / 64) * conv_windows(cd);
  if (int rc = launch(conv_mfma_kernel<kWN2, kWN1, kWF, WideNet::MT4, true>, dim3(std::min(items, 256)), dim3(256),
                      lds, s, d_next, img + align_f(WideNet::W2), (const float*)nullptr, y_curr, d_curr, cd))
    return rc;
  return 1;
}

namespace {
bool g2_geom(uint32_t out_w, uint32_t out_h, uint32_t batch, G2Geom* g2) {
  g2->w2 = (int)out_w;
  g2->h2 = (int)out_h;
  g2->w1 = g2->w2 + kWF - 1;
  g2->h1 = g2->h2 + kWF - 1;
  // full-width bands where a few whole rows fit the band images, else
  // 16-column x 4-row windows (A1 image 20 x 8 = 160 pixels)
  g2->cols = g2->w2;
  g2->rows = std::min(8, kBandPx / std::max(1, g2->w2));
  if (g2->rows < 1 || (g2->rows + kWF - 1) * g2->w1 > kGAPx) {
    g2->cols = 16;
    g2->rows = kBandPx / 16;
  }
  g2->nbx = (g2->w2 + g2->cols - 1) / g2->cols;
  g2->aw = g2->cols + kWF - 1;
  g2->nbands = g2->nbx * ((g2->h2 + g2->rows - 1) / g2->rows);
  g2->batch = (int)batch;
  g2->groups = (int)std::min<uint32_t>(batch, 64);
  return true;
}
}  // namespace

size_t op_grad_workspace_bytes(uint32_t n_prev, uint32_t n_cur, uint32_t f, uint32_t out_w,
                               uint32_t out_h, uint32_t batch) {
  G2Geom g2;
  if (n_prev != kWN1 || n_cur != kWN2 || f != kWF || !g2_geom(out_w, out_h, batch, &g2)) return 0;
  return (size_t)g2.groups * WideNet::P2 * sizeof(float);
}

int op_conv_grad_acc(const float* in, const float* d, float* gW, float* gB, uint32_t n_prev,
                     uint32_t n_cur, uint32_t f, uint32_t out_w, uint32_t out_h, uint32_t batch,
                     void* ws, size_t ws_bytes, hipStream_t s) {
  G2Geom g2;
  if (n_prev != kWN1 || n_cur != kWN2 || f != kWF || !g2_geom(out_w, out_h, batch, &g2)) return 0;
  const size_t need = (size_t)g2.groups * WideNet::P2 * sizeof(float);
  if (ws_bytes < need)
    return fail(SRCNN_ERR_WORKSPACE, "backpropagate: workspace %zu B < %zu B", ws_bytes, need);
  float* slab2 = static_cast<float*>(ws);
  {
    SRCNN_PROFILE("grad_wide_mfma", s);
    const size_t lds = 2 * (size_t)kGBuf * sizeof(float);
    if (int rc = launch(wgrad2_kernel<kWN1, kWN2, kWF>, dim3(g2.groups * (kWN1 / 32)), dim3(512), lds, s, in, d,
                        slab2, g2))
      return rc;
  }
  {
    SRCNN_PROFILE("slab_reduce", s);
    const int nW = WideNet::W2;
    const fused::SlabSeg segs[2] = {{slab2, gW, g2.groups, nW, WideNet::P2},
                                    {slab2 + nW, gB, g2.groups, kWN2, WideNet::P2}};
    if (int rc = fused::reduce_slabs(segs, 2, s)) return rc;
  }
  return 1;
}

int preload(const srcnn_net* net) {
  if (!is_wide_net(net)) return 0;
  using NetT = WideNet;
  // the training step's kernels (and the op-level delta1 / forward ones)
  const void* k[] = {(const void*)prepack_w2_kernel<128, 64, 5, true>, (const void*)wl1_fwd_kernel<128, 9>,
                     (const void*)conv_mfma_kernel<128, 64, 5, NetT::MT2, false>,
                     (const void*)wl3l_kernel<64, 5>, (const void*)wl3_kernel<64, 5>,
                     (const void*)d1g16_kernel<64, 128, 5, 9>,
                     (const void*)conv_mfma_kernel<64, 128, 5, NetT::MT4, true>,
                     (const void*)prepack_w2_kernel<128, 64, 5>, (const void*)wgrad2_kernel<128, 64, 5>,
                     (const void*)wprep_w2x6_kernel<128, 64, 5>, (const void*)wl2x6_fwd_kernel<128, 64, 5, NetT::MT2>,
                     (const void*)wgrad2x6_kernel<128, 64, 5>, (const void*)wprep_d1x6_kernel<128, 64, 5>,
                     (const void*)wd1x6_kernel<64, 128, 5, NetT::MT4>, (const void*)wl1x6_fwd_kernel,
                     (const void*)wg1x6_kernel};
  int rc = resolve_kernels(k, 16);
  return rc ? rc : 1;
}

}  // namespace wide
}  // namespace srcnn
