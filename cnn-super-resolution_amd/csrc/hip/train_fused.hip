// train_fused.hip -- gfx950 fused training step for SRCNN nets with a 1x1
// middle layer (f2 == 1), e.g. the reference default n1=64, n2=32, f1=9, f3=5.
//
// The reference runs one OpenCL kernel per op (ConfigBasedDataPipeline.cpp:
// 200-323): 3 forward, last delta, 2 deltas, 3 gradient kernels, every tensor
// round-tripping through global memory and the gradients summed serially per
// weight (backpropagate.cl:89-106).  Here the same mathematics runs as three
// kernels plus a deterministic reduction:
//
//   l12_fwd      L1 (f1 x f1 x 1 -> n1) and L2 (1x1, n1 -> n2) as fp32 MFMA
//                implicit GEMMs per 32-pixel chunk; A1 goes to HBM (needed by
//                backward) and through a per-wave LDS transpose into L2.
//   l3_delta     per sample: A2 tile in LDS; L3 (f3 x f3 x n2 -> 1, MFMA Q trick),
//                last-layer delta with the reference quirk, delta2 (MFMA over
//                the 25 taps), gW3 (MFMA over pixels), gB3, squared error.
//   d1_grad12    delta1 = relu'(A1) * (delta2 . W2^T) (MFMA), then gW2 and gW1
//                consume delta1 / A1 straight from the accumulator registers
//                (mfma.hpp: k-slot <-> pixel pairing), gB1 via a ones row.
//   slab_reduce  per-block partial gradients summed in block order -> grads.
//
// HBM traffic per 33x33 tile: X 4.4 KB + A1 160 KB (write + read) + A2 80 KB
// (write + read) + delta2 80 KB (write + read) ~ 650 KB vs 1.54 MB for the
// layer-by-layer dataflow.  Results are deterministic: the
// sample -> block -> wave assignment is static and every sum has a fixed
// order; no float atomics anywhere.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "common.hpp"
#include "lds_dma.hpp"
#include "mfma.hpp"
#include "ops.hpp"
#include "split.hpp"

namespace srcnn {
namespace fused {

using mfma::crow;
using mfma::f32x16;
using mfma::f32x4;
using mfma::mma;
using mfma::zero16;

constexpr int kXsMax = 1536;  // input sample / region tile (floats) staged in LDS (<= 39x39)
// l12_fwd X tile in LDS: rows at the fixed stride kL12S (w <= kL12S, h <= kL12Rows).
// A chunk's 32 consecutive L1 pixels (flattened over ow) gather from banks
// (row * kL12S + col) mod 32 (ds_read_b32 banks 32 lanes at a time), which
// is (pixel index + const) mod 32 -- 32 distinct banks -- when kL12S == ow
// (mod 32): 57 = 25 + 32 makes the default 33x33 tile (ow 25) conflict-free.
constexpr int kL12S = 57;
constexpr int kL12Rows = 40;
constexpr int kL12Tile = kL12S * (kL12Rows + 1);  // + a zero row read by the padded tap
constexpr int kL12Regs = (kXsMax + 255) / 256;    // register-staged X tile (w * h <= kXsMax)

struct Geom {
  int W, H;      // input sample
  int ow, oh;    // L1 (and L2) output
  int batch;
};

// ---------------------------------------------------------------------------
// Kernel 1: L1 (+ L2) forward, one sample per work item
// ---------------------------------------------------------------------------
// Both layers run TRANSPOSED (rows = channels, cols = the chunk's 32 pixels):
//   L1^T: A1^T[ch][p] = sum_tap W1[tap][ch] X[p + off(tap)]   A = W1 (registers),
//         B = X gathers from LDS; the padded k-slot (tap 81) reads 1.0 against
//         B1, so the bias rides in the GEMM
//   L2^T: A2^T[n][p] = sum_c W2[c][n] A1^T[c][p]   B = the L1 accumulator
//         registers as they stand (register s of half h is channel crow(s, h),
//         mfma.hpp), A = W2 (registers); one extra MFMA adds B2
// so L2 needs no LDS transpose at all, and each lane ends with consecutive
// channels of ONE pixel: A1 / A2 leave as 16-B stores straight from registers.
// held-clock probe slots (common.hpp): 0 l12_fwd, 1 l3_delta, 2 d1_grad12
__device__ unsigned long long g_clk[3][kClockBlocks][2];

// streaming-cache hints (bits): 1 l3 A2 DMA nt, 2 l3 D2 stores nt, 4 d1
// operand DMA nt, 8 l12 A1 stores nt.  Default 1 | 8 (same-box A/B, steady
// state, 2 reps: step 0.938 -> 0.931 ms): A1 (655 MB per step, read back only
// by d1) streams past the caches, so more of the A2 that l12 writes just
// before l3 reads it stays in the 256 MB MALL (l3 -4.5%); nt on the D2
// stores or the d1 DMA was slower.
constexpr int kNtMask = 9;
// L1 X-gather prefetch distance (k-steps), pinned by sched barriers
constexpr int kL12PD = 4;
// grid caps (blocks): 256 CUs x 2 resident blocks.  l12 writes the samples
// in index order, which l3 reads back in reverse (MALL)
constexpr int kL12Grid = 512, kL3RGrid = 512;
// A2 leaves l12 as whole 128-B pixel rows (n2 = 32): at each chunk end the
// wave regroups its A2 tile through a 4.6 KB LDS scratch into row order (one
// write and one read per quad, a single LDS round trip per chunk), and the
// stores inside the next chunk's MFMA stream write 1 KB contiguous each.  As
// held, each store wrote 32 rows x 32 B; those stores cost 6% of l12
// (round-4 diagnostic build).  Same-box A/B (profiles/r04_ab_a2rows): l12
// 0.3068 -> 0.3049 ms, l3 0.1559 -> 0.1547 ms, step 0.8668 -> 0.8641 ms at
// batch 4096; the 512-tile shard unchanged (l12 +0.4 us)
constexpr int kL12A2S = 36;  // A2 scratch row stride (floats)
// kLazy (srcnn_train_fwd_bwd_lazy): the previous data-parallel step's SGD
// update rides in the prologue.  Every block forms the updated W1 / B1 / W2 /
// B2 it needs in registers from lz's (P, M, G) -- the same sgd_step as
// update_all_kernel, so every block holds the same values -- and writes its
// slice of the updated parameters and momentum (all six segments) to lz.Po /
// lz.Mo, which l3 and d1 read after this kernel.  No update launch between
// the gradient all-reduce and the next step.
template <int N1, int N2, int F1, bool kLazy = false>
__global__ __launch_bounds__(256, 2) void l12_fwd_kernel(
    const float* __restrict__ X, const float* __restrict__ W1, const float* __restrict__ B1,
    const float* __restrict__ W2, const float* __restrict__ B2, float* __restrict__ A1,
    float* __restrict__ A2, Geom g, LazyUpdate lz) {
  constexpr int K1 = F1 * F1, KS1 = (K1 + 1) / 2, NT1 = N1 / 32;
  static_assert(N2 <= 32 && N2 % 8 == 0 && K1 % 2 == 1 && N1 % 32 == 0,
                "transposed l12: one 32-row L2 tile, odd tap count");
  __shared__ float xs[kL12Tile];  // X tile at the fixed row stride kL12S (+ zero rows)
  constexpr bool kA2Rows = N2 == 32;  // (a row = 8 quads)
  __shared__ __attribute__((aligned(16))) float a2sc[kA2Rows ? 4 * 32 * kL12A2S : 4];
  // L2 bias as the accumulator's initial value: register r of half h is
  // channel crow(r, h) (one 16x32 image, read as 4 broadcast 16-B loads)
  // instead of one more MFMA (b2 x 1) per chunk; the same fp32 values
  __shared__ __attribute__((aligned(16))) float b2i[2][16];

  SRCNN_CLOCK_BEGIN();
  const int lane = mfma::lane_id(), wave = mfma::wave_id();
  const int h = lane >> 5, li = lane & 31;
  const int npx = g.ow * g.oh;
  const int nch = (npx + 31) / 32;
  // The next sample's X tile is register-staged during the current sample
  // (its loads retire under the MFMAs instead of stalling both barriers);
  // the LDS copy uses a fixed row stride so every L1 B operand is a per-half
  // base + immediate (tap 2s+1 sits 1 or kL12S - F1 + 1 floats past tap 2s).
  for (int i = threadIdx.x; i < kL12Tile; i += blockDim.x) xs[i] = 0.0f;
  const int xn = g.W * g.H;
  float xr[kL12Regs];
  auto xload = [&](int smp) {
    const float* src = X + (size_t)smp * xn;
#pragma unroll
    for (int k = 0; k < kL12Regs; k++) {
      const int i = threadIdx.x + 256 * k;
      xr[k] = i < xn ? src[i] : 0.0f;
    }
  };
  // (issued first: its loads are in flight under the parameter loads)
  if ((int)blockIdx.x < g.batch) xload(blockIdx.x);
  // kLazy: the updated W1 | B1 | W2 | B2 (the flat buffer's first P12
  // floats) are formed once per block into LDS, each by one thread with
  // coalesced loads; the register operands below are read from there
  constexpr int P12 = F1 * F1 * N1 + N1 + N1 * N2 + N2;
  __shared__ float lzs[kLazy ? P12 : 1];
  if constexpr (kLazy) {
    // every load of the thread in flight at once (a rolled loop waited out
    // one L2 round trip per element: l12 +9 us at one sample per block)
    constexpr int kIt = (P12 + 255) / 256;
    float lw[kIt], lm[kIt], lgr[kIt];
#pragma unroll
    for (int k = 0; k < kIt; k++) {
      const int i = threadIdx.x + 256 * k;
      if (i < P12) {
        lw[k] = lz.P[i];
        lm[k] = lz.M[i];
        lgr[k] = lz.G[i];
      }
    }
    lazy_write_slice(lz);
#pragma unroll
    for (int k = 0; k < kIt; k++) {
      const int i = threadIdx.x + 256 * k;
      if (i < P12) {
        const int seg = param_seg(lz.off, i);
        sgd_step(lw[k], lm[k], seg, lgr[k], lz.lr[seg >> 1], lz.mu, lz.wd, lz.batch);
        lzs[i] = lw[k];
      }
    }
    __syncthreads();
  }
  // parameter i of segment seg (W1 0, B1 1, W2 2, B2 3) as this step uses it
  auto prm = [&](int seg, int i) -> float {
    if constexpr (kLazy) return lzs[(seg > 0 ? K1 * N1 : 0) + (seg > 1 ? N1 : 0) + (seg > 2 ? N1 * N2 : 0) + i];
    return (seg == 0 ? W1 : seg == 1 ? B1 : seg == 2 ? W2 : B2)[i];
  };

  // A operands of L1^T: W1[tap = 2s + h][ch = 32t + li]; tap K1 is the bias slot
  // (W1 in registers: read from LDS at each MFMA instead, for a third wave
  // per SIMD, l12 ran 0.323-0.325 vs 0.307 ms)
  float w1f[KS1][NT1];
#pragma unroll
  for (int s = 0; s < KS1; s++)
#pragma unroll
    for (int t = 0; t < NT1; t++) {
      const int tap = 2 * s + h;
      w1f[s][t] = tap < K1 ? prm(0, tap * N1 + 32 * t + li) : prm(1, 32 * t + li);
    }
  // A operands of L2^T: W2[c = 32t + crow(s, h)][n = li]; bias MFMA: B2[li] (half 0)
  float w2f[NT1][16];
#pragma unroll
  for (int t = 0; t < NT1; t++)
#pragma unroll
    for (int s = 0; s < 16; s++) w2f[t][s] = li < N2 ? prm(2, (32 * t + crow(s, h)) * N2 + li) : 0.0f;
  if (threadIdx.x < 32) {
    const int c_ = crow(threadIdx.x & 15, threadIdx.x >> 4);
    b2i[threadIdx.x >> 4][threadIdx.x & 15] = c_ < N2 ? prm(3, c_) : 0.0f;
  }

  for (int sample = blockIdx.x; sample < g.batch; sample += gridDim.x) {
    __syncthreads();  // previous sample's readers are done with xs
#pragma unroll
    for (int k = 0; k < kL12Regs; k++) {
      const int i = threadIdx.x + 256 * k;
      if (i < xn) {
        const int y = i / g.W;
        xs[y * kL12S + i - y * g.W] = xr[k];
      }
    }
    __syncthreads();
    if (sample + (int)gridDim.x < g.batch) xload(sample + gridDim.x);

    // Software-pipelined stores: chunk c's A1 / A2 rows (12 16-B stores per
    // lane) are issued one at a time inside chunk c+1's L1 MFMA stream, so
    // the write traffic streams out under the matrix core instead of in a
    // burst that stalls the wave between chunks.
    constexpr int NST = 4 * NT1 + N2 / 8;  // 16-B stores per lane per chunk
    f32x16 pa1[NT1], pa2 = zero16();
#pragma unroll
    for (int t = 0; t < NT1; t++) pa1[t] = zero16();
    bool pok = false;    // a chunk is pending (wave-uniform)
    bool pval = false;   // ... and this lane's pixel is inside the sample (A2)
    float* pa1p = A1;
    float* pa2p = A2;
    int pc0 = 0;  // kA2Rows: the pending chunk's first pixel
    auto store_prev = [&](int k) {  // store k of the pending chunk (exec-masked)
      if (pok) {
        if (k < 4 * NT1) {
          // blocked A1 (internal to the fused step, read only by d1): block k
          // of a chunk is 64 lanes x 16 B in lane order, one contiguous 1-KB
          // store; lanes past the sample store their clamped pixel's copy
          const int t = k / 4, q = k % 4;
          if (kNtMask & 8) {
            f32x4 v_;
#pragma unroll
            for (int e = 0; e < 4; e++) v_[e] = pa1[t][4 * q + e];
            __builtin_nontemporal_store(v_, reinterpret_cast<f32x4*>(pa1p + 256 * k));
          } else {
            *reinterpret_cast<float4*>(pa1p + 256 * k) =
                make_float4(pa1[t][4 * q], pa1[t][4 * q + 1], pa1[t][4 * q + 2], pa1[t][4 * q + 3]);
          }
        } else if (kA2Rows && k >= 4 * NT1) {
          // row store q: pixels 8q .. 8q + 7 of the chunk, lane L -> pixel
          // 8q + L / 8, quad L % 8 (already relu'd, in pa2's quad q)
          const int q = k - 4 * NT1;
          if (pc0 + 8 * q + (lane >> 3) < npx) {
            f32x4 v_;
#pragma unroll
            for (int e = 0; e < 4; e++) v_[e] = pa2[4 * q + e];
            *reinterpret_cast<f32x4*>(pa2p + (8 * q + (lane >> 3)) * N2 + 4 * (lane & 7)) = v_;
          }
        } else if (!kA2Rows && k >= 4 * NT1 && pval) {
          const int q = k - 4 * NT1;
          *reinterpret_cast<float4*>(pa2p + 8 * q) =
              make_float4(fmaxf(pa2[4 * q], 0.0f), fmaxf(pa2[4 * q + 1], 0.0f),
                          fmaxf(pa2[4 * q + 2], 0.0f), fmaxf(pa2[4 * q + 3], 0.0f));
        }
      }
    };
    for (int c = wave; c < nch; c += 4) {
      // this lane's pixel (B-operand column li)
      const int pl = c * 32 + li;
      const int pc = min(pl, npx - 1);
      const int iy = pc / g.ow, ix = pc - iy * g.ow;
      const int xbA = iy * kL12S + ix + h, xbB = xbA + h * (kL12S - F1);

      f32x16 acc1[NT1];
#pragma unroll
      for (int t = 0; t < NT1; t++) acc1[t] = zero16();
      constexpr int kStoreEvery = (KS1 - 1) / NST;
      // B operand of k-step s (tap K1 = the bias slot)
      auto xg = [&](int s) {
        const int k0 = 2 * s;
        const int o0 = (k0 / F1) * kL12S + (k0 % F1);
        const float v = xs[((k0 % F1) + 1 < F1 ? xbA : xbB) + o0];
        return s == KS1 - 1 ? (h ? 1.0f : v) : v;
      };
      // gathers run kL12PD k-steps ahead of their MFMAs, pinned by sched
      // barriers: left alone, the scheduler issues each one just before its
      // MFMA pair and the wave waits out the full LDS latency every step
      float xq[KS1];
#pragma unroll
      for (int s = 0; s < kL12PD && s < KS1; s++) xq[s] = xg(s);
#pragma unroll
      for (int s = 0; s < KS1; s++) {
        if (s + kL12PD < KS1) xq[s + kL12PD] = xg(s + kL12PD);
        if (kL12PD > 0) __builtin_amdgcn_sched_barrier(0);
        const float xv = kL12PD > 0 ? xq[s] : xg(s);
#pragma unroll
        for (int t = 0; t < NT1; t++) acc1[t] = mma(w1f[s][t], xv, acc1[t]);
        if (s % kStoreEvery == kStoreEvery - 1 && s / kStoreEvery < NST) store_prev(s / kStoreEvery);
      }
      // ReLU (layer_uber_kernel.cl:88-95); the bias is already in
#pragma unroll
      for (int t = 0; t < NT1; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc1[t][r] = fmaxf(acc1[t][r], 0.0f);
      f32x16 acc2;
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const f32x4 v_ = *reinterpret_cast<const f32x4*>(&b2i[h][4 * q]);
#pragma unroll
        for (int e = 0; e < 4; e++) acc2[4 * q + e] = v_[e];
      }
#pragma unroll
      for (int t = 0; t < NT1; t++)
#pragma unroll
        for (int s = 0; s < 16; s++) acc2 = mma(w2f[t][s], acc1[t][s], acc2);
      // this chunk becomes the pending one; registers 4q..4q+3 of tile t are
      // channels 32t + 8q + 4h .. +3 of pixel pl
#pragma unroll
      for (int t = 0; t < NT1; t++) pa1[t] = acc1[t];
      if (kA2Rows) {
        // A2 tile -> row order through this wave's scratch: register 4m + e
        // of half h is channel 8m + 4h + e of pixel li (written relu'd); read
        // back, quad q of this lane is pixel 8q + lane/8, channels 4 (lane%8)..
        float* sc = a2sc + wave * 32 * kL12A2S;
#pragma unroll
        for (int m = 0; m < 4; m++) {
          f32x4 v_;
#pragma unroll
          for (int e = 0; e < 4; e++) v_[e] = fmaxf(acc2[4 * m + e], 0.0f);
          *reinterpret_cast<f32x4*>(sc + li * kL12A2S + 8 * m + 4 * h) = v_;
        }
        // other lanes' values are read back: no compiler motion across this
        // point (the wave's LDS operations themselves complete in order)
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const f32x4 v_ = *reinterpret_cast<const f32x4*>(sc + (8 * q + (lane >> 3)) * kL12A2S + 4 * (lane & 7));
#pragma unroll
          for (int e = 0; e < 4; e++) pa2[4 * q + e] = v_[e];
        }
        pc0 = c * 32;
      } else {
        pa2 = acc2;
      }
      pok = true;
      pval = pl < npx;
      pa1p = A1 + ((size_t)sample * nch + c) * (32 * N1) + 4 * lane;
      pa2p = kA2Rows ? A2 + ((size_t)sample * npx + c * 32) * N2 : A2 + ((size_t)sample * npx + pc) * N2 + 4 * h;
    }
#pragma unroll
    for (int k = 0; k < NST; k++) store_prev(k);
    pok = false;
  }
  SRCNN_CLOCK_END(g_clk, 0);
}

#include "runs.hpp"
#include "d3taps.hpp"
#include "d6tr.hpp"
#include "l12x6.hpp"
#include "d1x6.hpp"
#include "l3_delta.hpp"
#include "l3r.hpp"

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
#include "d1c.hpp"

// ---------------------------------------------------------------------------
// deterministic slab reduction: dst[i] += sum_b slab[b][i] in a fixed order
// ---------------------------------------------------------------------------
// Fixed-order sums of the per-block gradient slabs of up to kMaxSlabSegs
// kernels in one launch: blocks [first[k], first[k+1]) serve segment k,
// kSlabCols columns each, 64 row lanes per column (enough blocks to spread
// over every CU).  SlabSeg / reduce_slabs are declared in ops.hpp.
constexpr int kSlabCols = 32;  // wide net slab reduce 42 -> 33 us at 32 vs 16; fused neutral (same-box A/B)
constexpr int kSlabRows = 1024 / kSlabCols;
constexpr int kSlabInflight = 8;  // 16 / 32 loads in flight measured slower
struct SlabSegs {
  SlabSeg seg[kMaxSlabSegs];
  int first[kMaxSlabSegs + 1];
  SlabUpdate up;  // up.nseg = 0: plain reduction
  int assign;     // segments k < assign: dst = sum (srcnn_train_fwd_bwd_lazy) instead of dst += sum
};

__global__ __launch_bounds__(1024) void slab_reduce_kernel(SlabSegs ss) {
  __shared__ float part[kSlabRows][kSlabCols + 1];
  int k = 0;
  while (k < kMaxSlabSegs - 1 && (int)blockIdx.x >= ss.first[k + 1]) k++;
  const SlabSeg sg = ss.seg[k];
  const int cl = threadIdx.x % kSlabCols, row = threadIdx.x / kSlabCols;
  const int col = ((int)blockIdx.x - ss.first[k]) * kSlabCols + cl;
  const size_t stride = sg.stride ? sg.stride : sg.P;
  // srcnn_train_step: the finishing lanes load their parameter, momentum and
  // gradient before the slab loads, so the update waits on no fresh load
  const bool upd = k < ss.up.nseg && row == 0 && col < sg.P;
  const uint32_t ui = upd ? (uint32_t)(sg.dst - ss.up.G) + col : 0;
  float uw = 0.0f, um = 0.0f, ug = 0.0f;
  if (upd) {
    uw = ss.up.P[ui];
    um = ss.up.M[ui];
    ug = ss.up.G[ui];
  }
  float acc = 0.0f;
  if (col < sg.P) {
    // kSlabInflight loads in flight per thread, summed in slab order
    int b = row;
    for (; b + (kSlabInflight - 1) * kSlabRows < sg.nslab; b += kSlabInflight * kSlabRows) {
      float v[kSlabInflight];
#pragma unroll
      for (int j = 0; j < kSlabInflight; j++) v[j] = sg.slab[(size_t)(b + j * kSlabRows) * stride + col];
#pragma unroll
      for (int j = 0; j < kSlabInflight; j++) acc += v[j];
    }
    for (; b < sg.nslab; b += kSlabRows) acc += sg.slab[(size_t)b * stride + col];
  }
  part[row][cl] = acc;
  __syncthreads();
  if (row == 0 && col < sg.P) {
    float t = 0.0f;
#pragma unroll 8
    for (int r = 0; r < kSlabRows; r++) t += part[r][cl];
    if (upd) {
      // this element's gradient is complete, so its SGD step runs here (the
      // same arithmetic as update_all_kernel)
      const SlabUpdate& u = ss.up;
      int seg = 0;
#pragma unroll
      for (int j = 1; j < 6; j++) seg += ui >= u.off[j];
      sgd_step(uw, um, seg, ug + t, u.lr[seg >> 1], u.mu, u.wd, u.batch);
      u.P[ui] = uw;
      u.M[ui] = um;
      u.G[ui] = 0.0f;
    } else if (k < ss.assign) {
      sg.dst[col] = t;
    } else {
      sg.dst[col] += t;
    }
  }
}

int reduce_slabs(const SlabSeg* segs, int nseg, hipStream_t s, const SlabUpdate* up, int assign) {
  SlabSegs ss{};
  if (up) ss.up = *up;
  ss.assign = assign;
  int blocks = 0;
  for (int k = 0; k < kMaxSlabSegs; k++) {
    ss.first[k] = blocks;
    if (k < nseg) {
      ss.seg[k] = segs[k];
      blocks += (segs[k].P + kSlabCols - 1) / kSlabCols;
    } else {
      ss.seg[k] = SlabSeg{nullptr, nullptr, 0, 0, 0};
    }
  }
  ss.first[kMaxSlabSegs] = blocks;
  hipLaunchKernelGGL(slab_reduce_kernel, dim3(blocks), dim3(1024), 0, s, ss);
  SRCNN_LAUNCH_TRY();
  return SRCNN_OK;
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
template <int N1_, int N2_, int F1_, int F3_>
struct Net {
  static constexpr int N1 = N1_, N2 = N2_, F1 = F1_, F3 = F3_;
  static constexpr int P12 = F1 * F1 * N1 + N1 + N1 * N2 + N2;
  static constexpr int P3 = F3 * F3 * N2 + 1;
  // layers 1-2 of the default net: the split-bf16 pair and d1c are built for them
  static constexpr bool kDefault12 = N1 == 64 && N2 == 32 && F1 == 9;
};

// The instantiated nets, once: f(Net<..>{}) of the one that `net` is, else 0.
// plan, run and preload all dispatch through here.
template <typename F, typename... Ns>
static int first_net(const srcnn_net* net, F&& f, Ns... ns) {
  int rc = 0;
  auto is = [&](auto n) {
    return net->n1 == (uint32_t)n.N1 && net->n2 == (uint32_t)n.N2 && net->f1 == (uint32_t)n.F1 &&
           net->f2 == 1 && net->f3 == (uint32_t)n.F3;
  };
  (void)((is(ns) && (rc = f(ns), true)) || ...);
  return rc;
}
template <typename F>
static int with_net(const srcnn_net* net, F&& f) {
  return first_net(net, f, Net<64, 32, 9, 5>{},  // reference default (BASELINE.json configs[1])
                   Net<32, 16, 9, 5>{},          // example_config.json
                   Net<64, 32, 9, 3>{}, Net<32, 16, 9, 3>{});  // the same with a 3x3 last layer
}

static int grid_for_batch(uint32_t batch, int cap) { return (int)std::min<uint32_t>(batch, cap); }

// Everything the step decides before its first launch.  plan_step fills it
// from the shape and the arithmetic alone: no buffer, no HIP call.
struct StepPlan {
  int ow, oh, w3, h3;
  // x6: split-bf16 l12x6 + d1x6.  l3r / l3_fused: layer 3 by l3r_delta, else
  // by l3_delta, else (not l3_fused) by the op-level kernels.  d3mode: l3r
  // leaves delta3 and layer 2's relu' mask in the D2 region and d1x6 forms
  // delta2 (d1x6.hpp kD3).  kD1c: the fp32 delta1 kernel is d1c, split over
  // d1c_parts ranges of chunks per sample.
  bool x6, l3r, l3_fused, d3mode, kD1c;
  bool d1tr;                 // d3mode: d1x6 with the delta2 part images (D6Lds::tr)
  int d1c_parts;
  RunGeom rg;
  int g12, g3, gd;           // grids of l12, layer 3 and delta1 (one slab per block of the last two)
  size_t lds12, lds3, ldsd;  // their dynamic LDS bytes
  size_t s12, s3, ssq;       // slab regions in floats: layers 1-2 | layer 3 | squared error
  size_t bytes;              // the three in bytes
  size_t m2_off;             // d3mode: dwords from D2 to the mask (delta3 first, 256-B aligned)
  int a1_layout;             // what l12 writes: kA1Runs or kA1Blocked
};

template <typename NetT>
static bool plan_step(uint32_t w, uint32_t h, uint32_t batch, int arith, StepPlan* out) {
  constexpr int N2 = NetT::N2, F1 = NetT::F1, F3 = NetT::F3;
  StepPlan& p = *out = {};
  const int ow = p.ow = w - F1 + 1, oh = p.oh = h - F1 + 1;
  const int w3 = p.w3 = ow - F3 + 1, h3 = p.h3 = oh - F3 + 1;
  if ((int)(w * h) > kXsMax || (int)w > kL12S || (int)h > kL12Rows || w3 <= 0 || h3 <= 0) return false;
  // l3_delta holds two A2 tiles in LDS: up to 640 A2 pixels (33x33 tiles at
  // f1 = 9).  Larger tiles (e.g. the reference's 36x36 samples, profile.py:7)
  // keep l12 and d1 and run layer 3 through the op-level kernels instead
  // (ops_fast.hip: L3 forward, last delta, delta2, gW3 over HWC A2 / A3 / D3).
  // n2 = 32: l3r (A2 in registers, two blocks per CU) where the tile fits it
  p.l3r = N2 == 32 && l3r_fits<F3>(ow, oh, w3, h3);
  p.lds3 = p.l3r ? L3RLds<F3>(ow, oh).bytes() : l3_lds_bytes<N2, F3>(ow, oh);
  // (n2 = 32 tiles past l3r's 512 outputs, e.g. f3 = 3 on 33x33: l3_delta)
  p.l3_fused =
      p.l3r || (p.lds3 <= 160 * 1024 && w3 * h3 <= kL3MaxOut &&
                ((ow * oh + 15) / 16 + kL3Threads / 64 - 1) / (kL3Threads / 64) <= L3Lds<N2, F3>::kUnitsPerWave);
  p.g12 = grid_for_batch(batch, kL12Grid);
  // split-bf16 products (l12x6.hpp, d1x6.hpp) serve the default net where both fit
  p.x6 = NetT::kDefault12 && arith == 0 && l12x6_fits(w, h) && d1x6_fits(w, h);
  p.a1_layout = p.x6 ? kA1Runs : kA1Blocked;
  p.rg = run_geom(ow, oh);
  // l3r: up to 2 resident blocks per CU; between 256 and 1024 samples keep
  // two samples per block, so the second sample's A2 loads run under the first
  // one's delta2 phase (512 tiles: l3 0.0306 -> 0.0295 ms; at batch 4096 a
  // 256-block grid is slower, 0.155 -> 0.167 ms; profiles/r04_ab_l3rgrid)
  const int b3 = (int)batch;
  p.g3 = p.l3r ? std::min(kL3RGrid, std::max(std::min(b3, 256), (b3 + 1) / 2)) : grid_for_batch(batch, 256);
  p.kD1c = NetT::kDefault12 && d1c_fits(w, h);
  // d1c below kD1cGrid samples: each sample's chunks split into `parts`
  // ranges (work items), so the grid still fills every CU's 4 block slots
  const int nch1 = (ow * oh + 31) / 32;
  p.d1c_parts = p.kD1c ? std::max(1, std::min({4, nch1, kD1cGrid / (int)std::max<uint32_t>(batch, 1)})) : 1;
  while (p.d1c_parts > 1 && (p.d1c_parts - 1) * ((nch1 + p.d1c_parts - 1) / p.d1c_parts) >= nch1)
    p.d1c_parts--;  // every part holds at least one chunk (the kernel's DMA pipeline assumes it)
  // split-bf16 with l3r: delta2 is formed in d1x6 from l3r's delta3, where
  // delta3 and the mask (one dword per A2 pixel) fit the region sized for
  // delta2 (ow * oh * N2 floats per sample)
  p.m2_off = ((size_t)batch * w3 * h3 + 63) & ~(size_t)63;
  p.d3mode = p.x6 && p.l3r && F3 <= 5 && d1x6_fits(w, h, true) && l3r_d3_fits<F3>(ow, oh) &&
             p.m2_off + (size_t)batch * ow * oh <= (size_t)batch * ow * oh * N2;
  const int gd6 = grid_for_batch(batch, 256);  // d1x6
  const int gdf = p.kD1c ? (int)std::min<size_t>((size_t)batch * p.d1c_parts, kD1cGrid) : grid_for_batch(batch, 512);
  p.gd = p.x6 ? gd6 : gdf;
  p.lds12 = p.x6 ? H6Lds(w, h).bytes : 0;
  const D6Lds ld6(w, h, p.rg, p.d3mode);
  p.ldsd = p.x6 ? ld6.bytes : p.kD1c ? d1c_lds_bytes(w, h) : 0;
  // d1x6 in delta3 mode: its form with the delta2 part images (d6tr.hpp) where
  // D6Lds has room for them
  p.d1tr = p.x6 && p.d3mode && ld6.tr;
  // (the workspace holds either arithmetic's slabs: srcnn_set_arith between
  // the size query and the step needs no new query)
  p.s12 = (size_t)std::max(gd6, gdf) * NetT::P12;
  p.s3 = (size_t)p.g3 * NetT::P3;  // gW3 slabs
  p.ssq = p.g3;
  if (!p.l3_fused) {  // the op-level gW3 slabs; the same space serves the squared-error reduction
    p.s3 = fast::grad_workspace_bytes(N2, 1, F3, w3, h3, batch) / sizeof(float);
    if (p.s3 == 0) return false;  // the op-level layer-3 kernels do not take this tile either
    p.s3 = std::max<size_t>(p.s3, reduce_blocks((size_t)batch * w3 * h3) + 1);
    p.ssq = 0;
  }
  p.bytes = (p.s12 + p.s3 + p.ssq) * sizeof(float);
  return true;
}

// the A1 region and layout this thread's last step wrote (a1_layout_written:
// srcnn_train_activations)
static thread_local const float* t_a1_region = nullptr;
static thread_local int t_a1_layout = -1;

// Carves the slab and launches in order; every decision comes from the plan.
template <typename NetT>
static int run(const StepPlan& p, const srcnn_net* net, uint32_t w, uint32_t h, uint32_t batch,
               const StepBuffers& b, hipStream_t s, const SlabUpdate* up, const LazyUpdate* lz) {
  constexpr int N1 = NetT::N1, N2 = NetT::N2, F1 = NetT::F1, F3 = NetT::F3;
  if (b.slab_bytes < p.bytes)
    return fail(SRCNN_ERR_WORKSPACE, "fused train step: slab workspace %zu B < %zu B", b.slab_bytes, p.bytes);
  float* slab12 = b.slab;
  float* slab3 = slab12 + p.s12;
  float* sqs = slab3 + p.s3;
  const float *X = b.X, *T = b.T;
  float *grads = b.grads, *A1 = b.A1, *A2 = b.A2, *D2 = b.D2, *A3 = b.A3;
  // lazy: l12 applies the pending update and the step runs on lz->Po
  const bool lazy = lz && lz->batch > 0.0f;
  const LazyUpdate lu = lazy ? *lz : LazyUpdate{};
  const auto P = split_params(lazy ? lz->Po : b.params, net);
  const int ow = p.ow, oh = p.oh, w3 = p.w3, h3 = p.h3;
  const Geom g{(int)w, (int)h, ow, oh, (int)batch};
  {
    SRCNN_PROFILE("l12_fwd_mfma", s);
    kernels_note(p.x6 ? (lazy ? "l12x6_fwd_lazy" : "l12x6_fwd") : lazy ? "l12_fwd_lazy" : "l12_fwd");
    note_a1_layout(A1, p.a1_layout);
    const dim3 grid(p.g12), blk(256);
    // l12x6: 78 KB of LDS for 33x33 tiles, two blocks per CU
    int rc = p.x6 ? (lazy ? launch(l12x6_fwd_kernel<true>, grid, blk, p.lds12, s, X, P.W1, P.B1, P.W2, P.B2, A1, A2, g, p.rg, lu)
                          : launch(l12x6_fwd_kernel<false>, grid, blk, p.lds12, s, X, P.W1, P.B1, P.W2, P.B2, A1, A2, g, p.rg, lu))
                  : (lazy ? launch(l12_fwd_kernel<N1, N2, F1, true>, grid, blk, 0, s, X, P.W1, P.B1, P.W2, P.B2, A1, A2, g, lu)
                          : launch(l12_fwd_kernel<N1, N2, F1>, grid, blk, 0, s, X, P.W1, P.B1, P.W2, P.B2, A1, A2, g, lu));
    if (rc) return rc;
  }
  // lazy, layer 3 on the op-level kernels: they accumulate, so their
  // gradient segment starts from zero (after l12 has read the pending one)
  if (lz && !p.l3_fused)
    SRCNN_HIP_TRY(hipMemsetAsync(grads + NetT::P12, 0, NetT::P3 * sizeof(float), s));
  const L3Geom lg{(int)w, (int)h, ow, oh, w3, h3, (int)batch};
  uint32_t* M2 = p.d3mode ? reinterpret_cast<uint32_t*>(D2) + p.m2_off : nullptr;
  if (p.l3_fused) {
    SRCNN_PROFILE("l3_delta_fused", s);
    kernels_note(!p.l3r ? "l3_delta" : p.d3mode ? "l3r_d3" : "l3r_delta");
    const dim3 grid(p.g3);
    int rc = !p.l3r ? launch(l3_delta_kernel<N2, F3>, grid, dim3(kL3Threads), p.lds3, s, A2, T, P.W3, P.B3, D2, slab3, sqs, A3, lg)
             : p.d3mode ? launch(l3r_delta_kernel<F3, true>, grid, dim3(kL3RThreads), p.lds3, s, A2, T, P.W3, P.B3, D2, slab3, sqs, A3, M2, lg)
                        : launch(l3r_delta_kernel<F3, false>, grid, dim3(kL3RThreads), p.lds3, s, A2, T, P.W3, P.B3, D2, slab3, sqs, A3, M2, lg);
    if (rc) return rc;
  } else {
    // ConfigBasedDataPipeline.cpp:200-323 for layer 3 on the op-level kernels
    kernels_note("l3_op_level");
    const int rf = fast::try_conv_fwd(A2, A3, P.W3, P.B3, ow, oh, N2, 1, F3, 0, batch, s);
    if (rf != 1) return rf < 0 ? rf : fail(SRCNN_ERR_INVALID, "fused step: no layer-3 kernel for %dx%d", ow, oh);
    if (b.sq_err)
      if (int rc = reduce(2, A3, T, (size_t)batch * w3 * h3, w, h, w3, h3, b.sq_err, 1, slab3,
                          p.s3 * sizeof(float), s))
        return rc;
    if (int rc = generic::last_delta(T, A3, b.D3, w, h, w3, h3, batch, s)) return rc;
    const int rd = fast::try_conv_delta(b.D3, A2, D2, P.W3, F3, N2, 1, ow, oh, batch, s);
    if (rd != 1) return rd < 0 ? rd : fail(SRCNN_ERR_INVALID, "fused step: no delta2 kernel for %dx%d", ow, oh);
    const int rg = fast::try_conv_grad_acc(A2, b.D3, grads + NetT::P12, grads + NetT::P12 + NetT::P3 - 1, N2, 1,
                                           F3, w3, h3, batch, slab3, p.s3 * sizeof(float), s);
    if (rg != 1) return rg < 0 ? rg : fail(SRCNN_ERR_INVALID, "fused step: no gW3 kernel for %dx%d", ow, oh);
  }
  {
    SRCNN_PROFILE("delta1_grad12_fused", s);
    // (d1x6_d3: the form with the part images; d1x6_d3_sc: the fp32 scratch form)
    kernels_note(p.x6 ? (p.d1tr ? "d1x6_d3" : p.d3mode ? "d1x6_d3_sc" : "d1x6_grad12") : p.kD1c ? "d1c_grad12" : "d1_grad12");
    const dim3 grid(p.gd), blk(256);
    const D3Geom dg{w3, h3, F3};
    // d1x6<true>: D2 holds delta3 and M2 the mask; A2 is not read then
    int rc = p.x6 ? (p.d1tr     ? launch(d1x6_grad12_kernel<true, true>, grid, blk, p.ldsd, s, X, A1, D2, A2, M2, P.W2, P.W3, slab12, g, p.rg, dg)
                     : p.d3mode ? launch(d1x6_grad12_kernel<true>, grid, blk, p.ldsd, s, X, A1, D2, A2, M2, P.W2, P.W3, slab12, g, p.rg, dg)
                                : launch(d1x6_grad12_kernel<false>, grid, blk, p.ldsd, s, X, A1, D2, A2, M2, P.W2, P.W3, slab12, g, p.rg, dg))
             : p.kD1c ? launch(d1c_grad12_kernel<9>, grid, dim3(256 * kD1cTeams), p.ldsd, s, X, A1, D2, P.W2, slab12, g,
                               d1c_xs_floats(h), p.d1c_parts)
                      : launch(d1_grad12_kernel<N1, N2, F1>, grid, blk, 0, s, X, A1, D2, P.W2, slab12, g);
    if (rc) return rc;
  }
  SRCNN_PROFILE("slab_reduce", s);
  const bool update = up && p.l3_fused;
  kernels_note(update ? "slab_reduce_update" : "slab_reduce");
  const SlabSeg segs[3] = {{slab12, grads, p.gd, NetT::P12, 0},
                           {slab3, grads + NetT::P12, p.g3, NetT::P3, 0},
                           {sqs, b.sq_err, p.g3, 1, 0}};
  // with `up`, segments 0 and 1 are every parameter: the update rides along
  SlabUpdate u{};
  if (update) {
    u = *up;
    u.nseg = 2;
  }
  // lazy: the slabs are this step's whole gradient (assigned, not added)
  const int assign = lz ? (p.l3_fused ? 2 : 1) : 0;
  if (int rc = p.l3_fused ? reduce_slabs(segs, b.sq_err ? 3 : 2, s, &u, assign) : reduce_slabs(segs, 1, s, nullptr, assign))
    return rc;
  return update ? 2 : 1;
}

bool train_plan(const srcnn_net* net, uint32_t w, uint32_t h, uint32_t batch, StepNeed* need) {
  return with_net(net, [&](auto n) {
    StepPlan p;
    if (!plan_step<decltype(n)>(w, h, batch, g_arith, &p)) return 0;
    *need = {p.bytes, p.a1_layout};
    return 1;
  });
}

int train_fwd_bwd(const srcnn_net* net, uint32_t w, uint32_t h, uint32_t batch, const StepBuffers& b,
                  hipStream_t s, const SlabUpdate* up, const LazyUpdate* lz) {
  return with_net(net, [&](auto n) {
    StepPlan p;
    if (!plan_step<decltype(n)>(w, h, batch, g_arith, &p)) return 0;
    return run<decltype(n)>(p, net, w, h, batch, b, s, up, lz);
  });
}

int preload(const srcnn_net* net) {
  return with_net(net, [&](auto n) {
    using N = decltype(n);
    const void* k[] = {(const void*)l12_fwd_kernel<N::N1, N::N2, N::F1>, (const void*)l12_fwd_kernel<N::N1, N::N2, N::F1, true>,
                       (const void*)l3_delta_kernel<N::N2, N::F3>, (const void*)d1_grad12_kernel<N::N1, N::N2, N::F1>,
                       (const void*)slab_reduce_kernel, (const void*)l3r_delta_kernel<N::F3, false>,
                       (const void*)l3r_delta_kernel<N::F3, true>, (const void*)d1c_grad12_kernel<9>,
                       (const void*)l12x6_fwd_kernel<false>, (const void*)l12x6_fwd_kernel<true>,
                       (const void*)d1x6_grad12_kernel<false>, (const void*)d1x6_grad12_kernel<true>,
                       (const void*)d1x6_grad12_kernel<true, true>};
    const int rc = resolve_kernels(k, N::kDefault12 ? 13 : 7);
    return rc ? rc : 1;
  });
}

// blocked A1 (l12_fwd_kernel's store layout) -> reference HWC, for
// srcnn_train_activations: channel 32t + 8q + 4h + e of pixel 32c + li sits
// at float 256(4t + q) + 4(li + 32h) + e of chunk c
__global__ void unblock_a1_kernel(const float* __restrict__ A1b, float* __restrict__ A1, int n1,
                                  int npx, size_t total) {
  const int nch = (npx + 31) / 32;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total;
       i += (size_t)gridDim.x * blockDim.x) {
    const int ch = (int)(i % n1);
    const size_t sp = i / n1;
    const int p = (int)(sp % npx);
    const size_t s = sp / npx;
    const int c = p >> 5, li = p & 31, t = ch >> 5, r = ch & 31;
    const int q = r >> 3, hh = (r >> 2) & 1, e = r & 3;
    A1[i] = A1b[(s * nch + c) * (size_t)(32 * n1) + 256 * (4 * t + q) + 4 * (li + 32 * hh) + e];
  }
}

// l12x6's A1 (runs.hpp order, [chunk][64 channels][32 slots]) -> HWC
__global__ void unrun_a1_kernel(const float* __restrict__ A1t, float* __restrict__ A1, RunGeom rg,
                                size_t total) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total;
       i += (size_t)gridDim.x * blockDim.x) {
    const int ch = (int)(i % 64);
    const size_t sp = i / 64;
    const int p = (int)(sp % ((size_t)rg.ow * rg.oh));
    const size_t s = sp / ((size_t)rg.ow * rg.oh);
    const int iy = p / rg.ow, ix = p - iy * rg.ow;
    int k, e;
    if (ix < 4 * rg.a) {
      k = iy * rg.a + ix / 4;
      e = ix % 4;
    } else {
      k = rg.nrow + (ix - 4 * rg.a) * rg.cr + iy / 4;
      e = iy % 4;
    }
    const int c = k / 8, slot = (k % 8) * 4 + e;
    A1[i] = A1t[((s * rg.nch + c) * 64 + ch) * 32 + slot];
  }
}

void note_a1_layout(const float* A1, int layout) {
  t_a1_region = A1;
  t_a1_layout = layout;
}

int a1_layout_written(const float* A1) { return A1 && A1 == t_a1_region ? t_a1_layout : -1; }

size_t a1_chunks(uint32_t ow, uint32_t oh) {
  return std::max<size_t>((ow * oh + 31) / 32, run_geom((int)ow, (int)oh).nch);
}

int unrun_a1(const float* A1t, float* A1, uint32_t ow, uint32_t oh, uint32_t batch, hipStream_t s) {
  const size_t total = (size_t)batch * ow * oh * 64;
  if (total == 0) return SRCNN_OK;
  const int blocks = (int)std::min<size_t>((total + 255) / 256, 4096);
  hipLaunchKernelGGL(unrun_a1_kernel, dim3(blocks), dim3(256), 0, s, A1t, A1, run_geom((int)ow, (int)oh), total);
  SRCNN_LAUNCH_TRY();
  return SRCNN_OK;
}

int unblock_a1(const float* A1b, float* A1, uint32_t n1, uint32_t npx, uint32_t batch, hipStream_t s) {
  const size_t total = (size_t)batch * npx * n1;
  if (total == 0) return SRCNN_OK;
  const int blocks = (int)std::min<size_t>((total + 255) / 256, 4096);
  hipLaunchKernelGGL(unblock_a1_kernel, dim3(blocks), dim3(256), 0, s, A1b, A1, (int)n1, (int)npx,
                     total);
  SRCNN_LAUNCH_TRY();
  return SRCNN_OK;
}

int train_clock(int slot, double* ghz) {
  unsigned long long a[3][kClockBlocks][2];
  SRCNN_HIP_TRY(hipMemcpyFromSymbol(a, HIP_SYMBOL(g_clk), sizeof(a)));
  *ghz = clock_ghz(a[slot]);
  return SRCNN_OK;
}

}  // namespace fused
}  // namespace srcnn

