// bicubic.hpp -- what the x S resampling kernels of upscale.hip
// and yuv.hip share: the tile geometry, the fp32 weight table
// of the Keys cubic at the S phases of the half-pixel map, the horizontal
// pass over a staged source patch, and the vertical pass of a luma tile into
// the padded plane.  Everything sits in an unnamed namespace: each translation
// unit gets its own copy of the table in constant memory.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "keys.hpp"

namespace srcnn {
namespace {

constexpr int kThreads = 256;
// Tile geometry, by measurement at 1920 x 1080 x2.
// upscale_luma: 32 x 16 source pixels at every scale (64 x 8 and 64 x 16 at
// S = 2 were 6 - 8 % slower).  upscale_compose: 64 x 8 at S <= 2, which makes
// a tile's rgb rows 192 - 384 bytes, so that most of the 128-byte lines a row
// touches are written whole by one workgroup, and keeps the three channels of
// the horizontal pass within 25 KB of LDS (32 x 16 was 13 % slower); 32 x 16
// at S >= 3.
template <int S, bool COMPOSE>
struct Tile {
  static constexpr int JX = COMPOSE && S <= 2 ? 64 : 32, JY = COMPOSE && S <= 2 ? 8 : 16;  // source pixels
  static constexpr int TX = JX * S, TY = JY * S;                                // output pixels
  static constexpr int PC = JX + 4, PR = JY + 4;                                // staged patch
  static constexpr int PCP = PC + 1;                                            // its LDS pitch
};

// (keys(): the Keys cubic, a = -0.5, keys.hpp)
// phase k of scale s: d = (k+0.5)/s - 0.5, b = floor(d) (-1 or 0), t = d - b;
// taps j+b-1 .. j+b+2 at distances t+1, t, 1-t, 2-t
constexpr int tap_base(int s, int k) { return 2 * k + 1 < s ? -1 : 0; }
struct Weights {
  float w[5][4][4];  // [scale][phase][tap], computed in double, rounded once
};
constexpr Weights make_weights() {
  Weights t{};
  for (int s = 1; s <= 4; s++)
    for (int k = 0; k < s; k++) {
      const double d = (k + 0.5) / s - 0.5, tt = d - tap_base(s, k);
      for (int i = 0; i < 4; i++) t.w[s][k][i] = (float)keys(tt + 1 - i);
    }
  return t;
}
__constant__ Weights c_up = make_weights();

// the four weights of phase ky (not a compile-time value in the vertical
// pass): selected from the S phases' weights, which are uniform scalar loads,
// instead of a per-lane load from the table
template <int S>
__device__ __forceinline__ void phase_weights(int ky, float (&w)[4]) {
#pragma unroll
  for (int i = 0; i < 4; i++) {
    float v = c_up.w[S][0][i];
#pragma unroll
    for (int k = 1; k < S; k++) v = ky == k ? c_up.w[S][k][i] : v;
    w[i] = v;
  }
}

// horizontal pass: patch row r, source column jj -> S values per channel;
// tap(r, c, ch) is the staged value of channel ch, put(ch, r, x, v) stores
template <int S, typename T, int NCH, typename Tap, typename Put>
__device__ __forceinline__ void hpass(Tap tap, Put put) {
  const int jj = threadIdx.x % T::JX;
  for (int r = threadIdx.x / T::JX; r < T::PR; r += kThreads / T::JX) {
#pragma unroll
    for (int k = 0; k < S; k++) {
      const float* wk = c_up.w[S][k];
      const int c = jj + tap_base(S, k) + 1;
#pragma unroll
      for (int ch = 0; ch < NCH; ch++)
        put(ch, r, jj * S + k,
            wk[0] * tap(r, c, ch) + wk[1] * tap(r, c + 1, ch) + wk[2] * tap(r, c + 2, ch) +
                wk[3] * tap(r, c + 3, ch));
    }
  }
}

// vertical pass of a luma tile (Tile<S, false>) from the horizontal pass's
// rows s_h into the padded plane [(S*h+P)][(S*w+P)]: the tile's own pixels
// shifted by the margin P/2, plus the margin itself on the image's edges
template <int S>
__device__ __forceinline__ void store_plane_tile(const float (&s_h)[Tile<S, false>::PR][Tile<S, false>::TX + 1],
                                                 float* __restrict__ out, int w, int h, int P,
                                                 int tx, int ty, int i0, int tiles_x, int tiles_y) {
  using T = Tile<S, false>;
  constexpr int TX = T::TX, TY = T::TY;
  const int tid = threadIdx.x;
  // the plane rows and columns this tile owns: its own pixels shifted by the
  // margin m, plus the margin itself on the image's edges
  const int W = w * S, H = h * S, m = P / 2;
  const int X0 = tx * TX, Y0 = ty * TY;
  const int Xp0 = tx == 0 ? 0 : m + X0, Xp1 = tx == tiles_x - 1 ? W + P : m + X0 + TX;
  const int Yp0 = ty == 0 ? 0 : m + Y0, Yp1 = ty == tiles_y - 1 ? H + P : m + Y0 + TY;
  const int n = Xp1 - Xp0;
  const size_t pitch = (size_t)W + P;

  // LPR lanes share a row; each stores 16 bytes where the row's address allows
  constexpr int LPR = TX <= 64 ? 16 : 32, RPI = kThreads / LPR;
  const int l = tid % LPR;
  for (int Y = Yp0 + tid / LPR; Y < Yp1; Y += RPI) {
    const int Yi = min(max(Y - m, 0), H - 1);
    const int jy = Yi / S, ky = Yi - jy * S;
    const int rb = jy - i0 + tap_base(S, ky) + 1;  // patch row of the first tap
    float wv[4];
    phase_weights<S>(ky, wv);
    const float w0 = wv[0], w1 = wv[1], w2 = wv[2], w3 = wv[3];
    auto val = [&](int X) {
      const int cx = min(max(X - m, 0), W - 1) - X0;
      return w0 * s_h[rb][cx] + w1 * s_h[rb + 1][cx] + w2 * s_h[rb + 2][cx] + w3 * s_h[rb + 3][cx];
    };
    float* orow = out + (size_t)Y * pitch;
    // floats up to the first 16-byte boundary, float4 groups, the rest
    const int head = min((int)(((16 - ((uintptr_t)(orow + Xp0) & 15)) & 15) >> 2), n);
    if (l < head) orow[Xp0 + l] = val(Xp0 + l);
    const int ng = (n - head) >> 2;
    for (int g = l; g < ng; g += LPR) {
      const int X = Xp0 + head + 4 * g;
      *reinterpret_cast<float4*>(orow + X) = make_float4(val(X), val(X + 1), val(X + 2), val(X + 3));
    }
    const int X = Xp0 + head + 4 * ng + l;
    if (X < Xp1) orow[X] = val(X);
  }
}

inline uint32_t tiles(uint32_t n, int t) { return (n + t - 1) / t; }

}  // namespace
}  // namespace srcnn
