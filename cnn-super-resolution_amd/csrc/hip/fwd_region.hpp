// fwd_region.hpp -- the region code that fwd_l123 (fwd_l123.hpp) and
// fwd_l123x6 (fwd_l123x6.hpp) share: what a region does that does not depend
// on the arithmetic of its three GEMMs.  Included by forward_fused.hip inside
// namespace srcnn::fused, after fwd_layout.hpp (FwdGeom, kFwdRW).
//
// Templates over what differs between the two: NT threads per block, TW the
// input tile's LDS row stride, F1 / F3, the Q^T image's row stride QS, EHM the
// partial-sum accumulator's rows per tap row.  A piece is here only if both
// kernels compile to the instructions their own copies compiled to
// (profiles/r15_fwd_split/isa_identity.md has the table).  Three did not, in
// any form tried, and stay written out in each kernel:
//   - the window-sum base tables (wrb / wwb): one more VGPR and a rescheduled
//     set-up in fwd_l123, two lines moved in fwd_l123x6
//   - the last chunk's drain (a loop over the two helpers below): fwd_l123x6's
//     region loop rescheduled (160 lines and more)
//   - one struct for a work item's (frame, row, column): both kernels' region
//     loops rescheduled, two more SGPRs; the item's decomposition is therefore
//     written in fwd_item_rows and again in fwd_xload

// Rows of work item wi's region (the frame's last region row may be short).
// Items run frame-major, then region row, then region column.
__device__ __forceinline__ int fwd_item_rows(const FwdGeom& g, int per_frame, int wi) {
  const int n = wi / per_frame, rr = wi - n * per_frame;
  const int ry = rr / g.nrx;
  const int oy0 = ry * g.rh;
  return min(g.rh, g.oh - oy0);
}

// The input tile of work item wi's region, register-staged: element i of the
// TW-strided LDS image is xr[i / NT] of thread i % NT (NR = tile floats / NT,
// rounded up); rows / columns past the frame read as 0.
template <int NT, int TW, int F1, int NR>
__device__ __forceinline__ void fwd_xload(const float* __restrict__ X, const FwdGeom& g, int per_frame, int wi,
                                          float (&xr)[NR]) {
  const int n = wi / per_frame, rr = wi - n * per_frame;
  const int ry = rr / g.nrx, rx = rr - ry * g.nrx;
  const int oy0 = ry * g.rh, ox0 = rx * kFwdRW;
  const int th = min(g.rh, g.oh - oy0) + F1 - 1, tw = min(kFwdRW, g.ow - ox0) + F1 - 1;
  const float* xsrc = X + (size_t)n * g.W * g.H + (size_t)oy0 * g.W + ox0;
#pragma unroll
  for (int k = 0; k < NR; k++) {
    const int i = threadIdx.x + NT * k;
    const int iy = i / TW, ix = i - iy * TW;
    xr[k] = (i < th * TW && ix < tw) ? xsrc[(size_t)iy * g.W + ix] : 0.0f;
  }
}

// L3 window sums.  A chunk (region row c) leaves Q^T[tap][pixel + F3-1] in its
// wave's image (F3-1 zero columns either side); tap row dy of it feeds partial
// row c + F3-1 - dy:
//   accs[dy][c + F3-1 - dy][e] = sum_dx Q[e - (F3-1) + dx][dy*F3 + dx]
//   (Q row e + dx of the padded image is pixel e - (F3-1) + dx)
// A lane takes items lane + 64 k, k < fwd_win_items<F3>(), of the F3 x EW (tap
// row dy, column e) per chunk; each kernel tabulates an item's base into the
// wave's Q image (rb; taps dx follow at a stride of QS + 1 floats) and into the
// accumulator (wb; + chunk row c * EW).
template <int F3>
constexpr int fwd_win_items() {
  return (F3 * (kFwdRW + F3 - 1) + 63) / 64;
}
// an item's F3 taps ...
template <int F3, int QS>
__device__ __forceinline__ void fwd_win_read(const float* qs, int rb, float* v) {
#pragma unroll
  for (int dx = 0; dx < F3; dx++) v[dx] = qs[rb + dx * (QS + 1)];
}
// ... summed into chunk pc's partial row (only some lanes hold the last item k = KW - 1)
template <int F3, int KW>
__device__ __forceinline__ void fwd_win_store(float* accs, int lane, int k, int wb, const float* v, int pc) {
  constexpr int EW = kFwdRW + F3 - 1;
  if (k < KW - 1 || lane + 64 * k < F3 * EW) {
    float t = 0.0f;
#pragma unroll
    for (int dx = 0; dx < F3; dx++) t += v[dx];
    accs[wb + pc * EW] = t;
  }
}

// Element i of the region's partial sums: partial row pr gets the tap rows dy
// whose chunk c = pr - (F3-1) + dy exists (crh chunks).
template <int F3, int EHM>
__device__ __forceinline__ float fwd_part_sum(const float (*accs)[EHM][kFwdRW + F3 - 1], int i, int crh) {
  constexpr int EW = kFwdRW + F3 - 1;
  const int pr = i / EW, e = i - pr * EW;
  float v = 0.0f;
#pragma unroll
  for (int dy = 0; dy < F3; dy++) {
    const int c = pr - (F3 - 1) + dy;
    if (c >= 0 && c < crh) v += accs[dy][pr][e];
  }
  return v;
}
