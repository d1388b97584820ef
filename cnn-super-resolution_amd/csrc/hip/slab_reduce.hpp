// slab_reduce.hpp -- the last kernel of every net-level training step and of
// the op-level gradient calls: the fixed-order sum of per-block gradient slabs,
// optionally with the SGD update (srcnn_train_step) riding along.  Included by
// train_fused.hip inside namespace srcnn::fused; its host entry point is
// reduce_slabs() there.  Uses ops.hpp's SlabSeg, SlabUpdate and sgd_step.
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
