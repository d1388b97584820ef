// fwd_seam.hpp -- the fused forward's second kernel: the regions' partial sums
// -> A3.  Included by forward_fused.hip inside namespace srcnn::fused, after
// fwd_layout.hpp (FwdGeom, kFwdRW); the plan (fwd_plan.hpp) sets its block
// width, rows per block (rb) and grid.
// ---------------------------------------------------------------------------
// A3[y][x] = B3 + the partials of the regions (ry, rx) in {y, y+f3-1}/rh x
// {x, x+f3-1}/32 (ConfigBasedDataPipeline.cpp:224-238, last layer: no ReLU).
// Grid (columns / blockDim.x, rows, frames): the row's region range is block
// uniform, a thread's column range a shift, and consecutive threads read
// consecutive partials (the 64-bit index division of a flat grid-stride loop
// cost more than the memory traffic).
template <int F3>
__global__ __launch_bounds__(256) void fwd_seam_kernel(const float* __restrict__ part,
                                                       const float* __restrict__ B3,
                                                       float* __restrict__ out, FwdGeom g, int rb) {
  constexpr int EW = kFwdRW + F3 - 1;
  const int w3 = g.ow - F3 + 1, h3 = g.oh - F3 + 1;
  const int EH = g.rh + F3 - 1;
  const float b3 = B3[0];
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= w3) return;
  const int rxa = x / kFwdRW, rxb = (x + F3 - 1) / kFwdRW;
  for (int n = blockIdx.z; n < g.batch; n += gridDim.z) {
    // rows [rb * blockIdx.y, +rb), then grid-strided
    for (int y = rb * blockIdx.y; y < h3; y += (y % rb == rb - 1) ? rb * (gridDim.y - 1) + 1 : 1) {
      const int rya = y / g.rh, ryb = (y + F3 - 1) / g.rh;
      const size_t fbase = (size_t)n * g.nry * g.nrx;
      float v = 0.0f;
      for (int ry = rya; ry <= ryb; ry++) {
        const int pr = y - ry * g.rh + F3 - 1;
        for (int rx = rxa; rx <= rxb; rx++) {
          const int e = x - rx * kFwdRW + F3 - 1;
          v += part[((fbase + (size_t)ry * g.nrx + rx) * EH + pr) * EW + e];
        }
      }
      out[((size_t)n * h3 + y) * w3 + x] = v + b3;
    }
  }
}
