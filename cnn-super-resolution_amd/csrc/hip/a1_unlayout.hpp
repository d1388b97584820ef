// a1_unlayout.hpp -- the fused step's two internal A1 layouts back to the
// reference's HWC, for srcnn_train_activations (unblock_a1 / unrun_a1 in
// train_fused.hip).  Included by train_fused.hip inside namespace srcnn::fused,
// after fused_layout.hpp (RunGeom).

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
