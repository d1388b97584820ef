// keys_down.hpp -- what the / S resampling kernels of pairs.hip
// and yuv_down.hip share: the taps of the Keys cubic stretched
// by S at half-pixel centres and their fp32 weight table.  Everything sits in
// an unnamed namespace, as in bicubic.hpp: each translation unit gets its own
// copy of the table in constant memory.
#pragma once
#include <hip/hip_runtime.h>

#include "keys.hpp"

namespace srcnn {
namespace {

// taps of scale s: source offsets o_min(s) .. s-1-o_min(s) from s*j, every
// integer o with |o - (s-1)/2| / s < 2: 3 / 8 / 11 / 16 taps at s = 1 .. 4
constexpr int o_min(int s) { return s % 2 ? -(3 * s + 1) / 2 + 1 : -3 * s / 2; }
constexpr int n_taps(int s) { return s - 2 * o_min(s); }
constexpr int kMaxTaps = n_taps(4);

struct DownWeights {
  float w[5][kMaxTaps];  // [scale][tap], computed in double, rounded once
};
constexpr DownWeights make_down_weights() {
  DownWeights t{};
  for (int s = 1; s <= 4; s++) {
    double k[kMaxTaps] = {}, sum = 0;
    for (int i = 0; i < n_taps(s); i++) {
      k[i] = keys((o_min(s) + i - (s - 1) / 2.0) / s);
      sum += k[i];
    }
    for (int i = 0; i < n_taps(s); i++) t.w[s][i] = (float)(k[i] / sum);
  }
  return t;
}
__constant__ DownWeights c_down = make_down_weights();

}  // namespace
}  // namespace srcnn
