// keys.hpp -- the Keys cubic (a = -0.5) behind the constexpr weight tables of
// bicubic.hpp (upscale.hip and yuv.hip) and pairs.hip
// (DESIGN.md 11.1).
#pragma once

namespace srcnn {

constexpr double keys(double x) {
  x = x < 0 ? -x : x;
  return x <= 1 ? (1.5 * x - 2.5) * x * x + 1 : x < 2 ? ((-0.5 * x + 2.5) * x - 4) * x + 2 : 0;
}

}  // namespace srcnn
