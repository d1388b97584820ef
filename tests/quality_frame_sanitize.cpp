// Host-sanitizer walk over srcnn_quality_frame's argument checks
// (abi_upscale.cpp): the workspace query over valid and invalid sizes, and the
// call with every kind of invalid argument.  Every call fails in its
// validation, before any launch, so this runs without a device.
// tools/sanitize_quality_frame.sh builds the two ABI units and this file with
// the host's AddressSanitizer and UBSan and runs the program, which prints
// one line per call (name, result, message) and exits non-zero if a result is
// not the one expected.
#include <cstdint>
#include <cstdio>
#include <functional>
#include <vector>

#include "srcnn.h"

namespace {
template <typename T>
T* at(uintptr_t a) { return reinterpret_cast<T*>(a); }  // never dereferenced

struct Args {
  srcnn_yuv_format fa{10, 0, SRCNN_YUV_PLANAR, 2, 2, SRCNN_YUV_LIMITED}, fb = fa;
  srcnn_yuv_frame a{at<uint8_t>(1 << 20), at<uint8_t>(2 << 20), at<uint8_t>(3 << 20), 46, 24};
  srcnn_yuv_frame b{at<uint8_t>(5 << 20), at<uint8_t>(6 << 20), at<uint8_t>(7 << 20), 46, 24};
  const srcnn_yuv_format *pfa = &fa, *pfb = &fb;
  const srcnn_yuv_frame *pa = &a, *pb = &b;
  uint32_t w = 23, h = 23, shave = 3;
  double* result = at<double>(8 << 20);
  void* ws = at<void>(9 << 20);
  size_t ws_bytes = 256;
};
int run(Args& g) {
  return srcnn_quality_frame(g.pfa, g.pa, g.pfb, g.pb, g.w, g.h, g.shave, g.result, g.ws, g.ws_bytes, nullptr);
}
void semi(Args& g) {
  g.fa.layout = g.fb.layout = SRCNN_YUV_SEMIPLANAR;
  g.a.v = g.b.v = nullptr;
  g.a.pitch_c = g.b.pitch_c = 48;
}

struct Case {
  const char* name;
  int want;
  std::function<void(Args&)> mutate;
};
}  // namespace

int main() {
  const int I = SRCNN_ERR_INVALID;
  const std::vector<Case> cases = {
      {"short_workspace", SRCNN_ERR_WORKSPACE, [](Args& g) { g.ws_bytes = 255; }},
      {"short_workspace_semiplanar", SRCNN_ERR_WORKSPACE, [](Args& g) { semi(g), g.ws_bytes = 0; }},
      {"null_fmt_a", I, [](Args& g) { g.pfa = nullptr; }},
      {"null_fmt_b", I, [](Args& g) { g.pfb = nullptr; }},
      {"null_frame_a", I, [](Args& g) { g.pa = nullptr; }},
      {"null_frame_b", I, [](Args& g) { g.pb = nullptr; }},
      {"null_result", I, [](Args& g) { g.result = nullptr; }},
      {"null_ws", I, [](Args& g) { g.ws = nullptr; }},
      {"bits_7", I, [](Args& g) { g.fa.bits = g.fb.bits = 7; }},
      {"bits_17", I, [](Args& g) { g.fa.bits = g.fb.bits = 17; }},
      {"bits_max", I, [](Args& g) { g.fa.bits = g.fb.bits = 0xffffffffu; }},
      {"msb_2", I, [](Args& g) { g.fb.msb = 2; }},
      {"msb_at_8_bits", I, [](Args& g) { g.fa.bits = g.fb.bits = 8, g.fa.msb = 1; }},
      {"layout_2", I, [](Args& g) { g.fa.layout = 2; }},
      {"subsampling_3x1", I, [](Args& g) { g.fa.cx = g.fb.cx = 3, g.fa.cy = g.fb.cy = 1; }},
      {"subsampling_0x0", I, [](Args& g) { g.fa.cx = g.fb.cx = 0, g.fa.cy = g.fb.cy = 0; }},
      {"range_2", I, [](Args& g) { g.fa.range = g.fb.range = 2; }},
      {"null_y", I, [](Args& g) { g.a.y = nullptr; }},
      {"null_u", I, [](Args& g) { g.b.u = nullptr; }},
      {"null_v_planar", I, [](Args& g) { g.b.v = nullptr; }},
      {"v_of_semiplanar", I, [](Args& g) { semi(g), g.a.v = g.a.u + 4096; }},
      {"odd_address_y", I, [](Args& g) { g.a.y += 1; }},
      {"odd_address_v", I, [](Args& g) { g.b.v += 1; }},
      {"odd_pitch_y", I, [](Args& g) { g.a.pitch_y = 47; }},
      {"odd_pitch_c", I, [](Args& g) { g.b.pitch_c = 25; }},
      {"pitch_y_below_row", I, [](Args& g) { g.b.pitch_y = 44; }},
      {"pitch_c_below_row", I, [](Args& g) { g.a.pitch_c = 22; }},
      {"pitch_c_below_pairs", I, [](Args& g) { semi(g), g.b.pitch_c = 46; }},
      {"bits_differ", I, [](Args& g) { g.fb.bits = 12; }},
      {"cx_differs", I, [](Args& g) { g.fb.cx = g.fb.cy = 1; }},
      {"cy_differs", I, [](Args& g) { g.fb.cy = 1; }},
      {"range_differs", I, [](Args& g) { g.fb.range = SRCNN_YUV_FULL; }},
      {"Ws_10", I, [](Args& g) { g.w = 16; }},
      {"Hs_10", I, [](Args& g) { g.h = 16; }},
      {"shave_wraps", I, [](Args& g) { g.shave = 0x80000003u; }},
      {"shave_max", I, [](Args& g) { g.shave = 0xffffffffu; }},
      {"size_max", I, [](Args& g) { g.w = g.h = 0xffffffffu, g.shave = 0; }},
      {"result_misaligned", I, [](Args& g) { g.result = at<double>((8 << 20) + 4); }},
      {"ws_misaligned", I, [](Args& g) { g.ws = at<void>((9 << 20) + 4); }},
      {"plane_over_2^31", I,
       [](Args& g) { g.w = g.h = 46341, g.shave = 0, g.a.pitch_y = g.b.pitch_y = 92682, g.a.pitch_c = g.b.pitch_c = 46342; }},
  };
  int bad = 0;
  for (const Case& c : cases) {
    Args g;
    c.mutate(g);
    const int rc = run(g);
    std::printf("%s\t%d\t%s\n", c.name, rc, srcnn_last_error());
    bad += rc != c.want;
  }
  // the query: valid sizes give whole 256-byte units, invalid ones 0
  const uint32_t big = 0xffffffffu;
  const uint32_t sizes[][5] = {{3840, 2160, 2, 2, 0}, {11, 11, 1, 1, 0}, {17, 17, 2, 2, 3}, {46340, 46340, 2, 1, 0},
                               {10, 11, 2, 2, 0}, {17, 17, 2, 2, 0x80000003u}, {17, 17, 3, 1, 0}, {17, 17, 0, 0, 0},
                               {46341, 46341, 2, 2, 0}, {0, 0, 2, 2, 0}, {big, big, 2, 2, big}, {big, 11, 1, 1, 0}};
  for (int i = 0; i < 12; ++i) {
    const uint32_t* s = sizes[i];
    const size_t n = srcnn_quality_frame_workspace_bytes(s[0], s[1], s[2], s[3], s[4]);
    std::printf("query/%ux%u_%ux%u_shave_%u\t%zu\n", s[0], s[1], s[2], s[3], s[4], n);
    bad += i < 4 ? (n == 0 || n % 256 != 0) : n != 0;
  }
  std::printf("%d unexpected results\n", bad);
  return bad ? 1 : 0;
}
