// Host-sanitizer walk over the image-level C ABI (abi.cpp, abi_upscale.cpp):
// invalid input to every entry point of the upscale family, and to the calls
// that moved with it.  Every call fails in its validation, before any launch,
// so this runs without a device.  tools/sanitize_abi.sh builds the two units
// and this file with the host's AddressSanitizer and UBSan, runs the program
// and compares what it prints (name, result, message) with the entries of the
// same names in tests/golden/upscale_abi_errors.json.
#include <cstdint>
#include <cstdio>
#include <functional>
#include <string>
#include <vector>

#include "srcnn.h"

namespace {
template <typename T>
T* at(uintptr_t a) { return reinterpret_cast<T*>(a); }  // never dereferenced

const srcnn_net kDefault{64, 32, 9, 1, 5}, kEven{64, 32, 9, 2, 5},
    kOverflow{64, 32, 0xffffffffu, 0xffffffffu, 0xffffffffu};
const srcnn_yuv_format k8{8, 0, SRCNN_YUV_PLANAR, 2, 2, SRCNN_YUV_FULL},
    k10{10, 0, SRCNN_YUV_PLANAR, 2, 2, SRCNN_YUV_FULL}, kSemi{8, 0, SRCNN_YUV_SEMIPLANAR, 2, 2, SRCNN_YUV_FULL};
void* const P = at<void>(64);
float* const F = at<float>(64);
uint8_t* const U = at<uint8_t>(64);
const size_t kBig = size_t(1) << 40;

srcnn_yuv_frame frame(uint32_t pitch_y, uint32_t pitch_c, uint8_t* y = U, uint8_t* u = U, uint8_t* v = U) {
  return {y, u, v, pitch_y, pitch_c};
}
// 37 x 23 at 4:2:0 and its x2 and 55 x 35 outputs, 8 bits
const srcnn_yuv_frame kSrc = frame(37, 19), kDst2 = frame(74, 37), kDstTo = frame(55, 28);

struct Case {
  const char* name;             // the golden table's, or extra/... for what it does not hold
  std::function<long long()> call;
  bool query;                   // returns bytes, not a status
};
}  // namespace

int main() {
  const std::vector<Case> cases = {
      {"upscale_luma/scale_5", [] { return srcnn_upscale_luma(U, F, 8, 8, 5, 12, nullptr); }},
      {"upscale_luma/plane_floats", [] { return srcnn_upscale_luma(U, F, 30000, 30000, 2, 12, nullptr); }},
      {"upscale_luma/null_source", [] { return srcnn_upscale_luma(nullptr, F, 8, 8, 2, 12, nullptr); }},
      {"upscale_compose/w0", [] { return srcnn_upscale_compose(U, F, U, 0, 8, 2, nullptr); }},
      {"upscale_compose/rgb_bytes", [] { return srcnn_upscale_compose(U, F, U, 15000, 15000, 2, nullptr); }},
      {"yuv_upscale_luma/short_pitch", [] { return srcnn_yuv_upscale_luma(U, 7, F, 8, 8, 2, 12, 1, nullptr); }},
      {"yuv_upscale_luma/range", [] { return srcnn_yuv_upscale_luma(U, 8, F, 8, 8, 2, 12, 2, nullptr); }},
      {"yuv_upscale_luma16/odd_address",
       [] { return srcnn_yuv_upscale_luma16(at<void>(65), 16, F, 8, 8, 2, 12, 10, 0, 1, nullptr); }},
      {"yuv_upscale_luma16/17_bits", [] { return srcnn_yuv_upscale_luma16(P, 16, F, 8, 8, 2, 12, 17, 0, 1, nullptr); }},
      {"yuv_compose_luma/short_pitch", [] { return srcnn_yuv_compose_luma(F, U, 15, 16, 16, 1, nullptr); }},
      {"yuv_compose_luma16/odd_pitch", [] { return srcnn_yuv_compose_luma16(F, P, 33, 16, 16, 10, 0, 1, nullptr); }},
      {"upscale_planes_u8/ow_above", [] { return srcnn_upscale_planes_u8(U, U, 8, 8, 8, U, U, 17, 17, 16, 2, nullptr); }},
      {"upscale_planes_u8/null_src1",
       [] { return srcnn_upscale_planes_u8(U, nullptr, 8, 8, 8, U, U, 16, 16, 16, 2, nullptr); }},
      {"upscale_planes/layout_2", [] { return srcnn_upscale_planes(P, P, 16, 8, 8, P, P, 32, 16, 16, 2, 10, 0, 2, nullptr); }},
      {"upscale_planes/odd_dst0",
       [] { return srcnn_upscale_planes(P, P, 16, 8, 8, at<void>(65), P, 32, 16, 16, 2, 10, 0, 0, nullptr); }},
      {"resize_luma/W_above_4w", [] { return srcnn_resize_luma(U, F, 8, 8, 33, 12, 12, nullptr); }},
      {"resize_luma/plane_floats", [] { return srcnn_resize_luma(U, F, 30000, 30000, 100000, 100000, 12, nullptr); }},
      {"resize_compose/rgb_bytes", [] { return srcnn_resize_compose(U, F, U, 20000, 20000, 30000, 30000, nullptr); }},
      {"yuv_resize_luma/odd_pitch", [] { return srcnn_yuv_resize_luma(P, 17, F, 8, 8, 12, 12, 12, 10, 0, 1, nullptr); }},
      {"yuv_resize_luma/W0", [] { return srcnn_yuv_resize_luma(P, 16, F, 8, 8, 0, 12, 12, 10, 0, 1, nullptr); }},
      {"resize_planes/zero_numerator",
       [] { return srcnn_resize_planes(P, P, 16, 8, 8, P, P, 24, 12, 12, 0, 3, 2, 3, 10, 0, 0, nullptr); }},
      {"resize_planes/ow_beyond_its_bound",
       [] { return srcnn_resize_planes(P, P, 16, 8, 8, P, P, 26, 13, 12, 2, 3, 2, 3, 10, 0, 0, nullptr); }},
      {"resize_planes/map_overflows",
       [] {
         return srcnn_resize_planes(P, P, 1u << 30, 1u << 30, 1, P, P, 1u << 30, 1u << 30, 1, 0xffffffffu, 0xffffffffu, 1,
                                    1, 8, 0, 0, nullptr);
       }},
      {"upscale/null_net", [] { return srcnn_upscale(nullptr, U, 8, 8, 2, F, U, P, kBig, nullptr); }},
      {"upscale/even_filter", [] { return srcnn_upscale(&kEven, U, 8, 8, 2, F, U, P, kBig, nullptr); }},
      {"upscale/padding_overflows", [] { return srcnn_upscale(&kOverflow, U, 8, 8, 2, F, U, P, kBig, nullptr); }},
      {"upscale/default/workspace_one_byte_short",
       [] {
         return srcnn_upscale(&kDefault, U, 37, 23, 2, F, U, P, srcnn_upscale_workspace_bytes(&kDefault, 37, 23, 2) - 1,
                              nullptr);
       }},
      {"upscale_to/W_below_w", [] { return srcnn_upscale_to(&kDefault, U, 8, 8, 7, 20, F, U, P, kBig, nullptr); }},
      {"upscale_to/null_rgba", [] { return srcnn_upscale_to(&kDefault, nullptr, 8, 8, 12, 20, F, U, P, kBig, nullptr); }},
      {"upscale_to/default/workspace_one_byte_short",
       [] {
         return srcnn_upscale_to(&kDefault, U, 37, 23, 55, 35, F, U, P,
                                 srcnn_upscale_to_workspace_bytes(&kDefault, 37, 23, 55, 35) - 1, nullptr);
       }},
      {"upscale_yuv/subsampling_1x2",
       [] { return srcnn_upscale_yuv(&kDefault, &kSrc, &kDst2, 37, 23, 1, 2, 2, 1, F, P, kBig, nullptr); }},
      {"upscale_yuv/null_source_y",
       [] {
         const srcnn_yuv_frame s = frame(37, 19, nullptr);
         return srcnn_upscale_yuv(&kDefault, &s, &kDst2, 37, 23, 2, 2, 2, 1, F, P, kBig, nullptr);
       }},
      {"upscale_yuv/output_c_pitch",
       [] {
         const srcnn_yuv_frame d = frame(74, 36);
         return srcnn_upscale_yuv(&kDefault, &kSrc, &d, 37, 23, 2, 2, 2, 1, F, P, kBig, nullptr);
       }},
      {"upscale_frame/null_fmt",
       [] { return srcnn_upscale_frame(&kDefault, nullptr, &kSrc, &kDst2, 37, 23, 2, F, P, kBig, nullptr); }},
      {"upscale_frame/odd_source_u",
       [] {
         const srcnn_yuv_frame s = frame(74, 38, U, at<uint8_t>(65)), d = frame(148, 74);
         return srcnn_upscale_frame(&kDefault, &k10, &s, &d, 37, 23, 2, F, P, kBig, nullptr);
       }},
      {"upscale_frame/v_in_a_semi_planar_source",
       [] {
         const srcnn_yuv_frame s = frame(37, 38), d = frame(74, 74, U, U, nullptr);
         return srcnn_upscale_frame(&kDefault, &kSemi, &s, &d, 37, 23, 2, F, P, kBig, nullptr);
       }},
      {"upscale_frame/default/workspace_one_byte_short",
       [] {
         return srcnn_upscale_frame(&kDefault, &k8, &kSrc, &kDst2, 37, 23, 2, F, P,
                                    srcnn_upscale_yuv_workspace_bytes(&kDefault, 37, 23, 2) - 1, nullptr);
       }},
      {"upscale_frame_to/H_above_4h",
       [] { return srcnn_upscale_frame_to(&kDefault, &k8, &kSrc, &kDstTo, 37, 23, 55, 93, F, P, kBig, nullptr); }},
      {"upscale_frame_to/odd_pitch_of_words",
       [] {
         const srcnn_yuv_frame s = frame(74, 39), d = frame(110, 56);
         return srcnn_upscale_frame_to(&kDefault, &k10, &s, &d, 37, 23, 55, 35, F, P, kBig, nullptr);
       }},
      {"upscale_frame_to/samples",
       [] {
         const srcnn_yuv_frame f = frame(65536, 32768);
         return srcnn_upscale_frame_to(&kDefault, &k8, &f, &f, 65536, 65536, 65536, 65536, F, P, kBig, nullptr);
       }},
      {"upscale_frame_to/default/workspace_one_byte_short",
       [] {
         return srcnn_upscale_frame_to(&kDefault, &k8, &kSrc, &kDstTo, 37, 23, 55, 35, F, P,
                                       srcnn_upscale_frame_to_workspace_bytes(&kDefault, 37, 23, 55, 35) - 1, nullptr);
       }},
      {"evaluate/no_window",
       [] { return srcnn_evaluate(&kDefault, U, 30, 30, 2, 10, F, at<double>(64), P, kBig, nullptr); }},
      {"evaluate/rgba_alignment",
       [] { return srcnn_evaluate(&kDefault, at<uint8_t>(66), 48, 40, 2, 4, F, at<double>(64), P, kBig, nullptr); }},
      {"evaluate/padding_overflows",
       [] { return srcnn_evaluate(&kOverflow, U, 48, 40, 2, 4, F, at<double>(64), P, kBig, nullptr); }},
      {"upscale_workspace_bytes/null/8x8/x2", [] { return srcnn_upscale_workspace_bytes(nullptr, 8, 8, 2); }, true},
      {"upscale_workspace_bytes/overflow/8x8/x2", [] { return srcnn_upscale_workspace_bytes(&kOverflow, 8, 8, 2); }, true},
      {"upscale_workspace_bytes/default/37x23/x3", [] { return srcnn_upscale_workspace_bytes(&kDefault, 37, 23, 3); }, true},
      {"upscale_yuv_workspace_bytes/default/37x23/x2",
       [] { return srcnn_upscale_yuv_workspace_bytes(&kDefault, 37, 23, 2); }, true},
      {"upscale_to_workspace_bytes/default/37x23/56x33",
       [] { return srcnn_upscale_to_workspace_bytes(&kDefault, 37, 23, 56, 33); }, true},
      {"upscale_frame_to_workspace_bytes/even/8x8/12x12",
       [] { return srcnn_upscale_frame_to_workspace_bytes(&kEven, 8, 8, 12, 12); }, true},
      {"evaluate_workspace_bytes/default/37x23/x2", [] { return srcnn_evaluate_workspace_bytes(&kDefault, 37, 23, 2); }, true},
      // what moved with the family
      {"extra/downscale_rgba/scale_5", [] { return srcnn_downscale_rgba(U, U, 8, 8, 5, nullptr); }},
      {"extra/gather_tiles/stride_0", [] { return srcnn_gather_tiles(F, 8, 8, 0, 0, 0, 1, 1, 4, 4, 0, F, nullptr, nullptr); }},
      {"extra/gather_batch/null", [] { return srcnn_gather_batch(nullptr, 1, nullptr, 1, 4, 4, F, F, nullptr, nullptr); }},
      {"extra/make_pairs/no_tile", [] { return srcnn_make_pairs(U, 48, 40, 2, 64, 14, F, F, P, kBig, nullptr); }},
      {"extra/make_pairs/workspace_short", [] { return srcnn_make_pairs(U, 48, 40, 2, 33, 14, F, F, P, 0, nullptr); }},
      {"extra/quality/unknown_format",
       [] { return srcnn_quality(P, 2, 48, P, SRCNN_PIX_RGB8, 48, 48, 40, 4, at<double>(64), P, kBig, nullptr); }},
      {"extra/make_pairs_workspace_bytes", [] { return srcnn_make_pairs_workspace_bytes(48, 40, 2); }, true},
      {"extra/quality_workspace_bytes", [] { return srcnn_quality_workspace_bytes(48, 40, 4); }, true},
  };
  int bad = 0;
  for (const Case& c : cases) {
    // the last error is sticky: every case starts from this one
    srcnn_fill_f32(nullptr, 0.0f, 1, nullptr);
    const long long r = c.call();
    printf("%s\t%lld\t%s\n", c.name, r, srcnn_last_error());
    if (!c.query && r != SRCNN_ERR_INVALID && r != SRCNN_ERR_WORKSPACE) {
      fprintf(stderr, "%s: returned %lld, not an error of its validation\n", c.name, r);
      bad++;
    }
  }
  return bad != 0;
}
