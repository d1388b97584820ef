// cnn_sr::DataPipeline -- validated launchers of the SRCNN operators.
//
// Drop-in for the reference's DataPipeline (src/DataPipeline.hpp:39-222):
// same method names, argument order and meaning, same lazy-allocation
// contract (an output handle that is gpu_nullptr is allocated at the exact
// size; a too-small one throws instead of being reallocated,
// src/DataPipeline.cpp:66-86), same runtime_error checks.  Each launcher is
// one call into libsrcnn_hip.so (include/srcnn.h) on the context's stream;
// cl_event becomes srcnn::Event.
#ifndef CNN_SR_DATA_PIPELINE_HPP
#define CNN_SR_DATA_PIPELINE_HPP

#include "Context.hpp"
#include "LayerData.hpp"

namespace cnn_sr {

using srcnn::Event;
using srcnn::ImageData;
using srcnn::Kernel;
using srcnn::MemoryHandle;
using srcnn::gpu_nullptr;

/** Device handles of one layer (reference src/DataPipeline.hpp:11-29). */
struct LayerAllocationPool {
  MemoryHandle weights = gpu_nullptr;                 // f*f*n_prev*n_cur
  MemoryHandle bias = gpu_nullptr;                    // n_cur
  MemoryHandle accumulating_grad_w = gpu_nullptr;     // sum over the batch
  MemoryHandle accumulating_grad_b = gpu_nullptr;
  MemoryHandle previous_batch_delta_w = gpu_nullptr;  // momentum state
  MemoryHandle previous_batch_delta_b = gpu_nullptr;
};

/** srcnn_quality's three results (psnr is +inf for identical images). */
struct QualityReport {
  double mse = 0, psnr = 0, ssim = 0;
};

/** srcnn_quality_frame's eight results: the mean squared
 * error of the integer code values and its PSNR per plane, the luma's SSIM,
 * and the PSNR over all three planes (+inf for identical planes). */
struct FrameQualityReport {
  double mse_y = 0, psnr_y = 0, ssim_y = 0, mse_u = 0, psnr_u = 0, mse_v = 0, psnr_v = 0, psnr_all = 0;
};

class DataPipeline {
 public:
  static int LOAD_KERNEL_LUMA;
  static int LOAD_KERNEL_LAYERS;
  static int LOAD_KERNEL_BACKPROPAGATE;
  static int LOAD_KERNEL_MISC;
  static int LOAD_KERNEL_NONE;
  static int LOAD_KERNEL_ALL;

  explicit DataPipeline(srcnn::Context*);
  virtual ~DataPipeline() {}
  virtual void init(int load_flags = DataPipeline::LOAD_KERNEL_ALL);
  srcnn::Context* context();

  /** Upload `img` as an RGBA image to raw_img and its luma (optionally /255)
   * to luma (reference :186-220). */
  Event extract_luma(ImageData&, MemoryHandle& gpu_buf_raw_img, MemoryHandle& gpu_buf_luma,
                     bool normalize, Event* ev = nullptr);

  /** RGB (3 bytes/px) image made of the new luma (centre new_luma_w x
   * new_luma_h) and the CbCr of `img` (reference :222-266). */
  Event swap_luma(ImageData&, MemoryHandle& gpu_buf_org_img, MemoryHandle gpu_buf_new_luma,
                  MemoryHandle& target, size_t new_luma_w, size_t new_luma_h,
                  Event* ev = nullptr);

  /** Extension (the reference expects an already scaled input): upload the
   * low-resolution `img` to raw_img and write its bicubic x `scale` luma,
   * edge-replicated by the margin of `total_padding`, to luma_padded:
   * (scale*h + total_padding) x (scale*w + total_padding) floats
   * (srcnn_upscale_luma). */
  Event upscale_luma(ImageData&, MemoryHandle& gpu_buf_raw_img, MemoryHandle& gpu_buf_luma_padded,
                     size_t scale, size_t total_padding, Event* ev = nullptr);

  /** Extension: RGB image of scale*w x scale*h made of the new luma (that
   * size) and the bicubic x `scale` colours of `img`, which the caller has
   * uploaded to gpu_buf_org_img (srcnn_upscale_compose). */
  Event upscale_compose(ImageData&, MemoryHandle gpu_buf_org_img, MemoryHandle gpu_buf_new_luma,
                        MemoryHandle& target, size_t scale, Event* ev = nullptr);

  /** Extension, Y'CbCr frames: the Y plane `y` (w x h
   * samples, rows pitch_y bytes apart, already on the device) as
   * upscale_luma's padded plane.  A sample has `bits` bits, 8 to 16: one byte
   * at 8 bits, else a 16-bit word with the value in its low (msb false) or
   * high bits.  full_range: Y / (2^bits - 1), else (Y - 16 up) / (219 up)
   * with up = 2^(bits-8) (srcnn_yuv_upscale_luma16). */
  Event yuv_upscale_luma(MemoryHandle y, size_t pitch_y, size_t w, size_t h, MemoryHandle& gpu_buf_luma_padded,
                         size_t scale, size_t total_padding, unsigned bits, bool msb, bool full_range,
                         Event* ev = nullptr);

  /** Extension: a frame's chroma of pw x ph bicubic x `scale`, rounded and
   * clamped to `bits` bits, the top-left ow x oh: two planes into dst0 and
   * dst1, or, semiplanar, src0's (U, V) pairs into dst0 with src1 and dst1
   * nullptr; pitches in bytes (srcnn_upscale_planes). */
  Event upscale_planes(MemoryHandle src0, MemoryHandle src1, size_t src_pitch, size_t pw, size_t ph,
                       MemoryHandle dst0, MemoryHandle dst1, size_t dst_pitch, size_t ow, size_t oh, size_t scale,
                       unsigned bits, bool msb, bool semiplanar, Event* ev = nullptr);

  /** Extension: the net's luma (w x h floats) back into a Y plane of `bits`
   * bits per sample (srcnn_yuv_compose_luma16). */
  Event yuv_compose_luma(MemoryHandle luma, size_t w, size_t h, MemoryHandle y, size_t pitch_y, unsigned bits,
                         bool msb, bool full_range, Event* ev = nullptr);

  /** Extension, any output size: upscale_luma to out_w x out_h,
   * each within [1x, 4x] of the image's (srcnn_resize_luma). */
  Event resize_luma(ImageData&, MemoryHandle& gpu_buf_raw_img, MemoryHandle& gpu_buf_luma_padded, size_t out_w,
                    size_t out_h, size_t total_padding, Event* ev = nullptr);

  /** Extension: upscale_compose to out_w x out_h (srcnn_resize_compose). */
  Event resize_compose(ImageData&, MemoryHandle gpu_buf_org_img, MemoryHandle gpu_buf_new_luma,
                       MemoryHandle& target, size_t out_w, size_t out_h, Event* ev = nullptr);

  /** Extension: yuv_upscale_luma to out_w x out_h (srcnn_yuv_resize_luma). */
  Event yuv_resize_luma(MemoryHandle y, size_t pitch_y, size_t w, size_t h, MemoryHandle& gpu_buf_luma_padded,
                        size_t out_w, size_t out_h, size_t total_padding, unsigned bits, bool msb,
                        bool full_range, Event* ev = nullptr);

  /** Extension: upscale_planes at explicit ratios, the source step per output
   * sample rx_num / rx_den and ry_num / ry_den (a frame's chroma takes the
   * luma's w / W and h / H): pw x ph -> ow x oh (srcnn_resize_planes). */
  Event resize_planes(MemoryHandle src0, MemoryHandle src1, size_t src_pitch, size_t pw, size_t ph,
                      MemoryHandle dst0, MemoryHandle dst1, size_t dst_pitch, size_t ow, size_t oh, size_t rx_num,
                      size_t rx_den, size_t ry_num, size_t ry_den, unsigned bits, bool msb, bool semiplanar,
                      Event* ev = nullptr);

  /** Extension, the inverse of the upscale: `img` antialiased-bicubic
   * downscaled by `scale` (1..4) on the device into `out`, RGBA of
   * (w / scale) x (h / scale), alpha 255 (srcnn_downscale_rgba). */
  void downscale(ImageData& img, unsigned scale, ImageData& out);

  /** Extension, Y'CbCr frames: the device frame `src` of W x H
   * luma samples downscaled by `scale` (1..4) into `dst`, (W / scale) x
   * (H / scale) in the same format: one srcnn_downscale_frame call.  Only
   * enqueues, on `stream`, or, with no stream, on the context's, where the
   * call is counted and timed. */
  void downscale_frame(const srcnn_yuv_format& fmt, const srcnn_yuv_frame& src, const srcnn_yuv_frame& dst,
                       unsigned W, unsigned H, unsigned scale, srcnn_stream_t stream = nullptr);

  /** Extension: PSNR and SSIM of `img` against `ref` (equal sizes, any of 1,
   * 3 or 4 channels each), measured on the device on the full-range luma
   * with `shave` pixels dropped per side (srcnn_quality).  Blocking. */
  QualityReport quality(ImageData& img, ImageData& ref, unsigned shave);

  /** Extension, Y'CbCr frames: PSNR per plane and SSIM on luma
   * of the device frames `a` and `b` of w x h luma samples, each with its own
   * format (equal bits, subsampling and range), `shave` luma pixels dropped
   * per side (srcnn_quality_frame).  Blocking. */
  FrameQualityReport quality_frame(const srcnn_yuv_format& fmt_a, const srcnn_yuv_frame& a,
                                   const srcnn_yuv_format& fmt_b, const srcnn_yuv_frame& b, unsigned w, unsigned h,
                                   unsigned shave);
  /** The same, enqueued: the eight doubles go to `result` (device) through the
   * caller's workspace (srcnn_quality_frame_workspace_bytes), on `stream`, or,
   * with no stream, on the context's, where the call is counted and timed. */
  void quality_frame(const srcnn_yuv_format& fmt_a, const srcnn_yuv_frame& a, const srcnn_yuv_format& fmt_b,
                     const srcnn_yuv_frame& b, unsigned w, unsigned h, unsigned shave, double* result, void* ws,
                     size_t ws_bytes, srcnn_stream_t stream);

  /** Extension: cut nx x ny tiles of tw x th floats, tile (ix, iy) from
   * (x0 + ix*stride, y0 + iy*stride), out of the plane_w x plane_h float plane
   * into `tiles` ([nx*ny][th][tw]), each minus its own mean when sub_mean;
   * `means` (optional) then receives the nx*ny means (srcnn_gather_tiles). */
  Event gather_tiles(MemoryHandle plane, size_t plane_w, size_t plane_h, size_t x0, size_t y0,
                     size_t stride, size_t nx, size_t ny, size_t tw, size_t th, bool sub_mean,
                     MemoryHandle& tiles, MemoryHandle* means = nullptr, Event* ev = nullptr);

  /** Extension: one batch of n tiles of tw x th floats gathered from resident
   * plane pairs: `planes` holds n_planes srcnn_plane_pair entries, `refs`
   * srcnn_tile_ref records, of which records [first, first + n) are taken;
   * X (each tile minus its footprint's mean) and T must hold n*tw*th floats
   * each, `means` (optional) n (srcnn_gather_batch). */
  Event gather_batch(MemoryHandle planes, size_t n_planes, MemoryHandle refs, size_t first, size_t n,
                     size_t tw, size_t th, MemoryHandle X, MemoryHandle T, MemoryHandle* means = nullptr,
                     Event* ev = nullptr);

  /** Forward of one layer over `sample_count` samples (reference :358-410). */
  Event execute_layer(Kernel&, const LayerData&, LayerAllocationPool&, MemoryHandle& gpu_buf_in,
                      size_t input_w, size_t input_h, size_t sample_count,
                      MemoryHandle& gpu_buf_out, Event* ev = nullptr);

  /** Sum of squared differences between the result and the ground-truth
   * centre; the value lands in `target` (reference :416-472). */
  Event squared_error(MemoryHandle gpu_buf_ground_truth, size_t ground_truth_w,
                      size_t ground_truth_h, size_t sample_count, MemoryHandle gpu_buf_algo_res,
                      MemoryHandle tmp_buffer, float& target, size_t total_padding,
                      Event* ev = nullptr);

  /** delta3 = (y - gt_centre) * [y > 0] (reference :474-520). */
  Event last_layer_delta(MemoryHandle gpu_buf_ground_truth, size_t ground_truth_w,
                         size_t ground_truth_h, size_t sample_count,
                         MemoryHandle gpu_buf_algo_res, MemoryHandle& gpu_buf_target,
                         size_t total_padding, Event* ev = nullptr);

  /** Deltas of `curr_layer` from the next layer's deltas (reference :522-594). */
  Event calculate_deltas(Kernel&, const LayerData& curr_layer, const LayerData& next_layer,
                         LayerAllocationPool& next_gpu_alloc, MemoryHandle curr_deltas,
                         MemoryHandle next_deltas, size_t next_layer_out_w,
                         size_t next_layer_out_h, size_t sample_count,
                         MemoryHandle curr_output, Event* ev = nullptr);

  /** Accumulate (+=) weight / bias gradients of one layer (reference
   * :596-663), summed race-free over samples. */
  Event backpropagate(LayerData&, MemoryHandle layer_input, MemoryHandle layer_deltas,
                      LayerAllocationPool&, size_t layer_out_w, size_t layer_out_h,
                      size_t sample_count, Event* ev = nullptr, size_t ev_cnt = 0);

  /** Momentum SGD with weight decay on one layer (reference :665-729). */
  Event update_parameters(LayerData&, LayerAllocationPool&, size_t batch_size, float momentum,
                          float w_decay, float learning_rate, Event* ev = nullptr);

  /** x -= mean(x); the mean is returned through `mean` (reference :268-280). */
  Event subtract_mean(MemoryHandle, float* mean = nullptr, Event* ev = nullptr);
  /** Blocking sum of all floats of the buffer, optionally squared (:282-313). */
  float sum(MemoryHandle, bool squared = false, Event* ev = nullptr);
  /** x -= value (reference :315-333). */
  Event subtract_from_all(MemoryHandle, float, Event* ev = nullptr);

  Kernel* create_layer_kernel(const LayerData&, bool skip_relu);
  Kernel* create_deltas_kernel(const LayerData&);

  void print_buffer(MemoryHandle, const char* name, size_t lines);

 protected:
  void check_initialized(int kernel_load_flags);
  virtual void load_kernels(int load_flags);
  bool allocation_has_right_size__(MemoryHandle, size_t, size_t line, const char* name);
  size_t element_count(MemoryHandle, size_t el_size);
  /** device scratch of at least `bytes` (grown on demand, stream-ordered) */
  void* scratch(size_t bytes);
  /** reduction workspace (second scratch: may be used beside scratch()) */
  void* reduce_scratch(size_t bytes);

  srcnn::Context* const _context;
  bool _initialized;
  int _loaded = 0;

  /** Single float. */
  MemoryHandle _tmp_gpu_float = gpu_nullptr;
  MemoryHandle _scratch = gpu_nullptr;
  MemoryHandle _reduce_scratch = gpu_nullptr;

  Kernel* _luma_kernel_norm = nullptr;
  Kernel* _luma_kernel_raw = nullptr;
  Kernel* _swap_luma_kernel = nullptr;
  Kernel* _upscale_luma_kernel = nullptr;
  Kernel* _upscale_compose_kernel = nullptr;
  Kernel* _yuv_upscale_luma_kernel = nullptr;
  Kernel* _upscale_planes_kernel = nullptr;
  Kernel* _yuv_compose_luma_kernel = nullptr;
  Kernel* _resize_luma_kernel = nullptr;
  Kernel* _resize_compose_kernel = nullptr;
  Kernel* _yuv_resize_luma_kernel = nullptr;
  Kernel* _resize_planes_kernel = nullptr;
  Kernel* _downscale_kernel = nullptr;
  Kernel* _gather_tiles_kernel = nullptr;
  Kernel* _gather_batch_kernel = nullptr;
  Kernel* _quality_kernel = nullptr;
  Kernel* _quality_frame_kernel = nullptr;
  Kernel* _downscale_frame_kernel = nullptr;
  Kernel* _squared_error_kernel = nullptr;
  Kernel* _sum_kernel = nullptr;
  Kernel* _sum_squared_kernel = nullptr;
  Kernel* _subtract_from_all_kernel = nullptr;
  Kernel* _last_layer_delta_kernel = nullptr;
  Kernel* _update_parameters_kernel = nullptr;
  Kernel* _backpropagate_kernel = nullptr;

 private:
  void pre_execute_layer_validation(const LayerData&, MemoryHandle, size_t, size_t);
};

}  // namespace cnn_sr

#endif  // CNN_SR_DATA_PIPELINE_HPP
