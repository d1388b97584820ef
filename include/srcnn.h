/*
 * srcnn.h -- C ABI of libsrcnn_hip.so, the MI355X (gfx950) SRCNN hot path.
 *
 * This is the drop-in boundary that replaces the reference's host/device
 * boundary (clEnqueue* inside src/opencl/Context.cpp and src/opencl/Kernel.cpp
 * of Scthe/cnn-Super-Resolution).  Plain pointers and sizes only; every
 * device pointer is HBM memory of the current device; every call is
 * stream-ordered on `stream` (a hipStream_t, NULL = the default stream).
 *
 * Numerics: fp32 throughout, same layouts as the reference:
 *   activations per-sample HWC  idx = s*C*W*H + (y*W + x)*C + c
 *               (src/kernel/layer_uber_kernel.cl:51-56)
 *   weights     W[dy][dx][c_in][c_out], c_out innermost
 *               (src/kernel/layer_uber_kernel.cl:3-13)
 *   flat net    [W1|B1|W2|B2|W3|B3] (one buffer, so one all-reduce covers
 *               every gradient; the per-layer LayerAllocationPool handles of
 *               src/DataPipeline.hpp:11-29 are views into it)
 *
 * Errors: every int-returning function returns SRCNN_OK (0) or a negative
 * SRCNN_ERR_*; srcnn_last_error() then holds a thread-local message.  Shape
 * validation mirrors the reference's runtime_error checks
 * (src/LayerData.cpp:20-42, src/DataPipeline.cpp:339-356, :62-86).
 *
 * Gradients are reduced deterministically (no float atomics): the racy
 * `target_grad_w[id] += grad_w` of src/kernel/backpropagate.cl:110 is
 * replaced by per-sample partial sums added in sample order.
 */
#ifndef SRCNN_H
#define SRCNN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SRCNN_API __attribute__((visibility("default")))
#define SRCNN_ABI_VERSION 1

enum {
  SRCNN_OK = 0,
  SRCNN_ERR_INVALID = -1,   /* bad shape / argument (reference: std::runtime_error) */
  SRCNN_ERR_HIP = -2,       /* HIP runtime failure (reference: check_error, Context.cpp:111-119) */
  SRCNN_ERR_WORKSPACE = -3, /* workspace smaller than the matching *_workspace_bytes() */
  SRCNN_ERR_ALLOC = -4,     /* device allocation failed */
  SRCNN_ERR_COMM = -5       /* RCCL failure (multi-GPU gradient reduction) */
};

typedef void* srcnn_stream_t; /* hipStream_t */
typedef void* srcnn_event_t;  /* hipEvent_t  */

SRCNN_API int srcnn_abi_version(void);
SRCNN_API const char* srcnn_last_error(void);

/* ---- runtime: replaces opencl::Context (src/opencl/Context.hpp:72-299) ---- */
SRCNN_API int srcnn_device_count(int* count);
SRCNN_API int srcnn_set_device(int device);                 /* Context::init, Context.cpp:45-79 */
SRCNN_API int srcnn_device_name(char* buf, size_t len);
SRCNN_API int srcnn_malloc(void** ptr, size_t bytes);       /* Context::allocate, Context.cpp:164-176 */
SRCNN_API int srcnn_free(void* ptr);                        /* RawMemoryHandle::release, Context.cpp:26-33 */
/* page-locked host memory, which an asynchronous copy needs in order to be
 * asynchronous (hipHostMalloc / hipHostFree; bytes == 0 gives NULL) */
SRCNN_API int srcnn_host_alloc(void** ptr, size_t bytes);
SRCNN_API int srcnn_host_free(void* ptr);
/* blocking H2D / D2H (write_buffer / read_buffer with block=true, Context.cpp:235-290) */
SRCNN_API int srcnn_memcpy_h2d(void* dst, const void* src, size_t bytes, srcnn_stream_t stream);
SRCNN_API int srcnn_memcpy_d2h(void* dst, const void* src, size_t bytes, srcnn_stream_t stream);
/* async D2D (copy_buffer, Context.cpp:312-341) */
SRCNN_API int srcnn_memcpy_d2d(void* dst, const void* src, size_t bytes, srcnn_stream_t stream);
/* async fill (zeros_float / fill_float, Context.cpp:296-310; no host vector) */
SRCNN_API int srcnn_fill_f32(float* dst, float value, size_t count, srcnn_stream_t stream);
SRCNN_API int srcnn_stream_create(srcnn_stream_t* stream);
SRCNN_API int srcnn_stream_destroy(srcnn_stream_t stream);
SRCNN_API int srcnn_stream_sync(srcnn_stream_t stream);     /* Context::block, Context.cpp:153-162 */
SRCNN_API int srcnn_device_sync(void);
SRCNN_API int srcnn_event_create(srcnn_event_t* ev);
SRCNN_API int srcnn_event_destroy(srcnn_event_t ev);
SRCNN_API int srcnn_event_record(srcnn_event_t ev, srcnn_stream_t stream);
SRCNN_API int srcnn_event_sync(srcnn_event_t ev);
SRCNN_API int srcnn_event_elapsed_ms(srcnn_event_t start, srcnn_event_t stop, float* ms);

/* HIP graphs (an MI355X extension; the reference enqueues every kernel
 * through clEnqueueNDRangeKernel each time, src/opencl/Kernel.cpp:85-116):
 * the library calls enqueued on `stream` between srcnn_graph_begin and
 * srcnn_graph_end are captured (thread-local stream capture) into one
 * replayable graph, with their arguments frozen -- e.g. one training step
 * (srcnn_train_step, or srcnn_train_fwd_bwd + srcnn_allreduce_grads +
 * srcnn_update_all) launched per step by srcnn_graph_launch without a
 * per-kernel host launch.  Profiling (srcnn_profile_enable) does not bracket
 * captured launches.  `stream` must be a created stream, not NULL. */
typedef void* srcnn_graph_t; /* hipGraphExec_t */
SRCNN_API int srcnn_graph_begin(srcnn_stream_t stream);
SRCNN_API int srcnn_graph_end(srcnn_stream_t stream, srcnn_graph_t* graph);
SRCNN_API int srcnn_graph_launch(srcnn_graph_t graph, srcnn_stream_t stream);
SRCNN_API int srcnn_graph_destroy(srcnn_graph_t graph);

/* ---- operators: one per reference L3 launcher (src/DataPipeline.hpp:62-175) ---- */

/* DataPipeline::execute_layer (src/DataPipeline.cpp:358-410) running kernel
 * `forward` (src/kernel/layer_uber_kernel.cl:36-96): valid correlation
 * f x f x n_prev -> n_cur, + bias, ReLU unless relu == 0 (SKIP_RELU).
 * in: [batch][in_h][in_w][n_prev]  out: [batch][in_h-f+1][in_w-f+1][n_cur] */
SRCNN_API int srcnn_conv_fwd(const float* in, float* out, const float* W,
                             const float* B, uint32_t in_w, uint32_t in_h,
                             uint32_t n_prev, uint32_t n_cur, uint32_t f,
                             int relu, uint32_t batch, srcnn_stream_t stream);

/* DataPipeline::last_layer_delta (src/DataPipeline.cpp:474-520), kernel
 * src/kernel/last_layer_delta.cl:14-50: d = (y - gt_centre) * [y > 0]. */
SRCNN_API int srcnn_last_delta(const float* gt, const float* y, float* d,
                               uint32_t gt_w, uint32_t gt_h, uint32_t out_w,
                               uint32_t out_h, uint32_t batch,
                               srcnn_stream_t stream);

/* DataPipeline::calculate_deltas (src/DataPipeline.cpp:522-594), kernel
 * src/kernel/layer_deltas.cl:42-127:
 *   d_curr[y,x,n] = [y_curr>0] * sum_{dy,dx,k} d_next[y-dy,x-dx,k] * W_next[dy,dx,n,k]
 * y_curr, d_curr: [batch][curr_h][curr_w][n_curr]
 * d_next:         [batch][curr_h-f_next+1][curr_w-f_next+1][n_next] */
SRCNN_API int srcnn_conv_delta(const float* d_next, const float* y_curr,
                               float* d_curr, const float* W_next,
                               uint32_t f_next, uint32_t n_curr,
                               uint32_t n_next, uint32_t curr_w,
                               uint32_t curr_h, uint32_t batch,
                               srcnn_stream_t stream);

/* DataPipeline::backpropagate (src/DataPipeline.cpp:596-663), kernel
 * src/kernel/backpropagate.cl:56-114: ACCUMULATES (+=) into gW / gB
 *   gW[dy,dx,k,n] += sum_s sum_{y,x} in_s[y+dy,x+dx,k] * d_s[y,x,n]
 *   gB[n]         += sum_s sum_{y,x} d_s[y,x,n]
 * in: [batch][out_h+f-1][out_w+f-1][n_prev]   d: [batch][out_h][out_w][n_cur] */
SRCNN_API size_t srcnn_conv_grad_workspace_bytes(uint32_t n_prev, uint32_t n_cur,
                                                 uint32_t f, uint32_t out_w,
                                                 uint32_t out_h, uint32_t batch);
SRCNN_API int srcnn_conv_grad_acc(const float* in, const float* delta,
                                  float* gW, float* gB, uint32_t n_prev,
                                  uint32_t n_cur, uint32_t f, uint32_t out_w,
                                  uint32_t out_h, uint32_t batch, void* ws,
                                  size_t ws_bytes, srcnn_stream_t stream);

/* DataPipeline::update_parameters (src/DataPipeline.cpp:665-729), kernel
 * src/kernel/update_parameters.cl:1-33:
 *   dW = mu*dW_prev + lr*gW + wd*W;  W -= dW / batch;  dW_prev = dW
 *   dB = mu*dB_prev + lr*gB;         B -= dB / batch;  dB_prev = dB */
SRCNN_API int srcnn_sgd_update(float* W, float* B, const float* gW,
                               const float* gB, float* dW_prev,
                               float* dB_prev, float momentum, float wd,
                               float lr, uint32_t batch, uint32_t nW,
                               uint32_t nB, srcnn_stream_t stream);

/* Deterministic reductions: DataPipeline::squared_error (src/DataPipeline.cpp:416-472,
 * kernel squared_error.cl:36-92) and DataPipeline::sum (:282-313, sum.cl:35-68).
 * The scalar result is written to device memory `result`. */
SRCNN_API size_t srcnn_reduce_workspace_bytes(size_t len);
SRCNN_API int srcnn_sq_err(const float* gt, const float* y, float* result,
                           uint32_t gt_w, uint32_t gt_h, uint32_t out_w,
                           uint32_t out_h, uint32_t batch, void* ws,
                           size_t ws_bytes, srcnn_stream_t stream);
SRCNN_API int srcnn_sum(const float* data, size_t len, int squared,
                        float* result, void* ws, size_t ws_bytes,
                        srcnn_stream_t stream);
/* DataPipeline::subtract_from_all (src/DataPipeline.cpp:315-333) */
SRCNN_API int srcnn_sub_scalar(float* data, float value, size_t len,
                               srcnn_stream_t stream);
/* DataPipeline::subtract_mean (src/DataPipeline.cpp:268-280) without the
 * host round trip: mean = sum/len computed and subtracted on the device,
 * also stored to `mean` (device, may be NULL). */
SRCNN_API int srcnn_sub_mean(float* data, size_t len, float* mean, void* ws,
                             size_t ws_bytes, srcnn_stream_t stream);
/* DataPipeline::extract_luma (src/DataPipeline.cpp:186-220, extract_luma.cl:7-23):
 * rgba [h][w][4] u8 -> luma [h][w] f32 (/255 if normalize). */
SRCNN_API int srcnn_extract_luma(const uint8_t* rgba, float* luma, uint32_t w,
                                 uint32_t h, int normalize,
                                 srcnn_stream_t stream);
/* DataPipeline::swap_luma (src/DataPipeline.cpp:222-266, swap_luma.cl:18-69):
 * new luma (centre luma_w x luma_h) + original CbCr -> rgb [h][w][3] u8. */
SRCNN_API int srcnn_swap_luma(const uint8_t* rgba, const float* new_luma,
                              uint8_t* rgb, uint32_t w, uint32_t h,
                              uint32_t luma_w, uint32_t luma_h,
                              srcnn_stream_t stream);

/* Upscaling front and back end (an MI355X extension; the reference expects an
 * input that is already scaled and has no counterpart).  scale s is 1, 2, 3
 * or 4; W = s*w, H = s*h.  The resampling is the separable Keys bicubic
 * (a = -0.5) at half-pixel centres with source indices clamped to the image,
 * fp32, horizontal pass first (DESIGN.md 10.1 is the spec).
 *
 * srcnn_upscale_luma: rgba [h][w][4] u8 -> luma_padded [(H+pad)][(W+pad)] f32:
 * plane[Y][X] is the bicubic value of the normalised luma (srcnn_extract_luma
 * with normalize) at X' = clamp(X - pad/2, 0, W-1), Y' = clamp(Y - pad/2, 0,
 * H-1), i.e. the upscaled luma with its edge replicated into a margin of
 * pad/2 pixels on the left and top and pad - pad/2 on the right and bottom.
 * A net with total padding `pad` turns this plane into exactly W x H outputs.
 * With s = 1 the interior is srcnn_extract_luma's output bit for bit.
 *
 * srcnn_upscale_compose: the same bicubic applied to the source's r, g, b
 * (unclamped floats) + new_luma [H][W] -> rgb [H][W][3] u8, with
 * srcnn_swap_luma's constants, clamp and truncation.  With s = 1 it is
 * srcnn_swap_luma(w, h, w, h) byte for byte.
 *
 * SRCNN_ERR_INVALID: scale outside 1..4, w or h zero, a null buffer, or a size
 * beyond the kernels' 32-bit index (the plane's floats and the rgb bytes must
 * each number at most 2^31-1). */
SRCNN_API int srcnn_upscale_luma(const uint8_t* rgba, float* luma_padded, uint32_t w, uint32_t h,
                                 uint32_t scale, uint32_t pad, srcnn_stream_t stream);
SRCNN_API int srcnn_upscale_compose(const uint8_t* rgba, const float* new_luma, uint8_t* rgb,
                                    uint32_t w, uint32_t h, uint32_t scale,
                                    srcnn_stream_t stream);

/* The same front and back end for planar Y'CbCr frames with 8-bit samples
 * (DESIGN.md 14 is the spec).  A plane is rows of bytes `pitch` bytes apart,
 * pitch >= the row's width; the bytes between a row's end and the next row are
 * never read and never written.  `range` selects how a Y byte maps to the
 * net's luma v:
 *   SRCNN_YUV_FULL     v = Y / 255            Y = rint(v * 255)
 *   SRCNN_YUV_LIMITED  v = (Y - 16) / 219     Y = rint(v * 219 + 16)
 * in fp32, Y clamped to [0, 255] after rounding to nearest, ties to even (not
 * the truncation srcnn_swap_luma inherits from the reference).
 *
 * srcnn_yuv_upscale_luma: Y [h][w] u8 -> luma_padded [(H+pad)][(W+pad)] f32,
 * srcnn_upscale_luma's plane (same resampling, same margins) of the luma v.
 * With s = 1 and full range the interior is float(Y) / 255.0f bit for bit.
 *
 * srcnn_upscale_planes_u8: src0, src1 [ph][pw] u8 -> dst0, dst1 [oh][ow] u8:
 * the top-left ow x oh of the bicubic x s of each plane, rounded to nearest
 * (ties to even) and clamped to [0, 255]; s*(pw-1) < ow <= s*pw and
 * s*(ph-1) < oh <= s*ph.  One call resamples a frame's two chroma planes; the
 * crop is what odd luma sizes need.  With s = 1 the output
 * is the source byte for byte.
 *
 * srcnn_yuv_compose_luma: luma [H][W] f32 (the net's output) -> Y [H][W] u8.
 *
 * SRCNN_ERR_INVALID: scale outside 1..4, a zero size, a pitch below the row's
 * width, an unknown range, an output size outside the bounds above, a null
 * buffer, or more than 2^31-1 elements in a plane. */
enum { SRCNN_YUV_LIMITED = 0, SRCNN_YUV_FULL = 1 };
SRCNN_API int srcnn_yuv_upscale_luma(const uint8_t* y, uint32_t pitch_y, float* luma_padded,
                                     uint32_t w, uint32_t h, uint32_t scale, uint32_t pad,
                                     int range, srcnn_stream_t stream);
SRCNN_API int srcnn_upscale_planes_u8(const uint8_t* src0, const uint8_t* src1,
                                      uint32_t src_pitch, uint32_t pw, uint32_t ph, uint8_t* dst0,
                                      uint8_t* dst1, uint32_t dst_pitch, uint32_t ow, uint32_t oh,
                                      uint32_t scale, srcnn_stream_t stream);
SRCNN_API int srcnn_yuv_compose_luma(const float* luma, uint8_t* y, uint32_t pitch_y, uint32_t W,
                                     uint32_t H, int range, srcnn_stream_t stream);

/* The same three for samples of 8 to 16 bits and for semi-planar chroma (NV12,
 * P010 / P012 / P016): DESIGN.md 15 is the spec.  At bits = 8 a sample is one
 * byte; above, it is a 16-bit little-endian word x that holds the value
 *   msb = 0   Y = x                  (Y4M's p10 family; nothing is masked)
 *   msb = 1   Y = x >> (16 - bits)   (P010 family); msb = 1 at 8 bits is invalid
 * A written sample is q = clamp(rint(.), 0, 2^bits - 1), stored as q or as
 * q << (16 - bits) with the low bits zero.  With k = 2^(bits-8):
 *   SRCNN_YUV_FULL     v = Y / (2^bits - 1)       Y = rint(v * (2^bits - 1))
 *   SRCNN_YUV_LIMITED  v = (Y - 16 k) / (219 k)   Y = rint(v * 219 k + 16 k)
 * in fp32; at bits = 8 these are the formulas above, and the three calls give
 * the results of the 8-bit calls byte for byte.  Chroma values are resampled as
 * they are and clamped to [0, 2^bits - 1] after rounding to nearest.
 *
 * Pitches are in bytes and at least the row's bytes: with B bytes per sample
 * w*B for luma, pw*B for a planar chroma plane, 2*pw*B for a semi-planar one.
 * For two-byte samples every plane address and every pitch must be even.  The
 * bytes between a row's end and the next row are never read and never written.
 *
 * srcnn_upscale_planes: layout SRCNN_YUV_PLANAR: src0, src1 [ph][pw] -> dst0,
 * dst1 [oh][ow] as srcnn_upscale_planes_u8 does.  SRCNN_YUV_SEMIPLANAR: src0
 * [ph][pw][2] holds (U, V) pairs -> dst0 [oh][ow][2]; src1 and dst1 must be
 * NULL; pw, ow and the crop rule count pairs; every sample equals that of the
 * planar call on the two de-interleaved planes.  With s = 1 the output is the
 * source for every sample within [0, 2^bits - 1].
 *
 * SRCNN_ERR_INVALID: what the 8-bit calls reject, plus bits outside 8..16, msb
 * not 0 or 1 or 1 at 8 bits, an unknown layout, an odd address or pitch for
 * two-byte samples, a plane pointer that the layout does not have (or lacks
 * one it has), or more than 2^31-1 samples in a plane (a semi-planar chroma
 * plane counts 2*pw*ph). */
enum { SRCNN_YUV_PLANAR = 0, SRCNN_YUV_SEMIPLANAR = 1 };
SRCNN_API int srcnn_yuv_upscale_luma16(const void* y, uint32_t pitch_y, float* luma_padded,
                                       uint32_t w, uint32_t h, uint32_t scale, uint32_t pad,
                                       uint32_t bits, uint32_t msb, int range,
                                       srcnn_stream_t stream);
SRCNN_API int srcnn_yuv_compose_luma16(const float* luma, void* y, uint32_t pitch_y, uint32_t W,
                                       uint32_t H, uint32_t bits, uint32_t msb, int range,
                                       srcnn_stream_t stream);
SRCNN_API int srcnn_upscale_planes(const void* src0, const void* src1, uint32_t src_pitch,
                                   uint32_t pw, uint32_t ph, void* dst0, void* dst1,
                                   uint32_t dst_pitch, uint32_t ow, uint32_t oh, uint32_t scale,
                                   uint32_t bits, uint32_t msb, uint32_t layout,
                                   srcnn_stream_t stream);

/* The same front and back end for any output size (DESIGN.md 16 is the spec):
 * the source is w x h, the output W x H with w <= W <= 4w and h <= H <= 4h,
 * each axis on its own (only upscaling, so nothing is antialiased).  The
 * resampling is the one above with the ratio as a fraction: the source step
 * per output sample is rn / rd (w / W, h / H); for output index X',
 * n = (2X'+1) rn - rd, D = 2 rd, b = floor(n / D), t = (n - b D) / D, taps
 * b-1 .. b+2 clamped to the source, the Keys weights at t+1, t, 1-t, 2-t
 * computed in double and rounded once to fp32.  Margins, luma, composition,
 * rounding, sample formats, pitches and ranges are those of the calls above.
 * At an integer ratio the results meet the same bounds as the scale calls'
 * but need not equal them bit for bit.
 *
 * srcnn_resize_luma: rgba [h][w][4] u8 -> luma_padded [(H+pad)][(W+pad)] f32.
 * With W = w and H = h the interior is srcnn_extract_luma's output bit for bit.
 * srcnn_resize_compose: rgba + new_luma [H][W] -> rgb [H][W][3] u8.  With
 * W = w and H = h it is srcnn_swap_luma(w, h, w, h) byte for byte.
 * srcnn_yuv_resize_luma: Y [h][w] of `bits` bits -> luma_padded; with W = w,
 * H = h and full range the interior is float(Y) / float(2^bits - 1).
 * srcnn_resize_planes: src0, src1 [ph][pw] -> dst0, dst1 [oh][ow] (or (U, V)
 * pairs in src0 / dst0, as srcnn_upscale_planes) at the explicit ratios
 * rx_num / rx_den and ry_num / ry_den; ow <= ceil(pw * rx_den / rx_num) and
 * oh <= ceil(ph * ry_den / ry_num).  A frame's chroma is resampled at the
 * luma's ratios w / W and h / H, not at CW / cw: DESIGN.md 14.1's crop rule,
 * generalised.  At ratios 1/1 the output is the source sample for sample.
 *
 * SRCNN_ERR_INVALID, before any launch: a zero size; W < w, W > 4w, H < h or
 * H > 4h; a ratio whose den / num lies outside [1, 4] or a zero numerator; ow
 * or oh beyond its bound; whatever the scale calls reject for pitches, bits,
 * msb, layout, range and null pointers; more than 2^31-1 plane floats, rgb
 * bytes or samples in a plane. */
SRCNN_API int srcnn_resize_luma(const uint8_t* rgba, float* luma_padded, uint32_t w, uint32_t h,
                                uint32_t W, uint32_t H, uint32_t pad, srcnn_stream_t stream);
SRCNN_API int srcnn_resize_compose(const uint8_t* rgba, const float* new_luma, uint8_t* rgb,
                                   uint32_t w, uint32_t h, uint32_t W, uint32_t H,
                                   srcnn_stream_t stream);
SRCNN_API int srcnn_yuv_resize_luma(const void* y, uint32_t pitch_y, float* luma_padded, uint32_t w,
                                    uint32_t h, uint32_t W, uint32_t H, uint32_t pad, uint32_t bits,
                                    uint32_t msb, int range, srcnn_stream_t stream);
SRCNN_API int srcnn_resize_planes(const void* src0, const void* src1, uint32_t src_pitch,
                                  uint32_t pw, uint32_t ph, void* dst0, void* dst1,
                                  uint32_t dst_pitch, uint32_t ow, uint32_t oh, uint32_t rx_num,
                                  uint32_t rx_den, uint32_t ry_num, uint32_t ry_den, uint32_t bits,
                                  uint32_t msb, uint32_t layout, srcnn_stream_t stream);

/* Training pairs from a full-size image, on the device (an MI355X extension;
 * the reference's pairs are made on the host, one file per sample).  The
 * training-side mirror of the upscaling front end: DESIGN.md 11.1 is the spec.
 *
 * srcnn_downscale_rgba: rgba [H][W][4] u8 -> small [H/s][W/s][4] u8 (integer
 * division; s = 1, 2, 3 or 4; W >= s, H >= s): the antialiased Keys bicubic
 * (a = -0.5, stretched by s) at half-pixel centres, source indices clamped to
 * the image, separable, fp32, horizontal pass first, rounded to nearest;
 * alpha = 255.  The trailing W - s*(W/s) columns and H - s*(H/s) rows have no
 * output pixel of their own but are tap sources.  With s = 1 the r, g, b bytes
 * are the source's.  Downscaling by s and srcnn_upscale_luma by s are aligned:
 * no shift between them.
 *
 * srcnn_gather_tiles: plane [ph][pw] f32 -> tiles [nx*ny][th][tw] f32; tile
 * i = iy*nx + ix is the window at (x0 + ix*stride, y0 + iy*stride).  With
 * sub_mean != 0 each tile has its own mean subtracted (srcnn_sub_mean per
 * sample): a fixed-order fp32 sum that depends on tw x th alone -- not on the
 * grid, the neighbouring tiles or what lies around the buffers -- divided by
 * (float)(tw*th); means (device, may be NULL) [nx*ny] then gets each tile's
 * mean.  With sub_mean == 0 the tiles are copies and means is not touched.
 * Writes exactly the nx*ny*th*tw floats of tiles (and the nx*ny of means).
 *
 * SRCNN_ERR_INVALID, before any launch: scale outside 1..4; W < s or H < s;
 * stride, nx, ny, tw or th zero; a grid that leaves the plane (x0 +
 * (nx-1)*stride + tw > pw, likewise in y); a null buffer; or a size beyond the
 * kernels' 32-bit index: the source's pixels W*H, the plane's floats pw*ph and
 * the tile count nx*ny must each number at most 2^31-1. */
SRCNN_API int srcnn_downscale_rgba(const uint8_t* rgba, uint8_t* small, uint32_t W, uint32_t H,
                                   uint32_t scale, srcnn_stream_t stream);
SRCNN_API int srcnn_gather_tiles(const float* plane, uint32_t pw, uint32_t ph, uint32_t x0,
                                 uint32_t y0, uint32_t stride, uint32_t nx, uint32_t ny,
                                 uint32_t tw, uint32_t th, int sub_mean, float* tiles,
                                 float* means, srcnn_stream_t stream);

/* One training chunk gathered straight from resident luma planes, in one
 * launch (an MI355X extension; the reference packs a chunk with two buffer
 * copies per sample, src/ConfigBasedDataPipeline.cpp:373-379): DESIGN.md 13 is
 * the spec.  Both tables live in device memory and have fixed layouts: little-
 * endian, the fields at the offsets their order gives, no padding (32 and 16
 * bytes).
 *
 * srcnn_plane_pair: the two planes of one image cut at scale s: x = what
 * srcnn_upscale_luma(small, W/s, H/s, s, pad = 0) writes (pitch Wc), t = what
 * srcnn_extract_luma(rgba, normalize) writes (pitch W), w = Wc, h = Hc: the two
 * planes srcnn_make_pairs builds in its workspace.
 *
 * srcnn_tile_ref: one sample.  The output tile is tw x th; op is an element of
 * the dihedral group: bit 0 mirrors the footprint's columns, bit 1 its rows,
 * bit 2 transposes afterwards (numpy: flip rows, flip columns, then .T).  The
 * source footprint at (x, y) is sw x sh = tw x th, or th x tw when bit 2 is
 * set; output element (r, c) takes the footprint's element (a', b'), where
 * (a, b) = bit 2 ? (c, r) : (r, c), a' = bit 1 ? sh-1-a : a, b' = bit 0 ?
 * sw-1-b : b.  X and T take the same permutation.
 *
 * X [n][th][tw]: each tile minus its footprint's mean, bit for bit the stated
 * permutation of srcnn_gather_tiles(x plane, x0 = x, y0 = y, nx = ny = 1, tw =
 * sw, th = sh, sub_mean = 1): the same fixed-order sum, over the footprint in
 * its own row-major order, whatever op, the neighbouring records, their order
 * or the pitches are.  T [n][th][tw]: the permutation of the t plane's values.
 * means (device, [n], may be NULL) receives each record's mean.
 *
 * The records are device data, so they are checked on the device: a record
 * with plane >= n_planes, op > 7, x + sw > w or y + sh > h (no 32-bit
 * wrap-around in the sums) reads nothing of any plane and gets a tile of quiet
 * NaNs in X and in T, and NaN in means.  Plane indexing is 64-bit: a plane of
 * any size is legal.
 *
 * SRCNN_ERR_INVALID, before any launch: null planes, refs, X or T; n_planes,
 * tw or th zero; tw*th beyond 2^31-1.  n = 0 is SRCNN_OK with no launch.
 * Stream-ordered, no workspace; writes exactly the n*tw*th floats of X and of
 * T and the n of means. */
typedef struct {             /* 32 bytes */
  const float* x;            /* degraded luma plane, [h][x_pitch] */
  const float* t;            /* ground-truth luma plane, [>= h][t_pitch] */
  uint32_t x_pitch, t_pitch; /* row pitches in floats, each >= w */
  uint32_t w, h;             /* the extent tiles may be cut from, common to both */
} srcnn_plane_pair;

typedef struct {             /* 16 bytes */
  uint32_t plane;            /* index into the plane table */
  uint32_t x, y;             /* origin of the source footprint */
  uint32_t op;               /* orientation, 0..7 */
} srcnn_tile_ref;

SRCNN_API int srcnn_gather_batch(const srcnn_plane_pair* planes, uint32_t n_planes,
                                 const srcnn_tile_ref* refs, uint32_t n, uint32_t tw, uint32_t th,
                                 float* X, float* T, float* means, srcnn_stream_t stream);

/* One full-size image ->the (X, T) tile batches srcnn_train_fwd_bwd reads:
 * X [count][tile][tile] = the image degraded by exactly the resampling the
 * inference path applies (down by s, then srcnn_upscale_luma by s), each tile
 * minus its own mean; T [count][tile][tile] = the image's own luma.  The grid:
 * Wc = s*(W/s), Hc = s*(H/s); nx = (Wc-tile)/stride + 1, ny likewise, origin
 * (0, 0), tile i = iy*nx + ix.  srcnn_make_pairs_count returns count = nx*ny
 * (nx, ny may be NULL), 0 if the image is too small for one tile or an
 * argument is invalid.
 *
 * Byte-identical to srcnn_downscale_rgba -> srcnn_upscale_luma(small, W/s,
 * H/s, s, pad = 0) into the X plane [Hc][Wc] -> srcnn_extract_luma(rgba,
 * normalize) into the T plane [H][W] -> srcnn_gather_tiles(X plane, sub_mean =
 * 1) -> srcnn_gather_tiles(T plane, sub_mean = 0): five launches per image.
 * Stream-ordered, no host synchronisation, no allocation.  `ws` holds the
 * low-resolution image and the two planes (each 256-byte aligned) under the
 * memory contract at srcnn_train_workspace_bytes; the call writes every one of
 * the count*tile*tile floats of X and of T.  srcnn_make_pairs_workspace_bytes
 * returns 0 for an invalid scale or size.  Errors as srcnn_downscale_rgba and
 * srcnn_gather_tiles (tile or stride zero, count zero), with srcnn_upscale_luma's
 * limit on the cropped size (3*Wc*Hc at most 2^31-1), plus SRCNN_ERR_WORKSPACE for a
 * workspace that is too small. */
SRCNN_API size_t srcnn_make_pairs_count(uint32_t W, uint32_t H, uint32_t scale, uint32_t tile,
                                        uint32_t stride, uint32_t* nx, uint32_t* ny);
SRCNN_API size_t srcnn_make_pairs_workspace_bytes(uint32_t W, uint32_t H, uint32_t scale);
SRCNN_API int srcnn_make_pairs(const uint8_t* rgba, uint32_t W, uint32_t H, uint32_t scale,
                               uint32_t tile, uint32_t stride, float* X, float* T, void* ws,
                               size_t ws_bytes, srcnn_stream_t stream);

/* PSNR and SSIM of two images, on the device (an MI355X extension; the
 * reference has no metric code: DESIGN.md 12.1 is the spec).  a and b are W x H
 * pixels, each in its own format and with its own row pitch in pixels (pitch
 * >= W; a sub-window of a larger image is a pointer offset plus the pitch):
 *   SRCNN_PIX_RGB8      3 bytes per pixel, any byte alignment of the base
 *                       (what srcnn_upscale writes)
 *   SRCNN_PIX_RGBA8     4 bytes per pixel, 4-byte aligned (the decoders',
 *                       srcnn_downscale_rgba's)
 *   SRCNN_PIX_LUMA_F32  normalised luma (srcnn_extract_luma with normalize,
 *                       srcnn_forward), 4-byte aligned
 * Both are measured on the luma at the 0 - 255 scale, Y = 0.299f r + 0.587f g
 * + 0.114f b with srcnn_extract_luma's operation sequence (Y = 255.0f v for
 * the float format), not rounded, not clamped: the project's full-range luma,
 * not Matlab's studio-range rgb2ycbcr.  `shave` pixels are dropped on all four
 * sides first; Ws = W - 2*shave and Hs = H - 2*shave must be at least 11.
 *
 * result (device, 3 doubles) = {mse, psnr, ssim}: mse = the mean over Ws*Hs of
 * (Ya - Yb)^2, each square formed in fp32 and summed in double; psnr =
 * 10 log10(255^2 / mse), +inf for mse == 0; ssim = the mean over the
 * (Ws-10) x (Hs-10) valid placements of the 11 x 11 Gaussian window (sigma
 * 1.5) of Wang et al.'s SSIM with C1 = (0.01*255)^2, C2 = (0.03*255)^2, fp32
 * per window on the lumas centred at 128, summed in double.  Identical images
 * give exactly {0, +inf, 1}.  No atomics: the order of both sums depends on
 * (Ws, Hs) alone -- not on the pitches, the formats, where the window sits in
 * a larger buffer or what lies around it -- so that srcnn_quality(shave = k)
 * is bit-identical to the call on the pointer-offset interior with shave = 0,
 * and two calls on the same inputs are bit-identical.
 *
 * `ws` (srcnn_quality_workspace_bytes: two doubles per workgroup) falls under
 * the memory contract at srcnn_train_workspace_bytes; the call writes the
 * three doubles of result and reads a and b inside the shaved window only.
 * Stream-ordered, two launches, no host synchronisation.
 *
 * SRCNN_ERR_INVALID, before any launch: an unknown format; a null buffer;
 * pitch < W; Ws < 11 or Hs < 11 (2*shave wrapping around included); an RGBA8
 * or F32 base that is not 4-byte aligned (result and ws, which hold doubles:
 * 8-byte); or a size beyond the kernels' 32-bit index (pitch*H pixels of
 * either image must number at most 2^31-1).
 * SRCNN_ERR_WORKSPACE for a workspace that is too small;
 * srcnn_quality_workspace_bytes returns 0 for invalid sizes. */
enum { SRCNN_PIX_LUMA_F32 = 1, SRCNN_PIX_RGB8 = 3, SRCNN_PIX_RGBA8 = 4 };
SRCNN_API size_t srcnn_quality_workspace_bytes(uint32_t W, uint32_t H, uint32_t shave);
SRCNN_API int srcnn_quality(const void* a, int fmt_a, uint32_t pitch_a, const void* b, int fmt_b,
                            uint32_t pitch_b, uint32_t W, uint32_t H, uint32_t shave,
                            double* result, void* ws, size_t ws_bytes, srcnn_stream_t stream);

/* ---- network level: ConfigBasedDataPipeline (src/ConfigBasedDataPipeline.cpp) ---- */
typedef struct srcnn_net {
  uint32_t n1, n2, f1, f2, f3; /* Config n1,n2,f1,f2,f3 (src/Config.hpp:27-28) */
} srcnn_net;

/* Resolve, on the current device, every gfx950 kernel the net-level calls
 * (srcnn_train_fwd_bwd, srcnn_update_all, srcnn_forward, srcnn_upscale,
 * srcnn_upscale_yuv, srcnn_upscale_to, srcnn_upscale_frame_to) launch for this
 * net, and the kernels of srcnn_make_pairs, srcnn_quality,
 * srcnn_quality_frame and srcnn_downscale_planes.
 * No kernel runs.  The HIP runtime otherwise sets a kernel up lazily at its
 * first launch; resolving them beforehand keeps that out of the first step
 * (the reference builds its kernels up front too: src/ConfigBasedDataPipeline
 * .cpp:54-75 create_layer_kernel / create_deltas_kernel at init). */
SRCNN_API int srcnn_preload(const srcnn_net* net);

/* offsets (in floats) of W1,B1,W2,B2,W3,B3 inside the flat parameter buffer */
SRCNN_API int srcnn_net_offsets(const srcnn_net* net, size_t offsets[6]);
SRCNN_API size_t srcnn_net_param_count(const srcnn_net* net);

/* One chunk of ConfigBasedDataPipeline::execute_batch(backpropagate=true)
 * (src/ConfigBasedDataPipeline.cpp:128-195): forward L1..L3 (:200-241),
 * last-layer delta, deltas and gradients (:243-323).  Gradients are
 * ACCUMULATED into `grads` (flat layout).  X = mean-subtracted input luma,
 * T = ground-truth luma, both [batch][h][w].  If sq_err != NULL the chunk's
 * squared error (validation metric) is ADDED to *sq_err (device).
 *
 * Memory contract of every call that takes a workspace (the net-level calls
 * here and below, srcnn_conv_grad_acc and the reductions):
 *   - `ws` is ws_bytes >= the matching *_workspace_bytes() of device memory
 *     (exactly that many suffice) and needs NO initialisation: the call reads nothing of
 *     `ws` that a kernel of the same call has not written before (its previous
 *     contents -- zeros, NaN, anything -- never reach a result);
 *   - the call writes nothing outside [ws, ws + ws_bytes) and the documented
 *     extent of its outputs (grads: srcnn_net_param_count floats; sq_err: one
 *     float; params / momentum_bufs / params_out / mom_out likewise; out: the
 *     A3 extent; srcnn_train_activations: the three extents it documents;
 *     rgb: 3*W*H bytes; srcnn_upscale_yuv: the row bytes of dst's three
 *     planes, not the pitch gaps between them; srcnn_make_pairs: count*tile*tile floats of X and of
 *     T each; srcnn_gather_batch, which takes no workspace: n*tw*th floats of
 *     X and of T each and the n of means; srcnn_quality / srcnn_evaluate /
 *     srcnn_quality_frame / srcnn_evaluate_frame: the 3 / 6 / 8 / 16 doubles of
 *     result; srcnn_make_pairs_frame as srcnn_make_pairs);
 *   - buffers the call only reads (X, T, params) are not written, and nothing
 *     outside their extent reaches a result.
 * The results are bit-identical whatever `ws` held before and whatever lies
 * around the buffers (tests/test_memory_hygiene_gpu.py pins this with
 * exact-size poisoned workspaces and guard bands). */
SRCNN_API size_t srcnn_train_workspace_bytes(const srcnn_net* net, uint32_t w,
                                             uint32_t h, uint32_t batch);
SRCNN_API int srcnn_train_fwd_bwd(const srcnn_net* net, const float* X,
                                  const float* T, uint32_t w, uint32_t h,
                                  uint32_t batch, const float* params,
                                  float* grads, float* sq_err, void* ws,
                                  size_t ws_bytes, srcnn_stream_t stream);

/* ConfigBasedDataPipeline::update_parameters (src/ConfigBasedDataPipeline.cpp:325-361):
 * update all layers with per-layer lr[3], shared momentum / wd, then zero
 * the gradient accumulators (:353-358).  batch must be > 0 (the update
 * divides by it, update_parameters.cl:22). */
SRCNN_API int srcnn_update_all(const srcnn_net* net, float* params,
                               float* grads, float* momentum_bufs,
                               float momentum, float wd, const float* lr,
                               uint32_t batch, srcnn_stream_t stream);

/* Forward / inference (src/ConfigBasedDataPipeline.cpp:114-126, :200-241):
 * out = A3 [batch][h-pad][w-pad], pad = f1+f2+f3-3.  The memory contract at
 * srcnn_train_workspace_bytes holds here too: `ws` (srcnn_forward_workspace_bytes
 * bytes suffice) needs no initialisation, the call reads nothing of it that it
 * did not write itself, and it writes only inside `ws` and the
 * batch x (h-pad) x (w-pad) floats of `out`, every one of which it writes. */
SRCNN_API size_t srcnn_forward_workspace_bytes(const srcnn_net* net,
                                               uint32_t w, uint32_t h,
                                               uint32_t batch);
SRCNN_API int srcnn_forward(const srcnn_net* net, const float* X, uint32_t w,
                            uint32_t h, uint32_t batch, const float* params,
                            float* out, void* ws, size_t ws_bytes,
                            srcnn_stream_t stream);

/* Low-resolution image in, super-resolved image out, on the device:
 * srcnn_upscale_luma (pad = f1+f2+f3-3) -> srcnn_sub_mean over the whole
 * padded plane (what the net sees; as in the reference flow the mean is not
 * added back) -> srcnn_forward -> srcnn_upscale_compose.  rgba [h][w][4] u8 ->
 * rgb [scale*h][scale*w][3] u8; every output pixel passes through the net, no
 * border frame is left.  Works for every net srcnn_forward accepts and is
 * byte-identical to those four calls; stream-ordered, no host synchronisation,
 * no allocation.  `ws` holds the plane, the net output, the reduction scratch
 * and the forward workspace (each 256-byte aligned) under the memory contract
 * at srcnn_train_workspace_bytes.  srcnn_upscale_workspace_bytes returns 0 for
 * an invalid net, scale or size.  Errors as srcnn_upscale_luma, plus
 * SRCNN_ERR_INVALID for an invalid net and SRCNN_ERR_WORKSPACE for a
 * workspace that is too small. */
SRCNN_API size_t srcnn_upscale_workspace_bytes(const srcnn_net* net, uint32_t w, uint32_t h,
                                               uint32_t scale);
SRCNN_API int srcnn_upscale(const srcnn_net* net, const uint8_t* rgba, uint32_t w, uint32_t h,
                            uint32_t scale, const float* params, uint8_t* rgb, void* ws,
                            size_t ws_bytes, srcnn_stream_t stream);

/* One planar Y'CbCr frame in, the super-resolved frame out, on the device.
 * Only luma passes through the net; chroma is resampled as bytes.  The frame
 * is w x h luma samples with chroma subsampled by (cx, cy) = (2, 2) for 4:2:0,
 * (2, 1) for 4:2:2 or (1, 1) for 4:4:4: u and v are [ceil(h/cy)][ceil(w/cx)].
 * The output frame is W x H = s*w x s*h with chroma [ceil(H/cy)][ceil(W/cx)].
 * The call is
 *   srcnn_yuv_upscale_luma(src->y, pad = f1+f2+f3-3) -> plane
 *   srcnn_sub_mean over the whole padded plane (not added back, as in
 *     srcnn_upscale)
 *   srcnn_forward(plane) -> out [H][W]
 *   srcnn_yuv_compose_luma(out -> dst->y)
 *   srcnn_upscale_planes_u8(src->u, src->v -> dst->u, dst->v)
 * and byte-identical to those calls; it works for every net srcnn_forward
 * accepts; stream-ordered, no host synchronisation, no allocation.  `ws` holds
 * the plane, the net output, the reduction scratch and the forward workspace
 * (each 256-byte aligned) under the memory contract at
 * srcnn_train_workspace_bytes; of dst it writes the W bytes of each Y row and
 * the ceil(W/cx) bytes of each u and v row and nothing between the rows.
 * srcnn_upscale_yuv_workspace_bytes returns 0 where the call would be invalid.
 * Errors as the op-level calls, before any launch, plus SRCNN_ERR_INVALID for
 * an invalid net or a subsampling other than the three and
 * SRCNN_ERR_WORKSPACE for a workspace that is too small. */
typedef struct srcnn_yuv_frame {
  uint8_t *y, *u, *v;        /* device planes (of src only read) */
  uint32_t pitch_y, pitch_c; /* bytes between rows of y, and of u and v */
} srcnn_yuv_frame;
SRCNN_API size_t srcnn_upscale_yuv_workspace_bytes(const srcnn_net* net, uint32_t w, uint32_t h,
                                                   uint32_t scale);
SRCNN_API int srcnn_upscale_yuv(const srcnn_net* net, const srcnn_yuv_frame* src,
                                const srcnn_yuv_frame* dst, uint32_t w, uint32_t h, uint32_t cx,
                                uint32_t cy, uint32_t scale, int range, const float* params,
                                void* ws, size_t ws_bytes, srcnn_stream_t stream);

/* srcnn_upscale_yuv for every frame format of DESIGN.md 15: fmt names the
 * sample format (bits, msb), the chroma layout, the subsampling (cx, cy) and
 * the range; source and output frame have the same format.  src and dst are
 * srcnn_yuv_frame: their uint8_t* members are byte addresses whatever the
 * sample size, their pitches are bytes; with SRCNN_YUV_SEMIPLANAR u holds the
 * (U, V) pairs and v must be NULL, in src and in dst.  The call is
 *   srcnn_yuv_upscale_luma16(src->y, pad = f1+f2+f3-3) -> plane
 *   srcnn_sub_mean, srcnn_forward as in srcnn_upscale_yuv
 *   srcnn_yuv_compose_luma16(out -> dst->y)
 *   srcnn_upscale_planes(src->u, src->v -> dst->u, dst->v)
 * and byte-identical to those calls; with {8, 0, SRCNN_YUV_PLANAR, cx, cy,
 * range} it is srcnn_upscale_yuv byte for byte.  Stream-ordered, no
 * allocation; the workspace is srcnn_upscale_yuv_workspace_bytes(net, w, h,
 * scale) under the same memory contract; of dst it writes the samples of each
 * row and nothing between the rows.  Errors as the op-level calls and as
 * srcnn_upscale_yuv, before any launch, plus SRCNN_ERR_INVALID for a null
 * fmt. */
typedef struct srcnn_yuv_format {
  uint32_t bits, msb, layout, cx, cy;
  int32_t range;
} srcnn_yuv_format;
SRCNN_API int srcnn_upscale_frame(const srcnn_net* net, const srcnn_yuv_format* fmt,
                                  const srcnn_yuv_frame* src, const srcnn_yuv_frame* dst,
                                  uint32_t w, uint32_t h, uint32_t scale, const float* params,
                                  void* ws, size_t ws_bytes, srcnn_stream_t stream);

/* srcnn_upscale and srcnn_upscale_frame to any output size W x H within
 * [1x, 4x] of the source per axis.  srcnn_upscale_to is
 *   srcnn_resize_luma (pad = f1+f2+f3-3) -> srcnn_sub_mean -> srcnn_forward ->
 *   srcnn_resize_compose
 * and srcnn_upscale_frame_to is
 *   srcnn_yuv_resize_luma(src->y, pad = f1+f2+f3-3) -> plane
 *   srcnn_sub_mean, srcnn_forward as in srcnn_upscale_yuv
 *   srcnn_yuv_compose_luma16(out -> dst->y)
 *   srcnn_resize_planes(src->u, src->v -> dst->u, dst->v) at the ratios w / W
 *     and h / H, the chroma planes [ceil(h/cy)][ceil(w/cx)] ->
 *     [ceil(H/cy)][ceil(W/cx)]
 * each byte-identical to its calls, for every net srcnn_forward accepts;
 * stream-ordered, no host synchronisation, no allocation.  `ws` holds the
 * plane, the net output, the reduction scratch and the forward workspace (each
 * 256-byte aligned) under the memory contract at srcnn_train_workspace_bytes;
 * of dst only the samples of each row are written, nothing between the rows.
 * The workspace queries return 0 where the call would be invalid.  Errors as
 * the op-level calls and as srcnn_upscale / srcnn_upscale_frame, before any
 * launch; SRCNN_ERR_WORKSPACE for a workspace that is too small. */
SRCNN_API size_t srcnn_upscale_to_workspace_bytes(const srcnn_net* net, uint32_t w, uint32_t h,
                                                  uint32_t W, uint32_t H);
SRCNN_API int srcnn_upscale_to(const srcnn_net* net, const uint8_t* rgba, uint32_t w, uint32_t h,
                               uint32_t W, uint32_t H, const float* params, uint8_t* rgb, void* ws,
                               size_t ws_bytes, srcnn_stream_t stream);
SRCNN_API size_t srcnn_upscale_frame_to_workspace_bytes(const srcnn_net* net, uint32_t w,
                                                        uint32_t h, uint32_t W, uint32_t H);
SRCNN_API int srcnn_upscale_frame_to(const srcnn_net* net, const srcnn_yuv_format* fmt,
                                     const srcnn_yuv_frame* src, const srcnn_yuv_frame* dst,
                                     uint32_t w, uint32_t h, uint32_t W, uint32_t H,
                                     const float* params, void* ws, size_t ws_bytes,
                                     srcnn_stream_t stream);

/* PSNR per plane and SSIM on luma of two Y'CbCr frames, on the device (an
 * MI355X extension; DESIGN.md 17.1 is the spec).  a and b are frames of w x h
 * luma samples with chroma [ceil(h/cy)][ceil(w/cx)], each a srcnn_yuv_frame
 * with its own srcnn_yuv_format: byte addresses and pitches in bytes as in
 * srcnn_upscale_frame.  bits, cx, cy and range must be equal in the two
 * formats; msb, layout and every pitch may differ (a P010 frame against a
 * planar 10-bit one).  A sample's value is its integer code x (DESIGN.md 15:
 * the byte, the 16-bit word, or the word >> (16 - bits) for msb = 1); the
 * range is validated and enters no arithmetic.  `shave` luma pixels are
 * dropped on all four sides, Ws = w - 2*shave and Hs = h - 2*shave at least
 * 11, and ceil(shave/cx) columns and ceil(shave/cy) rows per side of the
 * chroma planes.
 *
 * result (device, 8 doubles) = {mse_y, psnr_y, ssim_y, mse_u, psnr_u, mse_v,
 * psnr_v, psnr_all}: mse_p = (double)S_p / (double)N_p with S_p the sum over
 * the plane's N_p samples of the integer (xa - xb)^2, summed as an unsigned
 * 64-bit integer and so exact; psnr_p = 10 log10((2^bits - 1)^2 / mse_p), +inf
 * for S_p == 0; psnr_all likewise from (((double)S_y + (double)S_u) +
 * (double)S_v) / (double)(N_y + N_u + N_v); ssim_y = srcnn_quality's SSIM of
 * the lumas x * 2^-(bits - 8), exact in fp32 and in [0, 256): SSIM at the
 * dynamic range 255 * 2^(bits - 8), on purpose not 2^bits - 1.  Identical
 * frames give exactly {0, +inf, 1, 0, +inf, 0, +inf, +inf}.  No atomics: the
 * order of the SSIM sum depends on (Ws, Hs) alone, so that the luma results
 * with shave = k are bit-identical to the call on the pointer-offset interior
 * with shave = 0, whatever the layouts and pitches, and two calls on the same
 * inputs are bit-identical.
 *
 * `ws` (srcnn_quality_frame_workspace_bytes: two 8-byte words per luma
 * workgroup, one per chroma workgroup and plane) falls under the memory
 * contract at srcnn_train_workspace_bytes; the call writes the eight doubles
 * of result and reads a and b inside the shaved windows only, never between
 * the rows.  Stream-ordered, three launches, no host synchronisation, no
 * allocation.
 *
 * SRCNN_ERR_INVALID, before any launch: a null format, frame, result or
 * workspace; in a format or frame whatever srcnn_upscale_frame rejects (bits
 * outside 8..16, msb, layout, subsampling, range, a null plane or a v plane
 * of a semi-planar frame, an odd address or pitch of two-byte samples, a pitch
 * below the row's bytes); formats that differ in bits, cx, cy or range; Ws <
 * 11 or Hs < 11 (2*shave wrapping around included); an empty chroma window;
 * result or ws not 8-byte aligned; more than 2^31-1 samples in a plane.
 * SRCNN_ERR_WORKSPACE for a workspace that is too small;
 * srcnn_quality_frame_workspace_bytes returns 0 for invalid sizes. */
SRCNN_API size_t srcnn_quality_frame_workspace_bytes(uint32_t w, uint32_t h, uint32_t cx,
                                                     uint32_t cy, uint32_t shave);
SRCNN_API int srcnn_quality_frame(const srcnn_yuv_format* fmt_a, const srcnn_yuv_frame* a,
                                  const srcnn_yuv_format* fmt_b, const srcnn_yuv_frame* b,
                                  uint32_t w, uint32_t h, uint32_t shave, double* result,
                                  void* ws, size_t ws_bytes, srcnn_stream_t stream);

/* The planes of a Y'CbCr frame made smaller, on the device (an MI355X
 * extension; DESIGN.md 18.1 is the spec): the down direction of
 * srcnn_upscale_planes.  A plane is [ph][pw] samples of `bits` bits, laid out
 * and pitched as there; the output is [oh][ow] in the same
 * layout, 1 <= ow <= ceil(pw/s), 1 <= oh <= ceil(ph/s), s = 1, 2, 3 or 4.  The
 * resampling is srcnn_downscale_rgba's on the integer code values (for msb = 1
 * the word >> (16 - bits)): the antialiased Keys bicubic stretched by s at
 * half-pixel centres, source indices clamped to the plane, separable, fp32,
 * horizontal pass first, no intermediate rounding; the output sample is
 * clamp(rintf(v), 0, 2^bits - 1), ties to even as in the video family, not
 * srcnn_downscale_rgba's floor(v + 0.5).  With s = 1 the output is the source
 * for every sample within [0, 2^bits - 1].  Down by s, then
 * srcnn_yuv_upscale_luma16 by s, is shift-free.
 *
 * SRCNN_YUV_PLANAR with src1 == dst1 == NULL: one plane (a frame's luma); with
 * both non-null: two planes in one launch, each as the one-plane call gives
 * it.  SRCNN_YUV_SEMIPLANAR: src0 / dst0 hold (U, V) pairs, src1 and dst1 must
 * be NULL; sample for sample the planar call on the de-interleaved planes.
 * Gaps between rows are never read and never written.  Stream-ordered, one
 * launch, no workspace; two calls on the same input are bit-identical.
 *
 * SRCNN_ERR_INVALID, before any launch: scale outside 1..4; a zero size; ow
 * or oh beyond its bound; exactly one of src1 / dst1 null; and whatever
 * srcnn_upscale_planes rejects for pitches, bits, msb, layout, odd addresses
 * and the 2^31-1 samples of a plane.
 *
 * srcnn_downscale_frame: a whole frame of W x H luma samples (W >= s, H >= s)
 * -> w x h = W/s x H/s (integer division) in the same format, chroma
 * [ceil(H/cy)][ceil(W/cx)] -> [ceil(h/cy)][ceil(w/cx)] (always within the
 * bound above).  Two launches, no workspace; byte-identical to
 * srcnn_downscale_planes(src->y -> dst->y, planar, one plane) and
 * srcnn_downscale_planes(src->u, src->v -> dst->u, dst->v, fmt->layout).
 * Chroma is resampled plane-wise with the half-pixel map: exact for
 * centre-sited chroma; left-sited chroma keeps a residual shift (DESIGN.md
 * 18.1), uncorrected as in srcnn_upscale_frame.  Errors as the two calls and
 * as srcnn_upscale_frame for the format and the frames, before any launch. */
SRCNN_API int srcnn_downscale_planes(const void* src0, const void* src1, uint32_t src_pitch,
                                     uint32_t pw, uint32_t ph, void* dst0, void* dst1,
                                     uint32_t dst_pitch, uint32_t ow, uint32_t oh, uint32_t scale,
                                     uint32_t bits, uint32_t msb, uint32_t layout,
                                     srcnn_stream_t stream);
SRCNN_API int srcnn_downscale_frame(const srcnn_yuv_format* fmt, const srcnn_yuv_frame* src,
                                    const srcnn_yuv_frame* dst, uint32_t W, uint32_t H,
                                    uint32_t scale, srcnn_stream_t stream);

/* srcnn_make_pairs for the luma of a Y'CbCr frame: X and T [count][tile][tile]
 * with the grid and count of srcnn_make_pairs_count.  Byte-identical to
 *   srcnn_downscale_planes(frame->y -> small [h][w], rows w samples apart)
 *   srcnn_yuv_upscale_luma16(small, w, h, s, pad = 0, range) -> X plane [Hc][Wc]
 *   srcnn_yuv_upscale_luma16(frame->y, W, H, 1, pad = 0, range) -> T plane [H][W]
 *   srcnn_gather_tiles(X plane, sub_mean = 1), srcnn_gather_tiles(T plane, 0)
 * so that limited-range and deep material is trained on as inference sees it.
 * Only the Y plane is read: frame->u and frame->v may be NULL and pitch_c is
 * ignored; fmt is validated whole.  `ws` holds the small plane and the two
 * luma planes (each 256-byte aligned) under the memory contract at
 * srcnn_train_workspace_bytes; the X and T planes are what a srcnn_plane_pair
 * wants.  Stream-ordered, five launches, no allocation.  The workspace query
 * returns 0 where the call would be invalid; errors as the calls it makes and
 * as srcnn_make_pairs, before any launch, SRCNN_ERR_WORKSPACE for a workspace
 * that is too small. */
SRCNN_API size_t srcnn_make_pairs_frame_workspace_bytes(const srcnn_yuv_format* fmt, uint32_t W,
                                                        uint32_t H, uint32_t scale);
SRCNN_API int srcnn_make_pairs_frame(const srcnn_yuv_format* fmt, const srcnn_yuv_frame* frame,
                                     uint32_t W, uint32_t H, uint32_t scale, uint32_t tile,
                                     uint32_t stride, float* X, float* T, void* ws,
                                     size_t ws_bytes, srcnn_stream_t stream);

/* srcnn_evaluate for a Y'CbCr frame: the full-size truth goes in, result
 * (device, 16 doubles) = the net's eight srcnn_quality_frame values, then
 * plain bicubic's eight.  With w = W/s, h = H/s, Wc = s*w, Hc = s*h it is result
 * for result bit-identical to
 *   srcnn_downscale_frame(truth -> small)
 *   srcnn_upscale_frame(net, small -> out)
 *   srcnn_quality_frame(out; truth with its own pitches; Wc, Hc, shave) -> result[0..7]
 *   srcnn_yuv_upscale_luma16(small y, pad = 0) -> plane [Hc][Wc]
 *   srcnn_yuv_compose_luma16(plane -> out's y)
 *   srcnn_quality_frame(as above)                                      -> result[8..15]
 * The chroma planes are the same in both halves, so their numbers coincide.
 * `ws` holds the small frame, the output frame, the luma plane and the two
 * calls' workspaces (each 256-byte aligned) under the memory contract at
 * srcnn_train_workspace_bytes.  Stream-ordered, no host synchronisation, no
 * allocation.  Errors as the calls it makes, before any launch; result and ws
 * 8-byte aligned; SRCNN_ERR_WORKSPACE for a workspace that is too small; the
 * query returns 0 where the call would be invalid. */
SRCNN_API size_t srcnn_evaluate_frame_workspace_bytes(const srcnn_net* net,
                                                      const srcnn_yuv_format* fmt, uint32_t W,
                                                      uint32_t H, uint32_t scale);
SRCNN_API int srcnn_evaluate_frame(const srcnn_net* net, const srcnn_yuv_format* fmt,
                                   const srcnn_yuv_frame* truth, uint32_t W, uint32_t H,
                                   uint32_t scale, uint32_t shave, const float* params,
                                   double* result, void* ws, size_t ws_bytes,
                                   srcnn_stream_t stream);

/* "How many dB over bicubic?" in one call: the full-size ground truth rgba
 * [H][W][4] u8 goes in, the net's and plain bicubic's {mse, psnr, ssim} at
 * scale s come out: result (device, 6 doubles) = {net mse, psnr, ssim, bicubic
 * mse, psnr, ssim}.  With w = W/s, h = H/s, Wc = s*w, Hc = s*h it is result for
 * result bit-identical to
 *   srcnn_downscale_rgba(rgba -> small [h][w][4])
 *   srcnn_upscale(net, small -> rgb [Hc][Wc][3])
 *   srcnn_quality(rgb, RGB8, Wc; rgba, RGBA8, W; Wc, Hc, shave) -> result[0..2]
 *   srcnn_upscale_luma(small, pad = 0) -> plane [Hc][Wc]
 *   srcnn_upscale_compose(small, plane -> rgb)
 *   srcnn_quality(as above)                                     -> result[3..5]
 * Stream-ordered, no host synchronisation, no allocation.  `ws` holds the
 * low-resolution image, one rgb buffer, the luma plane, srcnn_upscale's
 * workspace and srcnn_quality's (each 256-byte aligned) under the memory
 * contract at srcnn_train_workspace_bytes; the call writes the six doubles of
 * result.  srcnn_evaluate_workspace_bytes returns 0 for an invalid net, scale
 * or size.  Errors as srcnn_downscale_rgba, srcnn_upscale and srcnn_quality
 * (Wc - 2*shave and Hc - 2*shave at least 11), before any launch, plus
 * SRCNN_ERR_WORKSPACE for a workspace that is too small. */
SRCNN_API size_t srcnn_evaluate_workspace_bytes(const srcnn_net* net, uint32_t W, uint32_t H,
                                                uint32_t scale);
SRCNN_API int srcnn_evaluate(const srcnn_net* net, const uint8_t* rgba, uint32_t W, uint32_t H,
                             uint32_t scale, uint32_t shave, const float* params, double* result,
                             void* ws, size_t ws_bytes, srcnn_stream_t stream);

/* ---- profiling: the reference's `profile` mode (src/opencl/Kernel.cpp:108-116,
 * src/opencl/Context.cpp:88-96) without blocking per launch: when enabled,
 * every kernel launch is bracketed by a pair of hipEvents on its stream;
 * srcnn_profile_count() waits for the recorded events and folds them into
 * per-kernel totals. ---- */
SRCNN_API int srcnn_profile_enable(int on);
SRCNN_API int srcnn_profile_reset(void);
SRCNN_API int srcnn_profile_count(int* n_kernels);
SRCNN_API int srcnn_profile_get(int index, char* name, size_t name_len,
                                uint64_t* launches, double* total_ms);
/* prints "Kernel '<name>' total execution time: <ns>ns = <s>s" per kernel */
SRCNN_API int srcnn_profile_print(void);
/* Shader clock (GHz) the chip held during the most recent launch of a fused
 * kernel ("l12_fwd_mfma", "l3_delta_fused", "delta1_grad12_fused",
 * "fwd_l123_mfma"): median over the kernel's first 8 workgroups of the
 * s_memtime / s_memrealtime (100 MHz) deltas they record in-kernel
 * (MI355X DVFS under MFMA load).  *ghz = -1 when the kernel has not run,
 * and always in the production library: the probe is compiled only into the
 * diagnostic build (make PROBE=1, -DSRCNN_CLOCK_PROBE), so the production
 * kernels carry no timing code.  An MI355X extension; the reference has no
 * counterpart.  Synchronous. */
SRCNN_API int srcnn_profile_clock(const char* kernel, double* ghz);

/* Kernel-path selection (for A/B measurement and parity tests):
 * 0 = auto (fast specialisations where the shape matches), 1 = generic only. */
SRCNN_API int srcnn_set_path(int path);
SRCNN_API int srcnn_get_path(void);
/* Matrix-core arithmetic of the fused default-net kernels (A/B and parity):
 * 0 = split bf16 (default): fp32 products as six exact bf16 part products on
 *     v_mfma_f32_32x32x16_bf16, at fp32 accuracy;
 * 1 = fp32 MFMA only (v_mfma_f32_32x32x2_f32 / 16x16x4_f32).
 * SRCNN_ARITH=f32 in the environment starts the library at 1.  For finite
 * operands below the bf16 maximum (|x| < 3.39e38) the results of the two
 * differ by fp32 rounding only.  The training step's two-part fp16 products
 * (l12x6's layers 1 and 2, d1x6's gW1) scale each operand by a power of two
 * taken from its largest magnitude -- W1 and W2 per launch, X and the bound on
 * |A1| per sample -- so that rounding is relative to the operand's largest
 * value in that sample or tensor (normwise, as an fp32 accumulation's is):
 * an element more than about 2^17 below it carries fewer than 22 bits, and a
 * sample whose bound max|X| max_c sum_tap |W1| + max|B1| passes fp32's range
 * loses layer 2's precision.  Non-finite operands differ: arith 0 splits
 * +-inf (or a value that rounds to a bf16 infinity) into inf - inf = NaN
 * parts, so a product that arith 1 returns as +-inf comes out NaN, and the
 * split kernels' ReLU keeps a NaN that arith 1's fmaxf turns into 0
 * (tests/test_split_arith_gpu.py pins both).  An MI355X extension. */
SRCNN_API int srcnn_set_arith(int arith);
SRCNN_API int srcnn_get_arith(void);
/* Kernel family that served the most recent operator / network call of this
 * thread, so a slow path is never silent:
 *   "fused"   train_fused.hip / forward_fused.hip (nets with f2 == 1)
 *   "wide"    train_wide.hip and its kernel headers, wl1.hpp .. wgrad2x6.hpp
 *             (nets with a spatial middle layer)
 *   "fast"    ops_fast.hip (gfx950 op-level specialisations)
 *   "generic" ops_generic.hip (any shape; one thread per output)
 *   ""        nothing launched yet on this thread */
SRCNN_API const char* srcnn_last_path(void);
/* The kernels, by variant, that this thread's most recent training call
 * (srcnn_train_fwd_bwd / _step / _lazy) launched, comma-separated, e.g.
 * "l12_fwd,l3r_delta,d1c_grad12,slab_reduce" -- so that a test can
 * assert which specialisation served a shape.  "" before any such call. */
SRCNN_API const char* srcnn_last_kernels(void);

/* One training step on one device: srcnn_train_fwd_bwd over the batch, then
 * srcnn_update_all(update_batch) -- src/Main_cl.cpp:161-175 (execute_batch
 * over the training samples, then update_parameters) with the whole batch in
 * one chunk.  Same results as those two calls; on the fused path (nets with
 * f2 == 1 whose tiles fit l3_delta) and the wide path the update runs inside
 * the gradient reduction, saving one launch.  Single device only: data-parallel training
 * calls srcnn_train_fwd_bwd, srcnn_allreduce_grads, srcnn_update_all. */
SRCNN_API int srcnn_train_step(const srcnn_net* net, const float* X,
                               const float* T, uint32_t w, uint32_t h,
                               uint32_t batch, float* params, float* grads,
                               float* momentum_bufs, float momentum, float wd,
                               const float* lr, uint32_t update_batch,
                               float* sq_err, void* ws, size_t ws_bytes,
                               srcnn_stream_t stream);

/* Inspection seam for the parity tests (no reference counterpart; the
 * reference's buffers are host-readable through Context::read_buffer,
 * src/opencl/Context.cpp:235-262): the activations of the three layers (A1,
 * A2 after ReLU; A3, the linear output) that the most recent
 * srcnn_train_fwd_bwd / srcnn_train_step with the same net, w, h, batch and
 * kernel path left in `ws`, copied out in the reference HWC layout:
 * A1 [batch][h-f1+1][w-f1+1][n1], A2 [batch][..][..][n2], A3 [batch][..][..].
 * The fused step keeps A1 blocked per 32-pixel chunk (or, split-bf16, in
 * run order) in its workspace; this undoes that, in the layout the step that
 * last wrote `ws` on this thread used, whatever srcnn_set_arith says since.
 * Stream-ordered. */
SRCNN_API int srcnn_train_activations(const srcnn_net* net, uint32_t w, uint32_t h,
                                      uint32_t batch, const void* ws, size_t ws_bytes,
                                      float* A1, float* A2, float* A3, srcnn_stream_t stream);

/* ---- multi-GPU: the RCCL gradient-reduction stage ----
 * The reference has one OpenCL queue and no multi-device path
 * (src/Main_cl.cpp:157-195 runs execute_batch over the whole training set,
 * then update_parameters).  Data-parallel training shards the tile batch:
 * each device accumulates its shard's gradients into the flat
 * [gW1|gB1|gW2|gB2|gW3|gB3] buffer (srcnn_train_fwd_bwd), ONE in-place
 * all-reduce(SUM) over xGMI combines them (srcnn_allreduce_grads), and every
 * device runs the same srcnn_update_all with batch = the global tile count. */
typedef void* srcnn_comm_t; /* ncclComm_t */
#define SRCNN_COMM_ID_BYTES 128
/* ncclGetUniqueId: called on ONE rank, the bytes shipped to the others */
SRCNN_API int srcnn_comm_id(uint8_t* id /* [SRCNN_COMM_ID_BYTES] */);
/* one process per GPU: communicator of `rank` on the current device */
SRCNN_API int srcnn_comm_init_rank(srcnn_comm_t* comm, int nranks, const uint8_t* id, int rank);
/* one process driving `ndev` GPUs (devices = NULL: 0 .. ndev-1); comms[i]
 * belongs to devices[i] and is used from the thread that drives it */
SRCNN_API int srcnn_comm_init_all(srcnn_comm_t* comms, int ndev, const int* devices);
SRCNN_API int srcnn_comm_destroy(srcnn_comm_t comm);
SRCNN_API int srcnn_comm_rank(srcnn_comm_t comm, int* rank, int* nranks);
/* ncclGroupStart / End: one thread issuing the collectives of several devices */
SRCNN_API int srcnn_comm_group_start(void);
SRCNN_API int srcnn_comm_group_end(void);
/* RCCL the library runs on: ncclGetVersion (e.g. 22707 = 2.27.7) and the file
 * the loader bound it to.  The library links librccl.so.1 by soname, so a
 * process gets the RCCL of the HIP runtime it loaded first: the ROCm
 * install's (/opt/rocm/lib) for a C++ host such as `cnn`, PyTorch's bundled
 * copy (torch/lib) in a Python process that imported torch -- each matching
 * its libamdhip64.so.7.  Either pointer may be NULL. */
SRCNN_API int srcnn_comm_version(int* version, char* path, size_t len);
/* in-place sum of `count` floats of `buf` over all ranks, enqueued on `stream`
 * (ordered after the gradient kernels, before the update; no host sync) */
SRCNN_API int srcnn_allreduce_grads(srcnn_comm_t comm, float* buf, size_t count,
                                    srcnn_stream_t stream);

/* The data-parallel step without an update launch (an MI355X extension of
 * src/Main_cl.cpp:161-175 / src/ConfigBasedDataPipeline.cpp:325-361, where
 * update_parameters follows execute_batch): the update of step t is applied by
 * the first kernel of step t + 1.  With update_batch > 0 the call first applies
 * the pending update of `grads` (the previous step's all-reduced gradients)
 * OUT OF PLACE -- params_out / mom_out = srcnn_update_all's arithmetic on
 * params_in / mom_in / grads with batch = update_batch -- then runs
 * srcnn_train_fwd_bwd on params_out and OVERWRITES grads with this step's
 * gradients.  With update_batch == 0 (nothing pending) it runs on params_in,
 * writes neither params_out nor mom_out (they may be NULL) and overwrites
 * grads.  A data-parallel step is then
 *     srcnn_train_fwd_bwd_lazy (ping-ponging two parameter / momentum buffers)
 *     srcnn_allreduce_grads
 * and srcnn_update_all(current params, grads, current momentum) applies the
 * last pending update.  The sequence is bit-identical to srcnn_train_fwd_bwd
 * (on zeroed grads) + srcnn_allreduce_grads + srcnn_update_all per step.  On
 * the fused path (nets with f2 == 1) the update runs in the prologue of the
 * first kernel; elsewhere one update launch precedes the step.  params_in,
 * params_out, mom_out and grads must not overlap (SRCNN_ERR_INVALID). */
SRCNN_API int srcnn_train_fwd_bwd_lazy(const srcnn_net* net, const float* X,
                                       const float* T, uint32_t w, uint32_t h,
                                       uint32_t batch, const float* params_in,
                                       float* params_out, const float* mom_in,
                                       float* mom_out, float* grads, float momentum,
                                       float wd, const float* lr, uint32_t update_batch,
                                       float* sq_err, void* ws, size_t ws_bytes,
                                       srcnn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SRCNN_H */
