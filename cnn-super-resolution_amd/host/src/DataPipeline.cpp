#include "DataPipeline.hpp"

#include <iomanip>
#include <iostream>
#include <string>
#include <vector>

namespace cnn_sr {

using srcnn::check;
using srcnn::require;

int DataPipeline::LOAD_KERNEL_LUMA = 1;
int DataPipeline::LOAD_KERNEL_LAYERS = 2;
int DataPipeline::LOAD_KERNEL_MISC = 4;
int DataPipeline::LOAD_KERNEL_BACKPROPAGATE = 8;
int DataPipeline::LOAD_KERNEL_NONE = 0;
int DataPipeline::LOAD_KERNEL_ALL = 1 | 2 | 4 | 8;

#define SRCNN_HAS_SIZE(H, BYTES) allocation_has_right_size__((H), (BYTES), __LINE__, #H)

DataPipeline::DataPipeline(srcnn::Context* ctx) : _context(ctx), _initialized(false) {}

void DataPipeline::init(int load_flags) {
  require(_context && _context->is_initialized(), "DataPipeline needs an initialized Context");
  load_kernels(load_flags);
  _initialized = true;
}

srcnn::Context* DataPipeline::context() { return _context; }

void DataPipeline::check_initialized(int flags) {
  if (!_initialized) throw std::runtime_error("Tried to use DataPipeline before it was initialized");
  load_kernels(flags);
}

void DataPipeline::load_kernels(int flags) {
  using srcnn::KernelKind;
  auto& c = *_context;
  if ((flags & LOAD_KERNEL_LUMA) && !_luma_kernel_norm) {
    // names / defines of the reference's kernels (src/DataPipeline.cpp:121-159)
    _luma_kernel_norm = c.create_kernel(KernelKind::Luma, "extract_luma", 0, 0, 0, false, "-D NORMALIZE");
    _luma_kernel_raw = c.create_kernel(KernelKind::Luma, "extract_luma");
    _swap_luma_kernel = c.create_kernel(KernelKind::SwapLuma, "swap_luma");
  }
  if ((flags & LOAD_KERNEL_MISC) && !_sum_kernel) {
    _squared_error_kernel = c.create_kernel(KernelKind::SquaredError, "squared_error");
    _sum_kernel = c.create_kernel(KernelKind::Sum, "sum");
    _sum_squared_kernel = c.create_kernel(KernelKind::Sum, "sum", 0, 0, 0, false, "-D SUM_SQUARED");
    _subtract_from_all_kernel = c.create_kernel(KernelKind::SubFromAll, "subtract_from_all");
  }
  if ((flags & LOAD_KERNEL_BACKPROPAGATE) && !_backpropagate_kernel) {
    _last_layer_delta_kernel = c.create_kernel(KernelKind::LastDelta, "last_layer_delta");
    _update_parameters_kernel = c.create_kernel(KernelKind::Update, "update_parameters");
    _backpropagate_kernel = c.create_kernel(KernelKind::Backprop, "backpropagate");
  }
  _loaded |= flags;
}

bool DataPipeline::allocation_has_right_size__(MemoryHandle h, size_t size, size_t line,
                                               const char* name) {
  if (h == gpu_nullptr) return false;
  auto* raw = _context->raw_memory(h);
  if (raw->is_usable() && raw->size >= size) return true;
  std::cout << "Was forced to reallocate gpu buffer. Set the MemoryHandle to gpu_nullptr to let "
               "DataPipeline allocate it at the right size. Expected: "
            << size << ", got: " << raw->size << ". Code line: " << line << ", variable: '"
            << name << "'" << std::endl;
  throw std::runtime_error("Was forced to realocate gpu buffer due too difference in sizes.");
}

size_t DataPipeline::element_count(MemoryHandle h, size_t el) {
  return _context->raw_memory(h)->size / el;
}

void* DataPipeline::scratch(size_t bytes) {
  bytes = bytes ? bytes : 4;
  if (_scratch != gpu_nullptr && _context->raw_memory(_scratch)->size < bytes) {
    _context->block();
    _context->raw_memory(_scratch)->release();
    _scratch = gpu_nullptr;
  }
  if (_scratch == gpu_nullptr) _scratch = _context->allocate(srcnn::MEM_READ_WRITE, bytes);
  return _context->ptr(_scratch);
}

void* DataPipeline::reduce_scratch(size_t bytes) {
  bytes = bytes ? bytes : 4;
  if (_reduce_scratch != gpu_nullptr && _context->raw_memory(_reduce_scratch)->size < bytes) {
    _context->block();
    _context->raw_memory(_reduce_scratch)->release();
    _reduce_scratch = gpu_nullptr;
  }
  if (_reduce_scratch == gpu_nullptr)
    _reduce_scratch = _context->allocate(srcnn::MEM_READ_WRITE, bytes);
  return _context->ptr(_reduce_scratch);
}

void DataPipeline::print_buffer(MemoryHandle h, const char* name, size_t lines) {
  size_t len = element_count(h, sizeof(float));
  std::vector<float> v(len);
  _context->block();
  _context->read_buffer(h, v.data(), true);
  size_t per = lines ? (len + lines - 1) / lines : len;
  std::cout << name << ": [" << std::endl;
  for (size_t i = 0; i < len; ++i) {
    std::cout << std::setw(9) << std::setprecision(4) << v[i] << ((i + 1) % per ? ", " : ",\n");
  }
  std::cout << "]" << std::endl << std::endl;
}

Kernel* DataPipeline::create_layer_kernel(const LayerData& d, bool skip_relu) {
  return _context->create_kernel(srcnn::KernelKind::Layer, "layer_uber_kernel", d.n_prev_filter_cnt,
                                 d.current_filter_count, d.f_spatial_size, skip_relu);
}

Kernel* DataPipeline::create_deltas_kernel(const LayerData& d) {
  return _context->create_kernel(srcnn::KernelKind::Deltas, "layer_deltas", d.n_prev_filter_cnt,
                                 d.current_filter_count, d.f_spatial_size);
}

// ---------------------------------------------------------------- luma / misc

Event DataPipeline::extract_luma(ImageData& img, MemoryHandle& raw_img, MemoryHandle& luma,
                                 bool normalize, Event* ev) {
  check_initialized(LOAD_KERNEL_LUMA);
  _context->wait(ev);
  size_t px = size_t(img.w) * img.h;
  if (!SRCNN_HAS_SIZE(raw_img, px * 4)) raw_img = _context->create_image(srcnn::MEM_READ_WRITE, img.w, img.h);
  _context->write_image(raw_img, img, true);
  if (!SRCNN_HAS_SIZE(luma, px * sizeof(float)))
    luma = _context->allocate(srcnn::MEM_READ_WRITE, px * sizeof(float));
  Kernel& k = normalize ? *_luma_kernel_norm : *_luma_kernel_raw;
  srcnn::Context::Launch l(*_context, k);
  check(srcnn_extract_luma(static_cast<const uint8_t*>(_context->ptr(raw_img)), _context->fptr(luma),
                           img.w, img.h, normalize ? 1 : 0, _context->stream()),
        "extract_luma");
  return _context->mark();
}

Event DataPipeline::swap_luma(ImageData& img, MemoryHandle& org_img, MemoryHandle new_luma,
                              MemoryHandle& target, size_t luma_w, size_t luma_h, Event* ev) {
  check_initialized(LOAD_KERNEL_LUMA);
  _context->wait(ev);
  size_t px = size_t(img.w) * img.h;
  if (!SRCNN_HAS_SIZE(new_luma, luma_w * luma_h * sizeof(float)))
    throw std::runtime_error("Invalid size of new luma buffer");
  require(luma_w <= size_t(img.w) && luma_h <= size_t(img.h), "new luma bigger than the image");
  if (!SRCNN_HAS_SIZE(target, px * 3)) target = _context->allocate(srcnn::MEM_READ_WRITE, px * 3);
  if (!SRCNN_HAS_SIZE(org_img, px * 4)) org_img = _context->create_image(srcnn::MEM_READ_WRITE, img.w, img.h);
  _context->write_image(org_img, img, true);
  srcnn::Context::Launch l(*_context, *_swap_luma_kernel);
  check(srcnn_swap_luma(static_cast<const uint8_t*>(_context->ptr(org_img)), _context->fptr(new_luma),
                        static_cast<uint8_t*>(_context->ptr(target)), img.w, img.h, luma_w, luma_h,
                        _context->stream()),
        "swap_luma");
  return _context->mark();
}

Event DataPipeline::upscale_luma(ImageData& img, MemoryHandle& raw_img, MemoryHandle& luma_padded,
                                 size_t scale, size_t padding, Event* ev) {
  check_initialized(LOAD_KERNEL_LUMA);
  require(scale >= 1 && scale <= 4, "upscale_luma: scale must be 1, 2, 3 or 4");
  _context->wait(ev);
  size_t px = size_t(img.w) * img.h;
  size_t plane = (img.w * scale + padding) * (img.h * scale + padding) * sizeof(float);
  if (!SRCNN_HAS_SIZE(raw_img, px * 4)) raw_img = _context->create_image(srcnn::MEM_READ_WRITE, img.w, img.h);
  _context->write_image(raw_img, img, true);
  if (!SRCNN_HAS_SIZE(luma_padded, plane)) luma_padded = _context->allocate(srcnn::MEM_READ_WRITE, plane);
  // (made at first use, so that the profile listing of a run that does not
  // upscale stays the reference's)
  if (!_upscale_luma_kernel)
    _upscale_luma_kernel = _context->create_kernel(srcnn::KernelKind::Luma, "upscale_luma");
  srcnn::Context::Launch l(*_context, *_upscale_luma_kernel);
  check(srcnn_upscale_luma(static_cast<const uint8_t*>(_context->ptr(raw_img)), _context->fptr(luma_padded),
                           img.w, img.h, uint32_t(scale), uint32_t(padding), _context->stream()),
        "upscale_luma");
  return _context->mark();
}

Event DataPipeline::upscale_compose(ImageData& img, MemoryHandle org_img, MemoryHandle new_luma,
                                    MemoryHandle& target, size_t scale, Event* ev) {
  check_initialized(LOAD_KERNEL_LUMA);
  require(scale >= 1 && scale <= 4, "upscale_compose: scale must be 1, 2, 3 or 4");
  _context->wait(ev);
  size_t out_px = size_t(img.w) * scale * img.h * scale;
  if (!SRCNN_HAS_SIZE(org_img, size_t(img.w) * img.h * 4))
    throw std::runtime_error("Invalid size of the original image buffer");
  if (!SRCNN_HAS_SIZE(new_luma, out_px * sizeof(float)))
    throw std::runtime_error("Invalid size of new luma buffer");
  if (!SRCNN_HAS_SIZE(target, out_px * 3)) target = _context->allocate(srcnn::MEM_READ_WRITE, out_px * 3);
  if (!_upscale_compose_kernel)
    _upscale_compose_kernel = _context->create_kernel(srcnn::KernelKind::SwapLuma, "upscale_compose");
  srcnn::Context::Launch l(*_context, *_upscale_compose_kernel);
  check(srcnn_upscale_compose(static_cast<const uint8_t*>(_context->ptr(org_img)), _context->fptr(new_luma),
                              static_cast<uint8_t*>(_context->ptr(target)), img.w, img.h, uint32_t(scale),
                              _context->stream()),
        "upscale_compose");
  return _context->mark();
}

Event DataPipeline::yuv_upscale_luma(MemoryHandle y, size_t pitch_y, size_t w, size_t h, MemoryHandle& luma_padded,
                                     size_t scale, size_t padding, unsigned bits, bool msb, bool full_range,
                                     Event* ev) {
  check_initialized(LOAD_KERNEL_LUMA);
  const size_t B = bits > 8 ? 2 : 1;
  require(scale >= 1 && scale <= 4, "yuv_upscale_luma: scale must be 1, 2, 3 or 4");
  require(w > 0 && h > 0 && pitch_y >= w * B, "yuv_upscale_luma: empty plane or pitch below the row's bytes");
  _context->wait(ev);
  if (_context->raw_memory(y)->size < pitch_y * (h - 1) + w * B)
    throw std::runtime_error("Invalid size of the Y plane buffer");
  const size_t plane = (w * scale + padding) * (h * scale + padding) * sizeof(float);
  if (!SRCNN_HAS_SIZE(luma_padded, plane)) luma_padded = _context->allocate(srcnn::MEM_READ_WRITE, plane);
  if (!_yuv_upscale_luma_kernel)
    _yuv_upscale_luma_kernel =
        _context->create_kernel(srcnn::KernelKind::Luma, bits == 8 ? "yuv_upscale_luma" : "yuv_upscale_luma16");
  srcnn::Context::Launch l(*_context, *_yuv_upscale_luma_kernel);
  check(srcnn_yuv_upscale_luma16(_context->ptr(y), uint32_t(pitch_y), _context->fptr(luma_padded), uint32_t(w),
                                 uint32_t(h), uint32_t(scale), uint32_t(padding), bits, msb ? 1 : 0,
                                 full_range ? SRCNN_YUV_FULL : SRCNN_YUV_LIMITED, _context->stream()),
        "yuv_upscale_luma");
  return _context->mark();
}

Event DataPipeline::upscale_planes(MemoryHandle src0, MemoryHandle src1, size_t src_pitch, size_t pw, size_t ph,
                                   MemoryHandle dst0, MemoryHandle dst1, size_t dst_pitch, size_t ow, size_t oh,
                                   size_t scale, unsigned bits, bool msb, bool semiplanar, Event* ev) {
  check_initialized(LOAD_KERNEL_LUMA);
  const size_t px = (bits > 8 ? 2 : 1) * (semiplanar ? 2 : 1);  // bytes of a pixel of a plane
  require(scale >= 1 && scale <= 4, "upscale_planes: scale must be 1, 2, 3 or 4");
  require(pw > 0 && ph > 0 && ow > 0 && oh > 0 && src_pitch >= pw * px && dst_pitch >= ow * px,
          "upscale_planes: empty plane or pitch below the row's bytes");
  require(semiplanar ? !src1 && !dst1 : src1 && dst1,
          "upscale_planes: two planes each way, or one each way when semi-planar");
  _context->wait(ev);
  for (MemoryHandle s : {src0, src1})
    if (s && _context->raw_memory(s)->size < src_pitch * (ph - 1) + pw * px)
      throw std::runtime_error("Invalid size of a source plane buffer");
  for (MemoryHandle d : {dst0, dst1})
    if (d && _context->raw_memory(d)->size < dst_pitch * (oh - 1) + ow * px)
      throw std::runtime_error("Invalid size of a target plane buffer");
  if (!_upscale_planes_kernel)
    _upscale_planes_kernel = _context->create_kernel(
        srcnn::KernelKind::SwapLuma, bits == 8 && !semiplanar ? "upscale_planes_u8" : "upscale_planes");
  srcnn::Context::Launch l(*_context, *_upscale_planes_kernel);
  check(srcnn_upscale_planes(_context->ptr(src0), src1 ? _context->ptr(src1) : nullptr, uint32_t(src_pitch),
                             uint32_t(pw), uint32_t(ph), _context->ptr(dst0), dst1 ? _context->ptr(dst1) : nullptr,
                             uint32_t(dst_pitch), uint32_t(ow), uint32_t(oh), uint32_t(scale), bits, msb ? 1 : 0,
                             semiplanar ? SRCNN_YUV_SEMIPLANAR : SRCNN_YUV_PLANAR, _context->stream()),
        "upscale_planes");
  return _context->mark();
}

Event DataPipeline::yuv_compose_luma(MemoryHandle luma, size_t w, size_t h, MemoryHandle y, size_t pitch_y,
                                     unsigned bits, bool msb, bool full_range, Event* ev) {
  check_initialized(LOAD_KERNEL_LUMA);
  const size_t B = bits > 8 ? 2 : 1;
  require(w > 0 && h > 0 && pitch_y >= w * B, "yuv_compose_luma: empty plane or pitch below the row's bytes");
  _context->wait(ev);
  if (!SRCNN_HAS_SIZE(luma, w * h * sizeof(float))) throw std::runtime_error("Invalid size of new luma buffer");
  if (_context->raw_memory(y)->size < pitch_y * (h - 1) + w * B)
    throw std::runtime_error("Invalid size of the Y plane buffer");
  if (!_yuv_compose_luma_kernel)
    _yuv_compose_luma_kernel =
        _context->create_kernel(srcnn::KernelKind::SwapLuma, bits == 8 ? "yuv_compose_luma" : "yuv_compose_luma16");
  srcnn::Context::Launch l(*_context, *_yuv_compose_luma_kernel);
  check(srcnn_yuv_compose_luma16(_context->fptr(luma), _context->ptr(y), uint32_t(pitch_y), uint32_t(w), uint32_t(h),
                                 bits, msb ? 1 : 0, full_range ? SRCNN_YUV_FULL : SRCNN_YUV_LIMITED,
                                 _context->stream()),
        "yuv_compose_luma");
  return _context->mark();
}

Event DataPipeline::resize_luma(ImageData& img, MemoryHandle& raw_img, MemoryHandle& luma_padded, size_t out_w,
                                size_t out_h, size_t padding, Event* ev) {
  check_initialized(LOAD_KERNEL_LUMA);
  require(img.w > 0 && img.h > 0 && out_w >= size_t(img.w) && out_w <= 4 * size_t(img.w) &&
              out_h >= size_t(img.h) && out_h <= 4 * size_t(img.h),
          "resize_luma: the output size must lie within 1x .. 4x of the image's per axis");
  _context->wait(ev);
  size_t px = size_t(img.w) * img.h;
  size_t plane = (out_w + padding) * (out_h + padding) * sizeof(float);
  if (!SRCNN_HAS_SIZE(raw_img, px * 4)) raw_img = _context->create_image(srcnn::MEM_READ_WRITE, img.w, img.h);
  _context->write_image(raw_img, img, true);
  if (!SRCNN_HAS_SIZE(luma_padded, plane)) luma_padded = _context->allocate(srcnn::MEM_READ_WRITE, plane);
  if (!_resize_luma_kernel) _resize_luma_kernel = _context->create_kernel(srcnn::KernelKind::Luma, "resize_luma");
  srcnn::Context::Launch l(*_context, *_resize_luma_kernel);
  check(srcnn_resize_luma(static_cast<const uint8_t*>(_context->ptr(raw_img)), _context->fptr(luma_padded), img.w,
                          img.h, uint32_t(out_w), uint32_t(out_h), uint32_t(padding), _context->stream()),
        "resize_luma");
  return _context->mark();
}

Event DataPipeline::resize_compose(ImageData& img, MemoryHandle org_img, MemoryHandle new_luma, MemoryHandle& target,
                                   size_t out_w, size_t out_h, Event* ev) {
  check_initialized(LOAD_KERNEL_LUMA);
  require(img.w > 0 && img.h > 0 && out_w >= size_t(img.w) && out_w <= 4 * size_t(img.w) &&
              out_h >= size_t(img.h) && out_h <= 4 * size_t(img.h),
          "resize_compose: the output size must lie within 1x .. 4x of the image's per axis");
  _context->wait(ev);
  size_t out_px = out_w * out_h;
  if (!SRCNN_HAS_SIZE(org_img, size_t(img.w) * img.h * 4))
    throw std::runtime_error("Invalid size of the original image buffer");
  if (!SRCNN_HAS_SIZE(new_luma, out_px * sizeof(float)))
    throw std::runtime_error("Invalid size of new luma buffer");
  if (!SRCNN_HAS_SIZE(target, out_px * 3)) target = _context->allocate(srcnn::MEM_READ_WRITE, out_px * 3);
  if (!_resize_compose_kernel)
    _resize_compose_kernel = _context->create_kernel(srcnn::KernelKind::SwapLuma, "resize_compose");
  srcnn::Context::Launch l(*_context, *_resize_compose_kernel);
  check(srcnn_resize_compose(static_cast<const uint8_t*>(_context->ptr(org_img)), _context->fptr(new_luma),
                             static_cast<uint8_t*>(_context->ptr(target)), img.w, img.h, uint32_t(out_w),
                             uint32_t(out_h), _context->stream()),
        "resize_compose");
  return _context->mark();
}

Event DataPipeline::yuv_resize_luma(MemoryHandle y, size_t pitch_y, size_t w, size_t h, MemoryHandle& luma_padded,
                                    size_t out_w, size_t out_h, size_t padding, unsigned bits, bool msb,
                                    bool full_range, Event* ev) {
  check_initialized(LOAD_KERNEL_LUMA);
  const size_t B = bits > 8 ? 2 : 1;
  require(w > 0 && h > 0 && pitch_y >= w * B, "yuv_resize_luma: empty plane or pitch below the row's bytes");
  require(out_w >= w && out_w <= 4 * w && out_h >= h && out_h <= 4 * h,
          "yuv_resize_luma: the output size must lie within 1x .. 4x of the plane's per axis");
  _context->wait(ev);
  if (_context->raw_memory(y)->size < pitch_y * (h - 1) + w * B)
    throw std::runtime_error("Invalid size of the Y plane buffer");
  const size_t plane = (out_w + padding) * (out_h + padding) * sizeof(float);
  if (!SRCNN_HAS_SIZE(luma_padded, plane)) luma_padded = _context->allocate(srcnn::MEM_READ_WRITE, plane);
  if (!_yuv_resize_luma_kernel)
    _yuv_resize_luma_kernel = _context->create_kernel(srcnn::KernelKind::Luma, "yuv_resize_luma");
  srcnn::Context::Launch l(*_context, *_yuv_resize_luma_kernel);
  check(srcnn_yuv_resize_luma(_context->ptr(y), uint32_t(pitch_y), _context->fptr(luma_padded), uint32_t(w),
                              uint32_t(h), uint32_t(out_w), uint32_t(out_h), uint32_t(padding), bits, msb ? 1 : 0,
                              full_range ? SRCNN_YUV_FULL : SRCNN_YUV_LIMITED, _context->stream()),
        "yuv_resize_luma");
  return _context->mark();
}

Event DataPipeline::resize_planes(MemoryHandle src0, MemoryHandle src1, size_t src_pitch, size_t pw, size_t ph,
                                  MemoryHandle dst0, MemoryHandle dst1, size_t dst_pitch, size_t ow, size_t oh,
                                  size_t rx_num, size_t rx_den, size_t ry_num, size_t ry_den, unsigned bits, bool msb,
                                  bool semiplanar, Event* ev) {
  check_initialized(LOAD_KERNEL_LUMA);
  const size_t px = (bits > 8 ? 2 : 1) * (semiplanar ? 2 : 1);  // bytes of a pixel of a plane
  require(pw > 0 && ph > 0 && ow > 0 && oh > 0 && src_pitch >= pw * px && dst_pitch >= ow * px,
          "resize_planes: empty plane or pitch below the row's bytes");
  require(rx_num > 0 && ry_num > 0 && rx_den <= 0xffffffffu && ry_den <= 0xffffffffu && rx_num <= rx_den &&
              ry_num <= ry_den,
          "resize_planes: a ratio's numerator must be positive and at most its denominator");
  require(semiplanar ? !src1 && !dst1 : src1 && dst1,
          "resize_planes: two planes each way, or one each way when semi-planar");
  _context->wait(ev);
  for (MemoryHandle s : {src0, src1})
    if (s && _context->raw_memory(s)->size < src_pitch * (ph - 1) + pw * px)
      throw std::runtime_error("Invalid size of a source plane buffer");
  for (MemoryHandle d : {dst0, dst1})
    if (d && _context->raw_memory(d)->size < dst_pitch * (oh - 1) + ow * px)
      throw std::runtime_error("Invalid size of a target plane buffer");
  if (!_resize_planes_kernel)
    _resize_planes_kernel = _context->create_kernel(srcnn::KernelKind::SwapLuma, "resize_planes");
  srcnn::Context::Launch l(*_context, *_resize_planes_kernel);
  check(srcnn_resize_planes(_context->ptr(src0), src1 ? _context->ptr(src1) : nullptr, uint32_t(src_pitch),
                            uint32_t(pw), uint32_t(ph), _context->ptr(dst0), dst1 ? _context->ptr(dst1) : nullptr,
                            uint32_t(dst_pitch), uint32_t(ow), uint32_t(oh), uint32_t(rx_num), uint32_t(rx_den),
                            uint32_t(ry_num), uint32_t(ry_den), bits, msb ? 1 : 0,
                            semiplanar ? SRCNN_YUV_SEMIPLANAR : SRCNN_YUV_PLANAR, _context->stream()),
        "resize_planes");
  return _context->mark();
}

void DataPipeline::downscale(ImageData& img, unsigned scale, ImageData& out) {
  check_initialized(LOAD_KERNEL_LUMA);
  require(scale >= 1 && scale <= 4, "downscale: scale must be 1, 2, 3 or 4");
  require(img.w >= int(scale) && img.h >= int(scale), "downscale: image smaller than the scale");
  const size_t w = size_t(img.w) / scale, h = size_t(img.h) / scale;
  MemoryHandle rgba = _context->create_image(srcnn::MEM_READ_WRITE, img.w, img.h);
  _context->write_image(rgba, img, true);
  MemoryHandle small = _context->create_image(srcnn::MEM_READ_WRITE, w, h);
  if (!_downscale_kernel)
    _downscale_kernel = _context->create_kernel(srcnn::KernelKind::Luma, "downscale_rgba");
  {
    srcnn::Context::Launch l(*_context, *_downscale_kernel);
    check(srcnn_downscale_rgba(static_cast<const uint8_t*>(_context->ptr(rgba)),
                               static_cast<uint8_t*>(_context->ptr(small)), img.w, img.h, scale,
                               _context->stream()),
          "downscale");
  }
  out = ImageData(int(w), int(h), 4);
  _context->read_buffer(small, 0, out.data.size(), out.data.data(), true);
  _context->raw_memory(small)->release();
  _context->raw_memory(rgba)->release();
}

QualityReport DataPipeline::quality(ImageData& img, ImageData& ref, unsigned shave) {
  check_initialized(LOAD_KERNEL_LUMA);
  require(img.w > 0 && img.h > 0, "quality: empty image");
  require(img.w == ref.w && img.h == ref.h,
          "quality: the images differ in size: " + std::to_string(img.w) + "x" + std::to_string(img.h) +
              " / " + std::to_string(ref.w) + "x" + std::to_string(ref.h));
  const size_t ws = srcnn_quality_workspace_bytes(img.w, img.h, shave);
  require(ws > 0, std::string("quality: ") + srcnn_last_error());
  MemoryHandle a = _context->create_image(srcnn::MEM_READ_WRITE, img.w, img.h);
  MemoryHandle b = _context->create_image(srcnn::MEM_READ_WRITE, ref.w, ref.h);
  _context->write_image(a, img, true);
  _context->write_image(b, ref, true);
  MemoryHandle res = _context->allocate(srcnn::MEM_READ_WRITE, 3 * sizeof(double));
  void* wsp = scratch(ws);
  if (!_quality_kernel) _quality_kernel = _context->create_kernel(srcnn::KernelKind::Luma, "srcnn_quality");
  {
    srcnn::Context::Launch l(*_context, *_quality_kernel);
    check(srcnn_quality(_context->ptr(a), SRCNN_PIX_RGBA8, img.w, _context->ptr(b), SRCNN_PIX_RGBA8, ref.w,
                        img.w, img.h, shave, static_cast<double*>(_context->ptr(res)), wsp, ws,
                        _context->stream()),
          "quality");
  }
  double r[3];
  _context->read_buffer(res, 0, sizeof(r), r, true);
  _context->raw_memory(res)->release();
  _context->raw_memory(b)->release();
  _context->raw_memory(a)->release();
  QualityReport q;
  q.mse = r[0];
  q.psnr = r[1];
  q.ssim = r[2];
  return q;
}

void DataPipeline::downscale_frame(const srcnn_yuv_format& fmt, const srcnn_yuv_frame& src,
                                   const srcnn_yuv_frame& dst, unsigned W, unsigned H, unsigned scale,
                                   srcnn_stream_t stream) {
  check_initialized(LOAD_KERNEL_LUMA);
  if (stream) {
    check(srcnn_downscale_frame(&fmt, &src, &dst, W, H, scale, stream), "downscale_frame");
    return;
  }
  if (!_downscale_frame_kernel)
    _downscale_frame_kernel = _context->create_kernel(srcnn::KernelKind::Luma, "srcnn_downscale_frame");
  srcnn::Context::Launch l(*_context, *_downscale_frame_kernel);
  check(srcnn_downscale_frame(&fmt, &src, &dst, W, H, scale, _context->stream()), "downscale_frame");
}

void DataPipeline::quality_frame(const srcnn_yuv_format& fmt_a, const srcnn_yuv_frame& a,
                                 const srcnn_yuv_format& fmt_b, const srcnn_yuv_frame& b, unsigned w, unsigned h,
                                 unsigned shave, double* result, void* ws, size_t ws_bytes, srcnn_stream_t stream) {
  check_initialized(LOAD_KERNEL_LUMA);
  if (stream) {
    check(srcnn_quality_frame(&fmt_a, &a, &fmt_b, &b, w, h, shave, result, ws, ws_bytes, stream), "quality_frame");
    return;
  }
  if (!_quality_frame_kernel)
    _quality_frame_kernel = _context->create_kernel(srcnn::KernelKind::Luma, "srcnn_quality_frame");
  srcnn::Context::Launch l(*_context, *_quality_frame_kernel);
  check(srcnn_quality_frame(&fmt_a, &a, &fmt_b, &b, w, h, shave, result, ws, ws_bytes, _context->stream()),
        "quality_frame");
}

FrameQualityReport DataPipeline::quality_frame(const srcnn_yuv_format& fmt_a, const srcnn_yuv_frame& a,
                                               const srcnn_yuv_format& fmt_b, const srcnn_yuv_frame& b, unsigned w,
                                               unsigned h, unsigned shave) {
  check_initialized(LOAD_KERNEL_LUMA);
  const size_t ws = srcnn_quality_frame_workspace_bytes(w, h, fmt_a.cx, fmt_a.cy, shave);
  require(ws > 0, std::string("quality_frame: ") + srcnn_last_error());
  MemoryHandle res = _context->allocate(srcnn::MEM_READ_WRITE, 8 * sizeof(double));
  quality_frame(fmt_a, a, fmt_b, b, w, h, shave, static_cast<double*>(_context->ptr(res)), scratch(ws), ws, nullptr);
  double r[8];
  _context->read_buffer(res, 0, sizeof(r), r, true);
  _context->raw_memory(res)->release();
  return FrameQualityReport{r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7]};
}

Event DataPipeline::gather_tiles(MemoryHandle plane, size_t pw, size_t ph, size_t x0, size_t y0,
                                 size_t stride, size_t nx, size_t ny, size_t tw, size_t th,
                                 bool sub_mean, MemoryHandle& tiles, MemoryHandle* means, Event* ev) {
  check_initialized(LOAD_KERNEL_LUMA);
  const size_t lim = 0xffffffffu;
  require(pw <= lim && ph <= lim && x0 <= lim && y0 <= lim && stride <= lim && nx <= lim && ny <= lim &&
              tw <= lim && th <= lim,
          "gather_tiles: argument beyond 32 bits");
  if (!SRCNN_HAS_SIZE(plane, pw * ph * sizeof(float)))
    throw std::runtime_error("Invalid size of the plane buffer");
  _context->wait(ev);
  const size_t n = nx * ny;
  if (!SRCNN_HAS_SIZE(tiles, n * tw * th * sizeof(float)))
    tiles = _context->allocate(srcnn::MEM_READ_WRITE, std::max<size_t>(n * tw * th, 1) * sizeof(float));
  float* mp = nullptr;
  if (means && sub_mean) {
    if (!SRCNN_HAS_SIZE(*means, n * sizeof(float)))
      *means = _context->allocate(srcnn::MEM_READ_WRITE, std::max<size_t>(n, 1) * sizeof(float));
    mp = _context->fptr(*means);
  }
  if (!_gather_tiles_kernel)
    _gather_tiles_kernel = _context->create_kernel(srcnn::KernelKind::Luma, "gather_tiles");
  srcnn::Context::Launch l(*_context, *_gather_tiles_kernel);
  check(srcnn_gather_tiles(_context->fptr(plane), uint32_t(pw), uint32_t(ph), uint32_t(x0), uint32_t(y0),
                           uint32_t(stride), uint32_t(nx), uint32_t(ny), uint32_t(tw), uint32_t(th),
                           sub_mean ? 1 : 0, _context->fptr(tiles), mp, _context->stream()),
        "gather_tiles");
  return _context->mark();
}

Event DataPipeline::gather_batch(MemoryHandle planes, size_t n_planes, MemoryHandle refs, size_t first,
                                 size_t n, size_t tw, size_t th, MemoryHandle X, MemoryHandle T,
                                 MemoryHandle* means, Event* ev) {
  check_initialized(LOAD_KERNEL_LUMA);
  const size_t lim = 0xffffffffu;
  require(n_planes <= lim && n <= lim && tw <= lim && th <= lim, "gather_batch: argument beyond 32 bits");
  auto holds = [this](MemoryHandle h, size_t bytes) {
    return h != gpu_nullptr && _context->raw_memory(h)->is_usable() && _context->raw_memory(h)->size >= bytes;
  };
  require(holds(planes, n_planes * sizeof(srcnn_plane_pair)), "gather_batch: plane table smaller than n_planes");
  require(holds(refs, (first + n) * sizeof(srcnn_tile_ref)), "gather_batch: record list smaller than first + n");
  require(holds(X, n * tw * th * sizeof(float)) && holds(T, n * tw * th * sizeof(float)),
          "gather_batch: X or T smaller than n tiles");
  require(!means || holds(*means, n * sizeof(float)), "gather_batch: means smaller than n");
  _context->wait(ev);
  if (!_gather_batch_kernel)
    _gather_batch_kernel = _context->create_kernel(srcnn::KernelKind::Luma, "gather_batch");
  srcnn::Context::Launch l(*_context, *_gather_batch_kernel);
  check(srcnn_gather_batch(static_cast<const srcnn_plane_pair*>(_context->ptr(planes)), uint32_t(n_planes),
                           static_cast<const srcnn_tile_ref*>(_context->ptr(refs)) + first, uint32_t(n),
                           uint32_t(tw), uint32_t(th), _context->fptr(X), _context->fptr(T),
                           means ? _context->fptr(*means) : nullptr, _context->stream()),
        "gather_batch");
  return _context->mark();
}

float DataPipeline::sum(MemoryHandle data, bool squared, Event* ev) {
  check_initialized(LOAD_KERNEL_MISC);
  _context->wait(ev);
  size_t len = element_count(data, sizeof(float));
  if (!SRCNN_HAS_SIZE(_tmp_gpu_float, sizeof(float)))
    _tmp_gpu_float = _context->allocate(srcnn::MEM_READ_WRITE, sizeof(float));
  size_t ws = srcnn_reduce_workspace_bytes(len);
  void* w = reduce_scratch(ws);
  {
    srcnn::Context::Launch l(*_context, squared ? *_sum_squared_kernel : *_sum_kernel);
    check(srcnn_sum(_context->fptr(data), len, squared ? 1 : 0, _context->fptr(_tmp_gpu_float), w, ws,
                    _context->stream()),
          "sum");
  }
  float result = 0.f;
  _context->read_buffer(_tmp_gpu_float, 0, sizeof(float), &result, true);
  return result;
}

Event DataPipeline::subtract_from_all(MemoryHandle data, float v, Event* ev) {
  check_initialized(LOAD_KERNEL_MISC);
  _context->wait(ev);
  srcnn::Context::Launch l(*_context, *_subtract_from_all_kernel);
  check(srcnn_sub_scalar(_context->fptr(data), v, element_count(data, sizeof(float)), _context->stream()),
        "subtract_from_all");
  return _context->mark();
}

Event DataPipeline::subtract_mean(MemoryHandle data, float* mean, Event* ev) {
  check_initialized(LOAD_KERNEL_MISC);
  float s = sum(data, false, ev);  // blocking, as the reference
  float m = s / static_cast<float>(element_count(data, sizeof(float)));
  if (mean) *mean = m;
  return subtract_from_all(data, m);
}

// ---------------------------------------------------------------- forward

void DataPipeline::pre_execute_layer_validation(const LayerData& d, MemoryHandle in, size_t w,
                                                size_t h) {
  LayerData::validate(d);
  require(in != gpu_nullptr, "Layer input buffer is not allocated");
  size_t expected = d.input_size(w, h), cnt = element_count(in, sizeof(float));
  if (expected > cnt) {
    throw std::runtime_error("Declared input_w(" + std::to_string(w) + ")*input_h(" +
                             std::to_string(h) + ")*n_prev_filter_cnt(" +
                             std::to_string(d.n_prev_filter_cnt) + ")=" + std::to_string(expected) +
                             " is bigger then allocated gpu memory (" + std::to_string(cnt) +
                             " elements).");
  }
}

Event DataPipeline::execute_layer(Kernel& kernel, const LayerData& d, LayerAllocationPool& a,
                                  MemoryHandle& in, size_t w, size_t h, size_t n,
                                  MemoryHandle& out, Event* ev) {
  check_initialized(LOAD_KERNEL_LAYERS);
  pre_execute_layer_validation(d, in, w, h);
  require(kernel.kind == srcnn::KernelKind::Layer, "execute_layer needs a layer kernel");
  require(kernel.n_prev == d.n_prev_filter_cnt && kernel.n_cur == d.current_filter_count &&
              kernel.f == d.f_spatial_size,
          "Kernel was created for a different layer shape");
  require(w >= d.f_spatial_size && h >= d.f_spatial_size, "Input smaller than the filter");
  require(d.input_size(w, h) * n <= element_count(in, sizeof(float)),
          "Input buffer smaller than sample_count samples");
  _context->wait(ev);
  size_t od[2];
  d.get_output_dimensions(od, w, h);
  size_t out_bytes = sizeof(float) * od[0] * od[1] * d.current_filter_count * n;
  if (!SRCNN_HAS_SIZE(a.weights, sizeof(float) * d.weight_size())) {
    a.weights = _context->allocate(srcnn::MEM_READ_WRITE, sizeof(float) * d.weight_size());
    _context->write_buffer(a.weights, 0, sizeof(float) * d.weight_size(), d.weights_ptr(), true);
  }
  if (!SRCNN_HAS_SIZE(a.bias, sizeof(float) * d.bias_size())) {
    a.bias = _context->allocate(srcnn::MEM_READ_WRITE, sizeof(float) * d.bias_size());
    _context->write_buffer(a.bias, 0, sizeof(float) * d.bias_size(), d.bias_ptr(), true);
  }
  if (!SRCNN_HAS_SIZE(out, out_bytes)) out = _context->allocate(srcnn::MEM_READ_WRITE, out_bytes);
  srcnn::Context::Launch l(*_context, kernel);
  check(srcnn_conv_fwd(_context->fptr(in), _context->fptr(out), _context->fptr(a.weights),
                       _context->fptr(a.bias), w, h, d.n_prev_filter_cnt, d.current_filter_count,
                       d.f_spatial_size, kernel.skip_relu ? 0 : 1, n, _context->stream()),
        "execute_layer");
  return _context->mark();
}

// ---------------------------------------------------------------- backward

Event DataPipeline::squared_error(MemoryHandle gt, size_t gt_w, size_t gt_h, size_t n,
                                  MemoryHandle algo, MemoryHandle tmp, float& target,
                                  size_t padding, Event* ev) {
  check_initialized(LOAD_KERNEL_MISC);
  require(gt_w > padding && gt_h > padding, "padding larger than the ground truth");
  size_t aw = gt_w - padding, ah = gt_h - padding;
  if (!SRCNN_HAS_SIZE(algo, sizeof(float) * aw * ah))
    throw std::runtime_error("Allocated gpu_buf_algo_res buffer size did not match calculated size");
  require(element_count(algo, sizeof(float)) >= aw * ah * n, "algo result smaller than sample_count samples");
  require(element_count(gt, sizeof(float)) >= gt_w * gt_h * n, "ground truth smaller than sample_count samples");
  if (tmp == gpu_nullptr) {
    if (!SRCNN_HAS_SIZE(_tmp_gpu_float, sizeof(float)))
      _tmp_gpu_float = _context->allocate(srcnn::MEM_READ_WRITE, sizeof(float));
    tmp = _tmp_gpu_float;
  }
  require(_context->raw_memory(tmp)->size >= sizeof(float), "tmp buffer must hold one float");
  _context->wait(ev);
  size_t ws = srcnn_reduce_workspace_bytes(aw * ah * n);
  void* w = reduce_scratch(ws);
  {
    srcnn::Context::Launch l(*_context, *_squared_error_kernel);
    check(srcnn_sq_err(_context->fptr(gt), _context->fptr(algo), _context->fptr(tmp), gt_w, gt_h, aw,
                       ah, n, w, ws, _context->stream()),
          "squared_error");
  }
  return _context->read_buffer(tmp, 0, sizeof(float), &target, true);
}

Event DataPipeline::last_layer_delta(MemoryHandle gt, size_t gt_w, size_t gt_h, size_t n,
                                     MemoryHandle algo, MemoryHandle& target, size_t padding,
                                     Event* ev) {
  check_initialized(LOAD_KERNEL_BACKPROPAGATE);
  require(gt_w > padding && gt_h > padding, "padding larger than the ground truth");
  size_t aw = gt_w - padding, ah = gt_h - padding;
  if (!SRCNN_HAS_SIZE(algo, sizeof(float) * aw * ah))
    throw std::runtime_error("Allocated gpu_buf_algo_res buffer size did not match calculated size");
  require(element_count(algo, sizeof(float)) >= aw * ah * n, "algo result smaller than sample_count samples");
  require(element_count(gt, sizeof(float)) >= gt_w * gt_h * n, "ground truth smaller than sample_count samples");
  if (!SRCNN_HAS_SIZE(target, sizeof(float) * aw * ah * n))
    target = _context->allocate(srcnn::MEM_READ_WRITE, sizeof(float) * aw * ah * n);
  _context->wait(ev);
  srcnn::Context::Launch l(*_context, *_last_layer_delta_kernel);
  check(srcnn_last_delta(_context->fptr(gt), _context->fptr(algo), _context->fptr(target), gt_w, gt_h,
                         aw, ah, n, _context->stream()),
        "last_layer_delta");
  return _context->mark();
}

Event DataPipeline::calculate_deltas(Kernel& kernel, const LayerData& curr, const LayerData& next,
                                     LayerAllocationPool& next_alloc, MemoryHandle curr_deltas,
                                     MemoryHandle next_deltas, size_t next_w, size_t next_h,
                                     size_t n, MemoryHandle curr_output, Event* ev) {
  check_initialized(LOAD_KERNEL_BACKPROPAGATE);
  LayerData::validate(next);
  if (curr.current_filter_count != next.n_prev_filter_cnt) {
    throw std::runtime_error(
        "When calculating deltas for layer it's filter count should be equal to next layer's "
        "previous filter count");
  }
  require(kernel.kind == srcnn::KernelKind::Deltas, "calculate_deltas needs a deltas kernel");
  size_t cw = next_w + next.f_spatial_size - 1, ch = next_h + next.f_spatial_size - 1;
  size_t out_bytes = sizeof(float) * cw * ch * next.n_prev_filter_cnt;
  if (!SRCNN_HAS_SIZE(next_alloc.weights, sizeof(float) * next.weight_size())) {
    next_alloc.weights = _context->allocate(srcnn::MEM_READ_WRITE, sizeof(float) * next.weight_size());
    _context->write_buffer(next_alloc.weights, 0, sizeof(float) * next.weight_size(), next.weights_ptr(), true);
  }
  if (!SRCNN_HAS_SIZE(curr_output, out_bytes)) {
    throw std::runtime_error(
        "Tried to calculate deltas for previous layer, but there are no previous layer output "
        "values.They are normally allocated during forward step.");
  }
  require(curr_deltas != gpu_nullptr && element_count(curr_deltas, 4) >= cw * ch * next.n_prev_filter_cnt * n,
          "Target deltas buffer is not allocated or too small");
  require(next_deltas != gpu_nullptr &&
              element_count(next_deltas, 4) >= next_w * next_h * next.current_filter_count * n,
          "Next layer deltas buffer is not allocated or too small");
  require(element_count(curr_output, 4) >= cw * ch * next.n_prev_filter_cnt * n,
          "Previous layer output smaller than sample_count samples");
  _context->wait(ev);
  srcnn::Context::Launch l(*_context, kernel);
  check(srcnn_conv_delta(_context->fptr(next_deltas), _context->fptr(curr_output),
                         _context->fptr(curr_deltas), _context->fptr(next_alloc.weights),
                         next.f_spatial_size, next.n_prev_filter_cnt, next.current_filter_count, cw,
                         ch, n, _context->stream()),
        "calculate_deltas");
  return _context->mark();
}

Event DataPipeline::backpropagate(LayerData& d, MemoryHandle input, MemoryHandle deltas,
                                  LayerAllocationPool& a, size_t ow, size_t oh, size_t n,
                                  Event* ev, size_t ev_cnt) {
  LayerData::validate(d);
  check_initialized(LOAD_KERNEL_BACKPROPAGATE);
  size_t iw = ow + d.f_spatial_size - 1, ih = oh + d.f_spatial_size - 1;
  size_t in_bytes = sizeof(float) * iw * ih * d.n_prev_filter_cnt;
  if (!SRCNN_HAS_SIZE(input, in_bytes)) {
    throw std::runtime_error(
        "Tried to calculate gradients, but there are no previous layer output values.They are "
        "normally allocated during forward step.");
  }
  require(element_count(input, 4) >= iw * ih * d.n_prev_filter_cnt * n,
          "Layer input smaller than sample_count samples");
  require(deltas != gpu_nullptr && element_count(deltas, 4) >= ow * oh * d.current_filter_count * n,
          "Tried to calculate gradients, but deltas for current layer are not valid");
  if (!SRCNN_HAS_SIZE(a.accumulating_grad_w, sizeof(float) * d.weight_size())) {
    a.accumulating_grad_w = _context->allocate(srcnn::MEM_READ_WRITE, sizeof(float) * d.weight_size());
    _context->zeros_float(a.accumulating_grad_w, false);
  }
  if (!SRCNN_HAS_SIZE(a.accumulating_grad_b, sizeof(float) * d.bias_size())) {
    a.accumulating_grad_b = _context->allocate(srcnn::MEM_READ_WRITE, sizeof(float) * d.bias_size());
    _context->zeros_float(a.accumulating_grad_b, false);
  }
  _context->wait(ev, ev ? (ev_cnt ? int(ev_cnt) : 1) : 0);
  size_t ws = srcnn_conv_grad_workspace_bytes(d.n_prev_filter_cnt, d.current_filter_count,
                                              d.f_spatial_size, ow, oh, n);
  void* w = scratch(ws);
  srcnn::Context::Launch l(*_context, *_backpropagate_kernel);
  check(srcnn_conv_grad_acc(_context->fptr(input), _context->fptr(deltas),
                            _context->fptr(a.accumulating_grad_w), _context->fptr(a.accumulating_grad_b),
                            d.n_prev_filter_cnt, d.current_filter_count, d.f_spatial_size, ow, oh, n,
                            w, ws, _context->stream()),
        "backpropagate");
  return _context->mark();
}

Event DataPipeline::update_parameters(LayerData& d, LayerAllocationPool& a, size_t batch,
                                      float momentum, float wd, float lr, Event* ev) {
  LayerData::validate(d);
  check_initialized(LOAD_KERNEL_BACKPROPAGATE);
  size_t wb = sizeof(float) * d.weight_size(), bb = sizeof(float) * d.bias_size();
  if (!SRCNN_HAS_SIZE(a.weights, wb))
    throw std::runtime_error("Tried to update weights, but old values are not valid. Impossible if forward pass was completed");
  if (!SRCNN_HAS_SIZE(a.bias, bb))
    throw std::runtime_error("Tried to update bias, but old values are not valid. Impossible if forward pass was completed");
  if (!SRCNN_HAS_SIZE(a.accumulating_grad_w, wb))
    throw std::runtime_error("Tried to update weights, but gradient values are not valid. Impossible if backpropagation was completed");
  if (!SRCNN_HAS_SIZE(a.accumulating_grad_b, bb))
    throw std::runtime_error("Tried to update bias, but gradient values are not valid. Impossible if backpropagation was completed");
  if (!SRCNN_HAS_SIZE(a.previous_batch_delta_w, wb)) {
    a.previous_batch_delta_w = _context->allocate(srcnn::MEM_READ_WRITE, wb);
    _context->zeros_float(a.previous_batch_delta_w, false);
  }
  if (!SRCNN_HAS_SIZE(a.previous_batch_delta_b, bb)) {
    a.previous_batch_delta_b = _context->allocate(srcnn::MEM_READ_WRITE, bb);
    _context->zeros_float(a.previous_batch_delta_b, false);
  }
  _context->wait(ev);
  srcnn::Context::Launch l(*_context, *_update_parameters_kernel);
  check(srcnn_sgd_update(_context->fptr(a.weights), _context->fptr(a.bias),
                         _context->fptr(a.accumulating_grad_w), _context->fptr(a.accumulating_grad_b),
                         _context->fptr(a.previous_batch_delta_w), _context->fptr(a.previous_batch_delta_b),
                         momentum, wd, lr, batch, d.weight_size(), d.bias_size(), _context->stream()),
        "update_parameters");
  return _context->mark();
}

}  // namespace cnn_sr
