// cnn_sr::ConfigBasedDataPipeline -- the three-layer SRCNN driven by a Config.
//
// Drop-in for the reference class (src/ConfigBasedDataPipeline.hpp:46-156):
// init() loads parameters.json or draws random parameters, execute_batch()
// runs forward + backpropagation (or forward + squared error) over a sample
// set in mini-batches, update_parameters() applies momentum SGD and zeroes
// the gradient accumulators, write_params_to_file() / write_result_image()
// save results.
//
// MI355X design: when the three LayerAllocationPools are left to the
// pipeline (all gpu_nullptr, the reference's normal use), the pipeline
// allocates ONE flat parameter buffer [W1|B1|W2|B2|W3|B3] (plus flat
// gradient and momentum buffers) and hands out views of it as the pools'
// handles.  A training chunk is then one srcnn_train_fwd_bwd call (the fused
// gfx950 kernels), the update one srcnn_update_all call, and the flat
// gradient buffer is what a data-parallel run all-reduces.  Pools that the
// caller allocated itself take the per-layer op-level path instead (same
// results; tests pin both).
#ifndef CNN_SR_CONFIG_BASED_DATA_PIPELINE_HPP
#define CNN_SR_CONFIG_BASED_DATA_PIPELINE_HPP

#include <cstdint>
#include <vector>

#include "Config.hpp"
#include "DataPipeline.hpp"

namespace cnn_sr {

/** Device buffers of one image (reference :12-31). */
struct SampleAllocationPool {
  MemoryHandle input_data = gpu_nullptr;  // RGBA image
  MemoryHandle input_luma = gpu_nullptr;  // w*h floats
  size_t input_w = 0, input_h = 0;
  MemoryHandle expected_data = gpu_nullptr;
  MemoryHandle expected_luma = gpu_nullptr;
  SampleAllocationPool() = default;
};

/** All allocations of a run (reference :34-40). */
struct GpuAllocationPool {
  LayerAllocationPool layer_1;
  LayerAllocationPool layer_2;
  LayerAllocationPool layer_3;
  std::vector<SampleAllocationPool> samples;
};

/** The one exchange step of data-parallel training (an extension; the
 * reference trains on one device): an in-place sum of `count` floats of device
 * memory over the ranks, ordered after the work already on `ctx`'s stream. */
class GradientExchange {
 public:
  virtual ~GradientExchange() = default;
  virtual void allreduce(srcnn::Context& ctx, float* buf, size_t count) = 0;
};

/** RCCL over xGMI: srcnn_allreduce_grads on the context's stream. */
class RcclExchange : public GradientExchange {
 public:
  explicit RcclExchange(srcnn_comm_t comm) : _comm(comm) {}
  void allreduce(srcnn::Context& ctx, float* buf, size_t count) override;

 private:
  srcnn_comm_t _comm;
};

class ConfigBasedDataPipeline : public DataPipeline {
 public:
  ConfigBasedDataPipeline(Config&, srcnn::Context*);

  void init(int load_flags = DataPipeline::LOAD_KERNEL_ALL) override;

  void set_mini_batch_size(size_t);
  size_t mini_batch_size() const { return _mini_batch_size; }

  /** Forward + (backpropagate ? gradient accumulation : squared error) over
   * all samples (same dims), in mini-batches; returns the summed squared
   * error of a validation run (0 for training). */
  float execute_batch(bool backpropagate, GpuAllocationPool&, std::vector<SampleAllocationPool*>&);

  /** Inference of one image; the result stays in result_buffer(). */
  Event forward(LayerAllocationPool&, LayerAllocationPool&, LayerAllocationPool&,
                SampleAllocationPool&);

  void update_parameters(LayerAllocationPool&, LayerAllocationPool&, LayerAllocationPool&,
                         size_t batch_size, Event* ev = nullptr);

  void write_params_to_file(const char* file_path, LayerAllocationPool, LayerAllocationPool,
                            LayerAllocationPool);

  void write_result_image(const char* out_path, ImageData& input_img, SampleAllocationPool&);

  const Config* config() const { return _config; }
  const LayerData* layer_1() const { return &layer_data_1; }
  const LayerData* layer_2() const { return &layer_data_2; }
  const LayerData* layer_3() const { return &layer_data_3; }

  // ---- extensions (not in the reference) ----
  /** seed the random initialisation (the reference seeds with the clock) */
  void set_random_seed(uint64_t seed) { _seed = seed; _seeded = true; }
  size_t epochs() const { return _epochs; }
  /** opt-in (the reference restarts momentum at zero on resume,
   * ConfigBasedDataPipeline.cpp:419-465): write_params_to_file() also stores
   * each layer's momentum ("momentum_weights" / "momentum_bias", keys the
   * reference's loader skips), and a parameters file that holds them resumes
   * the pipeline-owned momentum buffers from them */
  void set_save_momentum(bool on) { _save_momentum = on; }
  /** Low-resolution image in, image of `scale` (1..4) times the size out,
   * all on the device: uploads the RGBA, makes one srcnn_upscale call on the
   * pipeline's flat parameters (bicubic luma into the edge-replicated padded
   * plane, mean subtraction, the net, composition with the bicubic colours)
   * and reads the RGB result back.  Every output pixel passes through the
   * net: no border frame is left, also with scale 1. */
  void super_resolve(ImageData& low_res, unsigned scale, ImageData& result);
  /** super_resolve_frame for a planar frame of 8 bits per sample
   * (DESIGN.md 14). */
  void super_resolve_yuv(const srcnn_yuv_frame& src, const srcnn_yuv_frame& dst, unsigned w, unsigned h,
                         unsigned cx, unsigned cy, unsigned scale, bool full_range, void* ws, size_t ws_bytes,
                         srcnn_stream_t stream = nullptr);
  /** One Y'CbCr frame that is already on the device in, the frame of `scale`
   * (1..4) times the size out, in any frame format of DESIGN.md 15 (8 to 16
   * bits per sample, planar or semi-planar chroma; `fmt` also holds the
   * subsampling and the range): one srcnn_upscale_frame call on the pipeline's
   * flat parameters.  Only enqueues: no upload, no download, no allocation, no
   * synchronisation, so a caller can keep several frames in flight, each with
   * its own `stream`, workspace (`ws`, at least
   * super_resolve_yuv_workspace_bytes) and device frames.  `stream` nullptr:
   * the context's stream, and the call is counted (and in profile mode timed)
   * as kernel 'srcnn_upscale_frame'. */
  void super_resolve_frame(const srcnn_yuv_format& fmt, const srcnn_yuv_frame& src, const srcnn_yuv_frame& dst,
                           unsigned w, unsigned h, unsigned scale, void* ws, size_t ws_bytes,
                           srcnn_stream_t stream = nullptr);
  /** 0 if the net, the size or the scale is invalid (srcnn_last_error says why) */
  size_t super_resolve_yuv_workspace_bytes(unsigned w, unsigned h, unsigned scale);
  /** super_resolve to any output size out_w x out_h within [1x, 4x] of the
   * image's per axis: one srcnn_upscale_to call, counted as
   * kernel 'srcnn_upscale_to'. */
  void super_resolve_to(ImageData& low_res, unsigned out_w, unsigned out_h, ImageData& result);
  /** 0 if the net or the sizes are invalid (srcnn_last_error says why) */
  size_t super_resolve_to_workspace_bytes(unsigned w, unsigned h, unsigned out_w, unsigned out_h);
  /** super_resolve_frame to any output size out_w x out_h within [1x, 4x] of
   * the frame's per axis: one srcnn_upscale_frame_to call (`ws`: at least
   * super_resolve_frame_to_workspace_bytes), counted as kernel
   * 'srcnn_upscale_frame_to' on the context's stream. */
  void super_resolve_frame_to(const srcnn_yuv_format& fmt, const srcnn_yuv_frame& src, const srcnn_yuv_frame& dst,
                              unsigned w, unsigned h, unsigned out_w, unsigned out_h, void* ws, size_t ws_bytes,
                              srcnn_stream_t stream = nullptr);
  size_t super_resolve_frame_to_workspace_bytes(unsigned w, unsigned h, unsigned out_w, unsigned out_h);
  /** Training pairs of one full-size image, cut on the device: one
   * srcnn_make_pairs call (the image degraded by the resampling super_resolve
   * applies: down by `scale`, bicubic up again; then a grid of tile x tile
   * windows at `stride`, the input tiles minus their own mean) appends one
   * sample per tile to `out` and returns their number, 0 if the image is too
   * small for one tile.  The samples' input_luma / expected_luma are views
   * into the two batch buffers of the call (never released on their own);
   * input_w = input_h = tile. */
  size_t make_training_pairs(ImageData& full, unsigned scale, size_t tile, size_t stride,
                             std::vector<SampleAllocationPool>& out);
  /** The grid make_training_pairs would cut from an image (srcnn_make_pairs_count). */
  struct TrainingGrid {
    size_t nx = 0, ny = 0, count = 0;  // count = nx*ny; 0: the image holds no tile
    size_t plane = 0;                  // index of the image's pair in the plane table
    size_t w = 0, h = 0;               // the extent tiles may be cut from (Wc x Hc)
  };
  /** Planes instead of tiles: the image's degraded luma plane (down by
   * `scale`, srcnn_upscale_luma with pad 0) and its ground-truth luma plane
   * (srcnn_extract_luma, normalised) are made by the three plane calls
   * srcnn_make_pairs starts with, into buffers that stay resident, and
   * registered as one srcnn_plane_pair.  Returns the image's grid; count 0 (too
   * small for one tile): nothing is kept.  Every call of a run takes the same
   * `tile`. */
  TrainingGrid make_training_planes(ImageData& full, unsigned scale, size_t tile, size_t stride);
  /** make_training_pairs for the luma of a Y'CbCr frame that is already on the
   * device: one srcnn_make_pairs_frame call (only frame.y is
   * read), counted as kernel 'srcnn_make_pairs_frame'. */
  size_t make_training_pairs(const srcnn_yuv_format& fmt, const srcnn_yuv_frame& frame, unsigned W, unsigned H,
                             unsigned scale, size_t tile, size_t stride, std::vector<SampleAllocationPool>& out);
  /** make_training_planes for such a frame: the same one call into a workspace
   * that stays resident; its X and T planes are registered as one
   * srcnn_plane_pair (the tiles the call also cuts are dropped). */
  TrainingGrid make_training_planes(const srcnn_yuv_format& fmt, const srcnn_yuv_frame& frame, unsigned W,
                                    unsigned H, unsigned scale, size_t tile, size_t stride);
  /** "How many dB over bicubic?" for a Y'CbCr frame that is already on the
   * device: one srcnn_evaluate_frame call on the pipeline's flat parameters;
   * the 16 doubles go to `result` (device) through the caller's workspace
   * (evaluate_frame_workspace_bytes; 0 where the call would be invalid).  Only
   * enqueues, on `stream`, or, with no stream, on the context's, where the
   * call is counted and timed. */
  void evaluate_frame(const srcnn_yuv_format& fmt, const srcnn_yuv_frame& truth, unsigned W, unsigned H,
                      unsigned scale, unsigned shave, double* result, void* ws, size_t ws_bytes,
                      srcnn_stream_t stream = nullptr);
  size_t evaluate_frame_workspace_bytes(const srcnn_yuv_format& fmt, unsigned W, unsigned H, unsigned scale);
  /** the registered plane pairs to the device; call after the last make_training_planes */
  void upload_plane_table();
  size_t plane_count() const { return _plane_table.size(); }
  /** execute_batch over samples named by records instead of held as tiles:
   * the records are uploaded once, then every chunk of mini_batch_size() is
   * one srcnn_gather_batch from the resident planes into the batch buffers,
   * followed by the chunk execute_batch runs.  An invalid record gives NaN
   * tiles, hence a NaN error / NaN gradients. */
  float execute_batch_refs(bool backpropagate, GpuAllocationPool&, const std::vector<srcnn_tile_ref>&);
  /** "How many dB over bicubic?": the full-size ground truth in, the quality
   * of the net's x `scale` result (`net`) and of plain bicubic's (`bicubic`)
   * out, with `shave` pixels dropped per side: one srcnn_evaluate call on the
   * pipeline's flat parameters (down by `scale`, super_resolve's resampling
   * and net, srcnn_quality against the truth's top-left scale*(w/scale) x
   * scale*(h/scale) pixels).  False, with nothing measured, if what is left
   * after the crop and the shave is smaller than the 11 x 11 SSIM window. */
  bool evaluate(ImageData& truth, unsigned scale, unsigned shave, QualityReport& net,
                QualityReport& bicubic);
  /** L3 output of the last forward / execute_batch chunk */
  MemoryHandle result_buffer() const { return _out_3_gpu_buf; }
  /** the flat [gW1|gB1|gW2|gB2|gW3|gB3] buffer (gpu_nullptr before training
   * on pipeline-owned pools): the one buffer a data-parallel run all-reduces */
  MemoryHandle flat_gradients() const { return _flat_grads; }
  MemoryHandle flat_parameters() const { return _flat_params; }
  srcnn_net net() const;

  /** Data-parallel extension (the reference is single-device): sum the
   * flat gradient buffer over the ranks in place, on this context's stream
   * (by default srcnn_allreduce_grads, RCCL over xGMI).  Call between
   * execute_batch(true, ...) on this rank's shard and update_parameters(...,
   * global training-set size).  The pools must be the pipeline's own flat
   * views (left unallocated by the caller; they are bound here if needed). */
  void allreduce_gradients(GpuAllocationPool&, GradientExchange& ex);
  void allreduce_gradients(GpuAllocationPool&, srcnn_comm_t comm);
  /** sum of one host float over the ranks (blocking) */
  float allreduce_sum(float value, GradientExchange& ex);
  float allreduce_sum(float value, srcnn_comm_t comm);

 protected:
  void load_kernels(int load_flags) override;

 private:
  /** the net shape as the defines a net-level kernel is created with */
  std::string net_defines() const;
  void allocate_buffers(size_t w, size_t h);
  /** make the pools views of the flat buffers if they are unallocated;
   * true when the pools are the pipeline's flat views */
  bool bind_flat(LayerAllocationPool&, LayerAllocationPool&, LayerAllocationPool&);
  Event forward(LayerAllocationPool&, LayerAllocationPool&, LayerAllocationPool&, size_t w,
                size_t h, size_t n);
  Event backpropagate(LayerAllocationPool&, LayerAllocationPool&, LayerAllocationPool&, size_t w,
                      size_t h, size_t n, Event* ev = nullptr);
  /** one chunk of n samples of w x h already in the batch buffers: forward +
   * (backprop ? gradient accumulation : squared error, which is returned) */
  float run_chunk(bool backprop, bool flat, GpuAllocationPool&, size_t w, size_t h, size_t n);
  /** what super_resolve / super_resolve_to and super_resolve_frame /
   * super_resolve_frame_to share: `who` in their errors, the ABI call srcnn_<abi> */
  template <typename Query, typename Call>
  void upscale_image(const std::string& who, const char* abi, Kernel*& kernel, ImageData& low_res, size_t out_w,
                     size_t out_h, Query query, Call call, ImageData& result);
  template <typename Call>
  void upscale_frame(const std::string& who, const char* abi, Kernel*& kernel, srcnn_stream_t stream, Call call);
  void fill_random_parameters(LayerData&, ParametersDistribution&, uint64_t seed);
  size_t load_parameters_file(const char* file);

  Config* const _config;
  LayerData layer_data_1;
  LayerData layer_data_2;
  LayerData layer_data_3;
  size_t _epochs = 0;
  size_t _mini_batch_size = 0;
  uint64_t _seed = 0;
  bool _seeded = false;
  bool _save_momentum = false;
  std::vector<float> _momentum_in[3][2];  // momentum read from the parameters file [layer][W, B]

  size_t _buf_w = 0, _buf_h = 0, _buf_n = 0;
  MemoryHandle _ground_truth_gpu_buf = gpu_nullptr;
  MemoryHandle _forward_gpu_buf = gpu_nullptr;
  MemoryHandle _out_1_gpu_buf = gpu_nullptr, _out_2_gpu_buf = gpu_nullptr,
               _out_3_gpu_buf = gpu_nullptr;
  MemoryHandle _delta_1_gpu_buf = gpu_nullptr, _delta_2_gpu_buf = gpu_nullptr,
               _delta_3_gpu_buf = gpu_nullptr;

  // flat parameter / gradient / momentum buffers and their per-layer views
  MemoryHandle _flat_params = gpu_nullptr, _flat_grads = gpu_nullptr, _flat_moms = gpu_nullptr;
  LayerAllocationPool _views[3];

  Kernel* _layer_1_kernel = nullptr;
  Kernel* _layer_2_kernel = nullptr;
  Kernel* _layer_3_kernel = nullptr;
  Kernel* _layer_1_deltas_kernel = nullptr;
  Kernel* _layer_2_deltas_kernel = nullptr;
  Kernel* _train_kernel = nullptr;
  Kernel* _forward_kernel = nullptr;
  Kernel* _upscale_kernel = nullptr;
  Kernel* _upscale_frame_kernel = nullptr;
  Kernel* _upscale_to_kernel = nullptr;
  Kernel* _upscale_frame_to_kernel = nullptr;
  Kernel* _make_pairs_kernel = nullptr;
  Kernel* _planes_kernel = nullptr;
  Kernel* _make_pairs_frame_kernel = nullptr;
  Kernel* _evaluate_frame_kernel = nullptr;

  // resident planes of make_training_planes and the records of the current epoch
  std::vector<srcnn_plane_pair> _plane_table;
  size_t _plane_tile = 0;
  MemoryHandle _plane_table_gpu_buf = gpu_nullptr;
  size_t _plane_table_uploaded = 0;
  MemoryHandle _refs_gpu_buf = gpu_nullptr;
  Kernel* _evaluate_kernel = nullptr;
  Kernel* _update_all_kernel = nullptr;
  Kernel* _allreduce_kernel = nullptr;
  MemoryHandle _comm_scalar = gpu_nullptr;
};

}  // namespace cnn_sr

#endif  // CNN_SR_CONFIG_BASED_DATA_PIPELINE_HPP
