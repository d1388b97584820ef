// cnn -- the command line of the reference (src/Main_cl.cpp) on the MI355X
// pipeline:
//
//   cnn [-h] [train | upscale | downscale | quality | evaluate] [dry] [profile]
//       -c CONFIG -i IN [-o OUT] [-e EPOCHS] [--scale S] [--seed N] [--device D]
//       [--devices N] [--validation-percent P] [--mini-batches M] [--save-momentum]
//       [--from-images] [--tile N] [--stride N] [--ref REF] [--shave N]
//       [--device-batches] [--augment] [--random-origins] [--frames N]
//       [--range full|limited] [--slots N] [--size WxH] [--frame-step N]
//
// forward:  IN is an image (JPEG / PNG / PNM) that is already scaled, OUT the
//           result image of the same size (its outermost total_padding / 2
//           pixels are the input's)
// upscale:  (extension) IN is a low-resolution image, OUT the image of S times
//           the size (--scale 1, 2, 3 or 4; default 2): bicubic resampling, the
//           net and the composition all run on the device (srcnn_upscale), and
//           every output pixel passes through the net.  --scale 1 is the
//           "same size, no border frame" mode for inputs that are already scaled.
//           If IN starts with the YUV4MPEG2 magic it is a Y4M video (8-bit,
//           or 9 to 16 bits as C420p10 and its kin; 4:2:0, 4:2:2 or 4:4:4,
//           progressive) and is streamed: every frame is upscaled by S on the
//           device as planar Y'CbCr -- luma through the net, chroma plain
//           bicubic (srcnn_upscale_frame) --
//           and OUT is a Y4M of S times the size and the same depth with the
//           same F, I, A, C and XCOLORRANGE tokens.  Two frame slots, each with its own stream, pinned host
//           buffers, device frames and workspace: while one slot computes, the
//           next frame is read into the other; a slot is drained and its frame
//           written before it is reused, so frames leave in order (--slots 1:
//           one slot).  --frames N stops after N frames; --range full|limited
//           overrides the header's XCOLORRANGE (default limited).  A truncated
//           frame ends the run with an error after the frames in front of it
//           have been written.  With `profile` both slots use the pipeline's
//           stream, so that the calls can be timed.
//           --size WxH instead of --scale: OUT is W x H, each axis within
//           [1x, 4x] of IN's, whatever the ratios (1280x720 -> 1920x1080,
//           720x480 -> 1920x1080): srcnn_upscale_to for an image,
//           srcnn_upscale_frame_to for every frame of a Y4M video, whose
//           header then carries W, H and, where the two ratios differ, the A
//           that keeps the picture's shape.
// downscale: (extension) IN is a full-size image, OUT the image of 1/S the
//           size (RGB), resampled on the device by the inverse of the upscale
//           mode's bicubic (srcnn_downscale_rgba): the tool that makes an input
//           for `cnn upscale`.  Needs no CONFIG.
//           A Y4M video is streamed frame by frame through
//           srcnn_downscale_frame: OUT is a Y4M of W/S x H/S with the same F,
//           I, A, C and XCOLORRANGE tokens, at every depth upscale accepts;
//           --frames N stops after N frames.
//           --ref TRUTH.y4m (Y4M input only): TRUTH has the output's size,
//           subsampling and depth; each of its frames is uploaded into the
//           slot and the upscaled frame is measured against it where it lies,
//           on the device (srcnn_quality_frame on the slot's stream), --shave
//           pixels dropped per side (default --scale; 0 with --size).  Prints
//           what `cnn quality` prints for OUT against TRUTH; -o is optional.
// quality:  (extension) IN and --ref REF are two image files of equal size; prints
//           the PSNR, SSIM and MSE of IN against REF, measured on the device
//           on the full-range luma (srcnn_quality), --shave pixels dropped per
//           side (default 0).  Needs no CONFIG and no OUT.
//           If IN starts with the YUV4MPEG2 magic, IN and REF are Y4M videos
//           of equal size, subsampling and depth: the frames stream through
//           two slots and each pair is measured on the code values
//           (srcnn_quality_frame): one line per frame with the
//           PSNR of Y, U, V and of all three and the luma's SSIM, then the
//           stream's numbers: the PSNR of the mean of the frames' mse per
//           plane, the mean SSIM, and the lowest psnr y with its frame.
//           --frames N stops after N pairs; -o writes the numbers as JSON.
// evaluate: (extension) IN is a full-size image or a directory of them; each
//           is downscaled by S, upscaled again by the net and by plain bicubic
//           on the device and both results are measured against the image
//           (srcnn_evaluate): one line per image with the net's and bicubic's
//           PSNR and SSIM and the gain in dB, then the means.  --shave defaults
//           to S (the literature's rule); -o writes the numbers as JSON.
//           A Y4M video is evaluated frame by frame (srcnn_evaluate_frame): one
//           line per frame for the net and one for bicubic as `cnn quality`
//           prints them, the gain in dB, then both streams' numbers; the JSON
//           holds the two reports in `cnn quality`'s shape under "net" and
//           "bicubic".  --frames N stops after N frames.
// train:    IN is a directory of <name>_large.<ext> / <name>_small.<ext> pairs
//           (ground truth / degraded input, tools/make_samples.py makes
//           them), OUT the parameters.json written at the end.
//           With --from-images (extension) IN is a directory of full-size
//           images; each is cut on the device into --tile x --tile pairs at
//           --stride (defaults 33 and 14, the paper's sub-image size and
//           stride), the input tiles degraded by exactly what `cnn upscale
//           --scale S` applies at inference (srcnn_make_pairs).  A Y4M video
//           in the directory contributes the luma of every --frame-step'th
//           frame, cut by srcnn_make_pairs_frame on its code values and range;
//           the closing line counts frames as images.
//           --device-batches keeps each image's two luma planes on the device
//           instead of its tiles; every chunk of every epoch is then gathered
//           from them by a list of {plane, origin, orientation} records in one
//           launch (srcnn_gather_batch).  Same samples, same order, same
//           parameters file.  --augment (a random one of the eight flips and
//           rotations per training sample and epoch) and --random-origins (a
//           random crop per training sample and epoch instead of its grid
//           position) build on it; validation samples stay as they are.  Their
//           draws come from a second generator seeded from --seed, so the
//           shuffle and the split are the same with and without them.
// Differences from the reference, on purpose: paths are joined with '/'
// (the reference hard-codes "\\", src/Main_cl.cpp:284-287), the epoch
// shuffle is seeded (--seed; the reference uses unseeded rand()).
// Extension: `train --devices N` trains data-parallel on devices D .. D+N-1
// of one node: one host thread per device, the epoch's training set sharded
// contiguously over them, one RCCL all-reduce of the flat gradient buffer per
// epoch (srcnn_allreduce_grads over ncclCommInitAll communicators), the same
// update on every device.  Test seam: `--exchange host`
// replaces the RCCL all-reduce by a host-side sum in rank order (ranks may
// then share a device: `--same-device` puts every rank on --device), so the
// sharding, the split validation sums and the exchange logic of this driver
// run on a one-GPU machine.
#include <dirent.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <mutex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <memory>
#include <random>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "Config.hpp"
#include "ConfigBasedDataPipeline.hpp"
#include "Context.hpp"
#include "Image.hpp"
#include "Y4m.hpp"

using namespace cnn_sr;

namespace {

struct Args {
  bool train = false, upscale = false, downscale = false, quality = false, evaluate = false, dry = false, profile = false, help = false, version = false;
  unsigned scale = 2;      // upscale, downscale, train --from-images: --scale
  bool scale_set = false;
  unsigned size_w = 0, size_h = 0;  // upscale: --size WxH instead of --scale
  bool size_set = false;
  bool from_images = false;  // train --from-images: cut the pairs on the device
  size_t tile = 33, stride = 14;
  bool tile_set = false, stride_set = false;
  bool device_batches = false;  // --from-images: keep planes, gather every chunk on the device
  bool augment = false;         // ... with a random orientation per training sample and epoch
  bool random_origins = false;  // ... with a random crop per training sample and epoch
  std::string config, in, out;
  std::string ref;       // quality: --ref; upscale, Y4M: the truth to measure against
  size_t frames = 0;     // upscale, quality, Y4M: --frames (0: all)
  bool frames_set = false;
  size_t frame_step = 1;  // train --from-images, Y4M: every Nth frame
  bool frame_step_set = false;
  int range = -1;        // upscale, Y4M: --range (-1: the header's, 0 limited, 1 full)
  unsigned slots = 2;    // upscale, Y4M: --slots
  bool slots_set = false;
  unsigned shave = 0;    // quality, evaluate, upscale --ref: --shave (evaluate, upscale --scale: default --scale)
  bool shave_set = false;
  size_t epochs = 0;
  uint64_t seed = 0;
  bool seeded = false;
  int device = 0;
  int devices = 1;
  bool devices_set = false;  // --devices given: the data-parallel driver (also for N = 1)
  bool host_exchange = false;  // --exchange host: the host-sum test seam instead of RCCL
  bool same_device = false;    // --same-device: every rank on --device (needs --exchange host)
  bool save_momentum = false;  // --save-momentum: momentum into the parameters file (resumable)
  size_t validation_percent = 20;  // src/Main_cl.cpp:87
  size_t mini_batches = 2;         // src/Main_cl.cpp:88
};

void usage() {
  std::cout
      << "usage: cnn [-h] [train | upscale | downscale | quality | evaluate] [dry] [profile]\n"
         "           -c CONFIG -i IN [-o OUT] [-e EPOCHS] [--scale S] [--seed N] [--device D]\n"
         "           [--devices N] [--validation-percent P] [--mini-batches M] [--save-momentum]\n"
         "           [--from-images] [--tile N] [--stride N] [--ref REF] [--shave N]\n"
         "           [--device-batches] [--augment] [--random-origins] [--frames N]\n"
         "           [--range full|limited] [--slots N] [--size WxH] [--frame-step N]\n\n"
         "  -h, --help            print this help\n"
         "  --version             library ABI, HIP runtime and RCCL the binary runs on\n"
         "  train                 train mode\n"
         "  upscale               upscale mode: IN is a low-resolution image, OUT the image\n"
         "                        of --scale times the size (bicubic + net on the device;\n"
         "                        no un-enhanced border frame)\n"
         "                        A Y4M video (YUV4MPEG2; 4:2:0, 4:2:2 or 4:4:4 at 8 bits,\n"
         "                        or at 9 to 16 as C420p10 and its kin) is\n"
         "                        streamed frame by frame: luma through the net, chroma\n"
         "                        bicubic, OUT a Y4M of --scale times the size\n"
         "  downscale             downscale mode: IN is a full-size image, OUT the image of\n"
         "                        1 / --scale the size (the inverse of the upscale mode's\n"
         "                        bicubic, on the device; -c is not needed)\n"
         "                        A Y4M video is streamed frame by frame, luma and chroma\n"
         "                        planes alike on their code values; OUT is a Y4M of\n"
         "                        1 / --scale the size, same depth and tokens\n"
         "  quality               quality mode: PSNR, SSIM and MSE of the image IN against\n"
         "                        --ref REF (equal sizes), measured on the device on the\n"
         "                        full-range luma; -c and -o are not needed\n"
         "                        Two Y4M videos (equal size, subsampling and depth) are\n"
         "                        measured frame by frame on their code values: PSNR of Y,\n"
         "                        U, V and of all three, SSIM of Y, then the stream's\n"
         "                        numbers; -o writes them as JSON\n"
         "  evaluate              evaluate mode: IN is a full-size image or a directory of\n"
         "                        them; each is downscaled by --scale, upscaled again by the\n"
         "                        net and by plain bicubic, and both are measured against\n"
         "                        it: PSNR, SSIM and the gain in dB per image and their\n"
         "                        means; -o writes them as JSON\n"
         "                        A Y4M video is evaluated frame by frame on its code\n"
         "                        values: the net's and bicubic's PSNR of Y, U, V and all,\n"
         "                        SSIM of Y and the gain in dB, then the stream's numbers\n"
         "  dry                   do not store the result\n"
         "  profile               print kernel execution times\n"
         "  -c, --config CONFIG   CNN configuration (config.json)\n"
         "  -i, --in IN           image during forward / upscale, samples directory during\n"
         "                        training\n"
         "  -o, --out OUT         output path (result image or new parameters file)\n"
         "  -e, --epochs EPOCHS   number of epochs during training\n"
         "  --scale S             scale factor 1, 2, 3 or 4 (default 2; upscale, downscale,\n"
         "                        evaluate and train --from-images only; upscale 1: same\n"
         "                        size, every pixel through the net)\n"
         "  --size WxH            upscale: the output size instead of --scale, each axis\n"
         "                        within 1x .. 4x of the input's (any ratio, also a\n"
         "                        different one per axis)\n"
         "  --frames N            upscale, downscale, quality, evaluate, Y4M: stop after N\n"
         "                        frames\n"
         "  --frame-step N        train --from-images: of a Y4M video in the directory take\n"
         "                        every Nth frame (default 1)\n"
         "  --range full|limited  upscale, Y4M: the luma range (default: the header's\n"
         "                        XCOLORRANGE, else limited)\n"
         "  --slots N             upscale, Y4M: frames in flight, 1 or 2 (default 2)\n"
         "  --ref REF             quality: the image or Y4M video IN is measured against\n"
         "                        upscale, Y4M: the Y4M video of the output's size every\n"
         "                        upscaled frame is measured against on the device; prints\n"
         "                        what quality prints (-o is then optional)\n"
         "  --shave N             quality, evaluate, upscale --ref: pixels dropped on every\n"
         "                        side before measuring (default: 0 for quality, --scale\n"
         "                        for evaluate and upscale --scale, 0 for upscale --size)\n"
         "  --from-images         train: IN is a directory of full-size images; the sample\n"
         "                        pairs are cut on the device, the inputs degraded by\n"
         "                        --scale as the upscale mode resamples; a Y4M video in the\n"
         "                        directory contributes its frames' luma\n"
         "  --tile N              --from-images: sample size (default 33)\n"
         "  --stride N            --from-images: step between samples (default 14)\n"
         "  --device-batches      --from-images: keep the images' luma planes on the device\n"
         "                        instead of their tiles and gather every chunk from them\n"
         "                        in one launch (same samples, same result)\n"
         "  --augment             --from-images: a random flip / rotation (one of eight) per\n"
         "                        training sample and epoch (implies --device-batches)\n"
         "  --random-origins      --from-images: a random crop per training sample and epoch\n"
         "                        instead of its grid position (implies --device-batches)\n"
         "  --seed N              seed of the random parameters and the epoch shuffles\n"
         "  --device D            HIP device index (default 0)\n"
         "  --devices N           train data-parallel on devices D .. D+N-1 (default 1)\n"
         "  --exchange rccl|host  data-parallel gradient exchange (default rccl; host: a\n"
         "                        host-side sum, a test seam)\n"
         "  --same-device         every data-parallel rank on --device (with --exchange host)\n"
         "  --validation-percent  share of samples used for validation (default 20)\n"
         "  --mini-batches M      mini-batches per epoch (default 2)\n"
         "  --save-momentum       also store the momentum in the parameters file; a file\n"
         "                        that holds it resumes training with it (extension)\n";
}

/** whether the file starts with the YUV4MPEG2 magic (false if it cannot be read) */
bool is_y4m(const std::string& path) {
  std::ifstream in(path, std::ios::binary);
  char magic[9] = {};
  return in.read(magic, 9) && std::memcmp(magic, "YUV4MPEG2", 9) == 0;
}

bool parse(int argc, char** argv, Args& a) {
  for (int i = 1; i < argc; ++i) {
    std::string s = argv[i];
    auto value = [&](const char* name) -> std::string {
      if (i + 1 >= argc) throw std::runtime_error(std::string("missing value for ") + name);
      return argv[++i];
    };
    if (s == "-h" || s == "--help" || s == "help") a.help = true;
    else if (s == "--version") a.version = true;
    else if (s == "train") a.train = true;
    else if (s == "upscale") a.upscale = true;
    else if (s == "downscale") a.downscale = true;
    else if (s == "quality") a.quality = true;
    else if (s == "evaluate") a.evaluate = true;
    else if (s == "--ref") a.ref = value("--ref");
    else if (s == "--shave") {
      const std::string v = value("--shave");
      size_t n = 0, used = 0;
      try {
        n = std::stoul(v, &used);
      } catch (const std::exception&) {
        used = 0;
      }
      if (used != v.size() || v.empty() || v[0] == '-' || n > 0x7fffffffu)
        throw std::runtime_error("--shave must be a non-negative integer");
      a.shave = unsigned(n);
      a.shave_set = true;
    }
    else if (s == "--frames") {
      const std::string v = value("--frames");
      size_t n = 0, used = 0;
      try {
        n = std::stoul(v, &used);
      } catch (const std::exception&) {
        used = 0;
      }
      if (used != v.size() || v.empty() || v[0] == '-' || n == 0)
        throw std::runtime_error("--frames must be a positive integer");
      a.frames = n;
      a.frames_set = true;
    }
    else if (s == "--frame-step") {
      const std::string v = value("--frame-step");
      size_t n = 0, used = 0;
      try {
        n = std::stoul(v, &used);
      } catch (const std::exception&) {
        used = 0;
      }
      if (used != v.size() || v.empty() || v[0] == '-' || n == 0)
        throw std::runtime_error("--frame-step must be a positive integer");
      a.frame_step = n;
      a.frame_step_set = true;
    }
    else if (s == "--range") {
      const std::string v = value("--range");
      if (v != "full" && v != "limited") throw std::runtime_error("--range must be full or limited");
      a.range = v == "full";
    }
    else if (s == "--slots") {
      const std::string v = value("--slots");
      if (v != "1" && v != "2") throw std::runtime_error("--slots must be 1 or 2");
      a.slots = unsigned(v[0] - '0');
      a.slots_set = true;
    }
    else if (s == "--from-images") a.from_images = true;
    else if (s == "--device-batches") a.device_batches = true;
    else if (s == "--augment") a.augment = true;
    else if (s == "--random-origins") a.random_origins = true;
    else if (s == "--tile" || s == "--stride") {
      const std::string v = value(s.c_str());
      size_t n = 0;
      try {
        size_t used = 0;
        n = std::stoul(v, &used);
        if (used != v.size() || v[0] == '-') n = 0;
      } catch (const std::exception&) {
        n = 0;
      }
      if (n == 0 || n > 0xffffffffu) throw std::runtime_error(s + " must be a positive integer");
      (s == "--tile" ? a.tile : a.stride) = n;
      (s == "--tile" ? a.tile_set : a.stride_set) = true;
    }
    else if (s == "--scale") {
      const std::string v = value("--scale");
      if (v != "1" && v != "2" && v != "3" && v != "4")
        throw std::runtime_error("--scale must be 1, 2, 3 or 4");
      a.scale = unsigned(v[0] - '0');
      a.scale_set = true;
    }
    else if (s == "--size") {
      const std::string v = value("--size");
      const size_t x = v.find('x');
      auto number = [](const std::string& t) -> unsigned {
        if (t.empty() || t.size() > 9 || t.find_first_not_of("0123456789") != std::string::npos) return 0;
        return unsigned(std::stoul(t));
      };
      a.size_w = x == std::string::npos ? 0 : number(v.substr(0, x));
      a.size_h = x == std::string::npos ? 0 : number(v.substr(x + 1));
      if (a.size_w == 0 || a.size_h == 0) throw std::runtime_error("--size must be WxH, two positive integers");
      a.size_set = true;
    }
    else if (s == "dry") a.dry = true;
    else if (s == "profile") a.profile = true;
    else if (s == "-c" || s == "--config") a.config = value("--config");
    else if (s == "-i" || s == "--in") a.in = value("--in");
    else if (s == "-o" || s == "--out") a.out = value("--out");
    else if (s == "-e" || s == "--epochs") a.epochs = std::stoul(value("--epochs"));
    else if (s == "--seed") { a.seed = std::stoull(value("--seed")); a.seeded = true; }
    else if (s == "--device") a.device = std::stoi(value("--device"));
    else if (s == "--devices") { a.devices = std::stoi(value("--devices")); a.devices_set = true; }
    else if (s == "--exchange") {
      const std::string v = value("--exchange");
      if (v != "rccl" && v != "host") throw std::runtime_error("--exchange must be rccl or host");
      a.host_exchange = v == "host";
    }
    else if (s == "--same-device") a.same_device = true;
    else if (s == "--save-momentum") a.save_momentum = true;
    else if (s == "--validation-percent") a.validation_percent = std::stoul(value("--validation-percent"));
    else if (s == "--mini-batches") a.mini_batches = std::stoul(value("--mini-batches"));
    else throw std::runtime_error("unknown argument '" + s + "'");
  }
  if (a.help || a.version) return false;
  if (int(a.upscale) + int(a.train) + int(a.downscale) + int(a.quality) + int(a.evaluate) > 1)
    throw std::runtime_error("train, upscale, downscale, quality and evaluate are different modes");
  if (a.from_images && !a.train) throw std::runtime_error("--from-images needs the train mode");
  if ((a.tile_set || a.stride_set) && !a.from_images)
    throw std::runtime_error("--tile and --stride need train --from-images");
  if ((a.device_batches || a.augment || a.random_origins) && !a.from_images)
    throw std::runtime_error("--device-batches, --augment and --random-origins need train --from-images");
  if (a.augment || a.random_origins) a.device_batches = true;
  if (a.scale_set && !a.upscale && !a.downscale && !a.evaluate && !a.from_images)
    throw std::runtime_error(
        "--scale needs the upscale mode, the downscale mode, the evaluate mode or train --from-images");
  if (a.size_set && a.scale_set) throw std::runtime_error("--size and --scale exclude each other");
  if (a.size_set && !a.upscale) throw std::runtime_error("--size needs the upscale mode");
  if ((a.range >= 0 || a.slots_set) && !a.upscale)
    throw std::runtime_error("--range and --slots need the upscale mode");
  if (a.frames_set && !a.upscale && !a.quality && !a.downscale && !a.evaluate)
    throw std::runtime_error("--frames needs the upscale, downscale, quality or evaluate mode");
  if (a.frame_step_set && !a.from_images) throw std::runtime_error("--frame-step needs train --from-images");
  // (upscale --ref measures a Y4M stream's frames; an image input has nothing to measure per frame)
  if (!a.ref.empty() && !a.quality && !(a.upscale && is_y4m(a.in)))
    throw std::runtime_error("--ref needs the quality mode, or the upscale mode with a Y4M input");
  if (a.shave_set && !a.quality && !a.evaluate && !(a.upscale && !a.ref.empty()))
    throw std::runtime_error("--shave needs the quality mode or the evaluate mode (or upscale --ref)");
  if ((a.evaluate || (a.upscale && !a.ref.empty() && !a.size_set)) && !a.shave_set)
    a.shave = a.scale;  // the literature's rule
  if (a.quality) {
    if (a.in.empty() || a.ref.empty()) throw std::runtime_error("--in and --ref are required");
  } else if (a.downscale) {
    if (a.in.empty()) throw std::runtime_error("--in is required");
  } else if (a.config.empty() || a.in.empty()) {
    throw std::runtime_error("--config and --in are required");
  }
  if (a.devices < 1) throw std::runtime_error("--devices must be >= 1");
  if (a.same_device && !a.host_exchange)
    throw std::runtime_error("--same-device needs --exchange host (RCCL takes one rank per device)");
  return true;
}

/** <base>_large.* / <base>_small.* pairs of a samples directory
 * (src/Main_cl.cpp:267-301), sorted by base name. */
std::vector<std::pair<std::string, std::string>> training_samples(const std::string& dir) {
  DIR* d = opendir(dir.c_str());
  if (!d) throw srcnn::IOException("cannot open samples directory '" + dir + "'");
  std::map<std::string, std::pair<std::string, std::string>> by_base;
  while (dirent* e = readdir(d)) {
    std::string f = e->d_name;
    if (f == "." || f == "..") continue;
    size_t dot = f.rfind('.');
    std::string stem = dot == std::string::npos ? f : f.substr(0, dot);
    auto ends = [&](const char* suf) {
      size_t n = std::strlen(suf);
      return stem.size() > n && stem.compare(stem.size() - n, n, suf) == 0;
    };
    if (ends("_large")) by_base[stem.substr(0, stem.size() - 6)].first = dir + "/" + f;
    else if (ends("_small")) by_base[stem.substr(0, stem.size() - 6)].second = dir + "/" + f;
    else std::cout << "'" << f << "' is not a <name>_large / <name>_small image. Skipping sample" << std::endl;
  }
  closedir(d);
  std::vector<std::pair<std::string, std::string>> out;
  for (auto& kv : by_base) {
    if (kv.second.first.empty() || kv.second.second.empty())
      std::cout << "Only 1 image for pair with name '" << kv.first << "'. Skipping sample" << std::endl;
    else
      out.push_back(kv.second);
  }
  return out;
}

/** load + luma (normalised) on the device (src/Main_cl.cpp:303-318) */
void prepare_image(DataPipeline& p, const std::string& path, ImageData& img, MemoryHandle& data,
                   MemoryHandle& luma) {
  srcnn::image::load(path, img, 4);
  p.extract_luma(img, data, luma, true);
}

int forward(ConfigBasedDataPipeline& p, const Args& a) {
  auto& ctx = *p.context();
  ImageData img;
  SampleAllocationPool sample;
  prepare_image(p, a.in, img, sample.input_data, sample.input_luma);
  p.subtract_mean(sample.input_luma);
  sample.input_w = img.w;
  sample.input_h = img.h;
  ctx.block();
  GpuAllocationPool pools;
  p.forward(pools.layer_1, pools.layer_2, pools.layer_3, sample);
  if (!a.dry && !a.out.empty()) p.write_result_image(a.out.c_str(), img, sample);
  ctx.block();
  return 0;
}

/** --size against the input's size, read from the file's header or image on
 * the host, before any device is opened: each axis within [1x, 4x] */
void check_size(const Args& a) {
  uint64_t w, h;
  std::ifstream in(a.in, std::ios::binary);
  char magic[9] = {};
  if (in.read(magic, 9) && std::memcmp(magic, "YUV4MPEG2", 9) == 0) {
    in.seekg(0);
    const srcnn::y4m::Header hd = srcnn::y4m::read_header(in);
    w = hd.w, h = hd.h;
  } else {
    ImageData img;
    srcnn::image::load(a.in, img, 4);
    w = uint64_t(img.w), h = uint64_t(img.h);
  }
  if (a.size_w >= w && a.size_w <= 4 * w && a.size_h >= h && a.size_h <= 4 * h) return;
  throw std::runtime_error("--size " + std::to_string(a.size_w) + "x" + std::to_string(a.size_h) +
                           " is outside 1x .. 4x of the input's " + std::to_string(w) + "x" + std::to_string(h) +
                           " per axis: the width must lie in " + std::to_string(w) + " .. " + std::to_string(4 * w) +
                           ", the height in " + std::to_string(h) + " .. " + std::to_string(4 * h));
}

/** One frame in flight of `cnn upscale` on a Y4M stream: its own stream,
 * pinned host buffers, device frames and workspace.  Everything is released
 * when the slot goes, whatever ended the run. */
struct FrameSlot {
  srcnn_stream_t stream = nullptr;
  void *host_in = nullptr, *host_out = nullptr;  // pinned
  void *dev_in = nullptr, *dev_out = nullptr, *ws = nullptr;
  srcnn_yuv_frame src{}, dst{};
  bool busy = false;  // a frame is enqueued and not yet written
  // --ref: the truth frame, the metric's workspace and its 8 doubles (device, and a pinned copy)
  void *host_ref = nullptr, *dev_ref = nullptr, *qws = nullptr, *dev_res = nullptr, *host_res = nullptr;
  srcnn_yuv_frame ref{};

  FrameSlot() = default;
  FrameSlot(const FrameSlot&) = delete;
  FrameSlot& operator=(const FrameSlot&) = delete;
  ~FrameSlot() {
    if (stream) srcnn_stream_sync(stream);
    srcnn_free(dev_in);
    srcnn_free(dev_out);
    srcnn_free(ws);
    srcnn_free(dev_ref);
    srcnn_free(qws);
    srcnn_free(dev_res);
    srcnn_host_free(host_in);
    srcnn_host_free(host_out);
    srcnn_host_free(host_ref);
    srcnn_host_free(host_res);
    if (stream) srcnn_stream_destroy(stream);
  }
  static srcnn_yuv_frame planes(void* base, const srcnn::y4m::Header& hd) {
    uint8_t* b = static_cast<uint8_t*>(base);
    const uint32_t B = uint32_t(hd.sample_bytes());  // pitches are bytes
    return srcnn_yuv_frame{b, b + hd.luma_bytes(), b + hd.luma_bytes() + hd.chroma_bytes(), hd.w * B, hd.cw() * B};
  }
  void init(const srcnn::y4m::Header& in, const srcnn::y4m::Header& out, size_t ws_bytes, bool own_stream) {
    if (own_stream) srcnn::check(srcnn_stream_create(&stream), "stream_create");
    srcnn::check(srcnn_host_alloc(&host_in, in.frame_bytes()), "host_alloc");
    srcnn::check(srcnn_host_alloc(&host_out, out.frame_bytes()), "host_alloc");
    srcnn::check(srcnn_malloc(&dev_in, in.frame_bytes()), "malloc");
    srcnn::check(srcnn_malloc(&dev_out, out.frame_bytes()), "malloc");
    srcnn::check(srcnn_malloc(&ws, ws_bytes), "malloc");
    src = planes(dev_in, in);
    dst = planes(dev_out, out);
  }
  /** the buffers of --ref: a truth frame of `out`'s geometry and the metric's */
  void init_ref(const srcnn::y4m::Header& out, size_t qws_bytes) {
    srcnn::check(srcnn_host_alloc(&host_ref, out.frame_bytes()), "host_alloc");
    srcnn::check(srcnn_host_alloc(&host_res, 8 * sizeof(double)), "host_alloc");
    srcnn::check(srcnn_malloc(&dev_ref, out.frame_bytes()), "malloc");
    srcnn::check(srcnn_malloc(&qws, qws_bytes), "malloc");
    srcnn::check(srcnn_malloc(&dev_res, 8 * sizeof(double)), "malloc");
    ref = planes(dev_ref, out);
  }
};

/** doubles as the reports print them: 17 significant digits, so that a reader
 * gets the device's value back bit for bit; "inf" for identical images */
std::string num(double v) {
  if (std::isinf(v)) return v > 0 ? "inf" : "-inf";
  char buf[40];
  std::snprintf(buf, sizeof(buf), "%.17g", v);
  return buf;
}
/** the same for the JSON report, which has no infinity: null */
std::string json_num(double v) { return std::isfinite(v) ? num(v) : "null"; }

/** The frames' srcnn_quality_frame results of one stream (`cnn quality` on two
 * Y4M files, `cnn upscale --ref`): one line per frame as it arrives, then the
 * stream's numbers.  A frame's mse over all planes is the
 * planes' mse weighted by their sample counts. */
class StreamQuality {
 public:
  StreamQuality(const srcnn::y4m::Header& hd, unsigned shave) : _hd(hd), _shave(shave) {
    const uint64_t sx = (shave + hd.cx - 1) / hd.cx, sy = (shave + hd.cy - 1) / hd.cy;
    _ny = double((hd.w - 2 * uint64_t(shave)) * (hd.h - 2 * uint64_t(shave)));
    _nc = double((hd.cw() - 2 * sx) * (hd.ch() - 2 * sy));
    _peak2 = double((1u << hd.bits) - 1) * double((1u << hd.bits) - 1);
  }
  /** the call's own complaint about sizes too small for the metric, before any frame */
  static void check(const srcnn::y4m::Header& hd, unsigned shave) {
    const size_t ws = srcnn_quality_frame_workspace_bytes(hd.w, hd.h, hd.cx, hd.cy, shave);
    srcnn::require(ws > 0, std::string("quality: ") + srcnn_last_error());
  }
  /** label: what is measured, where one stream has several reports (" net") */
  void add(const double* r, const char* label = "") {
    const FrameQualityReport q{r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7]};
    std::cout << "frame " << _frames.size() << label << ": psnr y " << num(q.psnr_y) << " dB u " << num(q.psnr_u) << " dB v "
              << num(q.psnr_v) << " dB all " << num(q.psnr_all) << " dB ssim " << num(q.ssim_y) << std::endl;
    _frames.push_back(q);
  }
  size_t count() const { return _frames.size(); }
  struct Totals {
    double mse_y = 0, mse_u = 0, mse_v = 0, mse_all = 0, ssim = 0, min_psnr_y = INFINITY;
    size_t min_frame = 0;
  };
  Totals totals() const {
    Totals t;
    const double n = double(_frames.size());
    for (size_t i = 0; i < _frames.size(); ++i) {
      const FrameQualityReport& q = _frames[i];
      t.mse_y += q.mse_y, t.mse_u += q.mse_u, t.mse_v += q.mse_v, t.ssim += q.ssim_y;
      t.mse_all += mse_all(q);
      if (q.psnr_y < t.min_psnr_y) t.min_psnr_y = q.psnr_y, t.min_frame = i;
    }
    t.mse_y /= n, t.mse_u /= n, t.mse_v /= n, t.mse_all /= n, t.ssim /= n;
    return t;
  }
  double psnr(double mse) const { return mse == 0 ? double(INFINITY) : 10.0 * std::log10(_peak2 / mse); }
  void print_stream(const char* label = "") const {
    if (_frames.empty()) return;
    const Totals t = totals();
    std::cout << "stream" << label << ", " << _frames.size() << " frames: mse y " << num(t.mse_y) << " u " << num(t.mse_u) << " v "
              << num(t.mse_v) << " all " << num(t.mse_all) << std::endl
              << "stream" << label << ", " << _frames.size() << " frames: psnr y " << num(psnr(t.mse_y)) << " dB u "
              << num(psnr(t.mse_u)) << " dB v " << num(psnr(t.mse_v)) << " dB all " << num(psnr(t.mse_all))
              << " dB ssim " << num(t.ssim) << std::endl
              << "lowest psnr y" << label << ": " << num(t.min_psnr_y) << " dB at frame " << t.min_frame << std::endl;
  }
  double psnr_y(size_t frame) const { return _frames[frame].psnr_y; }
  void write_json(const std::string& path) const {
    std::ofstream out(path);
    if (!out) throw srcnn::IOException("cannot write report '" + path + "'");
    write_json(out);
    out.flush();
    if (!out) throw srcnn::IOException("cannot write report '" + path + "'");
    std::cout << "Saving report to: '" << path << "'" << std::endl;
  }
  /** the report as one JSON object */
  void write_json(std::ostream& out) const {
    out << "{\n  \"width\": " << _hd.w << ", \"height\": " << _hd.h << ", \"bits\": " << _hd.bits
        << ", \"chroma\": \"" << _hd.chroma << "\", \"shave\": " << _shave << ",\n  \"frames\": [\n";
    for (size_t i = 0; i < _frames.size(); ++i) {
      const FrameQualityReport& q = _frames[i];
      out << "    {\"frame\": " << i << ", \"mse_y\": " << json_num(q.mse_y) << ", \"psnr_y\": " << json_num(q.psnr_y)
          << ", \"ssim_y\": " << json_num(q.ssim_y) << ", \"mse_u\": " << json_num(q.mse_u)
          << ", \"psnr_u\": " << json_num(q.psnr_u) << ", \"mse_v\": " << json_num(q.mse_v)
          << ", \"psnr_v\": " << json_num(q.psnr_v) << ", \"psnr_all\": " << json_num(q.psnr_all) << "}"
          << (i + 1 < _frames.size() ? "," : "") << "\n";
    }
    const Totals t = totals();
    out << "  ],\n  \"stream\": {\"count\": " << _frames.size();
    if (!_frames.empty())
      out << ", \"mse_y\": " << json_num(t.mse_y) << ", \"mse_u\": " << json_num(t.mse_u)
          << ", \"mse_v\": " << json_num(t.mse_v) << ", \"mse_all\": " << json_num(t.mse_all)
          << ", \"psnr_y\": " << json_num(psnr(t.mse_y)) << ", \"psnr_u\": " << json_num(psnr(t.mse_u))
          << ", \"psnr_v\": " << json_num(psnr(t.mse_v)) << ", \"psnr_all\": " << json_num(psnr(t.mse_all))
          << ", \"ssim_y\": " << json_num(t.ssim) << ", \"min_psnr_y\": " << json_num(t.min_psnr_y)
          << ", \"min_psnr_y_frame\": " << t.min_frame;
    out << "}\n}\n";
  }

 private:
  double mse_all(const FrameQualityReport& q) const {
    return ((q.mse_y * _ny + q.mse_u * _nc) + q.mse_v * _nc) / (_ny + 2 * _nc);
  }
  srcnn::y4m::Header _hd;
  unsigned _shave;
  double _ny, _nc, _peak2;
  std::vector<FrameQualityReport> _frames;
};

/** TRUTH / REF against the stream it is measured with: size, subsampling and
 * depth must agree (one message, before any frame is read) */
void check_same_geometry(const std::string& name_a, const srcnn::y4m::Header& a, const std::string& name_b,
                         const srcnn::y4m::Header& b) {
  auto desc = [](const srcnn::y4m::Header& h) {
    return std::to_string(h.w) + "x" + std::to_string(h.h) + " " + std::to_string(h.cx) + "x" +
           std::to_string(h.cy) + " chroma subsampling, " + std::to_string(h.bits) + " bits";
  };
  if (a.w != b.w || a.h != b.h || a.cx != b.cx || a.cy != b.cy || a.bits != b.bits)
    throw std::runtime_error("the streams differ in size, subsampling or bit depth: '" + name_a + "' is " + desc(a) +
                             ", '" + name_b + "' is " + desc(b));
}

/** `cnn upscale` on a Y4M stream: every frame through srcnn_upscale_frame
 * (--scale) or srcnn_upscale_frame_to (--size).  Any
 * failed call throws, which ends the run before another frame is started. */
int upscale_y4m(ConfigBasedDataPipeline& p, const Args& a, std::istream& in) {
  namespace y4m = srcnn::y4m;
  y4m::Header hd = y4m::read_header(in);
  if (a.range >= 0) {
    hd.full_range = a.range == 1;
    hd.has_range = true;
  }
  const y4m::Header ohd = a.size_set ? hd.resized(a.size_w, a.size_h) : hd.scaled(a.scale);
  // a deep stream holds its values in the low bits of two-byte words, in planes
  const srcnn_yuv_format fmt{hd.bits, 0, SRCNN_YUV_PLANAR, hd.cx, hd.cy, hd.full_range ? SRCNN_YUV_FULL : SRCNN_YUV_LIMITED};
  std::cout << "Y4M video: " << hd.w << "x" << hd.h << " C" << hd.chroma << ", "
            << (hd.full_range ? "full" : "limited") << " range -> " << ohd.w << "x" << ohd.h << std::endl;
  const size_t ws_bytes = a.size_set ? p.super_resolve_frame_to_workspace_bytes(hd.w, hd.h, ohd.w, ohd.h)
                                     : p.super_resolve_yuv_workspace_bytes(hd.w, hd.h, a.scale);
  srcnn::require(ws_bytes > 0, std::string("upscale: ") + srcnn_last_error());
  // --ref: the truth stream, measured against every output frame where it lies
  const bool measure = !a.ref.empty();
  std::ifstream truth;
  size_t qws_bytes = 0;
  if (measure) {
    truth.open(a.ref, std::ios::binary);
    if (!truth) throw srcnn::IOException("cannot open '" + a.ref + "'");
    check_same_geometry("the output of " + a.in, ohd, a.ref, y4m::read_header(truth));
    StreamQuality::check(ohd, a.shave);
    qws_bytes = srcnn_quality_frame_workspace_bytes(ohd.w, ohd.h, ohd.cx, ohd.cy, a.shave);
    std::cout << "Measuring against: " << a.ref << ", shave: " << a.shave << std::endl;
  }
  StreamQuality report(ohd, a.shave);
  std::ofstream out;
  const bool store = !a.dry && !a.out.empty();
  if (store) {
    out.open(a.out, std::ios::binary);
    if (!out) throw srcnn::IOException("cannot open '" + a.out + "' for writing");
    y4m::write_header(out, ohd);
  }
  // profile mode: both slots on the pipeline's stream, where the calls are timed
  const bool own_streams = !a.profile;
  FrameSlot slots[2];
  for (unsigned i = 0; i < a.slots; ++i) {
    slots[i].init(hd, ohd, ws_bytes, own_streams);
    if (measure) slots[i].init_ref(ohd, qws_bytes);
  }
  auto stream_of = [&](FrameSlot& s) { return own_streams ? s.stream : p.context()->stream(); };
  size_t written = 0;
  // the slot's frame back to the host (the copy waits for the slot's work) and out
  auto drain = [&](FrameSlot& s) {
    if (!s.busy) return;
    if (store || !measure)
      srcnn::check(srcnn_memcpy_d2h(s.host_out, s.dev_out, ohd.frame_bytes(), stream_of(s)), "memcpy_d2h");
    if (measure) {  // the 8 doubles return with the frame
      srcnn::check(srcnn_memcpy_d2h(s.host_res, s.dev_res, 8 * sizeof(double), stream_of(s)), "memcpy_d2h");
      report.add(static_cast<const double*>(s.host_res));
    }
    s.busy = false;
    if (store) y4m::write_frame(out, ohd, static_cast<const unsigned char*>(s.host_out));
    ++written;
  };
  int rc = 0;
  const auto t0 = std::chrono::steady_clock::now();
  size_t k = 0;
  for (; !a.frames_set || k < a.frames; ++k) {
    FrameSlot& s = slots[k % a.slots];
    drain(s);  // frame k - slots: written before its slot is reused, so frames leave in order
    try {
      if (!y4m::read_frame(in, hd, static_cast<unsigned char*>(s.host_in))) break;
    } catch (const srcnn::IOException& e) {
      std::cout << "[ERROR] frame " << k << ": " << e.what() << std::endl;
      rc = 1;
      break;
    }
    if (measure) {
      try {
        if (!y4m::read_frame(truth, ohd, static_cast<unsigned char*>(s.host_ref))) {
          std::cout << "[ERROR] '" << a.ref << "' ends after " << k << " frames, before '" << a.in << "'" << std::endl;
          rc = 1;
          break;
        }
      } catch (const srcnn::IOException& e) {
        std::cout << "[ERROR] '" << a.ref << "' frame " << k << ": " << e.what() << std::endl;
        rc = 1;
        break;
      }
      srcnn::check(srcnn_memcpy_h2d(s.dev_ref, s.host_ref, ohd.frame_bytes(), stream_of(s)), "memcpy_h2d");
    }
    srcnn::check(srcnn_memcpy_h2d(s.dev_in, s.host_in, hd.frame_bytes(), stream_of(s)), "memcpy_h2d");
    if (a.size_set)
      p.super_resolve_frame_to(fmt, s.src, s.dst, hd.w, hd.h, ohd.w, ohd.h, s.ws, ws_bytes,
                               own_streams ? s.stream : nullptr);
    else
      p.super_resolve_frame(fmt, s.src, s.dst, hd.w, hd.h, a.scale, s.ws, ws_bytes, own_streams ? s.stream : nullptr);
    if (measure)
      p.quality_frame(fmt, s.dst, fmt, s.ref, ohd.w, ohd.h, a.shave, static_cast<double*>(s.dev_res), s.qws,
                      qws_bytes, own_streams ? s.stream : nullptr);
    s.busy = true;
  }
  for (unsigned i = 0; i < a.slots; ++i) drain(slots[(k + i) % a.slots]);  // the oldest first
  if (store) {
    out.flush();
    if (!out) throw srcnn::IOException("cannot write '" + a.out + "'");
  }
  const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  std::cout << "Frames: " << written << ", " << (sec > 0 ? double(written) / sec : 0.0) << " frames per second"
            << (store ? ", saved to '" + a.out + "'" : std::string()) << std::endl;
  if (measure) report.print_stream();
  p.context()->block();
  return rc;
}

/** `cnn upscale`: the low-resolution image through srcnn_upscale (--size:
 * srcnn_upscale_to), or a Y4M video through srcnn_upscale_frame (--size:
 * srcnn_upscale_frame_to) frame by frame */
int upscale(ConfigBasedDataPipeline& p, const Args& a) {
  {
    std::ifstream in(a.in, std::ios::binary);
    char magic[9] = {};
    if (in.read(magic, 9) && std::memcmp(magic, "YUV4MPEG2", 9) == 0) {
      in.seekg(0);
      return upscale_y4m(p, a, in);
    }
  }
  if (a.frames_set || a.range >= 0 || a.slots_set)
    throw std::runtime_error("--frames, --range and --slots need a Y4M input");
  ImageData img, res;
  srcnn::image::load(a.in, img, 4);
  if (a.size_set) p.super_resolve_to(img, a.size_w, a.size_h, res);
  else p.super_resolve(img, a.scale, res);
  if (!a.dry && !a.out.empty()) {
    std::cout << "Saving result image to: '" << a.out << "'" << std::endl;
    srcnn::image::write(a.out.c_str(), res);
  }
  p.context()->block();
  return 0;
}

/** Device and pinned host buffers of one streaming run, released when it ends,
 * whatever ended it. */
struct Buffers {
  std::vector<void*> dev, host;
  Buffers() = default;
  Buffers(const Buffers&) = delete;
  Buffers& operator=(const Buffers&) = delete;
  ~Buffers() {
    srcnn_device_sync();
    for (void* d : dev) srcnn_free(d);
    for (void* h : host) srcnn_host_free(h);
  }
  void* device(size_t bytes) {
    void* d = nullptr;
    srcnn::check(srcnn_malloc(&d, bytes), "malloc");
    dev.push_back(d);
    return d;
  }
  void* pinned(size_t bytes) {
    void* h = nullptr;
    srcnn::check(srcnn_host_alloc(&h, bytes), "host_alloc");
    host.push_back(h);
    return h;
  }
};

/** a Y4M stream's frame format: planes, the values in the low bits of their words */
srcnn_yuv_format format_of(const srcnn::y4m::Header& hd) {
  return srcnn_yuv_format{hd.bits, 0, SRCNN_YUV_PLANAR, hd.cx, hd.cy, hd.full_range ? SRCNN_YUV_FULL : SRCNN_YUV_LIMITED};
}

/** `cnn downscale` on a Y4M stream: every frame through srcnn_downscale_frame,
 * one at a time on the context's stream */
int downscale_y4m(DataPipeline& p, const Args& a, std::istream& in) {
  namespace y4m = srcnn::y4m;
  const y4m::Header hd = y4m::read_header(in);
  srcnn::require(hd.w >= a.scale && hd.h >= a.scale,
                 "frame " + std::to_string(hd.w) + "x" + std::to_string(hd.h) + " is smaller than the scale");
  y4m::Header ohd = hd;  // F, I, A, C and XCOLORRANGE as they are
  ohd.w = hd.w / a.scale;
  ohd.h = hd.h / a.scale;
  const srcnn_yuv_format fmt = format_of(hd);
  std::cout << "Y4M video: " << hd.w << "x" << hd.h << " C" << hd.chroma << " -> " << ohd.w << "x" << ohd.h << std::endl;
  std::ofstream out;
  const bool store = !a.dry && !a.out.empty();
  if (store) {
    out.open(a.out, std::ios::binary);
    if (!out) throw srcnn::IOException("cannot open '" + a.out + "' for writing");
    y4m::write_header(out, ohd);
  }
  Buffers b;
  unsigned char* host_in = static_cast<unsigned char*>(b.pinned(hd.frame_bytes()));
  unsigned char* host_out = static_cast<unsigned char*>(b.pinned(ohd.frame_bytes()));
  const srcnn_yuv_frame src = FrameSlot::planes(b.device(hd.frame_bytes()), hd);
  const srcnn_yuv_frame dst = FrameSlot::planes(b.device(ohd.frame_bytes()), ohd);
  srcnn_stream_t stream = p.context()->stream();
  int rc = 0;
  size_t k = 0;
  for (; !a.frames_set || k < a.frames; ++k) {
    try {
      if (!y4m::read_frame(in, hd, host_in)) break;
    } catch (const srcnn::IOException& e) {
      std::cout << "[ERROR] frame " << k << ": " << e.what() << std::endl;
      rc = 1;
      break;
    }
    srcnn::check(srcnn_memcpy_h2d(src.y, host_in, hd.frame_bytes(), stream), "memcpy_h2d");
    p.downscale_frame(fmt, src, dst, hd.w, hd.h, a.scale);
    srcnn::check(srcnn_memcpy_d2h(host_out, dst.y, ohd.frame_bytes(), stream), "memcpy_d2h");
    if (store) y4m::write_frame(out, ohd, host_out);
  }
  if (store) {
    out.flush();
    if (!out) throw srcnn::IOException("cannot write '" + a.out + "'");
  }
  std::cout << "Frames: " << k << (store ? ", saved to '" + a.out + "'" : std::string()) << std::endl;
  p.context()->block();
  return rc;
}

/** `cnn downscale`: the full-size image through srcnn_downscale_rgba, or a
 * Y4M video through srcnn_downscale_frame frame by frame */
int downscale(DataPipeline& p, const Args& a) {
  {
    std::ifstream in(a.in, std::ios::binary);
    char magic[9] = {};
    if (in.read(magic, 9) && std::memcmp(magic, "YUV4MPEG2", 9) == 0) {
      in.seekg(0);
      return downscale_y4m(p, a, in);
    }
  }
  if (a.frames_set) throw std::runtime_error("--frames needs a Y4M input");
  ImageData img, small;
  srcnn::image::load(a.in, img, 4);
  srcnn::require(img.w >= int(a.scale) && img.h >= int(a.scale),
                 "image " + std::to_string(img.w) + "x" + std::to_string(img.h) + " is smaller than the scale");
  p.downscale(img, a.scale, small);
  if (!a.dry && !a.out.empty()) {
    ImageData rgb(small.w, small.h, 3);
    for (size_t i = 0, n = size_t(small.w) * small.h; i < n; ++i)
      for (int c = 0; c < 3; ++c) rgb.data[3 * i + c] = small.data[4 * i + c];
    std::cout << "Saving result image to: '" << a.out << "'" << std::endl;
    srcnn::image::write(a.out.c_str(), rgb);
  }
  p.context()->block();
  return 0;
}

/** One pair of frames in flight of `cnn quality` on two Y4M streams: its own
 * stream, pinned host frames, device frames, the metric's workspace and its 8
 * doubles on the device and in pinned memory.  Released when the slot goes. */
struct QualitySlot {
  srcnn_stream_t stream = nullptr;
  void *host_a = nullptr, *host_b = nullptr, *host_res = nullptr;  // pinned
  void *dev_a = nullptr, *dev_b = nullptr, *ws = nullptr, *dev_res = nullptr;
  srcnn_yuv_frame a{}, b{};
  bool busy = false;  // a pair is enqueued and not yet reported

  QualitySlot() = default;
  QualitySlot(const QualitySlot&) = delete;
  QualitySlot& operator=(const QualitySlot&) = delete;
  ~QualitySlot() {
    if (stream) srcnn_stream_sync(stream);
    for (void* d : {dev_a, dev_b, ws, dev_res}) srcnn_free(d);
    for (void* h : {host_a, host_b, host_res}) srcnn_host_free(h);
    if (stream) srcnn_stream_destroy(stream);
  }
  void init(const srcnn::y4m::Header& hd, size_t ws_bytes, bool own_stream) {
    if (own_stream) srcnn::check(srcnn_stream_create(&stream), "stream_create");
    for (void** h : {&host_a, &host_b}) srcnn::check(srcnn_host_alloc(h, hd.frame_bytes()), "host_alloc");
    srcnn::check(srcnn_host_alloc(&host_res, 8 * sizeof(double)), "host_alloc");
    for (void** d : {&dev_a, &dev_b}) srcnn::check(srcnn_malloc(d, hd.frame_bytes()), "malloc");
    srcnn::check(srcnn_malloc(&ws, ws_bytes), "malloc");
    srcnn::check(srcnn_malloc(&dev_res, 8 * sizeof(double)), "malloc");
    a = FrameSlot::planes(dev_a, hd);
    b = FrameSlot::planes(dev_b, hd);
  }
};

/** `cnn quality` on two Y4M streams: every pair of frames through
 * srcnn_quality_frame, two pairs in flight as upscale_y4m keeps two frames */
int quality_y4m(DataPipeline& p, const Args& a, std::istream& in) {
  namespace y4m = srcnn::y4m;
  const y4m::Header hd = y4m::read_header(in);
  if (!is_y4m(a.ref)) throw std::runtime_error("'" + a.ref + "' is not a Y4M video (no YUV4MPEG2 magic)");
  std::ifstream rin(a.ref, std::ios::binary);
  const y4m::Header rhd = y4m::read_header(rin);
  check_same_geometry(a.in, hd, a.ref, rhd);
  StreamQuality::check(hd, a.shave);
  const size_t ws_bytes = srcnn_quality_frame_workspace_bytes(hd.w, hd.h, hd.cx, hd.cy, a.shave);
  // the range is validated and enters no arithmetic: both sides take IN's
  const srcnn_yuv_format fmt{hd.bits, 0, SRCNN_YUV_PLANAR, hd.cx, hd.cy, hd.full_range ? SRCNN_YUV_FULL : SRCNN_YUV_LIMITED};
  std::cout << "Y4M videos: " << hd.w << "x" << hd.h << " C" << hd.chroma << ", " << hd.bits << " bits" << std::endl;
  const bool own_streams = !a.profile;  // profile mode: the context's stream, where the calls are timed
  StreamQuality report(hd, a.shave);
  QualitySlot slots[2];
  for (auto& s : slots) s.init(hd, ws_bytes, own_streams);
  auto stream_of = [&](QualitySlot& s) { return own_streams ? s.stream : p.context()->stream(); };
  auto drain = [&](QualitySlot& s) {
    if (!s.busy) return;
    srcnn::check(srcnn_memcpy_d2h(s.host_res, s.dev_res, 8 * sizeof(double), stream_of(s)), "memcpy_d2h");
    s.busy = false;
    report.add(static_cast<const double*>(s.host_res));
  };
  int rc = 0;
  size_t k = 0;
  for (; !a.frames_set || k < a.frames; ++k) {
    QualitySlot& s = slots[k % 2];
    drain(s);  // pair k - 2: reported before its slot is reused, so the lines come in order
    try {
      const bool more_a = y4m::read_frame(in, hd, static_cast<unsigned char*>(s.host_a));
      const bool more_b = y4m::read_frame(rin, rhd, static_cast<unsigned char*>(s.host_b));
      if (!more_a && !more_b) break;
      if (more_a != more_b) {
        const std::string &shorter = more_a ? a.ref : a.in, &longer = more_a ? a.in : a.ref;
        std::cout << "[ERROR] '" << shorter << "' ends after " << k << " frames, before '" << longer << "'" << std::endl;
        rc = 1;
        break;
      }
    } catch (const srcnn::IOException& e) {
      std::cout << "[ERROR] frame " << k << ": " << e.what() << std::endl;
      rc = 1;
      break;
    }
    srcnn::check(srcnn_memcpy_h2d(s.dev_a, s.host_a, hd.frame_bytes(), stream_of(s)), "memcpy_h2d");
    srcnn::check(srcnn_memcpy_h2d(s.dev_b, s.host_b, hd.frame_bytes(), stream_of(s)), "memcpy_h2d");
    p.quality_frame(fmt, s.a, fmt, s.b, hd.w, hd.h, a.shave, static_cast<double*>(s.dev_res), s.ws, ws_bytes,
                    own_streams ? s.stream : nullptr);
    s.busy = true;
  }
  for (unsigned i = 0; i < 2; ++i) drain(slots[(k + i) % 2]);  // the older first
  report.print_stream();
  if (!a.dry && !a.out.empty()) report.write_json(a.out);
  p.context()->block();
  return rc;
}

/** `cnn quality`: the image against --ref through srcnn_quality, or a Y4M
 * video against another through srcnn_quality_frame */
int quality(DataPipeline& p, const Args& a) {
  {
    std::ifstream in(a.in, std::ios::binary);
    char magic[9] = {};
    if (in.read(magic, 9) && std::memcmp(magic, "YUV4MPEG2", 9) == 0) {
      in.seekg(0);
      return quality_y4m(p, a, in);
    }
  }
  if (a.frames_set) throw std::runtime_error("--frames needs a Y4M input");
  ImageData img, ref;
  srcnn::image::load(a.in, img, 4);
  srcnn::image::load(a.ref, ref, 4);
  srcnn::require(img.w == ref.w && img.h == ref.h,
                 "the images differ in size: " + std::to_string(img.w) + "x" + std::to_string(img.h) + " / " +
                     std::to_string(ref.w) + "x" + std::to_string(ref.h));
  srcnn::require(uint64_t(img.w) >= 2 * uint64_t(a.shave) + 11 && uint64_t(img.h) >= 2 * uint64_t(a.shave) + 11,
                 "image " + std::to_string(img.w) + "x" + std::to_string(img.h) + " with " +
                     std::to_string(a.shave) + " pixels shaved per side is smaller than the 11x11 SSIM window");
  const QualityReport q = p.quality(img, ref, a.shave);
  std::cout << "psnr: " << num(q.psnr) << " dB" << std::endl
            << "ssim: " << num(q.ssim) << std::endl
            << "mse: " << num(q.mse) << std::endl;
  p.context()->block();
  return 0;
}

/** `cnn evaluate` on a Y4M stream: every frame through srcnn_evaluate_frame, one
 * at a time on the context's stream; the net's and bicubic's numbers as two
 * stream reports of `cnn quality`'s shape */
int evaluate_y4m(ConfigBasedDataPipeline& p, const Args& a, std::istream& in) {
  namespace y4m = srcnn::y4m;
  const y4m::Header hd = y4m::read_header(in);
  srcnn::require(hd.w >= a.scale && hd.h >= a.scale,
                 "frame " + std::to_string(hd.w) + "x" + std::to_string(hd.h) + " is smaller than the scale");
  y4m::Header mhd = hd;  // what is measured: the truth's top-left s*(W/s) x s*(H/s)
  mhd.w = hd.w / a.scale * a.scale;
  mhd.h = hd.h / a.scale * a.scale;
  const srcnn_yuv_format fmt = format_of(hd);
  StreamQuality::check(mhd, a.shave);
  const size_t ws_bytes = p.evaluate_frame_workspace_bytes(fmt, hd.w, hd.h, a.scale);
  srcnn::require(ws_bytes > 0, std::string("evaluate: ") + srcnn_last_error());
  std::cout << "Y4M video: " << hd.w << "x" << hd.h << " C" << hd.chroma << ", " << hd.bits << " bits, scale " << a.scale
            << ", measured on " << mhd.w << "x" << mhd.h << ", shave " << a.shave << std::endl;
  StreamQuality net(mhd, a.shave), bic(mhd, a.shave);
  Buffers b;
  unsigned char* host = static_cast<unsigned char*>(b.pinned(hd.frame_bytes()));
  double* host_res = static_cast<double*>(b.pinned(16 * sizeof(double)));
  const srcnn_yuv_frame truth = FrameSlot::planes(b.device(hd.frame_bytes()), hd);
  void* ws = b.device(ws_bytes);
  double* dev_res = static_cast<double*>(b.device(16 * sizeof(double)));
  srcnn_stream_t stream = p.context()->stream();
  int rc = 0;
  for (size_t k = 0; !a.frames_set || k < a.frames; ++k) {
    try {
      if (!y4m::read_frame(in, hd, host)) break;
    } catch (const srcnn::IOException& e) {
      std::cout << "[ERROR] frame " << k << ": " << e.what() << std::endl;
      rc = 1;
      break;
    }
    srcnn::check(srcnn_memcpy_h2d(truth.y, host, hd.frame_bytes(), stream), "memcpy_h2d");
    p.evaluate_frame(fmt, truth, hd.w, hd.h, a.scale, a.shave, dev_res, ws, ws_bytes);
    srcnn::check(srcnn_memcpy_d2h(host_res, dev_res, 16 * sizeof(double), stream), "memcpy_d2h");
    net.add(host_res, " net");
    bic.add(host_res + 8, " bicubic");
    std::cout << "frame " << k << " gain: " << num(host_res[1] - host_res[9]) << " dB" << std::endl;
  }
  if (net.count() == 0) throw std::runtime_error("no frame to evaluate in '" + a.in + "'");
  net.print_stream(" net");
  bic.print_stream(" bicubic");
  const double gain = net.psnr(net.totals().mse_y) - bic.psnr(bic.totals().mse_y);
  std::cout << "stream gain: " << num(gain) << " dB" << std::endl;
  if (!a.dry && !a.out.empty()) {
    std::ofstream out(a.out);
    if (!out) throw srcnn::IOException("cannot write report '" + a.out + "'");
    out << "{\n\"scale\": " << a.scale << ",\n\"net\": ";
    net.write_json(out);
    out << ",\n\"bicubic\": ";
    bic.write_json(out);
    out << ",\n\"gain_db\": [";
    for (size_t i = 0; i < net.count(); ++i) out << (i ? ", " : "") << json_num(net.psnr_y(i) - bic.psnr_y(i));
    out << "],\n\"stream_gain_db\": " << json_num(gain) << "\n}\n";
    out.flush();
    if (!out) throw srcnn::IOException("cannot write report '" + a.out + "'");
    std::cout << "Saving report to: '" << a.out << "'" << std::endl;
  }
  p.context()->block();
  return rc;
}

/** `cnn evaluate`: IN, or every file of the directory IN that decodes, in name
 * order, through srcnn_evaluate; a Y4M video through srcnn_evaluate_frame frame
 * by frame */
int evaluate(ConfigBasedDataPipeline& p, const Args& a) {
  {
    std::ifstream in(a.in, std::ios::binary);
    char magic[9] = {};
    if (in.read(magic, 9) && std::memcmp(magic, "YUV4MPEG2", 9) == 0) {
      in.seekg(0);
      return evaluate_y4m(p, a, in);
    }
  }
  if (a.frames_set) throw std::runtime_error("--frames needs a Y4M input");
  std::vector<std::string> names;  // relative to `base`
  std::string base;
  if (DIR* d = opendir(a.in.c_str())) {
    while (dirent* e = readdir(d)) {
      std::string f = e->d_name;
      if (f != "." && f != "..") names.push_back(f);
    }
    closedir(d);
    std::sort(names.begin(), names.end());
    base = a.in + "/";
  } else {
    names.push_back(a.in);
  }
  struct Row {
    std::string name;
    int w, h;
    QualityReport net, bic;
  };
  std::vector<Row> rows;
  for (auto& f : names) {
    ImageData img;
    try {
      srcnn::image::load(base + f, img, 4);
    } catch (const std::exception& e) {
      if (base.empty()) throw;  // a single file that does not decode is an error
      std::cout << "'" << f << "' does not decode (" << e.what() << "). Skipping image" << std::endl;
      continue;
    }
    Row r{f, img.w, img.h, {}, {}};
    if (!p.evaluate(img, a.scale, a.shave, r.net, r.bic)) {
      std::cout << "'" << f << "' (" << img.w << "x" << img.h << ") is too small for one 11x11 window at scale "
                << a.scale << " with " << a.shave << " pixels shaved. Skipping image" << std::endl;
      continue;
    }
    std::cout << "'" << f << "' (" << img.w << "x" << img.h << "): net psnr " << num(r.net.psnr) << " dB ssim "
              << num(r.net.ssim) << " | bicubic psnr " << num(r.bic.psnr) << " dB ssim " << num(r.bic.ssim)
              << " | gain " << num(r.net.psnr - r.bic.psnr) << " dB" << std::endl;
    rows.push_back(r);
  }
  if (rows.empty()) throw std::runtime_error("no image to evaluate in '" + a.in + "'");
  QualityReport mn, mb;
  for (auto& r : rows) {
    mn.psnr += r.net.psnr / rows.size(), mn.ssim += r.net.ssim / rows.size();
    mb.psnr += r.bic.psnr / rows.size(), mb.ssim += r.bic.ssim / rows.size();
  }
  std::cout << "mean over " << rows.size() << " images: net psnr " << num(mn.psnr) << " dB ssim " << num(mn.ssim)
            << " | bicubic psnr " << num(mb.psnr) << " dB ssim " << num(mb.ssim) << " | gain "
            << num(mn.psnr - mb.psnr) << " dB" << std::endl;
  if (!a.dry && !a.out.empty()) {
    std::ofstream out(a.out);
    if (!out) throw srcnn::IOException("cannot write report '" + a.out + "'");
    auto esc = [](const std::string& s) {
      std::string o;
      for (char c : s) {
        if (c == '"' || c == '\\') o += '\\';
        if ((unsigned char)c < 0x20) o += ' ';
        else o += c;
      }
      return o;
    };
    auto q = [&](const QualityReport& r, bool with_mse) {
      return "{\"psnr\": " + json_num(r.psnr) + ", \"ssim\": " + json_num(r.ssim) +
             (with_mse ? ", \"mse\": " + json_num(r.mse) : std::string()) + "}";
    };
    out << "{\n  \"scale\": " << a.scale << ",\n  \"shave\": " << a.shave << ",\n  \"images\": [\n";
    for (size_t i = 0; i < rows.size(); ++i) {
      auto& r = rows[i];
      out << "    {\"name\": \"" << esc(r.name) << "\", \"width\": " << r.w << ", \"height\": " << r.h
          << ", \"net\": " << q(r.net, true) << ", \"bicubic\": " << q(r.bic, true)
          << ", \"gain_db\": " << json_num(r.net.psnr - r.bic.psnr) << "}" << (i + 1 < rows.size() ? "," : "")
          << "\n";
    }
    out << "  ],\n  \"mean\": {\"count\": " << rows.size() << ", \"net\": " << q(mn, false)
        << ", \"bicubic\": " << q(mb, false) << ", \"gain_db\": " << json_num(mn.psnr - mb.psnr) << "}\n}\n";
    std::cout << "Saving report to: '" << a.out << "'" << std::endl;
  }
  p.context()->block();
  return 0;
}

/** `train --from-images`: every file of the directory that decodes, in name
 * order, cut into sample pairs on the device (one srcnn_make_pairs call per
 * image); with --device-batches the images' planes are kept instead
 * (make_training_planes) and `grid` receives one record per sample, in the
 * order the samples would have: image order, then grid index, op 0; `extent`
 * the plane extent of each record's image */
void pairs_from_images(ConfigBasedDataPipeline& p, const Args& a, bool lead,
                       std::vector<SampleAllocationPool>& samples, std::vector<srcnn_tile_ref>& grid,
                       std::vector<std::pair<uint32_t, uint32_t>>& extent) {
  DIR* d = opendir(a.in.c_str());
  if (!d) throw srcnn::IOException("cannot open images directory '" + a.in + "'");
  std::vector<std::string> names;
  while (dirent* e = readdir(d)) {
    std::string f = e->d_name;
    if (f != "." && f != "..") names.push_back(f);
  }
  closedir(d);
  std::sort(names.begin(), names.end());
  size_t images = 0;
  // one sample per tile of the grid g, as records or as the tiles already appended
  auto record = [&](const ConfigBasedDataPipeline::TrainingGrid& g) {
    for (size_t i = 0; i < g.count; ++i) {
      grid.push_back({uint32_t(g.plane), uint32_t(i % g.nx * a.stride), uint32_t(i / g.nx * a.stride), 0});
      extent.push_back({uint32_t(g.w), uint32_t(g.h)});
    }
  };
  for (auto& f : names) {
    if (is_y4m(a.in + "/" + f)) {
      // a Y4M video: the luma of every --frame-step'th frame, cut on its code values
      namespace y4m = srcnn::y4m;
      std::ifstream in(a.in + "/" + f, std::ios::binary);
      const y4m::Header hd = y4m::read_header(in);
      const srcnn_yuv_format fmt = format_of(hd);
      Buffers b;
      unsigned char* host = static_cast<unsigned char*>(b.pinned(hd.frame_bytes()));
      const srcnn_yuv_frame frame{static_cast<uint8_t*>(b.device(hd.luma_bytes())), nullptr, nullptr,
                                  uint32_t(hd.w * hd.sample_bytes()), 0};
      for (size_t k = 0; y4m::read_frame(in, hd, host); ++k) {
        if (k % a.frame_step) continue;
        srcnn::check(srcnn_memcpy_h2d(frame.y, host, hd.luma_bytes(), p.context()->stream()), "memcpy_h2d");
        size_t n;
        if (a.device_batches) {
          const auto g = p.make_training_planes(fmt, frame, hd.w, hd.h, a.scale, a.tile, a.stride);
          n = g.count;
          record(g);
        } else {
          n = p.make_training_pairs(fmt, frame, hd.w, hd.h, a.scale, a.tile, a.stride, samples);
        }
        if (n == 0) {
          if (lead)
            std::cout << "'" << f << "' (" << hd.w << "x" << hd.h << ") is too small for one " << a.tile << "x"
                      << a.tile << " tile at scale " << a.scale << ". Skipping video" << std::endl;
          break;
        }
        ++images;
      }
      continue;
    }
    ImageData img;
    try {
      srcnn::image::load(a.in + "/" + f, img, 4);
    } catch (const std::exception& e) {
      if (lead) std::cout << "'" << f << "' does not decode (" << e.what() << "). Skipping image" << std::endl;
      continue;
    }
    size_t n;
    if (a.device_batches) {
      const auto g = p.make_training_planes(img, a.scale, a.tile, a.stride);
      n = g.count;
      record(g);
    } else {
      n = p.make_training_pairs(img, a.scale, a.tile, a.stride, samples);
    }
    if (n == 0) {
      if (lead)
        std::cout << "'" << f << "' (" << img.w << "x" << img.h << ") is too small for one " << a.tile << "x"
                  << a.tile << " tile at scale " << a.scale << ". Skipping image" << std::endl;
      continue;
    }
    ++images;
  }
  if (a.device_batches && !grid.empty()) p.upload_plane_table();
  if (lead)
    std::cout << "created " << (a.device_batches ? grid.size() : samples.size()) << " sample pairs from "
              << images << " images" << std::endl;
}

/** Contiguous slice [start, start + count) of n items for `rank` of `world`
 * (the remainder goes to the lowest ranks; srcnn_amd/parallel.py shard). */
std::pair<size_t, size_t> shard(size_t n, int rank, int world) {
  size_t base = n / world, rem = n % world, r = size_t(rank);
  return {r * base + std::min(r, rem), base + (r < rem ? 1 : 0)};
}

/** One training run (src/Main_cl.cpp:157-195).  comm == nullptr: a single
 * device.  Otherwise rank `rank` of a data-parallel run: every rank loads
 * all samples and draws the same epoch split (same shuffle seed), trains on
 * its shard of the training set, the gradients are all-reduced, and every
 * rank applies the update with batch = |training set|. */
int train(ConfigBasedDataPipeline& p, const Args& a, uint64_t shuffle_seed, GradientExchange* comm = nullptr,
          int rank = 0, int world = 1) {
  auto& ctx = *p.context();
  const bool lead = rank == 0;
  GpuAllocationPool pools;
  std::vector<std::pair<std::string, std::string>> files;
  std::vector<srcnn_tile_ref> grid;                    // --device-batches: the samples, as records
  std::vector<std::pair<uint32_t, uint32_t>> extent;  // ... and the extent of each one's image
  if (a.from_images) pairs_from_images(p, a, lead, pools.samples, grid, extent);
  else files = training_samples(a.in);
  const size_t total = a.device_batches ? grid.size() : a.from_images ? pools.samples.size() : files.size();
  if (total == 0) throw std::runtime_error("no training samples in '" + a.in + "'");
  const size_t nval = total * a.validation_percent / 100, ntrain = total - nval;
  if (lead) {
    if (nval == 0) std::cout << "[WARNING] Validation set is empty" << std::endl;
    else
      std::cout << "validation_set_size: " << nval << "/" << total << " = "
                << (nval * 100.0f / total) << "%" << std::endl;
  }
  srcnn::require(ntrain > 0, "Training set is empty");
  const size_t my_train = shard(ntrain, rank, world).second;
  p.set_mini_batch_size(std::max<size_t>(my_train, 1) / a.mini_batches + a.mini_batches);  // src/Main_cl.cpp:128-129

  for (auto& f : files) {
    ImageData large, small;
    SampleAllocationPool s;
    prepare_image(p, f.first, large, s.expected_data, s.expected_luma);
    prepare_image(p, f.second, small, s.input_data, s.input_luma);
    srcnn::require(large.w == small.w && large.h == small.h,
                   "sample pair sizes differ: " + f.first + " / " + f.second);
    p.subtract_mean(s.input_luma);
    s.input_w = small.w;
    s.input_h = small.h;
    ctx.block();
    ctx.raw_memory(s.input_data)->release();  // 3-channel images are not needed any more
    ctx.raw_memory(s.expected_data)->release();
    pools.samples.push_back(s);
  }
  const size_t px = a.device_batches ? a.tile * a.tile : pools.samples[0].input_w * pools.samples[0].input_h;

  std::mt19937_64 rng(shuffle_seed);
  // --augment / --random-origins draw from a generator of their own, so that
  // the shuffle and the split do not depend on them; per epoch, for every
  // training sample in the epoch's order (before sharding: every rank draws the
  // same): x, then y (--random-origins), then op (--augment)
  std::mt19937_64 aug_rng(shuffle_seed ^ 0x9e3779b97f4a7c15ull);
  auto draw = [&aug_rng](uint64_t k) {  // uniform over 0 .. k-1, by rejection
    const uint64_t lim = ~uint64_t(0) - ~uint64_t(0) % k;
    uint64_t v;
    do v = aug_rng();
    while (v >= lim);
    return uint32_t(v % k);
  };
  std::vector<size_t> order(total);
  bool error = false;
  for (size_t epoch = 0; epoch < a.epochs; ++epoch) {
    // new random validation / training split every epoch (src/Main_cl.cpp:244-261)
    for (size_t i = 0; i < order.size(); ++i) order[i] = i;
    std::shuffle(order.begin(), order.end(), rng);

    std::vector<SampleAllocationPool*> val, tr;
    std::vector<srcnn_tile_ref> rval, rtr;  // --device-batches: the two sets as records
    if (a.device_batches) {
      for (size_t i = 0; i < order.size(); ++i) {
        srcnn_tile_ref r = grid[order[i]];
        if (i >= nval) {
          if (a.random_origins) {
            r.x = draw(uint64_t(extent[order[i]].first) - a.tile + 1);
            r.y = draw(uint64_t(extent[order[i]].second) - a.tile + 1);
          }
          if (a.augment) r.op = draw(8);
        }
        (i < nval ? rval : rtr).push_back(r);
      }
    } else {
      for (size_t i = 0; i < order.size(); ++i) (i < nval ? val : tr).push_back(&pools.samples[order[i]]);
    }
    // forward (+ backpropagation) over `count` samples from `first` of the
    // epoch's training (backprop) or validation set
    auto execute = [&](bool backprop, size_t first, size_t count) {
      if (a.device_batches) {
        auto& set = backprop ? rtr : rval;
        if (count == set.size()) return p.execute_batch_refs(backprop, pools, set);
        std::vector<srcnn_tile_ref> mine(set.begin() + first, set.begin() + first + count);
        return p.execute_batch_refs(backprop, pools, mine);
      }
      auto& set = backprop ? tr : val;
      if (count == set.size()) return p.execute_batch(backprop, pools, set);
      std::vector<SampleAllocationPool*> mine(set.begin() + first, set.begin() + first + count);
      return p.execute_batch(backprop, pools, mine);
    };

    if (comm) {
      auto sh = shard(ntrain, rank, world);
      if (sh.second) execute(true, sh.first, sh.second);
      p.allreduce_gradients(pools, *comm);
    } else {
      execute(true, 0, ntrain);
    }
    p.update_parameters(pools.layer_1, pools.layer_2, pools.layer_3, ntrain);

    if (nval && (epoch % 25 == 0 || epoch == a.epochs - 1)) {
      float err;
      if (comm) {
        auto sh = shard(nval, rank, world);
        err = p.allreduce_sum(sh.second ? execute(false, sh.first, sh.second) : 0.f, *comm);
      } else {
        err = execute(false, 0, nval);
      }
      if (std::isnan(err)) {
        if (lead)
          std::cout << "Error: squared error is NAN, after " << epoch << "/" << a.epochs << " epochs"
                    << std::endl;
        error = true;
        break;
      }
      float mean = err / nval;
      if (lead)
        std::cout << "[" << epoch << "] mean validation error: " << mean << " (" << (mean / px)
                  << " per px)" << std::endl;
    }
  }
  p.set_save_momentum(a.save_momentum);
  if (lead && !a.dry && !a.out.empty())
    p.write_params_to_file(a.out.c_str(), pools.layer_1, pools.layer_2, pools.layer_3);
  ctx.block();
  if (lead) std::cout << "DONE" << std::endl;
  return error ? 1 : 0;
}

/** `--exchange host` (test seam): the ranks' buffers meet in host memory
 * and every rank adds them up in rank order, so all ranks get bit-identical
 * sums; two barriers per exchange (deposit, then read) keep a fast rank from
 * overwriting its slot while a slow one still reads it. */
class HostSumExchange {
 public:
  explicit HostSumExchange(int n) : _n(n), _slots(n) {}
  class Rank : public GradientExchange {
   public:
    Rank(HostSumExchange* h, int r) : _h(h), _r(r) {}
    void allreduce(srcnn::Context& ctx, float* buf, size_t count) override {
      auto& mine = _h->_slots[_r];
      mine.resize(count);
      srcnn::check(srcnn_memcpy_d2h(mine.data(), buf, count * sizeof(float), ctx.stream()),
                   "host exchange: read");
      _h->barrier();
      std::vector<float> sum(_h->_slots[0]);
      for (int k = 1; k < _h->_n; ++k)
        for (size_t i = 0; i < count; ++i) sum[i] += _h->_slots[k][i];
      _h->barrier();
      srcnn::check(srcnn_memcpy_h2d(buf, sum.data(), count * sizeof(float), ctx.stream()),
                   "host exchange: write");
    }

   private:
    HostSumExchange* _h;
    int _r;
  };

 private:
  void barrier() {
    std::unique_lock<std::mutex> lk(_mu);
    if (_aborted) throw std::runtime_error("host exchange: another rank failed");
    const unsigned gen = _gen;
    if (++_arrived == _n) {
      _arrived = 0;
      ++_gen;
      _cv.notify_all();
    } else {
      _cv.wait(lk, [&] { return _gen != gen || _aborted; });
      if (_gen == gen) throw std::runtime_error("host exchange: another rank failed");
    }
  }

 public:
  /** A failing rank releases the ranks parked in barrier(): they throw
   * instead of waiting for an arrival that will never come. */
  void abort() {
    std::lock_guard<std::mutex> lk(_mu);
    _aborted = true;
    _cv.notify_all();
  }

 private:
  const int _n;
  std::vector<std::vector<float>> _slots;
  std::mutex _mu;
  std::condition_variable _cv;
  int _arrived = 0;
  unsigned _gen = 0;
  bool _aborted = false;
};

/** `train --devices N`: one thread per device, each with its own Context
 * (HIP device and stream) and pipeline over the same config and seed. */
int train_data_parallel(const Config& cfg, const Args& a) {
  const int n = a.devices;
  std::vector<int> devs(n);
  for (int i = 0; i < n; ++i) devs[i] = a.same_device ? a.device : a.device + i;
  std::vector<srcnn_comm_t> comms(n, nullptr);
  std::vector<std::unique_ptr<GradientExchange>> ex(n);
  HostSumExchange host(n);
  if (a.host_exchange) {
    for (int r = 0; r < n; ++r) ex[r].reset(new HostSumExchange::Rank(&host, r));
  } else {
    srcnn::check(srcnn_comm_init_all(comms.data(), n, devs.data()), "srcnn_comm_init_all");
    for (int r = 0; r < n; ++r) ex[r].reset(new RcclExchange(comms[r]));
  }
  std::cout << "Data-parallel training on " << n << " devices (" << devs.front() << ".."
            << devs.back() << "), " << (a.host_exchange ? "host-sum" : "RCCL") << " gradient all-reduce"
            << std::endl;
  const uint64_t seed = a.seeded ? a.seed : std::random_device{}();
  std::vector<int> rcs(n, 0);
  std::vector<std::thread> threads;
  for (int r = 0; r < n; ++r) {
    threads.emplace_back([&, r]() {
      try {
        Config my_cfg = cfg;
        srcnn::Context context;
        context.init(a.profile && r == 0, devs[r]);
        ConfigBasedDataPipeline pipeline(my_cfg, &context);
        pipeline.set_random_seed(seed);  // identical initial replicas
        pipeline.init(DataPipeline::LOAD_KERNEL_ALL);
        rcs[r] = train(pipeline, a, seed, ex[r].get(), r, n);
      } catch (const std::exception& e) {
        std::cout << "[ERROR] rank " << r << ": " << e.what() << std::endl;
        std::cout.flush();
        if (a.host_exchange) {
          // the host-sum seam: release the ranks parked in its barrier (they
          // throw and report in turn), then join them as usual
          host.abort();
          rcs[r] = 1;
          return;
        }
        // RCCL: the other ranks may be parked in a collective this one will
        // never join and cannot be released from here; leave without
        // unwinding them
        _exit(1);
      }
    });
  }
  for (auto& t : threads) t.join();
  for (auto c : comms)
    if (c) srcnn_comm_destroy(c);
  int rc = 0;
  for (int v : rcs) rc |= v;
  return rc;
}

/** `cnn --version`: the C ABI version, the HIP runtime and the RCCL this
 * process loaded (the RCCL matches the HIP runtime) */
void print_version() {
  std::cout << "libsrcnn_hip ABI " << srcnn_abi_version() << std::endl;
  std::string hip;
  std::ifstream maps("/proc/self/maps");
  for (std::string line; std::getline(maps, line);) {
    const size_t at = line.find('/');
    if (at != std::string::npos && line.find("libamdhip64.so") != std::string::npos) {
      hip = line.substr(at);
      break;
    }
  }
  std::cout << "HIP runtime " << (hip.empty() ? "(not loaded)" : hip) << std::endl;
  int v = 0;
  char path[4096] = {0};
  srcnn::check(srcnn_comm_version(&v, path, sizeof(path)), "srcnn_comm_version");
  std::cout << "RCCL " << v / 10000 << "." << (v / 100) % 100 << "." << v % 100 << " " << path << std::endl;
}

}  // namespace

int main(int argc, char** argv) {
  Args a;
  try {
    if (!parse(argc, argv, a)) {
      if (a.version) {
        print_version();
        return 0;
      }
      usage();
      return 0;
    }
  } catch (const std::exception& e) {
    std::cout << e.what() << std::endl;
    usage();
    return 1;
  }
  if (!a.dry && a.out.empty() && !a.quality && !a.evaluate &&
      !(a.upscale && !a.ref.empty())) {  // (those print their result)
    std::cout << "Either provide out path or do the dry run" << std::endl;
    return 1;
  }
  if (a.profile)
    std::cout << "!!! RUNNING IN PROFILING MODE !!!" << std::endl;
  if (a.train)
    std::cout << "Training mode, epochs: " << a.epochs << std::endl
              << (a.from_images ? "Full-size images directory (pairs cut on the device, scale " +
                                      std::to_string(a.scale) + ", tile " + std::to_string(a.tile) +
                                      ", stride " + std::to_string(a.stride) + "): "
                                : std::string("Training samples directory: "))
              << a.in << std::endl
              << (a.device_batches
                      ? std::string("Batches gathered on the device from resident planes: ") +
                            (a.random_origins ? "random origins" : "grid origins") + ", " +
                            (a.augment ? "random orientations" : "orientation 0") + " for training samples\n"
                      : std::string())
              << "Output: " << (a.dry ? "-" : a.out) << std::endl;
  else if (a.downscale)
    std::cout << "Downscale mode, scale: " << a.scale << std::endl
              << "Input image: " << a.in << std::endl
              << "Output: " << (a.dry ? "-" : a.out) << std::endl;
  else if (a.quality)
    std::cout << "Quality mode, shave: " << a.shave << std::endl
              << "Input image: " << a.in << std::endl
              << "Reference image: " << a.ref << std::endl;
  else if (a.evaluate)
    std::cout << "Evaluate mode, scale: " << a.scale << ", shave: " << a.shave << std::endl
              << "Full-size image or directory: " << a.in << std::endl
              << "Report: " << (a.dry || a.out.empty() ? "-" : a.out) << std::endl;
  else if (a.upscale && a.size_set)
    std::cout << "Upscale mode, size: " << a.size_w << "x" << a.size_h << std::endl
              << "Input image: " << a.in << std::endl
              << "Output: " << (a.dry ? "-" : a.out) << std::endl;
  else if (a.upscale)
    std::cout << "Upscale mode, scale: " << a.scale << std::endl
              << "Input image: " << a.in << std::endl
              << "Output: " << (a.dry ? "-" : a.out) << std::endl;
  else
    std::cout << "Forward mode" << std::endl
              << "Input image: " << a.in << std::endl
              << "Output: " << (a.dry ? "-" : a.out) << std::endl;
  try {
    if (a.size_set) check_size(a);
    if (a.downscale) {
      srcnn::Context context;
      context.init(a.profile, a.device);
      DataPipeline pipeline(&context);
      pipeline.init(DataPipeline::LOAD_KERNEL_LUMA);
      return downscale(pipeline, a);
    }
    if (a.quality) {
      srcnn::Context context;
      context.init(a.profile, a.device);
      DataPipeline pipeline(&context);
      pipeline.init(DataPipeline::LOAD_KERNEL_LUMA);
      return quality(pipeline, a);
    }
    ConfigReader reader;
    Config cfg = reader.read(a.config.c_str());
    std::cout << cfg << std::endl;
    if (a.train && a.devices_set) return train_data_parallel(cfg, a);
    srcnn::Context context;
    context.init(a.profile, a.device);
    int rc;
    {
      ConfigBasedDataPipeline pipeline(cfg, &context);
      if (a.seeded) pipeline.set_random_seed(a.seed);
      pipeline.init(DataPipeline::LOAD_KERNEL_ALL);
      rc = a.train      ? train(pipeline, a, a.seeded ? a.seed : std::random_device{}())
           : a.upscale  ? upscale(pipeline, a)
           : a.evaluate ? evaluate(pipeline, a)
                        : forward(pipeline, a);
    }
    return rc;
  } catch (const std::exception& e) {
    std::cout << "[ERROR] " << e.what() << std::endl;
    return 1;
  }
}
