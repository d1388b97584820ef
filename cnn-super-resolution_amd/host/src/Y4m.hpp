// YUV4MPEG2 (Y4M) streams for `cnn upscale`: planar Y'CbCr video, one text
// header line and one "FRAME" line in front of every frame's Y, U and V
// planes.  A sample is one byte, or, in the formats with 9 to 16 bits, a
// little-endian 16-bit word with the value in its low bits.
//
// Read: header tokens W, H, F, I, A, C and X...; chroma C420jpeg, C420mpeg2,
// C420paldv, C420 (4:2:0), C422 and C444 at 8 bits, C420pN, C422pN and C444pN
// with N = 9, 10, 12, 14 or 16 above, C420jpeg when there is no C token;
// progressive only (Ip or I?); interlaced streams, Cmono and every other
// format are rejected with a message.  The luma range comes from an
// XCOLORRANGE=FULL|LIMITED token and is limited without one.  FRAME lines may
// carry parameters, which are skipped.
// The reader takes untrusted input: a header or FRAME line is at most 4096
// bytes, the dimensions pass image::check_dims, and a frame shorter than its
// planes is an IOException, not a short read.
// Write: the header repeats F, I, A, C and XCOLORRANGE.
#ifndef SRCNN_HOST_Y4M_HPP
#define SRCNN_HOST_Y4M_HPP

#include <cstddef>
#include <cstdint>
#include <istream>
#include <ostream>
#include <string>

namespace srcnn {
namespace y4m {

constexpr size_t kMaxLine = 4096;  // header and FRAME lines, the newline included

struct Header {
  uint32_t w = 0, h = 0;
  uint32_t cx = 2, cy = 2;         // chroma subsampling: 2x2, 2x1 or 1x1
  uint32_t bits = 8;               // per sample: 8, or 9..16 in two bytes
  std::string chroma = "420jpeg";  // the C token's value
  bool has_chroma = false;         // the input had a C token
  std::string rate, interlace, aspect;  // the F, I and A tokens' values ("" = absent)
  bool full_range = false;
  bool has_range = false;  // the input had an XCOLORRANGE token

  uint32_t cw() const { return (w + cx - 1) / cx; }
  uint32_t ch() const { return (h + cy - 1) / cy; }
  size_t sample_bytes() const { return bits > 8 ? 2 : 1; }
  size_t luma_bytes() const { return size_t(w) * h * sample_bytes(); }
  size_t chroma_bytes() const { return size_t(cw()) * ch() * sample_bytes(); }  // one plane
  size_t frame_bytes() const { return luma_bytes() + 2 * chroma_bytes(); }
  /** the header of the stream `scale` times as large */
  Header scaled(unsigned scale) const;
  /** the header of the stream resized to W x H: F, I, C and XCOLORRANGE as
   * they are; A as it is when both axes have the same ratio, else the reduced
   * fraction of A * (w * H) / (W * h), so that the picture keeps its shape
   * (0:0, an absent token and anything that is not n:d stay as they are) */
  Header resized(uint32_t W, uint32_t H) const;
};

/** Parse the header line off `in` (throws IOException). */
Header read_header(std::istream& in);

/** The next frame's planes (Y, U, V, tightly packed: frame_bytes()) into
 * `dst`.  False at a clean end of the stream (no byte follows the previous
 * frame); throws IOException for anything else that is not a whole frame. */
bool read_frame(std::istream& in, const Header& hd, unsigned char* dst);

void write_header(std::ostream& out, const Header& hd);
void write_frame(std::ostream& out, const Header& hd, const unsigned char* src);

}  // namespace y4m
}  // namespace srcnn

#endif  // SRCNN_HOST_Y4M_HPP
