// y4m_tool -- test driver of the Y4M reader and writer (no device needed):
//   y4m_tool IN OUT          read the YUV4MPEG2 stream IN and write it as OUT
// Prints "<w> <h> <cx> <cy> <full|limited> <frames>", and the bits per sample
// as a seventh field where they exceed 8.  Exit status 1 and the
// IOException message on unsupported / corrupt input; the frames in front of a
// truncated one are written.
#include <fstream>
#include <iostream>
#include <vector>

#include "Context.hpp"
#include "Y4m.hpp"

int main(int argc, char** argv) {
  if (argc != 3) {
    std::cerr << "usage: y4m_tool IN OUT" << std::endl;
    return 2;
  }
  size_t frames = 0;
  try {
    std::ifstream in(argv[1], std::ios::binary);
    if (!in) throw srcnn::IOException(std::string("cannot open '") + argv[1] + "'");
    const srcnn::y4m::Header hd = srcnn::y4m::read_header(in);
    std::ofstream out(argv[2], std::ios::binary);
    srcnn::y4m::write_header(out, hd);
    std::vector<unsigned char> frame(hd.frame_bytes());
    int rc = 0;
    try {
      while (srcnn::y4m::read_frame(in, hd, frame.data())) {
        srcnn::y4m::write_frame(out, hd, frame.data());
        ++frames;
      }
    } catch (const std::exception& e) {
      std::cout << "[ERROR] " << e.what() << std::endl;
      rc = 1;
    }
    std::cout << hd.w << " " << hd.h << " " << hd.cx << " " << hd.cy << " " << (hd.full_range ? "full" : "limited")
              << " " << frames;
    if (hd.bits > 8) std::cout << " " << hd.bits;
    std::cout << std::endl;
    return rc;
  } catch (const std::exception& e) {
    std::cout << "[ERROR] " << e.what() << std::endl;
    return 1;
  }
}
