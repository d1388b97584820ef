// y4m_resize_tool -- test driver of srcnn::y4m::Header::resized (no device
// needed):
//   y4m_resize_tool IN W H   read the header of the YUV4MPEG2 stream IN and
//                            print the header line of the stream resized to
//                            W x H, as write_header writes it
// Exit status 1 and the IOException message on unsupported / corrupt input.
#include <cstdlib>
#include <fstream>
#include <iostream>

#include "Context.hpp"
#include "Y4m.hpp"

int main(int argc, char** argv) {
  if (argc != 4) {
    std::cerr << "usage: y4m_resize_tool IN W H" << std::endl;
    return 2;
  }
  try {
    std::ifstream in(argv[1], std::ios::binary);
    if (!in) throw srcnn::IOException(std::string("cannot open '") + argv[1] + "'");
    const srcnn::y4m::Header hd = srcnn::y4m::read_header(in);
    srcnn::y4m::write_header(std::cout, hd.resized(uint32_t(std::strtoul(argv[2], nullptr, 10)),
                                                   uint32_t(std::strtoul(argv[3], nullptr, 10))));
    return 0;
  } catch (const std::exception& e) {
    std::cout << "[ERROR] " << e.what() << std::endl;
    return 1;
  }
}
