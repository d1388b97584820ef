// y4m_fuzz -- deterministic mutation fuzzing of the Y4M reader (Y4m.cpp), for
// a sanitizer build of its own (tests/test_y4m_sanitize.py: g++
// -fsanitize=address,undefined): the data path of `cnn upscale -i VIDEO.y4m`.
// Mutations hit the header's bytes, its fields (W, H, C, I, X tokens replaced
// by boundary values) and the file's length.  Every mutated stream must read
// to its end or throw; a crash, a hang or a sanitizer report is a failure.
//   y4m_fuzz [--iters N] [--seed S] FILE...
// Prints one summary line per seed file: mutations tried / read / rejected.
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <iterator>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "Context.hpp"
#include "Y4m.hpp"

// Context.cpp's srcnn::require (the harness links only the parsers, not the
// device-facing host library)
void srcnn::require(bool cond, const std::string& msg) {
  if (!cond) throw std::runtime_error(msg);
}

namespace {

struct Rng {  // xorshift64*: the same mutations on every run and host
  uint64_t s;
  explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 1) {}
  uint64_t next() {
    s ^= s >> 12;
    s ^= s << 25;
    s ^= s >> 27;
    return s * 0x2545F4914F6CDD1Dull;
  }
  size_t below(size_t n) { return n ? size_t(next() % n) : 0; }
};

typedef std::vector<unsigned char> Bytes;

size_t header_end(const Bytes& m) {
  const auto it = std::find(m.begin(), m.end(), '\n');
  return size_t(it - m.begin());
}

Bytes mutate(const Bytes& f, Rng& r) {
  Bytes m = f;
  if (m.empty()) return m;
  const size_t he = std::max<size_t>(header_end(m), 1);
  switch (r.below(7)) {
    case 0:  // the file's length: cut anywhere
      m.resize(r.below(m.size()));
      break;
    case 1: {  // the file's length: cut at or near a frame boundary, or grow
      const char pat[] = "\nFRAME";
      const auto last = std::find_end(m.begin(), m.end(), pat, pat + 6);
      const size_t k = r.below(3);
      if (k == 0 && last != m.end()) m.resize(size_t(last - m.begin()) + 1);  // whole frames only
      else if (k == 1) m.resize(m.size() - std::min(m.size(), r.below(16)));
      else m.insert(m.end(), r.below(64), uint8_t(r.next()));
      break;
    }
    case 2:  // a few random header bytes
      for (size_t k = 1 + r.below(4); k--;) m[r.below(he)] = uint8_t(r.next());
      break;
    case 3: {  // boundary byte values in the header
      static const uint8_t v[] = {0x00, 0xFF, ' ', '\n', '0', '9', '-', 'W', 'H', 'C', 'I', 'X'};
      m[r.below(he)] = v[r.below(sizeof(v))];
      break;
    }
    case 4: {  // a header field replaced by a boundary value
      static const char* const fields[] = {
          "W0", "W1", "W4294967295", "W4294967296", "W99999999999", "W16777216", "W16777217", "W-1", "W",
          "H0", "H1", "H65536", "H268435456", "H18446744073709551616", "H", "Cmono", "C420p10", "C444p16",
          "C422", "C444", "C420", "C", "It", "Ib", "Im", "I?", "Ip", "XCOLORRANGE=FULL", "XCOLORRANGE=", "X",
          "F0:0", "A", "Q1"};
      std::string h(m.begin(), m.begin() + he);
      std::vector<size_t> starts;
      for (size_t i = 0; i + 1 < h.size(); ++i)
        if (h[i] == ' ') starts.push_back(i + 1);
      const std::string nf = fields[r.below(sizeof(fields) / sizeof(fields[0]))];
      // in place of the field with the same tag, else of any field, else appended
      std::vector<size_t> same;
      for (size_t a : starts)
        if (h[a] == nf[0]) same.push_back(a);
      if (!same.empty() && r.below(4)) starts = same;
      if (starts.empty() || r.below(4) == 0) {
        h += " " + nf;
      } else {
        const size_t a = starts[r.below(starts.size())];
        size_t b = h.find(' ', a);
        if (b == std::string::npos) b = h.size();
        h.replace(a, b - a, nf);
      }
      m.erase(m.begin(), m.begin() + he);
      m.insert(m.begin(), h.begin(), h.end());
      break;
    }
    case 5: {  // duplicate a range of the header (long lines)
      const size_t a = r.below(he), n = 1 + r.below(he - a);
      Bytes seg(m.begin() + a, m.begin() + a + n);
      for (size_t k = 1 + r.below(64); k--;) m.insert(m.begin() + a, seg.begin(), seg.end());
      break;
    }
    default: {  // damage a FRAME line
      const char pat[] = "FRAME";
      auto it = std::search(m.begin() + he, m.end(), pat, pat + 5);
      if (it != m.end()) *(it + r.below(6)) = uint8_t(r.next());
      break;
    }
  }
  return m;
}

// true: read to the end of the stream, false: rejected with an exception
bool run_one(const Bytes& m) {
  try {
    std::istringstream in(std::string(m.begin(), m.end()));
    const srcnn::y4m::Header hd = srcnn::y4m::read_header(in);
    if (hd.w == 0 || hd.h == 0 || hd.cw() == 0 || hd.ch() == 0 || hd.frame_bytes() < hd.luma_bytes()) {
      std::cerr << "header with inconsistent sizes accepted" << std::endl;
      std::abort();
    }
    // a header may promise far more than the file holds: such a frame cannot
    // be whole, and the harness does not allocate for it
    if (hd.frame_bytes() > m.size()) {
      if (in.peek() == std::char_traits<char>::eof()) return true;
      throw std::runtime_error("frame larger than the file");
    }
    Bytes frame(hd.frame_bytes());
    std::ostringstream out;
    srcnn::y4m::write_header(out, hd.scaled(2));
    while (srcnn::y4m::read_frame(in, hd, frame.data())) srcnn::y4m::write_frame(out, hd, frame.data());
    return true;
  } catch (const std::exception&) {
    return false;
  }
}

}  // namespace

int main(int argc, char** argv) {
  long iters = 1200;
  uint64_t seed = 1;
  std::vector<std::string> files;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    if (a == "--iters" && i + 1 < argc) iters = std::stol(argv[++i]);
    else if (a == "--seed" && i + 1 < argc) seed = std::stoull(argv[++i]);
    else files.push_back(a);
  }
  if (files.empty()) {
    std::cerr << "usage: y4m_fuzz [--iters N] [--seed S] FILE..." << std::endl;
    return 2;
  }
  for (size_t fi = 0; fi < files.size(); ++fi) {
    std::ifstream in(files[fi], std::ios::binary);
    if (!in) {
      std::cerr << "cannot read " << files[fi] << std::endl;
      return 2;
    }
    const Bytes f((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    if (!run_one(f)) {
      std::cerr << "seed file does not read: " << files[fi] << std::endl;
      return 3;
    }
    Rng r(seed + 7919 * fi);
    long ok = 0, rejected = 0;
    for (long it = 0; it < iters; ++it) {
      Bytes m = mutate(f, r);
      for (size_t k = r.below(3); k--;) m = mutate(m, r);
      (run_one(m) ? ok : rejected)++;
    }
    std::cout << files[fi] << " y4m mutations=" << iters << " read=" << ok << " rejected=" << rejected << std::endl;
  }
  return 0;
}
