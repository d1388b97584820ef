#include "Y4m.hpp"

#include <cstring>

#include "Image.hpp"

namespace srcnn {
namespace y4m {
namespace {

const char kMagic[] = "YUV4MPEG2";

/** One line without its newline; false if the stream ends before any byte.
 * Throws if the line has no newline within kMaxLine bytes. */
bool read_line(std::istream& in, std::string& line, const char* what) {
  line.clear();
  for (size_t n = 0; n < kMaxLine; ++n) {
    const int c = in.get();
    if (c == std::char_traits<char>::eof()) {
      if (n == 0) return false;
      throw IOException(std::string("truncated Y4M ") + what);
    }
    if (c == '\n') return true;
    line.push_back(char(c));
  }
  throw IOException(std::string("Y4M ") + what + " longer than " + std::to_string(kMaxLine) + " bytes");
}

uint64_t parse_dim(const std::string& v, char tag) {
  if (v.empty() || v.size() > 10) throw IOException(std::string("invalid Y4M ") + tag + " token");
  uint64_t n = 0;
  for (char c : v) {
    if (c < '0' || c > '9') throw IOException(std::string("invalid Y4M ") + tag + " token");
    n = n * 10 + uint64_t(c - '0');
  }
  return n;
}

/** The depth of "420p10", "422p12", ...: the subsampling, then 'p', then one of
 * 9, 10, 12, 14 and 16; 0 for anything else. */
uint32_t deep_bits(const std::string& v) {
  if (v.size() < 5 || v.size() > 6 || v[3] != 'p') return 0;
  const std::string n = v.substr(4);
  for (const char* ok : {"9", "10", "12", "14", "16"})
    if (n == ok) return uint32_t(std::stoi(n));
  return 0;
}

void set_chroma(Header& hd, const std::string& v) {
  const std::string sub = v.substr(0, 3);
  const uint32_t deep = deep_bits(v);
  if (v == "420jpeg" || v == "420mpeg2" || v == "420paldv" || v == "420" || (deep && sub == "420")) {
    hd.cx = 2;
    hd.cy = 2;
  } else if (v == "422" || (deep && sub == "422")) {
    hd.cx = 2;
    hd.cy = 1;
  } else if (v == "444" || (deep && sub == "444")) {
    hd.cx = 1;
    hd.cy = 1;
  } else if (v == "mono") {
    throw IOException("unsupported Y4M chroma 'Cmono': no chroma planes");
  } else if (v.find('p') != std::string::npos && v.find("pal") == std::string::npos) {
    throw IOException("unsupported Y4M chroma 'C" + v + "': the depths above 8 bits are p9, p10, p12, p14 and p16");
  } else {
    throw IOException("unsupported Y4M chroma 'C" + v + "'");
  }
  hd.bits = deep ? deep : 8;
  hd.chroma = v;
  hd.has_chroma = true;
}

}  // namespace

Header Header::scaled(unsigned scale) const {
  Header o = *this;
  o.w = w * scale;
  o.h = h * scale;
  return o;
}

Header Header::resized(uint32_t W, uint32_t H) const {
  Header o = *this;
  o.w = W;
  o.h = H;
  // the picture keeps its shape: pixel aspect A * (w * H) / (W * h), reduced
  const uint64_t up = uint64_t(w) * H, down = uint64_t(W) * h;
  if (aspect.empty() || up == down || up == 0 || down == 0) return o;
  const size_t colon = aspect.find(':');
  if (colon == std::string::npos) return o;
  uint64_t n = 0, d = 0;
  try {
    n = parse_dim(aspect.substr(0, colon), 'A');
    d = parse_dim(aspect.substr(colon + 1), 'A');
  } catch (const IOException&) {
    return o;  // (not a fraction of integers: left as it is)
  }
  if (n == 0 || d == 0) return o;  // 0:0 is "unknown"
  auto gcd = [](unsigned __int128 a, unsigned __int128 b) {
    while (b) {
      const unsigned __int128 t = a % b;
      a = b;
      b = t;
    }
    return a;
  };
  unsigned __int128 num = (unsigned __int128)n * up, den = (unsigned __int128)d * down;
  const unsigned __int128 g = gcd(num, den);
  num /= g;
  den /= g;
  if (num > 0xffffffffffffffffull || den > 0xffffffffffffffffull) return o;
  o.aspect = std::to_string(uint64_t(num)) + ":" + std::to_string(uint64_t(den));
  return o;
}

Header read_header(std::istream& in) {
  std::string line;
  if (!read_line(in, line, "header")) throw IOException("empty Y4M stream");
  const size_t ml = sizeof(kMagic) - 1;
  if (line.compare(0, ml, kMagic) != 0 || (line.size() > ml && line[ml] != ' '))
    throw IOException("not a YUV4MPEG2 stream");
  Header hd;
  bool has_w = false, has_h = false;
  size_t pos = ml;
  while (pos < line.size()) {
    if (line[pos] == ' ') {
      ++pos;
      continue;
    }
    size_t end = line.find(' ', pos);
    if (end == std::string::npos) end = line.size();
    const char tag = line[pos];
    const std::string v = line.substr(pos + 1, end - pos - 1);
    pos = end;
    switch (tag) {
      case 'W':
        hd.w = 0;
        has_w = true;
        {
          const uint64_t n = parse_dim(v, 'W');
          image::check_dims(n, 1, 1);
          hd.w = uint32_t(n);
        }
        break;
      case 'H':
        has_h = true;
        {
          const uint64_t n = parse_dim(v, 'H');
          image::check_dims(1, n, 1);
          hd.h = uint32_t(n);
        }
        break;
      case 'F': hd.rate = v; break;
      case 'A': hd.aspect = v; break;
      case 'I':
        if (v != "p" && v != "?") throw IOException("unsupported Y4M interlacing 'I" + v + "': progressive only");
        hd.interlace = v;
        break;
      case 'C': set_chroma(hd, v); break;
      case 'X':
        if (v == "COLORRANGE=FULL" || v == "COLORRANGE=LIMITED") {
          hd.full_range = v == "COLORRANGE=FULL";
          hd.has_range = true;
        }
        break;
      default: throw IOException(std::string("unknown Y4M header token '") + tag + "'");
    }
  }
  if (!has_w || !has_h) throw IOException("Y4M header without W or H");
  image::check_dims(hd.w, hd.h, 1);
  return hd;
}

bool read_frame(std::istream& in, const Header& hd, unsigned char* dst) {
  std::string line;
  if (!read_line(in, line, "FRAME line")) return false;
  if (line.compare(0, 5, "FRAME") != 0 || (line.size() > 5 && line[5] != ' '))
    throw IOException("Y4M: expected a FRAME line");
  const size_t n = hd.frame_bytes();
  in.read(reinterpret_cast<char*>(dst), std::streamsize(n));
  if (size_t(in.gcount()) != n)
    throw IOException("truncated Y4M frame: " + std::to_string(size_t(in.gcount())) + " of " + std::to_string(n) +
                      " bytes");
  return true;
}

void write_header(std::ostream& out, const Header& hd) {
  out << kMagic << " W" << hd.w << " H" << hd.h;
  if (!hd.rate.empty()) out << " F" << hd.rate;
  if (!hd.interlace.empty()) out << " I" << hd.interlace;
  if (!hd.aspect.empty()) out << " A" << hd.aspect;
  if (hd.has_chroma) out << " C" << hd.chroma;
  if (hd.has_range) out << " XCOLORRANGE=" << (hd.full_range ? "FULL" : "LIMITED");
  out << "\n";
  if (!out) throw IOException("cannot write the Y4M header");
}

void write_frame(std::ostream& out, const Header& hd, const unsigned char* src) {
  out << "FRAME\n";
  out.write(reinterpret_cast<const char*>(src), std::streamsize(hd.frame_bytes()));
  if (!out) throw IOException("cannot write a Y4M frame");
}

}  // namespace y4m
}  // namespace srcnn
