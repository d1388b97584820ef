// fwd_plan.hpp -- what the fused forward decides on the host before a launch:
// the nets it serves and the forward's plan.  Included inside namespace
// srcnn::fused after fwd_layout.hpp; includes net.hpp (Net, first_net) itself.
// Host code without any HIP call or type (tests/fwd_plan_check.cpp prints and
// checks every plan on the CPU).
#include "net.hpp"

// The instantiated nets (net.hpp), once.
template <typename F>
static int with_fwd_net(const srcnn_net* net, F&& f) {
  return first_net(net, f, Net<64, 32, 9, 5>{},  // reference default
                   Net<32, 16, 9, 5>{});         // example_config.json
}

// Everything the forward decides before its first launch.  plan_forward
// fills it from the shape and the arithmetic alone: no buffer, no HIP call.
struct FwdPlan {
  bool x6;  // the default net in split-bf16 products (fwd_l123x6), fixed 24-row regions
  FwdGeom g;
  unsigned grid;      // fwd_l123 / fwd_l123x6 blocks
  size_t lds;         // and their dynamic LDS bytes
  size_t part_bytes;  // the workspace: the regions' partial sums
  int seam_bx, seam_rb;  // fwd_seam: threads per block, rows per block
  unsigned seam_gx, seam_gy, seam_gz;  // and its grid (column blocks, row blocks, frames)
};

template <typename NetT>
bool plan_forward(uint32_t w, uint32_t h, uint32_t batch, int arith, FwdPlan* out) {
  constexpr int F1 = NetT::F1, F3 = NetT::F3;
  FwdPlan& p = *out = {};
  const int ow = (int)w - F1 + 1, oh = (int)h - F1 + 1;
  if (ow < F3 || oh < F3) return false;
  p.x6 = NetT::kDefault && arith == 0;
  // region rows (fwd_layout.hpp)
  constexpr int rh_f32 = fwd_rh_f32(F1), rh_x6 = fwd_rh_x6();
  int rh = p.x6 ? rh_x6 : rh_f32;
  if (rh < F3) return false;
  rh = std::min(rh, oh);
  const FwdGeom g = p.g = {(int)w, (int)h, ow, oh, rh, (ow + kFwdRW - 1) / kFwdRW, (oh + rh - 1) / rh, (int)batch};
  const long items = (long)g.batch * g.nrx * g.nry;
  p.grid = (unsigned)std::min<long>(items, p.x6 ? 256 : kFwdGrid);
  p.lds = p.x6 ? F6Lds::bytes : 0;
  // partial sums of either arithmetic's regions (srcnn_set_arith between the
  // size query and the call needs no new query)
  auto part_bytes = [&](int r) {
    return (size_t)g.batch * g.nrx * ((oh + r - 1) / r) * (r + F3 - 1) * (kFwdRW + F3 - 1) * sizeof(float);
  };
  p.part_bytes = part_bytes(rh);
  if (NetT::kDefault)
    p.part_bytes = std::max({p.part_bytes, part_bytes(std::min(rh_f32, oh)), part_bytes(std::min(rh_x6, oh))});
  const int w3 = ow - F3 + 1, h3 = oh - F3 + 1;
  p.seam_bx = std::min(256, (w3 + 63) / 64 * 64);
  // up to 8 rows per block while the grid keeps >= 4096 blocks (4K frame:
  // 7 rows, 0.0307 -> 0.0267 ms; small frames: 1 row per block)
  const int nbx = (w3 + p.seam_bx - 1) / p.seam_bx;
  p.seam_rb = (int)std::max<long>(1, std::min<long>(8, (long)nbx * h3 * batch / 4096));
  p.seam_gx = (unsigned)nbx;
  p.seam_gy = (unsigned)std::min((h3 + p.seam_rb - 1) / p.seam_rb, 65535);
  p.seam_gz = (unsigned)std::min<uint32_t>(batch, 65535);
  return true;
}
