// wide_plan.hpp -- what the wide family decides on the host before a launch:
// the net it serves, the geometry builders shared by the training step and
// the op-level calls, and the step's plan.  Included inside namespace
// srcnn::wide after wide_layout.hpp; host code without any HIP call
// (tests/wide_plan_check.cpp prints and checks every plan on the CPU).

// The one net of the family (BASELINE.json configs[3]).  Kernel templates keep
// their parameters; the host names the net here and nowhere else.
struct WideNet {
  static constexpr int N1 = 128, N2 = 64, F1 = 9, F2 = 5, F3 = 5;
  static constexpr int W1 = F1 * F1 * N1, P1 = W1 + N1;
  static constexpr int W2 = F2 * F2 * N1 * N2, P2 = W2 + N2;
  static constexpr int W3 = F3 * F3 * N2, P3 = W3 + 1;
  static constexpr int MT2 = 7;   // L2 forward: up to 2 x 7 x 32 = 448 output pixels
  static constexpr int MT4 = 10;  // delta1: up to 640 pixels
};

static size_t align_f(size_t n) { return (n + 63) & ~(size_t)63; }

// L2 forward over in_w x in_h images: the whole image as one window where the
// register tiles and the chunk image hold it (the step takes only that:
// wo == 0), else 21x21 output windows (441 pixels of the 448 the register
// tiles hold; 25x25 = 625 staged pixels)
inline CGeom conv_fwd_geom(int in_w, int in_h, int batch) {
  constexpr int F = WideNet::F2;
  const int ow = in_w - F + 1, oh = in_h - F + 1;
  CGeom c{in_w, in_h, 0, in_w, in_h, ow, oh, ow * oh, batch, 0, 0, 0};
  if ((c.npx + 31) / 32 > 2 * WideNet::MT2 || c.img_w * c.img_h > kImgMax) {
    c.wo = 21;
    c.img_w = std::min(ow, c.wo) + F - 1;
    c.img_h = std::min(oh, c.wo) + F - 1;
  }
  return c;
}

// delta1 over out_w x out_h (layer-1) images from delta2 zero-padded by F - 1:
// the whole image, else 25x25 output windows (625 of the 640 pixels the
// register tiles hold; 29x29 = 841 staged pixels).  xw, xh (the X tile of the
// step's fused gW1) stay 0: the step sets them.
inline CGeom conv_delta_geom(int out_w, int out_h, int batch) {
  constexpr int F = WideNet::F2;
  const int nw = out_w - F + 1, nh = out_h - F + 1;
  CGeom c{nw, nh, F - 1, nw + 2 * (F - 1), nh + 2 * (F - 1), out_w, out_h, out_w * out_h, batch, 0, 0, 0};
  if ((c.npx + 31) / 32 > 2 * WideNet::MT4 || c.img_w * c.img_h > kImgMax) {
    c.wo = 25;
    c.img_w = std::min(out_w, c.wo) + F - 1;
    c.img_h = std::min(out_h, c.wo) + F - 1;
  }
  return c;
}

// wgrad2's bands over w2 x h2 outputs: full-width bands where a few whole
// rows fit the band images (true; the step takes only these), else
// 16-column x 4-row windows (A1 image 20 x 8 = 160 pixels; false)
inline bool g2_geom(int w2, int h2, uint32_t batch, G2Geom* g2) {
  constexpr int F = WideNet::F2;
  g2->w2 = w2;
  g2->h2 = h2;
  g2->w1 = w2 + F - 1;
  g2->h1 = h2 + F - 1;
  g2->cols = w2;
  g2->rows = std::min(8, kBandPx / std::max(1, w2));
  const bool full = g2->rows >= 1 && (g2->rows + F - 1) * g2->w1 <= kGAPx;
  if (!full) {
    g2->cols = 16;
    g2->rows = kBandPx / 16;
  }
  g2->nbx = (w2 + g2->cols - 1) / g2->cols;
  g2->aw = g2->cols + F - 1;
  g2->nbands = g2->nbx * ((h2 + g2->rows - 1) / g2->rows);
  g2->batch = (int)batch;
  g2->groups = (int)std::min<uint32_t>(batch, 64);
  return full;
}

// Everything the step decides before its first launch.  plan_step fills it
// from the shape and the arithmetic alone: no buffer, no HIP call.
struct WidePlan {
  WGeom g;
  CGeom cf, cd;  // L2 forward, delta1
  G2Geom g2;     // wgrad2 bands; groups = the launched kernel's sample groups
  // split-bf16 kernels: x6 wl2x6 (L2 forward), x6d wd1x6 (delta1 into D1,
  // then gW1 apart), x6f wl1x6 (L1 forward), x6g1 wg1x6 (gW1 after wd1x6, else
  // l1_grad_kernel), x6g wgrad2x6.  wl3l: layer 3 with the A2 image in LDS.
  bool x6, x6d, x6f, x6g1, x6g, wl3l;
  int qfloats;                                 // wl3's Q image
  RunGeom rg1;                                 // layer 1's runs (wl1x6, wg1x6)
  int GL1, GL2, G3, GD, GW1, GG1, GG2, nslab1;  // grids: L1, L2, layer 3, delta1, l1_grad, wg1x6, grad2; gW1 slabs
  size_t lds1, lds2, lds3, ldsd, ldsg1, ldsg2;  // dynamic LDS bytes of the launched variants
  // workspace in floats: Wf | Wd | Wx (split W2 image, wl2x6) | Wx1 (split flipped W2, wd1x6) | slab1 | slab2 | slab3 | sqs
  size_t nWf, nWd, nWx, n1, n2, n3, nsq, bytes;
};

static bool plan_step(uint32_t w, uint32_t h, uint32_t batch, int arith, WidePlan* out) {
  using NetT = WideNet;
  constexpr int N1 = NetT::N1, N2 = NetT::N2, F1 = NetT::F1, F2 = NetT::F2, F3 = NetT::F3;
  WidePlan& p = *out = {};
  WGeom& g = p.g;
  g.w = (int)w;
  g.h = (int)h;
  g.w1 = g.w - F1 + 1;
  g.h1 = g.h - F1 + 1;
  g.w2 = g.w1 - F2 + 1;
  g.h2 = g.h1 - F2 + 1;
  g.w3 = g.w2 - F3 + 1;
  g.h3 = g.h2 - F3 + 1;
  g.batch = (int)batch;
  if (g.w > kXS || g.h > kXS || g.w3 <= 0 || g.h3 <= 0) return false;
  const int npx2 = g.w2 * g.h2;
  // L2 forward / delta1 geometry limits (register tiles, LDS images): every
  // sample is one window
  const CGeom cf = p.cf = conv_fwd_geom(g.w1, g.h1, g.batch);
  p.cd = conv_delta_geom(g.w1, g.h1, g.batch);
  p.cd.xw = g.w;
  p.cd.xh = g.h;
  const CGeom cd = p.cd;
  if (cf.wo || cd.wo) return false;
  // wgrad2 bands, full-width
  G2Geom& g2 = p.g2;
  if (!g2_geom(g.w2, g.h2, batch, &g2)) return false;
  // the split-bf16 wgrad2 (wgrad2x6) takes fewer sample groups (one block per
  // CU); slab2 is sized for wgrad2's, so it holds either arithmetic's
  const int groups2 = g2.groups;
  p.x6g = arith == 0 && F2 == 5 && N2 == 64 && N1 % 16 == 0 && g.w2 <= kG6MaxW2;
  if (p.x6g) g2.groups = (int)std::min<uint32_t>(batch, kG6Groups);
  p.GG2 = p.x6g ? g2.groups * (N1 / 16) : groups2 * (N1 / 32);
  p.ldsg2 = p.x6g ? kG6Lds : kG2Lds;
  // layer 3: wl3l where its A2 image fits the LDS beside Q and the delta3
  // grid (the reduction reuses the A2 image), else wl3
  p.qfloats = Wl3Lds::q_floats(g, F3);
  const size_t lds3 = Wl3Lds(g, F3, p.qfloats).bytes;
  if (lds3 > 64 * 1024) return false;
  const size_t lds3l = Wl3lLds(g, N2, F3).bytes;
  p.wl3l = lds3l + Wl3lLds::kStatic <= (size_t)kLdsMax && npx2 * N2 >= 2 * 16 * 64 * 8 && g.w3 * g.h3 <= 512;
  p.lds3 = p.wl3l ? lds3l : lds3;
  p.G3 = (int)std::min<uint32_t>(batch, p.wl3l ? 256 : 512);  // all blocks resident
  // L1 forward: split-bf16 wl1x6, else wl1_fwd
  p.rg1 = run_geom(g.w1, g.h1);
  p.x6f = arith == 0 && wl1x6_fits(g.w, g.h, N1, F1);
  p.GL1 = (int)std::min<uint32_t>(batch, 1024);
  p.lds1 = p.x6f ? W1x6Lds(g.w, g.h, p.rg1).bytes : 0;
  // L2 forward: split-bf16 wl2x6 (two split chunk images in LDS), else conv_mfma
  const size_t lds6 = SplitImgLds(cf, 2).bytes;
  p.x6 = arith == 0 && N2 == 64 && N1 % 16 == 0 && cf.img_w * cf.img_h <= kW6ImgMax && lds6 <= (size_t)kLdsMax;
  p.GL2 = std::min(p.x6 ? g.batch : g.batch * (N2 / 64), 256);
  p.lds2 = p.x6 ? lds6 : DmaImgLds(cf).bytes;
  // delta1: split-bf16 wd1x6 into D1, then gW1 by wg1x6 (two blocks per CU)
  // or l1_grad_kernel (4 per CU) over their own slabs; else d1g16 does both
  const size_t lds_d6 = SplitImgLds(cd, 1).bytes;
  p.x6d = arith == 0 && N1 % 64 == 0 && N2 % 16 == 0 && cd.img_w * cd.img_h <= kWD6ImgMax && lds_d6 <= (size_t)kLdsMax;
  p.x6g1 = arith == 0 && wg1x6_fits(g.w, g.h, N1, F1);
  constexpr int NPD = N1 / 64;                // delta1 items per sample (64-channel parts)
  p.GD = std::min(g.batch * NPD, 256);        // a multiple of NPD: block parity = part
  const int G1 = p.GD / NPD;                  // d1g16's gW1 slabs: one per block pair
  p.GW1 = (int)std::min<uint32_t>(batch, 1024);
  p.GG1 = (int)std::min<uint32_t>(batch, 512);
  p.nslab1 = p.x6d ? (p.x6g1 ? p.GG1 : p.GW1) : G1;
  p.ldsd = p.x6d ? lds_d6 : D16Lds(cd).bytes;
  p.ldsg1 = p.x6d && p.x6g1 ? G1x6Lds(g.w, g.h, p.rg1).bytes : 0;
  p.nWf = p.nWd = align_f(NetT::W2);
  p.nWx = align_f((size_t)NetT::W2 * 3 / 2);
  p.n1 = align_f((size_t)std::max(G1, p.GW1) * NetT::P1);
  p.n2 = align_f((size_t)groups2 * NetT::P2);
  p.n3 = align_f((size_t)p.G3 * NetT::P3);
  p.nsq = align_f(p.G3);
  p.bytes = (p.nWf + p.nWd + 2 * p.nWx + p.n1 + p.n2 + p.n3 + p.nsq) * sizeof(float);
  return true;
}
