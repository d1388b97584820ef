// wide_layout.hpp -- the geometry structs, limits and LDS layouts of the wide
// family (train_wide.hip), included inside namespace srcnn::wide.
//
// Host-and-device code without any device intrinsic (as runs.hpp): the plan
// (wide_plan.hpp) takes every dynamic-LDS byte count from the layout struct
// whose offsets the kernel carves its regions by, constructed from the
// kernel's own arguments, so no LDS byte formula is written twice.
// tests/wide_plan_check.cpp compiles this header and the plan for the host
// with the qualifiers defined away.
#include "runs.hpp"

struct WGeom {
  int w, h;    // X / T tile
  int w1, h1;  // A1 / D1
  int w2, h2;  // A2 / D2
  int w3, h3;  // A3
  int batch;
};

constexpr int kLdsMax = 160 * 1024;  // LDS bytes of a CU

// ---- layer 1 (wl1.hpp, wl1x6.hpp, wg1x6.hpp) -------------------------------
constexpr int kXS = 40;                // LDS row stride of an X tile (w, h <= kXS)
constexpr int kXTile = kXS * (kXS + 1);  // + one zero row read by the padded tap

constexpr int kW1x6Regs = 6;  // X tile values per thread (w * h <= 1536)

struct W1x6Lds {
  int rs3, xs, rb, px, bytes;  // pair-image row stride (dwords); byte offsets
  __host__ __device__ W1x6Lds(int w, int h, const RunGeom& rg) {
    const int a4 = (4 * rg.a) % 32;
    rs3 = 3 * w + ((a4 - 3 * w) % 32 + 32) % 32;
    xs = ((rs3 * h + 1) * 4 + 15) & ~15;  // fp32 tile (tap 80, k-step 4)
    rb = (xs + w * h * 4 + 15) & ~15;     // slot -> pair-image row base iy rs3 + ix, and iy w + ix
    px = rb + rg.nch * 32 * 2 * 4;        // [chunk][half][register] -> output pixel (-1: dummy)
    bytes = px + rg.nch * 32 * 4;
  }
};

inline bool wl1x6_fits(int w, int h, int n1, int f1) {
  if (n1 != 128 || f1 != 9 || w * h > 256 * kW1x6Regs) return false;
  const RunGeom rg = run_geom(w - 8, h - 8);
  return W1x6Lds(w, h, rg).bytes <= 36 * 1024;
}

struct G1x6Lds {
  int st, tcols, rs, rdw, tdw, xbuf, offs, runs, cst, bytes;  // (as fused::D6Lds)
  __host__ __device__ G1x6Lds(int w, int h, const RunGeom& rg) {
    st = 4 * rg.cr + 9;
    if (st < h + 1) st = h + 1;
    tcols = rg.b ? rg.b + 8 : 0;
    rs = w + ((9 - w) % 64 + 64) % 64;
    rdw = 3 * (rs * h + 1);
    tdw = 3 * tcols * st;
    xbuf = rdw + tdw;
    offs = (2 * xbuf * 4 + 15) & ~15;   // [chunk][half][16]: byte offsets of the lane half's slots' rows
    runs = offs + rg.nch * 32 * 4;
    cst = runs + rg.nch * 8 * 4;
    bytes = cst + 32 * 4;
  }
};

inline bool wg1x6_fits(int w, int h, int n1, int f1) {
  if (n1 != 128 || f1 != 9 || w * h > 256 * kW1x6Regs || w > 57) return false;
  const RunGeom rg = run_geom(w - 8, h - 8);
  return G1x6Lds(w, h, rg).bytes <= 80 * 1024;
}

// ---- the conv geometry of the L2 forward and of delta1 ---------------------
struct CGeom {
  int in_w, in_h, pad;    // unpadded input, zero border
  int img_w, img_h;       // largest staged image (window output + F - 1 per side)
  int out_w, out_h, npx;  // output
  int batch;
  int xw, xh;             // delta1 + gW1: the X tile (layer-1 input)
  int wo;                 // > 0: windows of wo x wo outputs (op-level calls on large
                          // images); 0: the whole image is one window
};

__host__ __device__ inline int conv_windows(const CGeom& g) {
  return g.wo == 0 ? 1 : ((g.out_w + g.wo - 1) / g.wo) * ((g.out_h + g.wo - 1) / g.wo);
}

// ---- the DMA chunk image (wconv_mfma.hpp, wd1g16.hpp) ----------------------
constexpr int kCC = 16;       // input channels per LDS chunk
constexpr int kPS = kCC + 4;  // LDS floats per staged pixel (80 B rows)

constexpr int kImgMax = 960;                  // pixels of one chunk image (<= 31 x 31)
constexpr int kImgSlack = 256;                // floats: one DMA instruction past the image

// two buffers (the chunk consumed, the chunk staged) of the largest window's
// image, img_w x img_h pixels of kPS floats
struct DmaImgLds {
  int buf_floats, bytes;  // one buffer; both
  __host__ __device__ DmaImgLds(const CGeom& g) {
    buf_floats = g.img_w * g.img_h * kPS + kImgSlack;
    bytes = 2 * buf_floats * 4;
  }
};

constexpr int kXBuf = kXTile + 64;  // X tile buffer of the fused gW1 epilogue (d1g16)

constexpr int kD16MT = 20;                   // 16-pixel tiles per wave group
constexpr int kD16Slots = 2 * kD16MT * 16;  // pixel slots of the tile table

// d1g16: the two chunk images, then a tail of fixed size: 2 X tile buffers
// (item parity) | one int table: slot -> pixel | each 16-slot tile's tap mask |
// the tile order
struct D16Lds {
  static constexpr int kTab = 2 * kXBuf;  // the table's float offset in the tail
  // int offsets in the table
  static constexpr int kTabMask = kD16Slots, kTabPerm = kTabMask + 2 * kD16MT, kTabInts = kTabPerm + 2 * kD16MT;
  int buf_floats, tail, bytes;  // one chunk image; float offset of the tail
  __host__ __device__ D16Lds(const CGeom& g) {
    buf_floats = DmaImgLds(g).buf_floats;
    tail = 2 * buf_floats;
    bytes = (tail + kTab + kTabInts) * 4;
  }
};

// ---- the split chunk image (wl2x6.hpp) -------------------------------------
constexpr int kW6Row = 28;  // dwords per staged pixel: 3 parts x 16 bf16 + 16 B pad
// pixels of one chunk image: two images in the 160 KiB LDS
constexpr int kW6ImgMax = kLdsMax / (2 * kW6Row * 4);
// Image row pitch (dwords).  Lane j of an M tile reads output pixel 32 T + j,
// i.e. image pixel (oy, ox) at quad 7 ox + (pitch / 4) oy; its 16-lane
// ds_read_b128 groups hit 16 distinct quads mod 16 when that quad index is
// 7 (oy out_w + ox) mod 16 -- consecutive outputs, 7 odd -- also across the
// output-row wrap inside a tile.  So pitch / 4 = 7 out_w (mod 16): img_w
// pixels plus (7 (out_w - img_w)) mod 16 pad quads per row (4 for f = 5).
// At pitch = img_w pixels every wrapping tile read was conflicted: 56% / 49%
// of wl2x6 / wd1x6's LDS cycles were bank conflicts (profiles/pmc_r06.json).
__host__ __device__ inline int w6_pitch(int img_w, int out_w) {
  return kW6Row * img_w + 4 * (((7 * (out_w - img_w)) % 16 + 16) % 16);
}
constexpr int kWD6ImgMax = 900;  // staged pixels (30 x 30; one 100.8 KB image)

// nimg images of img_h rows of `pitch` dwords: wl2x6 keeps two (the chunk
// consumed, the chunk staged), wd1x6 one
struct SplitImgLds {
  int pitch, img, bytes;  // dwords per row, per image; all images
  __host__ __device__ SplitImgLds(const CGeom& g, int nimg) {
    pitch = w6_pitch(g.img_w, g.out_w);
    img = g.img_h * pitch;
    bytes = nimg * img * 4;
  }
};

// ---- layer 3 (wl3.hpp) -----------------------------------------------------
// wl3: Q [npx2][F3 F3] (later the cross-wave reduction of 4 waves x 2 tiles x
// 16 registers x 64 lanes) | the zero-bordered delta3 grid | the relu' mask
// bits of A2, two words per pixel
struct Wl3Lds {
  int gd, mbits, bytes;  // float offsets (Q at 0)
  __host__ __device__ static int q_floats(const WGeom& g, int f3) {
    const int q = g.w2 * g.h2 * f3 * f3, red = 2 * 16 * 64 * 4;
    return q > red ? q : red;
  }
  __host__ __device__ Wl3Lds(const WGeom& g, int f3, int qfloats) {
    gd = qfloats;
    mbits = gd + (g.w3 + 2 * (f3 - 1)) * (g.h3 + 2 * (f3 - 1));
    bytes = (mbits + 2 * g.w2 * g.h2) * 4;
  }
};
// wl3l: the A2 image [npx2][n2] (later the reduction of 8 waves) | Q | the
// delta3 grid; the kernel's static red_s[2][8] shares the CU's LDS with it
struct Wl3lLds {
  static constexpr int kStatic = 2 * 8 * 4;  // bytes
  int q, gd, bytes;                          // float offsets (A2 at 0)
  __host__ __device__ Wl3lLds(const WGeom& g, int n2, int f3) {
    q = g.w2 * g.h2 * n2;
    gd = q + g.w2 * g.h2 * f3 * f3;
    bytes = (gd + (g.w3 + 2 * (f3 - 1)) * (g.h3 + 2 * (f3 - 1))) * 4;
  }
};

// ---- gW2 / gB2 (wgrad2.hpp, wgrad2x6.hpp) ----------------------------------
constexpr int kGAS = 48;      // LDS floats per A1 pixel (32 channels + pad)
constexpr int kGDS = 80;      // LDS floats per delta2 pixel (64 channels + pad)
constexpr int kBandPx = 64;   // output pixels per band (16 quads)
constexpr int kGAPx = 192;    // A1 pixels per band image (max)
constexpr int kGAFl = kGAPx * kGAS;
constexpr int kGBuf = kGAFl + (kBandPx + 4) * kGDS + 256;
constexpr size_t kG2Lds = 2 * (size_t)kGBuf * sizeof(float);  // two band buffers

struct G2Geom {
  int w1, h1, w2, h2;
  int rows, nbands;  // output rows per band, bands per sample (nbx * band rows)
  int batch, groups;
  int cols, nbx;     // output columns per band (w2: full rows), bands per band row
  int aw;            // A1 band image width cols + F - 1 (a kernel argument, so the
                     // tap offsets stay scalar: 4 adds per k-step, not 7)
};

constexpr int kG6RowP = 48;                              // dwords per ring row (pair image)
constexpr int kG6Ring = 8;                               // ring rows: a band of 4 + F - 1
constexpr int kG6QP = kG6Ring * kG6RowP;                 // dwords per (channel, part)
constexpr int kG6CP = 3 * kG6QP + 1;                     // dwords per channel (= 1 mod 64)
constexpr int kG6A = 16 * kG6CP;                         // A ring dwords
constexpr int kG6NP = 12;                                // dwords per delta2 (part, row, n): 24 px
constexpr int kG6D = 3 * 4 * 64 * kG6NP;                 // delta2 image dwords
constexpr size_t kG6Lds = (size_t)(kG6A + kG6D) * 4;     // 110.7 KB: one block per CU
constexpr int kG6MaxW2 = 24, kG6Groups = 32;
