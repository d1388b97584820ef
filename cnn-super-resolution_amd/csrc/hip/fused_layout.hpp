// fused_layout.hpp -- the geometry structs, limits and LDS layouts of the
// fused family (train_fused.hip), included inside namespace srcnn::fused.
//
// Host-and-device code without any device intrinsic (as runs.hpp and
// d6tr.hpp, which it includes): the plan (fused_plan.hpp) takes every
// dynamic-LDS byte count and every "does this tile fit" answer from the layout
// struct whose offsets the kernel carves its regions by, constructed from the
// kernel's own arguments, so no LDS byte formula is written twice.
// tests/fused_plan_check.cpp compiles this header and the plan for the host
// with the qualifiers defined away.  Each section names the kernel header
// whose LDS it lays out; the reasons for a layout stand with the layout.
#include "runs.hpp"
#include "d6tr.hpp"

constexpr int kLdsMax = 160 * 1024;   // LDS bytes of a CU
constexpr int kLdsHalf = kLdsMax / 2;  // ... of each of two resident blocks

// ---- the tile (every kernel) ------------------------------------------------
struct Geom {
  int W, H;      // input sample
  int ow, oh;    // L1 (and L2) output
  int batch;
};

constexpr int kXsMax = 1536;  // input sample / region tile (floats) staged in LDS (<= 39x39)
// l12_fwd X tile in LDS: rows at the fixed stride kL12S (w <= kL12S, h <= kL12Rows).
// A chunk's 32 consecutive L1 pixels (flattened over ow) gather from banks
// (row * kL12S + col) mod 32 (ds_read_b32 banks 32 lanes at a time), which
// is (pixel index + const) mod 32 -- 32 distinct banks -- when kL12S == ow
// (mod 32): 57 = 25 + 32 makes the default 33x33 tile (ow 25) conflict-free.
constexpr int kL12S = 57;
constexpr int kL12Rows = 40;
constexpr int kL12Tile = kL12S * (kL12Rows + 1);  // + a zero row read by the padded tap
constexpr int kL12Regs = (kXsMax + 255) / 256;    // register-staged X tile (w * h <= kXsMax)
// grid caps (blocks): 256 CUs x 2 resident blocks.  l12 writes the samples
// in index order, which l3 reads back in reverse (MALL)
constexpr int kL12Grid = 512, kL3RGrid = 512;

// ---- layer 3 by l3_delta (l3_delta.hpp) --------------------------------------
struct L3Geom {
  int W, H;     // ground-truth sample (= network input size)
  int w2, h2;   // A2
  int w3, h3;   // A3
  int batch;
};

// (768 / 1024 threads per block measured slower: the three barrier-separated
// phases, not occupancy, set the pace)
constexpr int kL3Threads = 512;
constexpr int kL3TPF = (1024 + kL3Threads - 1) / kL3Threads;  // L3 outputs per thread (w3 * h3 <= 1024)
constexpr int kL3MaxOut = kL3TPF * kL3Threads;

// LDS geometry shared by host and device (floats)
template <int N2, int F3>
struct L3Lds {
  // 16-pixel units per wave of the largest A2 tile whose two regions fit the
  // 160 KB LDS (npx2 * max(N2, F3^2) <= 20480 floats)
  static constexpr int kMaxPx = 20480 / (N2 > F3 * F3 ? N2 : F3 * F3);
  static constexpr int kUnitsPerWave = ((kMaxPx + 15) / 16 + kL3Threads / 64 - 1) / (kL3Threads / 64);
  int region;  // one ping-pong region: max(A2 tile, Q of whole units, reduction scratch)
  int d3off;   // delta3 grid offset (F3-1) * (w2 + 1)
  int nd3;     // delta3 grid size (zero tail covers chunk overrun)
  __host__ __device__ L3Lds(int w2, int h2) {
    const int npx2 = w2 * h2, nch = (npx2 + 31) / 32;
    int r = npx2 * N2;
    const int npad = (npx2 + 15) / 16 * 16;  // Q is written for whole 16-pixel units
    if (npad * F3 * F3 > r) r = npad * F3 * F3;
    if (((N2 + 31) / 32) * 1024 > r) r = ((N2 + 31) / 32) * 1024;
    region = (r + 3) & ~3;
    d3off = (F3 - 1) * (w2 + 1);
    nd3 = nch * 32 + d3off + 4;
  }
  __host__ __device__ size_t bytes() const { return (2 * (size_t)region + nd3) * sizeof(float); }
};

template <int N2, int F3>
static size_t l3_lds_bytes(int w2, int h2) {
  return L3Lds<N2, F3>(w2, h2).bytes();
}

// ---- layer 3 by l3r (l3r.hpp) -----------------------------------------------
constexpr int kL3RThreads = 512;
constexpr int kL3RUnits = 5;  // 16-pixel units per wave (8 waves: 640 pixels)
constexpr int kL3RTPF = 1;    // L3 outputs per thread (w3 * h3 <= 512 for every A2 tile of <= 640 pixels)
constexpr int kL3RW3S = 36;   // W3 image row stride (floats): conflict-free 16-B reads
constexpr int kL3RScS = 36;   // transpose scratch row stride (floats) per channel

constexpr int kL3RWdS = 36;   // delta2 W3 image row stride (floats): 4 groups x 8 slots + pad

template <int F3>
struct L3RLds {
  int qreg;   // Q image [640][F3^2] (every unit slot); aliased by the transpose scratch and the final reduction
  int w3img;  // W3 image [tap][kL3RW3S] (Q's B operand)
  int wdimg;  // W3 image [c][h][lg][4] at row stride kL3RWdS (delta2's A operand; slot s = 4h + i)
  int d3off;  // delta3 grid offset (F3-1) * (w2 + 1)
  int nd3;    // delta3 grid size, after a 4-float zero lead (unused slots read below the grid)
  __host__ __device__ L3RLds(int w2, int h2) {
    // every wave runs all kL3RUnits unit slots (no data-dependent branches
    // around the A2 loads: the compiler's wait-count pass would then lose
    // track of them and wait for every load right after issuing it), so the
    // Q image and the delta3 grid cover all 8 * kL3RUnits units
    (void)h2;
    constexpr int npad = 16 * 8 * kL3RUnits;
    int r = npad * F3 * F3;
    if (r < 8 * 32 * kL3RScS) r = 8 * 32 * kL3RScS;
    if (r < 8 * 2 * 2 * 4 * 64) r = 8 * 2 * 2 * 4 * 64;  // the final reduction (8 waves x 16 x 64)
    qreg = (r + 3) & ~3;
    w3img = (F3 * F3 * kL3RW3S + 3) & ~3;
    wdimg = 32 * kL3RWdS;
    d3off = (F3 - 1) * (w2 + 1);
    nd3 = 4 + ((npad + d3off + 4 + 3) & ~3);
  }
  __host__ __device__ size_t bytes() const { return ((size_t)qreg + w3img + wdimg + nd3) * sizeof(float); }
};

// the shapes l3r takes: two blocks per CU, whole units per wave
template <int F3>
static bool l3r_fits(int w2, int h2, int w3, int h3) {
  const int nunit = (w2 * h2 + 15) / 16;
  return nunit <= 8 * kL3RUnits && w3 * h3 <= kL3RThreads * kL3RTPF &&
         L3RLds<F3>(w2, h2).bytes() <= kLdsHalf;
}

// kD3Out also keeps gW3's split delta3 pair images (3 x nd3 dwords) in the Q
// image past the transpose scratches
template <int F3>
static bool l3r_d3_fits(int w2, int h2) {
  const L3RLds<F3> L(w2, h2);
  return 8 * 32 * kL3RScS + 3 * L.nd3 <= L.qreg;
}

// ---- layers 1-2 forward in split products (l12x6.hpp) ----------------------
constexpr int kX6KS = 5;                  // 16-slot k-steps of layer 1
constexpr int kX6W1 = kX6KS * 2 * 3 * 512;  // W1 image in three bf16 parts (X6Lds's rule only)
constexpr int kX6W2 = 4 * 3 * 512;          // W2 image, bf16: [m][part][lane][8]

// per wave: the A2 regroup scratch [32 slots][32 channels] (16-B quads
// XOR-swizzled by slot: quad c of slot p at quad c ^ (p & 7)) and the
// slots' pixels
constexpr int kX6Sc = 32 * 32 + 32;
// The X pair image holds, per image row, the part rows side by side
// (dword y rs + w q + x = the part-q pair (x_{y,x}, x_{y,x+1})).  A
// half-wave's L1 B-operand read covers the 32 slots of a chunk: 8 row runs
// of 4 pixels, a row's ow / 4 runs then the next row's, so with rs3 = 4 (ow /
// 4) (mod 32) its 32 dwords are consecutive modulo 32 -- 32 distinct banks
// (ds_read_b32 banks (a / 4) mod 32 per half-wave).  At the unpadded stride
// (the round-5 part-major layout had rows of w dwords) two rows of a chunk
// shared banks: every such read was 2-way.  The padded stride where it fits
// in the 80 KB of two blocks per CU, else 3 w.  xs: the fp32 tile (tap (8, 8)
// and k-step 4), row stride w.
// X6Lds is that layout on the three-part (bf16) sizes the kernel had through
// round 11: kept as the rule by which a tile takes l12x6 (l12x6_fits) and the
// padded stride, so the dispatch stays what it was.
struct X6Lds {
  int rs3, r, xs, a2sc, bytes;  // pair-image row stride (dwords); byte offsets
  bool pad;                     // the padded stride fits
  __host__ __device__ X6Lds(int w, int h) {
    const int base = (kX6W1 + kX6W2) * 2 + (128 + 32) * 4;
    const int a4 = (4 * ((w - 8) / 4)) % 32;
    r = base;
    rs3 = 3 * w + ((a4 - 3 * w) % 32 + 32) % 32;
    pad = true;
    for (int k = 0; k < 2; k++) {
      xs = r + (rs3 * h + 1) * 4;
      a2sc = (xs + w * h * 4 + 15) & ~15;
      bytes = a2sc + 4 * kX6Sc * 4;
      if (bytes <= kLdsHalf) break;
      rs3 = 3 * w;
      pad = false;
    }
  }
};

inline bool l12x6_fits(int w, int h) {
  return w * h <= kXsMax && X6Lds(w, h).bytes <= kLdsHalf;
}

// What l12x6 itself lays out: the images in two fp16 parts (W1 image
// [s][t][2 parts][lane][8], W2 image [m][2 parts][lane][8], two part rows
// per pair-image row), behind the bias blocks the sample's scaled B2 and
// twelve floats of maxima slots (max |W1| and max |W2|, one per wave, in the
// prologue; max |X|, one per wave and sample), and the fp32 tile holding
// x 2^ex.  The stride is padded for the tiles X6Lds pads (rs = 4 (ow / 4) mod
// 32), else 2 w; the bytes never pass X6Lds's.
constexpr int kH6W1 = kX6KS * 2 * 2 * 512;  // W1 image, fp16
constexpr int kH6W2 = 4 * 2 * 512;          // W2 image, fp16
constexpr int kH6Cst = 128 + 32 + 32 + 12;  // floats: [W1 tap 80 | B1], B2, the sample's B2, slots
struct H6Lds {
  int rs, r, xs, a2sc, bytes;  // pair-image row stride (dwords); byte offsets
  __host__ __device__ H6Lds(int w, int h) {
    const int a4 = (4 * ((w - 8) / 4)) % 32;
    r = (kH6W1 + kH6W2) * 2 + kH6Cst * 4;
    rs = X6Lds(w, h).pad ? 2 * w + ((a4 - 2 * w) % 32 + 32) % 32 : 2 * w;
    xs = r + (rs * h + 1) * 4;
    a2sc = (xs + w * h * 4 + 15) & ~15;
    bytes = a2sc + 4 * kX6Sc * 4;
  }
};

// ---- delta1 and the layer 1-2 gradients in split products (d1x6.hpp) -------
constexpr int kD6W2 = 2 * 2 * 3 * 512;  // delta1's W2 image, bf16: [t][k][part][lane][8]
constexpr int kD6W3 = 2 * 3 * 512;      // delta2's W3 image (kD3), bf16: [s][part][lane][8]
constexpr int kD6Sc = 32 * 36;           // per-wave delta2 transpose scratch (floats)

// layer-3 geometry for the kD3 form (delta2 formed here from delta3)
struct D3Geom {
  int w3, h3, f3;
};
// kD3: how many slots of the launch maxima were written (the blocks of l12x6
// and of l3r that had a sample: min(grid, batch) each)
struct D6MaxGeom {
  int n12, n3;
};

struct D6Lds {
  int st;      // T image column stride (dwords per column, >= 4 cr + 9)
  int tcols;   // T image columns (the column runs' x range + 8)
  int rs;      // R image row stride (pixels): the least >= w with rs = 9 (mod 64)
  int rdw;     // R image dwords (3 parts interleaved)
  int tdw;     // T image dwords
  int xbuf;    // one X buffer (dwords): R then T
  // kD3: the delta3 pair image, rows of three part rows side by side: gw
  // columns per part, row stride gs (dwords), gh rows; one buffer d3buf dwords
  int gw, gs, gh, d3buf;
  int w2, xb, sc, slots, runs, cst, w3i, d3tab, d3img, bytes;  // byte offsets
  int tr;  // kD3: 1 = delta2 part images in the sc region (d6tr.hpp), 0 = the fp32 transpose scratch
  __host__ __device__ D6Lds(int w, int h, const RunGeom& rg, bool d3 = false) {
    st = 4 * rg.cr + 9;
    if (st < h + 1) st = h + 1;
    tcols = rg.b ? rg.b + 8 : 0;
    // a tap (dy, dx) of gW1's X operand sits 3 (dy rs + dx) dwords past its
    // run base, = 3 (9 dy + dx) = 3 tap (mod 64) for rs = 9 (mod 64): the 32
    // taps of a half-wave hit 32 distinct banks (at rs = w = 33 two taps
    // shared a bank: 53% of d1x6's LDS-active cycles were bank conflicts)
    rs = w + ((9 - w) % 64 + 64) % 64;
    rdw = 3 * (rs * h + 1);
    tdw = 3 * tcols * st;
    xbuf = rdw + tdw;
    w2 = 0;
    xb = kD6W2 * 2;
    sc = xb + 2 * xbuf * 4;
    sc = (sc + 15) & ~15;
    gw = gs = gh = d3buf = 0;
    // slot (py, px) reads delta3 at image row py + 5 - dy, column px + 7 - dx
    // (pairs of columns, d3taps.hpp); the padded row stride puts a chunk's 32
    // slots at one fixed offset on 32 banks (as l12x6's X image).
    // kD3 takes, in this order: the waves' delta2 part images (d6tr.hpp, tr)
    // with padded delta3 rows; the fp32 transpose scratch (1.5 KB less per
    // wave) with padded rows; the images with unpadded rows; the scratch with
    // unpadded rows.  The scratch forms are the layouts this kernel had before
    // the images, and padded rows come before the images: every shape fits
    // exactly where it did, and none loses the padded rows it had
    // (33x33: 151.8 KB with images and padded rows; unpadded rows' reads were
    // 11 of d1x6's 25 conflict points)
    const int ntry = d3 ? 4 : 1;
    for (int k = 0; k < ntry; k++) {
      tr = d3 && !(k & 1);
      const bool pad = k < 2;
      slots = sc + (tr ? d6tr_wave_off(4) : 4 * kD6Sc * 4);
      runs = slots + rg.nch * 32 * 4;
      cst = runs + rg.nch * 8 * 4;
      bytes = cst + 32 * 4;
      w3i = d3tab = d3img = bytes;
      if (!d3) break;
      gw = rg.ow + 8;
      gh = rg.oh + 5;
      const int a4 = (4 * rg.a) % 32;
      gs = pad ? 3 * gw + ((a4 - 3 * gw) % 32 + 32) % 32 : 3 * gw;
      d3buf = gh * gs;
      w3i = (cst + 32 * 4 + 15) & ~15;
      // (with the part images the slot's delta3 offset shares the slot
      // table's dword, d6_slot_pack: a table of its own is 2.5 KB at 33x33,
      // which the images need)
      d3tab = tr ? slots : w3i + kD6W3 * 2;
      d3img = tr ? w3i + kD6W3 * 2 : d3tab + rg.nch * 32 * 4;
      bytes = d3img + 3 * d3buf * 4 + 16;  // (+ the zeroing's last 16-B store)
      if (bytes <= kLdsMax) break;
    }
    // the final reduction's scratch and the slab staging after it
    const int red_bytes = 4 * 4 * 16 * 64 * 4 + (81 * 64 + 64 + 64 * 32 + 32) * 4;
    if (bytes < red_bytes) bytes = red_bytes;
  }
};

inline bool d1x6_fits(int w, int h, bool d3 = false) {
  const RunGeom rg = run_geom(w - 8, h - 8);
  return w <= 57 && D6Lds(w, h, rg, d3).bytes <= kLdsMax && (!d3 || rg.nch >= 4);
}

// ---- delta1 and the layer 1-2 gradients in fp32, cooperative (d1c.hpp) -----
// 4-wave teams per block, on alternate chunks of a sample (two teams per
// block, 512 slabs instead of 1024: d1 0.4065 vs 0.399 ms)
constexpr int kD1cTeams = 1;
constexpr int kD1cOcc = 4;                           // waves per SIMD (launch bound: 128 VGPRs)
constexpr int kD1cGrid = 256 * kD1cOcc / kD1cTeams;  // all blocks resident
constexpr int kD1cS = 40;       // X tile row stride in LDS (8 mod 32)
constexpr int kD1cMaxPx = 1024; // pixel slots of the X offset table (nch * 32)

inline bool d1c_fits(int w, int h) { return w <= kD1cS && ((w - 8) * (h - 8) + 31) / 32 * 32 <= kD1cMaxPx; }
inline int d1c_xs_floats(int h) { return (kD1cS * h + 63) / 64 * 64; }
inline size_t d1c_lds_bytes(int w, int h) {
  return (size_t)(kD1cTeams * 6144 + 2 * d1c_xs_floats(h) + ((w - 8) * (h - 8) + 31) / 32 * 32) * sizeof(float);
}
