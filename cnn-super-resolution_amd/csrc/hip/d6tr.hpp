// d6tr.hpp -- the per-wave bf16 image through which d1x6 (d1x6.hpp, kD3) turns
// delta2's split parts from the row layout (delta1's A operand) into gW2's B
// operand, included by train_fused.hip inside namespace srcnn::fused.  No
// device intrinsic: it compiles for the host with the qualifiers defined away
// (tests/d6_tr_image_check.cpp).
//
// The image is [slot][part][n]: 32 slot rows of three 64-B part rows (32
// channels of bf16), so a part's two 8-B writes of a k-step, and all three
// parts, sit within one ds_write2_b64's offsets of one address.  The 8-B quads
// of a part row are XOR-swizzled by the slot:
//   - a transposed read (ds_read_b64_tr_b16, bank = dword mod 64 per 32-lane
//     half) takes 4 whole part rows of one part, rows 192 B apart: 64 distinct
//     banks under any permutation of a row's quads;
//   - a write (bank = dword mod 32 per 16 consecutive lanes = 16 slots, one
//     quad column) would put 16 slots on 2 bank pairs at plain rows (8-way);
//     bits 0 and 2 of the quad index taken from the slot's bits 1 and 2 leave
//     slots s and s + 8 on one pair: 2-way.  Bit 1 of the quad index tells a
//     write's two quads apart (16 B, the ds_write2_b64 pair), so it stays.
constexpr int kD6TrPartRow = 64;                 // bytes: one slot's 32 channels of one part
constexpr int kD6TrRow = 3 * kD6TrPartRow;       // bytes per slot
constexpr int kD6TrWave = 32 * kD6TrRow;         // bytes per wave (6 KB)

// wave's region, from the first wave's (16-B aligned in LDS)
__host__ __device__ constexpr int d6tr_wave_off(int wave) { return wave * kD6TrWave; }

__host__ __device__ constexpr int d6tr_swz(int slot) { return ((slot >> 1) & 1) | (((slot >> 2) & 1) << 2); }

// byte offset (from the wave's region) of 8-B quad c (channels 4 c .. 4 c + 3)
// of slot's row in part q
__host__ __device__ constexpr int d6tr_off(int slot, int c, int q) {
  return slot * kD6TrRow + q * kD6TrPartRow + 8 * (c ^ d6tr_swz(slot));
}

// the write of lane (slot, h): elements 4 w .. 4 w + 3 of part q of delta1's A
// fragment of k-step k are channels n = 16 k + 8 w + 4 h + 0 .. 3
__host__ __device__ constexpr int d6tr_write_off(int slot, int h, int k, int q, int w) {
  return d6tr_off(slot, 4 * k + 2 * w + h, q);
}

// the address lane supplies to transposed read w (0, 1) of part q of gW2's B
// fragment of k-step m: lane 4 i + p of its 16-lane group points at row
// 16 m + 8 w + 4 h + i (slot crow(8 m + 4 w + i, h)), channels 16 g + 4 p ..,
// g = the group's channel half; it receives elements 4 w .. 4 w + 3 =
// delta2[slot crow(8 m + 4 w + 0 .. 3, h)][n = lane & 31]
__host__ __device__ constexpr int d6tr_read_off(int lane, int m, int q, int w) {
  const int h = lane >> 5, g = (lane >> 4) & 1, i = (lane >> 2) & 3, p = lane & 3;
  return d6tr_off(16 * m + 8 * w + 4 * h + i, 4 * g + p, q);
}

// a slot's table dword in this form: its output pixel (-1: a dummy slot) over
// its delta3 image offset.  Both lie below one delta3 buffer's dwords (gh rows
// of gs >= ow + 8 dwords for oh + 5 rows), and three buffers fit the 160 KB of
// LDS, so both are below kD6SlotMax
constexpr int kD6SlotMax = 160 * 1024 / (3 * 4);
static_assert(kD6SlotMax < (1 << 15), "d6_slot_pack: the pixel in 15 bits and a sign, the offset in 16");
__host__ __device__ constexpr int d6_slot_pack(int pix, int off) { return pix * 65536 + off; }
__host__ __device__ constexpr int d6_slot_pix(int v) { return v >> 16; }
__host__ __device__ constexpr int d6_slot_off(int v) { return v & 0xffff; }

// what d1x6's addressing relies on: a write's second quad 16 B past its first
// and the parts one part row apart (one address per k-step); every read a
// constant past the lane's first (one address register, immediates)
__host__ __device__ constexpr bool d6tr_addressable() {
  for (int s = 0; s < 32; s++)
    for (int h = 0; h < 2; h++)
      for (int k = 0; k < 2; k++)
        for (int q = 0; q < 3; q++) {
          const int o = d6tr_write_off(s, h, k, 0, 0);
          if (d6tr_write_off(s, h, k, q, 0) != o + q * kD6TrPartRow) return false;
          if (d6tr_write_off(s, h, k, q, 1) != o + q * kD6TrPartRow + 16) return false;
          if (d6tr_write_off(s, h, 1, 0, 0) != (d6tr_write_off(s, h, 0, 0, 0) ^ 32)) return false;
        }
  for (int l = 0; l < 64; l++)
    for (int m = 0; m < 2; m++)
      for (int q = 0; q < 3; q++)
        for (int w = 0; w < 2; w++)
          if (d6tr_read_off(l, m, q, w) != d6tr_read_off(l, 0, 0, 0) + (16 * m + 8 * w) * kD6TrRow + q * kD6TrPartRow)
            return false;
  return true;
}
static_assert(d6tr_addressable(), "d1x6's delta2 part image: one write address per k-step, one read address");
