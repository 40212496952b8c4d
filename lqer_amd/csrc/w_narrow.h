// The compact weight image of block_fp weights of width 2 and 3 (include/lqer_hip.h "compact weight image"): where its bits lie, written
// once for the four things that read or write them - the conversion kernels and their host twins (pack.hip) and the two decode-size
// kernels (smallm_tile.h: gemm_smallm.hip, decode1.hip).  Plain integer code, host and device.
//
// A compact panel covers what a standard panel covers (16 rows x 64 k) in 128 * width + 16 * E bytes:
//   [16 rows][4 q]  code dwords                                   256 B   offset 0
//   [16 rows][2]    sign dwords (width 3 only)                    128 B   offset 256
//   [16 rows][E]    biased exponent bytes, E = 1, 2 or 4          16 E B  offset 128 * width
// The unit is what ONE lane of the decode-size kernels multiplies per panel: weight row `row`, k group q = its 8 k of the panel's first 32
// (chunk q of the standard image) and its 8 k of the second 32 (chunk q + 4).  Byte j of a unit's code dword holds the four codes of
// k = j and 4 + j of chunk q and of chunk q + 4 - in 2-bit fields t = 0..3, the order the MFMA fragment pairs are expanded in:
//   width 2: field = sign << 1 | magnitude (1 bit)
//   width 3: field = magnitude (2 bits); the signs lie in the sign dword of the row's q pair {0, 1} or {2, 3}: bit 4 (q & 1) + t of byte j
// so that (dword >> 2 t) & 0x01.. / 0x03.. is the byte-wise table index of expand_frag_t and one shift + mask puts the signs on bit 7 of
// their bytes: the expand costs what the 4-bit nibbles' costs (plus one shift per panel at width 3).  A zero magnitude keeps its sign bit.
// Exponent byte i of a row covers 64 / E k of the panel; a lane reads the aligned dword that holds its row's bytes.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LQER_HD __host__ __device__ __forceinline__
#else
#define LQER_HD inline
#endif

namespace lqer {

constexpr int WN_SIGNS_OFF = 256;

// exponent bytes per row of a compact panel for weight blocks of `block` k (<= 0 or >= K: one block per row); 0: width not served
LQER_HD int wn_exps_per_row(int width, int block, int64_t K) {
  if (width != 2 && width != 3) return 0;
  if (block == 16 || block == 32) return 64 / block;
  if (block <= 0 || block >= K || block % 64 == 0) return 1;
  return 4;  // blocks that do not align to panels: one byte per 16 k, the standard image's repetition
}
LQER_HD int wn_panel_bytes(int width, int E) { return 128 * width + 16 * E; }
LQER_HD int wn_codes_off(int row, int q) { return row * 16 + q * 4; }
LQER_HD int wn_signs_off(int row, int q) { return WN_SIGNS_OFF + row * 8 + (q >> 1) * 4; }
LQER_HD int wn_exps_base(int width) { return 128 * width; }
// the aligned dword of the exponent area that holds row `row`'s E bytes, and the bit positions in it of the bytes that scale the
// lane's two fragments: 16-k segments q >> 1 and 2 + (q >> 1) of the panel
LQER_HD int wn_exps_off(int width, int E, int row) { return wn_exps_base(width) + ((row * E) & ~3); }
LQER_HD void wn_exps_shifts(int E, int row, int q, int& sh0, int& sh1) {
  const int base = 8 * ((row * E) & 3);
  sh0 = base + (E == 4 ? 8 * (q >> 1) : 0);
  sh1 = base + (E == 4 ? 16 + 8 * (q >> 1) : (E == 2 ? 8 : 0));
}
// Field t of a unit: the table indices (magnitudes) of its four bytes and their signs on bit 7.  sg: the unit's sign dword already shifted
// right by 4 (q & 1) (width 3; unused at width 2).  t = 0, 1: k 0..3 and 4..7 of chunk q; t = 2, 3: of chunk q + 4.
template <int W>
LQER_HD void wn_field(uint32_t codes, uint32_t sg, int t, uint32_t& idx, uint32_t& sign7) {
  static_assert(W == 2 || W == 3, "compact widths");
  if (W == 2) {
    idx = (codes >> (2 * t)) & 0x01010101u;
    sign7 = (codes << (6 - 2 * t)) & 0x80808080u;
  } else {
    idx = (codes >> (2 * t)) & 0x03030303u;
    sign7 = (sg << (7 - t)) & 0x80808080u;
  }
}

// byte offset of chunk c (8 k) of a row inside a standard panel (pack.hip: a row's words in the order {0,2,4,6,1,3,5,7})
LQER_HD int std_chunk_off(int row, int c) { return row * 32 + (c & 1) * 16 + (c >> 1) * 4; }

// (images are 4-byte aligned: every offset above is a multiple of 4 and the C ABI asks for 16-byte aligned buffers)
LQER_HD uint32_t wn_ld32(const uint8_t* p) { return *(const uint32_t*)p; }
LQER_HD void wn_st32(uint8_t* p, uint32_t v) { *(uint32_t*)p = v; }

// Padding.  The packer (pack.hip, k_w_pack) gives a 16-k segment that starts at or past K the byte of exponent 0, WN_PAD_BYTE(width),
// whatever block it lies in: in the one panel that K cuts, a compact byte that spans several segments (E < 4) can span live ones and
// such padding.  `live` = the panel's segments that start below K (0..4).  narrow keeps the byte of a span's first segment - live if
// any of the span is -, widen gives the padding its byte back: the round trip returns the packer's image byte for byte.  (The kernels
// that read the compact image scale the padding's all-zero codes with the span's byte instead: zeros either way.)
LQER_HD int wn_pad_byte(int width) { return 127 - (width - 1); }
LQER_HD int wn_live_segs(int64_t K, int64_t pk) {
  const int64_t left = (K - pk * 64 + 15) / 16;
  return left < 0 ? 0 : (left > 4 ? 4 : (int)left);
}

// one row of a standard panel -> the same row of the compact panel.  Returns false if the row is not the image of a width-W weight
// (a magnitude bit above W - 1, live exponent bytes of one compact byte's span that differ, padding with another byte than the
// packer's): widen(narrow(.)) would not give it back.
template <int W>
LQER_HD bool wn_narrow_row(const uint8_t* sp, uint8_t* np, int row, int E, int live) {
  constexpr uint32_t MAG = W == 2 ? 0x01010101u : 0x03030303u;
  bool ok = true;
  uint32_t sgn[2] = {0, 0};
  for (int q = 0; q < 4; ++q) {
    const uint32_t w[2] = {wn_ld32(sp + std_chunk_off(row, q)), wn_ld32(sp + std_chunk_off(row, q + 4))};
    uint32_t codes = 0, s4 = 0;
    for (int t = 0; t < 4; ++t) {
      const uint32_t nib = (t & 1) ? w[t >> 1] >> 4 : w[t >> 1];  // low nibbles: k 0..3, high nibbles: k 4..7
      const uint32_t mag = nib & 0x07070707u, sign = (nib >> 3) & 0x01010101u;
      ok = ok && (mag & ~MAG) == 0;
      if (W == 2) codes |= (mag | (sign << 1)) << (2 * t);
      else codes |= mag << (2 * t), s4 |= sign << t;
    }
    wn_st32(np + wn_codes_off(row, q), codes);
    sgn[q >> 1] |= s4 << (4 * (q & 1));
  }
  if (W == 3) wn_st32(np + wn_signs_off(row, 0), sgn[0]), wn_st32(np + wn_signs_off(row, 2), sgn[1]);
  const uint8_t* se = sp + 512 + row * 4;
  uint8_t* ne = np + wn_exps_base(W) + row * E;
  const int n = 4 / E;  // segments per compact byte
  for (int i = 0; i < E; ++i) {
    ne[i] = se[i * n];
    for (int j = 0; j < n && n > 1; ++j) ok = ok && se[i * n + j] == (i * n + j < live ? ne[i] : (uint8_t)wn_pad_byte(W));
  }
  return ok;
}

// one row of a compact panel -> the same row of the standard panel (through wn_field and the exponent dword: what the kernels read)
template <int W>
LQER_HD void wn_widen_row(const uint8_t* np, uint8_t* sp, int row, int E, int live) {
  const uint32_t ex = wn_ld32(np + wn_exps_off(W, E, row));
  for (int q = 0; q < 4; ++q) {
    const uint32_t codes = wn_ld32(np + wn_codes_off(row, q));
    const uint32_t sg = W == 3 ? wn_ld32(np + wn_signs_off(row, q)) >> (4 * (q & 1)) : 0u;
    uint32_t w[2] = {0, 0};
    for (int t = 0; t < 4; ++t) {
      uint32_t idx, sign7;
      wn_field<W>(codes, sg, t, idx, sign7);
      w[t >> 1] |= (idx | (sign7 >> 4)) << (4 * (t & 1));
    }
    wn_st32(sp + std_chunk_off(row, q), w[0]);
    wn_st32(sp + std_chunk_off(row, q + 4), w[1]);
    if ((q & 1) == 0) {  // the bytes of segments q >> 1 and 2 + (q >> 1), from the positions the kernels' lanes take them from
      int sh0, sh1;
      wn_exps_shifts(E, row, q, sh0, sh1);
      const int s0 = q >> 1, s1 = 2 + (q >> 1);
      sp[512 + row * 4 + s0] = (E < 4 && s0 >= live) ? (uint8_t)wn_pad_byte(W) : (uint8_t)(ex >> sh0);
      sp[512 + row * 4 + s1] = (E < 4 && s1 >= live) ? (uint8_t)wn_pad_byte(W) : (uint8_t)(ex >> sh1);
    }
  }
}

}  // namespace lqer
