// What the tile kernels of the fused GEMM share (device code only): k_lqer_gemm (gemm_w4a8.hip, 128- and 64-row tiles) and
// k_lqer_gemm_m256 (gemm_w4a8_m256.hip) take everything here; k_lqer_gemm_i8, qmm_image.h and xa_staged.hip the swizzle, the LDS
// pointer type and the tile order.  Ring depth, slot sizes and tile height are each kernel's own.
// Only pieces that leave every kernel's device code as it was live here (tools/codeobj_diff.py --by-symbol against the parent
// commit; profiles/tile_shared_codeobj.txt also lists the pieces that were tried as functions and moved registers).
#pragma once
#include "common.h"

namespace lqer {

// byte offset of 16-byte chunk `c` (8 bf16 along k) of tile row `r`; rows are 128 B.
// chunk ^ ((row >> 1) & 7): the 16 lanes of a ds_read_b128 group then hit 16 distinct 16-B slots.
__device__ __forceinline__ int swz(int r, int c) { return r * 128 + ((c ^ ((r >> 1) & 7)) << 4); }

typedef __attribute__((address_space(3))) void lds_void;
typedef __attribute__((address_space(1))) const void gbl_void;

// max over lanes l and l^32
__device__ __forceinline__ float pair32_max(float v) {
  auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}

// XCD-aware tile order: blocks b, b+8, ... share an XCD; each of the 8 XCDs gets a contiguous run of the nt tiles (same token
// rows -> the activation slab stays in that XCD's L2).  The grid is a multiple of 8 or covers nt.
__device__ __forceinline__ int xcd_tile(int b, int nt) {
  const int xcd = b & 7, q8 = nt >> 3, r8 = nt & 7;
  return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (b >> 3);
}

// The 16 weight panels of a k-step (16 x 576 B) are contiguous in the ring slot and are filled by nine 1-KiB LDS-DMAs with per-lane
// source offsets (576 = 36 x 16: a lane's 16 bytes lie inside one panel).  This lane's source offset for piece 0..8, from the
// first panel of the column tile; a panel's nk k-steps are contiguous.
__device__ __forceinline__ int w_piece_voff(int piece, int lane, int nk) {
  const int byte = piece * 1024 + lane * 16;
  const int pnl = byte / LQER_PANEL_BYTES;
  return pnl * nk * LQER_PANEL_BYTES + (byte - pnl * LQER_PANEL_BYTES);
}

// Hand-built buffer descriptor for the in-asm LDS-DMA of the main loop, four wave-uniform words: {ring_rsrc_base(base), bytes,
// 0x00020000} - this is words 0 and 1.  `bytes` is the EXACT range of what the tile may read: every step issues its prefetch, also
// past the end of K; those lanes read inside the tile's rows or are dropped by the range check.  (Words 2 and 3 stay with the
// caller: as a function's argument `bytes` would be computed ahead of the readfirstlanes, and the kernels' instruction order follows.)
// The compiler-visible descriptors of the prologue loads are each kernel's own __builtin_amdgcn_make_buffer_rsrc: the 128-row kernel
// gives them the same exact ranges, the 256-row kernel 0x7fffffff and guards its prologue steps with d < nk instead.  Both are right
// as they stand; do not align one with the other without looking at who relies on the range check.
__device__ __forceinline__ u32x2 ring_rsrc_base(const void* base) {
  const unsigned long long b64 = (unsigned long long)base;
  return u32x2{(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)b64),
               (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(b64 >> 32)) & 0xffffu};
}

// Text of the LOAD statements of the main loops (each LOAD stays ONE asm statement; the operands come in as "%N" strings):
// two activation fragments - m tiles 32 rows = 4096 B apart - from the per-lane address `addr` + the constant `off`; and one
// LDS-DMA request: M0 = LDS destination of the wave's piece, then 16 B per lane from `rsrc` at voff + soff.
#define LQER_READ_X2(d0, d1, addr, off) \
  "ds_read_b128 " d0 ", " addr " offset:" off "\n\tds_read_b128 " d1 ", " addr " offset:" off "+4096\n\t"
#define LQER_LDS_DMA(m0, voff, rsrc, soff) "s_mov_b32 m0, " m0 "\n\ts_nop 0\n\tbuffer_load_dwordx4 " voff ", " rsrc ", " soff " offen lds\n\t"

// column of accumulator register k of a 32x32 tile of the transposed MFMA (a lane owns token row lane & 31; per quad q, registers
// 4q .. 4q+3 are columns 8q + 4 lh + (0..3), lh = lane >> 5), from the wave's first column nb
__device__ __forceinline__ int acc_col(int nb, int k, int lh) { return nb + (k & 3) + 8 * (k >> 2) + 4 * lh; }

}  // namespace lqer
