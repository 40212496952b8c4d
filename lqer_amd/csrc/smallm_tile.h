// What the two decode-size kernels share (gemm_smallm.hip: M <= 64 behind the activation kernel; decode1.hip: M <= 8, one launch):
// a packed panel as a lane holds it (the standard 576-byte panel, or the compact panel of a 2- / 3-bit weight), the lane's place in it, its
// expansion to two MFMA fragments, and the maximum over the four lanes that hold a B_out block.  The kernels' schedules (request order, barriers, fences) stay in their own files - and so do
// the A_out quantizer of 4 rank entries per lane and the B_out re-quantization of an f32x4, written out twice with the same text:
// as functions of this header they change both kernels' device code (profiles/shared_pieces_codeobj.txt, "not taken").
#pragma once
#include "common.h"
#include "w_narrow.h"

namespace lqer {

struct SmPanel {
  u32x4 cw;      // the lane's 16-byte half of its row's codes: chunks {h, h+2, h+4, h+6}, h = (lane >> 4) & 1
  uint32_t ex;   // the row's 4 biased block exponents
};

// A lane's place in a 16 (rows) x 64 (k) panel of 576 B: weight row / token `row`, k group `q`.  Its words for the two 32-deep halves
// of the panel are chunks q and q + 4 = words q >> 1 and (q >> 1) + 2 of the half-row it loads; their block exponents are bytes
// q >> 1 and 2 + (q >> 1) of the row's exponent dword.
struct SmLane {
  int row, q;
  int codes_off, exps_off;  // byte offsets of SmPanel::cw / ::ex inside a panel
  bool hi;
  int sh0, sh1;
  __device__ __forceinline__ explicit SmLane(int lane)
      : row(lane & 15), q(lane >> 4), codes_off(row * 32 + (q & 1) * 16), exps_off(512 + row * 4), hi((q >> 1) != 0), sh0(8 * (q >> 1)),
        sh1(16 + 8 * (q >> 1)) {}
};

// the lane's two A fragments (16 weight rows x 32 k each) of a panel
template <bool F16>
__device__ __forceinline__ void sm_expand(const SmPanel& p, const SmLane& ln, bf16x8& wb0, bf16x8& wb1) {
  const uint32_t w0 = ln.hi ? p.cw[1] : p.cw[0], w1 = ln.hi ? p.cw[3] : p.cw[2];
  wb0 = expand_frag_t<F16>(w0, ((p.ex >> ln.sh0) & 0xffu) << 23);
  wb1 = expand_frag_t<F16>(w1, ((p.ex >> ln.sh1) & 0xffu) << 23);
}

// ---- the compact image of 2- and 3-bit weights (w_narrow.h): the same lane, the same two fragments, W = the codes' width (0: the
// standard panel above).  A lane holds its unit's code dword (width 3: and the sign dword of its q pair) and the aligned exponent dword
// of its row; E, the exponent bytes per row, only moves offsets and shifts, so it is a lane constant, not a template parameter.
template <int W>
struct SmPanelT {
  uint32_t cw;  // the unit's four 2-bit fields per byte
  uint32_t sg;  // width 3: the sign dword of rows' q pair (unused at width 2)
  uint32_t ex;  // the dword of the exponent area that holds the row's E bytes
};
template <>
struct SmPanelT<0> : SmPanel {};

template <int W>
struct SmLaneT {
  int row, q;
  int codes_off, signs_off, exps_off;  // byte offsets inside a compact panel
  int sgsh;                            // the lane's half of the sign dword: 4 (q & 1)
  int sh0, sh1;
  int panel_bytes;
  __device__ __forceinline__ SmLaneT(int lane, int E)
      : row(lane & 15), q(lane >> 4), codes_off(wn_codes_off(row, q)), signs_off(wn_signs_off(row, q)), exps_off(wn_exps_off(W, E, row)),
        sgsh(4 * (q & 1)), panel_bytes(wn_panel_bytes(W, E)) {
    wn_exps_shifts(E, row, q, sh0, sh1);
  }
};
template <>
struct SmLaneT<0> : SmLane {
  static constexpr int panel_bytes = LQER_PANEL_BYTES;
  __device__ __forceinline__ SmLaneT(int lane, int) : SmLane(lane) {}
};

// expand_frag_t on a compact unit's fields t0 (k 0..3) and t0 + 1 (k 4..7): the same e4m3 bytes, the same conversions, the same bits
template <bool F16, int W>
__device__ __forceinline__ bf16x8 wn_expand_frag(uint32_t codes, uint32_t sg, int t0, uint32_t scale_bits) {
  const float scale = __uint_as_float(scale_bits);
  constexpr uint32_t LUT_LO = 0x44403800u, LUT_HI = 0x4E4C4A48u;  // e4m3 bytes of 0,1,2,3 | 4,5,6,7 (expand_frag's table)
  uint32_t ie, se, io, so;
  wn_field<W>(codes, sg, t0, ie, se);
  wn_field<W>(codes, sg, t0 + 1, io, so);
  const uint32_t fe = __builtin_amdgcn_perm(LUT_HI, LUT_LO, ie) | se, fo = __builtin_amdgcn_perm(LUT_HI, LUT_LO, io) | so;
  u32x4 r;
  if constexpr (!F16) {
    r[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(fe, scale, false));
    r[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(fe, scale, true));
    r[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(fo, scale, false));
    r[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(fo, scale, true));
  } else {
    r[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(fe, scale, false));
    r[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(fe, scale, true));
    r[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(fo, scale, false));
    r[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(fo, scale, true));
  }
  return __builtin_bit_cast(bf16x8, r);
}

template <bool F16, int W>
__device__ __forceinline__ void sm_expand(const SmPanelT<W>& p, const SmLaneT<W>& ln, bf16x8& wb0, bf16x8& wb1) {
  if constexpr (W == 0) {
    sm_expand<F16>((const SmPanel&)p, (const SmLane&)ln, wb0, wb1);
  } else {
    const uint32_t sg = W == 3 ? p.sg >> ln.sgsh : 0u;
    wb0 = wn_expand_frag<F16, W>(p.cw, sg, 0, ((p.ex >> ln.sh0) & 0xffu) << 23);
    wb1 = wn_expand_frag<F16, W>(p.cw, sg, 2, ((p.ex >> ln.sh1) & 0xffu) << 23);
  }
}

__device__ __forceinline__ float quad16_max(float v) {  // max over lanes l, l^16, l^32, l^48 (no LDS crossbar: the swaps)
  auto r16 = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  v = fmaxf(__uint_as_float(r16[0]), __uint_as_float(r16[1]));
  auto r32 = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return fmaxf(__uint_as_float(r32[0]), __uint_as_float(r32[1]));
}

}  // namespace lqer
