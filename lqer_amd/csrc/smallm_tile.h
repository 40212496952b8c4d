// What the two decode-size kernels share (gemm_smallm.hip: M <= 64 behind the activation kernel; decode1.hip: M <= 8, one launch):
// a packed panel as a lane holds it, the lane's place in it, its expansion to two MFMA fragments, and the maximum over the four
// lanes that hold a B_out block.  The kernels' schedules (request order, barriers, fences) stay in their own files - and so do
// the A_out quantizer of 4 rank entries per lane and the B_out re-quantization of an f32x4, written out twice with the same text:
// as functions of this header they change both kernels' device code (profiles/shared_pieces_codeobj.txt, "not taken").
#pragma once
#include "common.h"

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

__device__ __forceinline__ float quad16_max(float v) {  // max over lanes l, l^16, l^32, l^48 (no LDS crossbar: the swaps)
  auto r16 = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  v = fmaxf(__uint_as_float(r16[0]), __uint_as_float(r16[1]));
  auto r32 = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return fmaxf(__uint_as_float(r32[0]), __uint_as_float(r32[1]));
}

}  // namespace lqer
