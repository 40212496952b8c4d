// The scalar arithmetic both fused attention kernels share (attn_q.hip: prefill, attn_decode.hip: up to 8 query rows): the ->DT
// rounding, exp for the softmax, the block-of-16 quantizer of P for a block split over a lane pair (mxint_bf16_image, common.h) and the
// fold of a lane pair's (max, sum).  One spelling, so the two kernels cannot drift apart in a last bit.
#pragma once
#include "qmm_image.h"

namespace lqer {

namespace attn {

template <int DT>
__device__ __forceinline__ float rnd(float x) {  // ->DT
  if constexpr (DT == LQER_F16) return (float)(_Float16)x;
  else if constexpr (DT == LQER_BF16) return __uint_as_float((uint32_t)f32_to_bf16_rne(x) << 16);
  else return x;
}

// exp(x) for x <= 0 on v_exp_f32 with the rounding of x log2(e) compensated (the bare product is off by |x| 2^-24 in the exponent:
// 30 ulps at x = -20): about 2 ulps.  Below -200 (-inf included) the result is 0; a NaN stays a NaN (the comparison is false for it).
__device__ __forceinline__ float exp_neg(float x) {
  x = x < -200.0f ? -200.0f : x;
  const float t = x * 1.44269502162933349609375f;
  const float r = __builtin_fmaf(x, 1.44269502162933349609375f, -t) + x * 1.925963033500011e-8f;
  const float e = __builtin_amdgcn_exp2f(t);
  return __builtin_fmaf(e, r * 0.693147182464599609375f, e);
}

// the 8 values a lane holds of a block of 16 (the other 8 sit in lane ^ 32) -> 8 exact bf16 values: quant16_bf16 with
// the maximum taken across the lane pair (block_exponent + mxint_bf16_image, common.h)
template <bool FLUSH_TINY>
__device__ __forceinline__ void quant8of16_bf16(const float (&v)[8], const QP& q, uint32_t (&w)[4]) {
  float am = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) am = fmaxf(am, fabsf(v[i]));
  const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(am), __float_as_uint(am), false, false);
  const float amax = fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
#pragma unroll
  for (int i = 0; i < 4; ++i) w[i] = 0;
  if (amax > 0.f) {
    const int e = block_exponent(amax, q);
    mxint_bf16_image<FLUSH_TINY, 8>(v, e, q, w);
  }
}

// The fold of two (max, sum) pairs {m_i, l_i = sum exp(s - m_i)}: M = max m_i, L = sum l_i exp_neg(m_i - M) (nothing visible in
// either: M = -inf and the reference 0) - here the pairs of lanes l and l ^ 32, the lower lane's first in both lanes: the end of
// k_attn_q's sweep 1 and of a subtile in k_attn_dec_scores.  (The folds over a chunk's subtiles and over a row's chunks, the same
// rule over an array, keep their loops in attn_decode.hip: as a function they move registers - profiles/attn_pieces_codeobj.txt.)
__device__ __forceinline__ void fold_lane_pair(float m, float l, float& M, float& L) {
  const auto sm = __builtin_amdgcn_permlane32_swap(__float_as_uint(m), __float_as_uint(m), false, false);
  const auto sl = __builtin_amdgcn_permlane32_swap(__float_as_uint(l), __float_as_uint(l), false, false);
  const float m0 = __uint_as_float(sm[0]), m1 = __uint_as_float(sm[1]), l0 = __uint_as_float(sl[0]), l1 = __uint_as_float(sl[1]);
  M = fmaxf(m0, m1);
  const float mr = M == -__builtin_inff() ? 0.f : M;
  L = l0 * exp_neg(m0 - mr) + l1 * exp_neg(m1 - mr);
}

// The tree rule of a draft-tree verify (the TREE kernels of attn_decode.hip and attn_q.hip), on top of the causal one: the last S_b
// keys of a sequence are its draft nodes in append order, `mask` is the query row's own word - bit j set iff node j is the row's node
// or one of its ancestors - and j = t - (T_b - S_b) the node that key t holds.  j < 0: the committed context, all of it visible.
// (j beyond the row's own node is the causal limit's to refuse: the bit read there is never used.)
__device__ __forceinline__ bool tree_sees(uint64_t mask, int64_t j) { return j < 0 || ((mask >> (j & 63)) & 1); }

}  // namespace attn

}  // namespace lqer
