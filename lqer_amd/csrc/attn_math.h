// The scalar arithmetic both fused attention kernels share (attn_q.hip: prefill, attn_decode.hip: up to 8 query rows): the ->DT
// rounding, exp for the softmax, and the block-of-16 quantizer of P for a block split over a lane pair (mxint_bf16_image, common.h).  One spelling, so the two
// kernels cannot drift apart in a last bit.
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

}  // namespace attn

}  // namespace lqer
