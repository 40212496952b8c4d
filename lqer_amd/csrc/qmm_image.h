// The operand-image side of the quantized attention products, shared by matmul_q.hip (the two separate products) and
// attn_q.hip (the fused attention): 16-element loads, the block-of-16 quantizer to exact bf16 values, and the two kernels
// that write w_quantizer(y) as a bf16 image [b][j][k], k contiguous.
#pragma once
#include <type_traits>

#include "gemm_tile.h"  // swz: the operand tiles have the fused GEMM's swizzled LDS layout

namespace lqer {

namespace qmm {

constexpr int BM = 128, BN = 128, BK = 64;

// 16 consecutive elements (or fewer at the end of a row), 128-bit loads when the piece is aligned and complete
template <int DT>
__device__ __forceinline__ void load16(const void* base, int64_t off, int64_t valid, bool vec, float (&v)[16]) {
  if (vec && valid >= 16) {
    if constexpr (DT == LQER_F32) {
      const float4* p = (const float4*)((const float*)base + off);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float4 t = p[i];
        v[4 * i] = t.x, v[4 * i + 1] = t.y, v[4 * i + 2] = t.z, v[4 * i + 3] = t.w;
      }
    } else {
      const uint4* p = (const uint4*)((const bf16_t*)base + off);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const uint4 t = p[i];
        const uint32_t w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if constexpr (DT == LQER_F16) {
            typedef __attribute__((ext_vector_type(2))) _Float16 h2;
            const h2 h = __builtin_bit_cast(h2, w[j]);
            v[8 * i + 2 * j] = (float)h[0], v[8 * i + 2 * j + 1] = (float)h[1];
          } else {
            v[8 * i + 2 * j] = __uint_as_float(w[j] << 16), v[8 * i + 2 * j + 1] = __uint_as_float(w[j] & 0xffff0000u);
          }
        }
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = i < valid ? load_elem<DT>(base, off + i) : 0.0f;
  }
}

// 16 consecutive elements as raw 16-byte loads (the aligned fast path: requested chunks ahead, converted at use)
template <int DT>
struct Raw16 {
  static constexpr int N = DT == LQER_F32 ? 4 : 2;
  uint4 r[N];
};
template <int DT>
__device__ __forceinline__ void raw_to_f32(const Raw16<DT>& raw, float (&v)[16]) {
  if constexpr (DT == LQER_F32) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[4 * i] = __uint_as_float(raw.r[i].x), v[4 * i + 1] = __uint_as_float(raw.r[i].y);
      v[4 * i + 2] = __uint_as_float(raw.r[i].z), v[4 * i + 3] = __uint_as_float(raw.r[i].w);
    }
  } else {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const uint32_t w[4] = {raw.r[i].x, raw.r[i].y, raw.r[i].z, raw.r[i].w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if constexpr (DT == LQER_F16) {
          typedef __attribute__((ext_vector_type(2))) _Float16 h2;
          const h2 h = __builtin_bit_cast(h2, w[j]);
          v[8 * i + 2 * j] = (float)h[0], v[8 * i + 2 * j + 1] = (float)h[1];
        } else {
          v[8 * i + 2 * j] = __uint_as_float(w[j] << 16), v[8 * i + 2 * j + 1] = __uint_as_float(w[j] & 0xffff0000u);
        }
      }
    }
  }
}

// one block of 16 -> 16 exact bf16 values (block_fp.py:7-82; zero block -> zeros; |x| <= 1e-8 flushed to 0 - FLUSH_TINY is
// false for fp16 inputs, which cannot hold a non-zero |x| <= 1e-8: four instructions less per pair in the hot loop)
template <bool FLUSH_TINY = true>
__device__ __forceinline__ void quant16_bf16(const float (&v)[16], const QP& q, uint32_t (&w)[8]) {
  float amax = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) amax = fmaxf(amax, fabsf(v[i]));
#pragma unroll
  for (int i = 0; i < 8; ++i) w[i] = 0;
  if (amax > 0.f) {
    const int e = block_exponent(amax, q);
    if (mxint16_fast_ok(e, q)) {
      mxint16_bf16_fast<FLUSH_TINY>(v, e, q, w);
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const uint32_t lo = exact_bf16_bits(ldexpf(mxint_mantissa(v[2 * i], e, q), e - q.mbits));
        const uint32_t hi = exact_bf16_bits(ldexpf(mxint_mantissa(v[2 * i + 1], e, q), e - q.mbits));
        w[i] = lo | (hi << 16);
      }
    }
  }
}

// PRE: the values are ALREADY the quantizer's outputs (the standalone quantizer ran over the operand: block lengths other than
// 16 - 16 n or whole rows - of formats whose values are bf16 numbers, width <= 9): the bf16 image is their high halves
template <bool PRE, bool FLUSH_TINY>
__device__ __forceinline__ void image16(const float (&v)[16], const QP& q, uint32_t (&w)[8]) {
  if constexpr (PRE) {
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = exact_bf16_bits(v[2 * i]) | (exact_bf16_bits(v[2 * i + 1]) << 16);
  } else {
    quant16_bf16<FLUSH_TINY>(v, q, w);
  }
}

// ---- y [b][k][j], j contiguous -> img [b][S2p][Kp] (blocks of 16 along j), transposed through LDS -------------------------
// One workgroup = 64 k x 64 j.  Thread t quantizes the block (k = t / 4, j = 16 (t % 4) ..): four threads read 128 B of a
// k row; the bf16 values go to an LDS tile [j][k] and leave as 32-byte pieces of the image's j rows.
// (the body: `y_off` is the element offset of this batch entry in y, `img` its image - shared with attn_q.hip, whose batch
// entries are (batch, kv head) pairs with a stride each)
template <int DT, bool PRE>
__device__ __forceinline__ void bimage_j_tile(const void* __restrict__ y, int64_t y_off, int64_t K, int64_t S2, int64_t y_ks, const QP& q,
                                              bf16_t* __restrict__ img, int64_t S2p, int64_t Kp, bool vec, int64_t k0, int64_t j0) {
  __shared__ bf16_t tile[64][64 + 2];  // (+2: the 16 two-byte stores of a thread walk 16 rows - spread them over banks)
  const int tid = threadIdx.x;
  {
    const int kl = tid >> 2, jb = (tid & 3) * 16;
    float v[16];
    const int64_t k = k0 + kl, j = j0 + jb;
    uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (k < K && j < S2) {
      load16<DT>(y, y_off + k * y_ks + j, S2 - j, vec, v);
      image16<PRE, DT != LQER_F16>(v, q, w);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      tile[jb + 2 * i][kl] = (bf16_t)(w[i] & 0xffff);
      tile[jb + 2 * i + 1][kl] = (bf16_t)(w[i] >> 16);
    }
  }
  __syncthreads();
  {
    const int jl = tid >> 2, kc = (tid & 3) * 16;
    if (j0 + jl < S2p && k0 + kc < Kp) {
      bf16_t* dst = img + (j0 + jl) * Kp + k0 + kc;
      uint32_t w[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) w[i] = (uint32_t)tile[jl][kc + 2 * i] | ((uint32_t)tile[jl][kc + 2 * i + 1] << 16);
      ((uint4*)dst)[0] = make_uint4(w[0], w[1], w[2], w[3]);
      ((uint4*)dst)[1] = make_uint4(w[4], w[5], w[6], w[7]);
    }
  }
}

template <int DT, bool PRE = false>  // PRE: y is the bf16 image of the standalone quantizer (DT = LQER_BF16): transposed only
__global__ __launch_bounds__(256) void k_qmm_bimage_j(const void* __restrict__ y, int64_t K, int64_t S2, int64_t y_bs, int64_t y_ks, QP q,
                                                      bf16_t* __restrict__ img, int64_t S2p, int64_t Kp, bool vec) {
  const int64_t b = blockIdx.z;
  bimage_j_tile<DT, PRE>(y, b * y_bs, K, S2, y_ks, q, img + b * S2p * Kp, S2p, Kp, vec, (int64_t)blockIdx.y * 64, (int64_t)blockIdx.x * 64);
}

// ---- y [b][k][j], k contiguous (the transposed view of a [j][k] tensor) -> img [b][S2p][Kp] -------------------------------
// A 64 (j) x 64 (k) tile per workgroup: four threads read 128 B of a j row, the fp32 values cross an LDS tile, thread (j block of
// 16, k) quantizes its block with the packed routine, the bf16 values cross a second tile and leave as 32-byte pieces of the
// image's rows.  (Round 2's kernel kept 16 x 8 values per thread - one wave per SIMD, 1,400 instructions per thread, a branch
// around a slow path per element: 18-20 us for a [32, 2048, 128] operand against 10 us.)
template <int DT>
__device__ __forceinline__ void bimage_k_tile(const void* __restrict__ y, int64_t y_off, int64_t K, int64_t S2, int64_t y_js, const QP& q,
                                              bf16_t* __restrict__ img, int64_t S2p, int64_t Kp, bool vec, int64_t k0, int64_t j0) {
  __shared__ float tf[64][64 + 1];
  __shared__ bf16_t tb[64][64 + 2];
  const int tid = threadIdx.x;
  {
    const int jl = tid >> 2, kc = (tid & 3) * 16;
    const int64_t j = j0 + jl, k = k0 + kc;
    float v[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = 0.f;
    if (j < S2 && k < K) load16<DT>(y, y_off + j * y_js + k, K - k, vec, v);
#pragma unroll
    for (int i = 0; i < 16; ++i) tf[jl][kc + i] = v[i];
  }
  __syncthreads();
  {
    const int jb = tid >> 6, kl = tid & 63;  // block of 16 consecutive j at one k: consecutive lanes = consecutive k (no bank conflict)
    float v[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) v[r] = tf[16 * jb + r][kl];
    uint32_t w[8];
    quant16_bf16<DT != LQER_F16>(v, q, w);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      tb[16 * jb + 2 * i][kl] = (bf16_t)(w[i] & 0xffff);
      tb[16 * jb + 2 * i + 1][kl] = (bf16_t)(w[i] >> 16);
    }
  }
  __syncthreads();
  {
    const int jl = tid >> 2, kc = (tid & 3) * 16;
    if (j0 + jl < S2p && k0 + kc < Kp) {
      bf16_t* dst = img + (j0 + jl) * Kp + k0 + kc;
      uint32_t w[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) w[i] = (uint32_t)tb[jl][kc + 2 * i] | ((uint32_t)tb[jl][kc + 2 * i + 1] << 16);
      ((uint4*)dst)[0] = make_uint4(w[0], w[1], w[2], w[3]);
      ((uint4*)dst)[1] = make_uint4(w[4], w[5], w[6], w[7]);
    }
  }
}

template <int DT>
__global__ __launch_bounds__(256) void k_qmm_bimage_k(const void* __restrict__ y, int64_t K, int64_t S2, int64_t y_bs, int64_t y_js, QP q,
                                                       bf16_t* __restrict__ img, int64_t S2p, int64_t Kp, bool vec) {
  const int64_t b = blockIdx.z;
  bimage_k_tile<DT>(y, b * y_bs, K, S2, y_js, q, img + b * S2p * Kp, S2p, Kp, vec, (int64_t)blockIdx.x * 64, (int64_t)blockIdx.y * 64);
}

}  // namespace qmm

}  // namespace lqer
