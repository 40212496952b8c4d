// The operand-image side of the quantized attention products, shared by matmul_q.hip (the two separate products) and
// attn_q.hip (the fused attention): the two kernels that write w_quantizer(y) as a bf16 image [b][j][k], k contiguous.  The
// 16-element loads are common.h's load16 / Raw16, the block-of-16 quantizer is common.h's quant16_bf16.
#pragma once
#include <type_traits>

#include "gemm_tile.h"  // swz: the operand tiles have the fused GEMM's swizzled LDS layout

namespace lqer {

namespace qmm {

constexpr int BM = 128, BN = 128, BK = 64;

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
