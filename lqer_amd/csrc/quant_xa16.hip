// Fused: activation quantize (blocks of 16) + side-path partial GEMM, padded rank <= 64.
// One workgroup = 32 token rows x 256 k.  Phase 1: every lane quantizes two 16-element blocks (consecutive
// lanes = consecutive 32-byte pieces of a row: fully coalesced), writes the bf16 image to HBM and to an LDS
// slab (XOR-swizzled 16-byte chunks).  Phase 2: the 4 waves run v_mfma_f32_32x32x16_bf16 over 64 k each,
// A^T fragments straight from L2; their partial tiles are summed in a fixed order through LDS and written as
// ONE partial per workgroup.  The activation image is not read back from HBM for the side path.
#include "xa_common.h"
namespace lqer {
__device__ __forceinline__ int qx_swz(int row, int chunk) { return row * (QX_K * 2) + ((chunk ^ (row & 15)) << 4); }

template <int DT, int NT>
__global__ __launch_bounds__(QX_K) void k_quant_xa16(const void* __restrict__ x, int64_t M, int64_t K, int64_t ldx, bool vec,
                                                    QP q, bf16_t* __restrict__ xq, int64_t Kp,
                                                    const bf16_t* __restrict__ a_t, int a_limbs, int rp, int row_groups,
                                                    float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) unsigned char slab[32 * QX_K * 2];   // 16 KiB
  __shared__ __attribute__((aligned(16))) float red[(QX_WAVES > 1 ? QX_WAVES - 1 : 1) * 32 * 32 * NT];  // waves 1.. park their tiles here
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nchunk = (int)((Kp + QX_K - 1) / QX_K);
  const int rg = blockIdx.x / nchunk, c = blockIdx.x - rg * nchunk;
  const int64_t kbase = (int64_t)c * QX_K;
  // the wave's A^T fragments (limb 0) are fetched first, so their L2 latency overlaps the activation loads
  const int r = lane & 31, h = lane >> 5;
  const int64_t kw = kbase + 64 * wave;
  bf16x8 af0[4][NT];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks)
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int n = t * 32 + r;
      af0[ks][t] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
      if (n < rp && kw < Kp && a_limbs > 0) af0[ks][t] = *(const bf16x8*)(a_t + (int64_t)n * Kp + kw + 16 * ks + 8 * h);
    }
  // ---- phase 1: quantize
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2) {
    const int s = tid + s2 * QX_K;          // 2 QX_K blocks of 16: row = s / (QX_K / 16), segment = s % (QX_K / 16)
    const int row = s / (QX_K / 16), seg = s % (QX_K / 16);
    const int64_t m = (int64_t)rg * 32 + row, k0 = kbase + seg * 16;
    uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (k0 < Kp) {
      if (m < M && k0 < K) {
        float v[16];
        load16<DT>(x, m * ldx + k0, K - k0, vec, v);
        float amax = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) amax = fmaxf(amax, fabsf(v[i]));
        if (amax > 0.f) {
          const int e = block_exponent_u(amax, q);
          mxint_bf16_image<DT != LQER_F16, 16>(v, e, q, w);
        }
      }
      uint4* dst = (uint4*)(xq + m * Kp + k0);   // rows up to the padded M are allocated
      dst[0] = make_uint4(w[0], w[1], w[2], w[3]);
      dst[1] = make_uint4(w[4], w[5], w[6], w[7]);
    }
    *(uint4*)(slab + qx_swz(row, 2 * seg)) = make_uint4(w[0], w[1], w[2], w[3]);
    *(uint4*)(slab + qx_swz(row, 2 * seg + 1)) = make_uint4(w[4], w[5], w[6], w[7]);
  }
  __syncthreads();
  // ---- phase 2: partial side GEMM, wave w covers k [64w, 64w + 64) of the slab
  f32x16 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[t][j] = 0.f;
  if (kw < Kp) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const bf16x8 xf = *(const bf16x8*)(slab + qx_swz(r, (64 * wave + 16 * ks) / 8 + h));
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xf, af0[ks][t], acc[t], 0, 0, 0);
      for (int l = 1; l < a_limbs; ++l) {  // fp16 / fp32 A: further exact bf16 limbs
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const int n = t * 32 + r;
          bf16x8 af = {0, 0, 0, 0, 0, 0, 0, 0};
          if (n < rp) af = *(const bf16x8*)(a_t + ((int64_t)l * rp + n) * Kp + kw + 16 * ks + 8 * h);
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xf, af, acc[t], 0, 0, 0);
        }
      }
    }
  }
  // fixed-order combine: ((w0 + w1) + w2) + w3
  if (wave > 0) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int j = 0; j < 16; ++j) red[(((wave - 1) * NT + t) * 16 + j) * 64 + lane] = acc[t][j];
  }
  __syncthreads();
  if (wave == 0) {
    float* dst = part + ((int64_t)c * row_groups + rg) * XA_ROWS * rp;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int n = t * 32 + r;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        float sum = acc[t][j];
#pragma unroll
        for (int w2 = 0; w2 < QX_WAVES - 1; ++w2) sum += red[((w2 * NT + t) * 16 + j) * 64 + lane];
        if (n < rp) dst[((j & 3) + 8 * (j >> 2) + 4 * h) * rp + n] = sum;
      }
    }
  }
}

// Decode sizes: the small-M GEMM can sum the fused kernel's partial tiles and apply A_out itself (gemm_smallm.hip) when
// A_out blocks are 16 wide - the reduce launch is then skipped.
bool xa_fused_partials_ok(const QP& qx, const QP& qa, int64_t r) {
  const int rp = (int)lqer_padded_r(r);
  return qx.kind == LQER_Q_MXINT && qx.block == 16 && qx.mbits <= 8 && rp <= 64 && qa.kind == LQER_Q_MXINT && qa.mbits <= 8 &&
         qa.block == 16;
}
void xa_fused_plan(int64_t M, int64_t K, int64_t r, int* nchunk, int64_t* cstride) {
  const int64_t Kp = lqer_padded_k(K);
  *nchunk = (int)((Kp + QX_K - 1) / QX_K);
  *cstride = ((M + XA_ROWS - 1) / XA_ROWS) * XA_ROWS * lqer_padded_r(r);
}

int quant_xa16_launch(const void* x, int dtype, int64_t M, int64_t K, int64_t ldx, const QP& q, bf16_t* xq, int64_t Kp, const bf16_t* a_t,
                      int a_limbs, int rp, const XaPlan& plan, float* part, hipStream_t st) {  // (plan: row groups x chunks of QX_K)
  const bool vec = ((uintptr_t)x % 16 == 0) && ((ldx * (dtype == LQER_F32 ? 4 : 2)) % 16 == 0);
  const unsigned grid = (unsigned)(plan.row_groups * plan.nchunk);
  return with_dtype(dtype, [&](auto dt) {
    return with_int<1, 2>((rp + 31) / 32, [&](auto nt) {
      return launch_k<k_quant_xa16<decltype(dt)::value, decltype(nt)::value>>("quantize_act_xa", grid, QX_K, 0, st, x, M, K, ldx, vec, q, xq, Kp, a_t,
                                                                              a_limbs, rp, plan.row_groups, part);
    });
  });
}

}  // namespace lqer
