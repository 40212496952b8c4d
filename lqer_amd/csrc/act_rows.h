// What the row-request activation kernels share (act_gated.hip: h = act(gate) * up; act_normed.hip: x = RMSNorm(h) or LayerNorm(h)): a workgroup of 8 waves
// owns 8 token rows over all of K, wave w the 512-k slabs s = w (mod 8), a lane 8 elements of a row.  Each kernel forms its own activation
// values in registers; from there on the two run the same three pieces:
//   quant_half_block  the block-of-16 quantizer on the lane's 8 values (the block's other half sits in lane ^ 1) -> 4 words of bf16 image
//   mult_part         HB MFMA steps of the wave's LDS slab against one fragment register set, one accumulator chain per rank tile
//   tiles_sum_aout    the 8 waves' partial tiles summed in wave order, A_out_quantizer, the bf16 store of xaq
// and the norms' own pieces, shared by act_normed.hip and the NORM instantiations of decode1.hip (whose workgroup is 8 waves over <= 8 rows too):
//   rms_norm_x, layer_norm_x   the elementwise rules;  row_sum, row_stats   a row's sums in the one fixed order, rstd and mean
#pragma once
#include "common.h"

namespace lqer {
namespace arow {

constexpr int ROWS = 8, WAVES = 8, SLAB = 512, PITCH = 1040, STEPS = SLAB / 32;

__host__ __device__ constexpr size_t lds_bytes(int rp) { return rp ? (size_t)WAVES * ROWS * PITCH + (size_t)WAVES * ROWS * rp * sizeof(float) : 0; }

// steps per fragment part: a register set holds HB x RT fragments, at most 32 registers
constexpr int part_steps(int rt) { return rt <= 1 ? 8 : (rt == 2 ? 4 : (rt <= 4 ? 2 : 1)); }

typedef __attribute__((ext_vector_type(8))) __bf16 bf16v8;

template <int DT>
__device__ __forceinline__ float round_dt(float v) {
  if constexpr (DT == LQER_F16) return (float)(_Float16)v;  // v_cvt_f16_f32 + back: round to nearest even, subnormals kept
  else return __uint_as_float((uint32_t)f32_to_bf16_rne(v) << 16);
}

// ---- the gated MLP's rule for one element of h (include/lqer_hip.h "gated MLP"), written once for act_gated.hip and the GATE
// instantiations of decode1_kernel.h: s = round_dt(g / (1 + exp(-g))) with the full-precision expf and a true division (relu: max(g, 0),
// exact), h = round_dt(float(s) * float(u)) - the product of two dt values is exact in fp32 - or, without up, h = s
template <int DT, bool UP>
__device__ __forceinline__ float gated(float g, float u, int act) {
  const float s = act == LQER_ACT_RELU ? (g > 0.f ? g : 0.f) : round_dt<DT>(g / (1.0f + expf(-g)));
  if constexpr (UP) return round_dt<DT>(s * u);
  else return s;
}

// ---- the norms in front of the quantizer (act_normed.hip; the NORM instantiations of decode1.hip): the rules of include/lqer_hip.h,
// "fused RMSNorm" and "fused LayerNorm", each written once
// RMSNorm's elementwise rule: HF LlamaRMSNorm's two roundings in dt (the product of two dt values is exact in fp32)
template <int DT>
__device__ __forceinline__ float rms_norm_x(float h, float rstd, float w) {
  return round_dt<DT>(w * round_dt<DT>(h * rstd));
}
// LayerNorm's elementwise rule: three fp32 roundings, then one to dt (contraction off: a multiply and the add behind it stay two operations)
template <int DT>
__device__ __forceinline__ float layer_norm_x(float h, float mean, float rstd, float w, float b) {
#pragma clang fp contract(off)
  const float d = h - mean;
  const float t = d * rstd;
  const float u = t * w;
  return round_dt<DT>(u + b);
}

// One sum over each of the workgroup's `rows` (<= 8) token rows, in THE order of the header: a lane's chain over its 8 consecutive elements
// in ascending k, slab after slab (512-k slab s belongs to wave s % 8: wave w holds slabs w + 8 si, si < NS); an xor tree over lane
// distances 32..1; lane j writes row j's wave sum to LDS area [WAVES][ROWS]; ONE workgroup barrier; the eight wave sums in wave order.
// chunk(si, j): the lane's 16 bytes (8 elements at k = (wave + 8 si) * 512 + 8 lane) of row j, anything where that k is not below K (it is
// masked to zero here); term(acc, v, live, j): the chain's step for element v of row j.  Returns, in lane l, the sum of row l & 7: one
// order whatever M and the grid are, no atomics.  Called by all 512 threads.
template <int DT, int NS, class Chunk, class Term>
__device__ __forceinline__ float row_sum(float* area, int wave, int lane, int64_t rows, int64_t K, Chunk chunk, Term term) {
  float mine = 0.f;
#pragma unroll
  for (int j = 0; j < ROWS; ++j) {
    float ss = 0.f;
    if (j < rows) {  // (wave-uniform)
#pragma unroll
      for (int si = 0; si < NS; ++si) {
        const bool live = (int64_t)(wave + WAVES * si) * SLAB + 8 * lane < K;  // (K % 8 == 0: a chunk is inside the tensor or outside it as a whole)
        const u32x4 c = chunk(si, j);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float a, b;
          pair_to_f32<DT>(live ? c[i] : 0u, a, b);
          ss = term(term(ss, a, live, j), b, live, j);
        }
      }
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) ss += __shfl_xor(ss, d, 64);
    }
    mine = lane == j ? ss : mine;
  }
  if (lane < ROWS) area[wave * ROWS + lane] = mine;
  __syncthreads();
  float S = 0.f;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) S += area[w * ROWS + (lane & 7)];
  return S;  // lane l: row l & 7
}

// The statistics of the rows: rstd (and LN: the mean) of row l & 7 in lane l.  RMSNorm: one row sum (the squares); LayerNorm: two, the
// centred squares behind the mean - each through a 256-B area of its own (part: [LN ? 2 : 1][WAVES][ROWS]; the second sum's partials may
// be written while a slow wave still reads the first's).  A chunk past K holds h = 0, its d would be -mean: it adds nothing to S2.
template <int DT, int NS, bool LN, class Chunk>
__device__ __forceinline__ void row_stats(float* part, int wave, int lane, int64_t rows, int64_t K, float eps, Chunk chunk, float& rstd,
                                          float& mean) {
  if constexpr (LN) {
    mean = row_sum<DT, NS>(part, wave, lane, rows, K, chunk, [](float acc, float v, bool, int) { return acc + v; }) / (float)K;
    float mn[ROWS];
#pragma unroll
    for (int j = 0; j < ROWS; ++j) mn[j] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mean), j));
    const float S2 = row_sum<DT, NS>(part + WAVES * ROWS, wave, lane, rows, K, chunk, [&](float acc, float v, bool live, int j) {
      const float d = live ? v - mn[j] : 0.f;
      return __builtin_fmaf(d, d, acc);
    });
    rstd = 1.0f / sqrtf(S2 / (float)K + eps);
  } else {
    const float S = row_sum<DT, NS>(part, wave, lane, rows, K, chunk, [](float acc, float v, bool, int) { return __builtin_fmaf(v, v, acc); });
    mean = 0.f;
    rstd = 1.0f / sqrtf(S / (float)K + eps);
  }
}

// the lane's 8 values of a block of 16 (dt values: an fp16 one cannot be a non-zero |v| <= 1e-8) -> w, which arrives zeroed
template <int DT>
__device__ __forceinline__ void quant_half_block(const float (&v)[8], const QP& qx, uint32_t (&w)[4]) {
  float amax = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) amax = fmaxf(amax, fabsf(v[i]));
  amax = fmaxf(amax, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(amax), 0xB1, 0xf, 0xf, true)));  // quad_perm [1,0,3,2]
  if (amax > 0.f) {
    const int e = block_exponent_u(amax, qx);
    if (mxint16_fast_ok(e, qx)) {
      mxint16_bf16_fast<DT != LQER_F16, 8>(v, e, qx, w);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const uint32_t lo = exact_bf16_bits(ldexpf(mxint_mantissa(v[2 * i], e, qx), e - qx.mbits));
        const uint32_t hi = exact_bf16_bits(ldexpf(mxint_mantissa(v[2 * i + 1], e, qx), e - qx.mbits));
        w[i] = lo | (hi << 16);
      }
    }
  }
}

// multiply part p of the wave's slab: HB steps of 32 k.  tok: the lane's place in the slab (row lane & 7, chunk lane / 16), + 64 per step
template <int HB, int NT>
__device__ __forceinline__ void mult_part(const unsigned char* tok, const u32x4 (&f)[HB][NT], int p, f32x4 (&acc)[NT]) {
  u32x4 tk[HB];
#pragma unroll
  for (int i = 0; i < HB; ++i) tk[i] = *(const u32x4*)(tok + 64 * (HB * p + i));
#pragma unroll
  for (int i = 0; i < HB; ++i)
#pragma unroll
    for (int t = 0; t < NT; ++t)
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16v8, tk[i]), __builtin_bit_cast(bf16v8, f[i][t]), acc[t], 0, 0, 0);
  __builtin_amdgcn_sched_barrier(0);
}

// (the wave reads back what it wrote itself: LDS executes a wave's accesses in order - no workgroup barrier; the fences keep the
// compiler from moving the reads above the writes, or the next slab's writes above the reads)
__device__ __forceinline__ void wave_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  __builtin_amdgcn_sched_barrier(0);
}

// The 8 partial tiles meet in LDS (red: [WAVES][ROWS][RP] behind the slabs) and are summed in wave order: bit-stable, no atomics.  A_out
// follows k_act16_fused's rules: a thread holds 4 columns of a row, a block of L columns is G = L / 4 neighbouring lanes that cross by
// shuffles.  ANYG: G need not be a power of two (one block per row of 48 or 96 columns): the maxima cross through LDS, over the slabs,
// which every wave has finished with at the barrier.  Called by all 512 threads.
template <int RT, bool ANYG>
__device__ __forceinline__ void tiles_sum_aout(unsigned char* smem, const f32x4 (&acc)[RT], int wave, int lane, int64_t m0, int64_t M,
                                               bf16_t* __restrict__ xaq, const QP& qa, int L_aout) {
  constexpr int RP = 16 * RT;
  float* const red = (float*)(smem + (size_t)WAVES * ROWS * PITCH);
  const int g4 = lane >> 4;
  // D layout: column n = lane & 15, rows 4 g4 + i: token rows 0-7 live in g4 = 0, 1
  if (g4 < 2) {
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) red[(wave * ROWS + 4 * g4 + i) * RP + 16 * t + (lane & 15)] = acc[t][i];
  }
  __syncthreads();
  const int tid = threadIdx.x;
  const bool live = tid < ROWS * RP / 4;
  const int r = tid / (RP / 4), c4 = tid - r * (RP / 4);
  float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
  if (live) {
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
      const float4 v = *(const float4*)(red + (w * ROWS + r) * RP + 4 * c4);
      sum.x += v.x, sum.y += v.y, sum.z += v.z, sum.w += v.w;
    }
  }
  float bmax = fmaxf(fmaxf(fabsf(sum.x), fabsf(sum.y)), fmaxf(fabsf(sum.z), fabsf(sum.w)));
  const int G = L_aout / 4;
  if (ANYG && (G & (G - 1)) != 0) {  // (workgroup-uniform)
    float* const bm = (float*)smem;
    bm[tid] = bmax;
    __syncthreads();
    if (live) {
      const int b0 = tid - c4 % G;
      for (int i = 0; i < G; ++i) bmax = fmaxf(bmax, bm[b0 + i]);
    }
  } else {
    if (tid >= 64 * ((ROWS * RP / 4 + 63) / 64)) return;  // (whole waves only: the shuffles below need their partners)
    for (int d = 1; d < G; d <<= 1) bmax = fmaxf(bmax, __shfl_xor(bmax, d, 64));
  }
  if (!live || m0 + r >= M) return;
  const bool anyb = bmax > 0.f;
  const int eb = anyb ? block_exponent(bmax, qa) : 0;
  const float v[4] = {sum.x, sum.y, sum.z, sum.w};
  uint32_t w2[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const float a = anyb ? mxint_mantissa(v[2 * i], eb, qa) : 0.f;
    const float b = anyb ? mxint_mantissa(v[2 * i + 1], eb, qa) : 0.f;
    w2[i] = exact_bf16_bits(ldexpf(a, eb - qa.mbits)) | (exact_bf16_bits(ldexpf(b, eb - qa.mbits)) << 16);
  }
  *(uint2*)(xaq + ((m0 + r) * RP + 4 * c4)) = make_uint2(w2[0], w2[1]);
}

// the A_out block of the dispatchers: L columns (4..64, a power-of-two count of 4-column lanes, dividing the padded rank), or the whole
// padded rank (one block per row); 0 = refused
__host__ inline int aout_block(const QP& qa, int64_t rp) {
  const int L = (qa.block <= 0 || qa.block >= rp) ? (int)rp : qa.block;
  if (L == rp && rp % 4 == 0) return L;
  const int G = L / 4;
  return (rp % L != 0 || L % 4 != 0 || (G & (G - 1)) != 0 || G > 64) ? 0 : L;
}

}  // namespace arow
}  // namespace lqer
