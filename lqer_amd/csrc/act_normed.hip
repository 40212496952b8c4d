// The activation side of the Linears behind an RMSNorm (Llama / Mistral: input_layernorm -> q/k/v, post_attention_layernorm -> gate/up), as
// ONE launch on the RAW hidden state h: the norm's row reduction, x = w * (h * rstd) formed in registers, then what the activation side
// does with an x tensor - x_quantizer in blocks of [1, 16] -> the bf16 activation image, x_q A on v_mfma_f32_16x16x32_bf16 and
// A_out_quantizer (reference quantized_layers/linear.py:148, 154-156).  The normalised x never reaches HBM.
//
//   S    = sum_k float(h_k)^2                   fp32, one fixed order (below); a square of a 16-bit value is exact in fp32
//   rstd = 1.0f / sqrtf(S / (float)K + eps)     correctly rounded division and square root (no fast-math)
//   n_k  = round_dt(float(h_k) * rstd)
//   x_k  = round_dt(float(w_k) * float(n_k))    HF LlamaRMSNorm's two roundings in dt (the product of two dt values is exact in fp32)
//
// Work split (act_rows.h: 8 waves own 8 token rows over all of K, wave w the 512-k slabs s = w (mod 8), a lane 8 elements of a row as one
// 16-byte load).  The quantizer cannot start before the whole row has been seen, so the kernel runs in two passes over REGISTERS:
//   pass 1  a wave requests the 8 rows of ALL its slabs (K <= 8192: at most NS = 2 slabs, 64 registers), its 16 bytes of w per slab and
//           the first two parts of its A^T fragments; then, per row, a lane adds the squares of its 8 elements in ascending k (slab
//           after slab), an xor-shuffle tree (32, 16, 8, 4, 2, 1) adds the lanes, lane j writes row j's partial to LDS [wave][row].  After ONE
//           workgroup barrier lane l of every wave adds the eight partials of row l & 7 in wave order: S has one order whatever M and the
//           grid are, no atomics.  The fragment and weight requests land under the reduction and the barrier.
//   pass 2  per slab, from the registers: n and x, the block-of-16 quantizer (a block's halves sit in lanes l, l ^ 1), the 16-byte image
//           store and the wave-private LDS slab, then the slab's 16 MFMA steps against two fragment register sets refilled in turn, one
//           accumulator chain per rank tile in ascending k.  The 8 partial tiles meet in LDS in wave order; A_out; the bf16 store.
// A row past M costs clamped loads (row M - 1 again) and no arithmetic; a wave with no slab (K <= 3584) still takes part in both
// reductions with zeros.  Padded k is zeros.  Rank tiles 1, 2, 3, 4, 6, 8 (a group's padded rank is the sum of its members': q/k/v at
// rank 32 = 96); a fragment register set is at most 32 registers (one step per part from 6 tiles on).
//
// LDS: 8 x 8 x 1040 B slabs + 8 x 8 x rp x 4 B partial tiles (65 KiB + 4..32 KiB) + 256 B of row partials.  rank 0: the 256 B alone.
//
// NORM = NORM_LAYER: the same kernel behind a LayerNorm with weight and bias (OPT: self_attn_layer_norm -> q/k/v, final_layer_norm -> fc1),
// the rule of include/lqer_hip.h "fused LayerNorm" - every step an fp32 operation rounded on its own, no fused multiply-add for a
// multiply followed by an add:
//   S1   = sum_k float(h_k)                     mean = S1 / (float)K
//   d_k  = float(h_k) - mean                    S2 = sum_k d_k * d_k (the lane's chain: fmaf(d, d, acc))
//   rstd = 1.0f / sqrtf(S2 / (float)K + eps)
//   x_k  = round_dt((d_k * rstd) * float(w_k) + float(b_k))
// The centred form needs the mean before the first square, so pass 1 runs TWO row reductions over the same registers, each in the order
// stated above, each through a 256-B LDS area of its own (the second reduction's partials may be written while a slow wave still reads
// the first's) and one barrier; the fragment requests land under both.  d is recomputed from the row registers wherever it is used -
// no second copy of the row.  A lane whose chunk lies past K (and so a wave with no slab) holds h = 0 but would hold d = -mean: it adds
// ZERO to S2 and writes zeros, not b, into the padded k.  The lane's 16 bytes of b per slab travel beside those of w.  LDS: 256 B more.
// The RMS instantiations keep the statement sequence (and the compiled instruction stream) they had before NORM existed.
#include "act_rows.h"

namespace lqer {
namespace an {

using namespace arow;

constexpr int MAX_K = 8192;  // two slabs per wave

// one 256-B area of row partials per reduction: RMSNorm one, LayerNorm two
__host__ inline size_t lds_bytes_n(int rp, int norm) { return lds_bytes(rp) + (size_t)(norm == NORM_LAYER ? 2 : 1) * WAVES * ROWS * sizeof(float); }

template <int DT, int RT, int NS, int NORM>
__global__ __launch_bounds__(512) void k_act_normed(const bf16_t* __restrict__ h, const bf16_t* __restrict__ nw, float eps, int64_t M, int64_t ldh,
                                                     int64_t K, int64_t Kp, const bf16_t* __restrict__ a_frag, bf16_t* __restrict__ xq,
                                                     bf16_t* __restrict__ xaq, QP qx, QP qa, int L_aout, const bf16_t* __restrict__ nb) {
  constexpr bool LN = NORM == NORM_LAYER;
  constexpr int NT = RT ? RT : 1, HB = part_steps(RT), NP = STEPS / HB;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t m0 = (int64_t)blockIdx.x * ROWS;
  const int nslab = (int)((Kp + SLAB - 1) / SLAB), nst = (int)(Kp / 32);
  float* const part = (float*)(smem + lds_bytes(16 * RT));  // [WAVES][ROWS] partial sums of squares (LN: [2][WAVES][ROWS], S1 then S2)
  unsigned char* const wb = smem + (size_t)wave * ROWS * PITCH;          // this wave's slab: [ROWS][PITCH]
  const unsigned char* const tok = wb + (lane & 7) * PITCH + 16 * (lane >> 4);

  // ---- pass 1, requests.  Every load is unconditional and inside its tensor: a row past M reads row M - 1, a chunk past K the row's last
  // chunk, a slab past the last one the last one, a step past the padded K fragment block 0; what is out of range is zeroed where it is used.
  u32x4 rh[NS][ROWS], rw[NS], rb[LN ? NS : 1];
  asm volatile("" ::: "memory");
#pragma unroll
  for (int si = 0; si < NS; ++si) {
    const int s = wave + WAVES * si;
    const int64_t k = (int64_t)(s < nslab ? s : nslab - 1) * SLAB + 8 * lane, kc = k < K ? k : K - 8;
#pragma unroll
    for (int j = 0; j < ROWS; ++j) {
      const int64_t r = m0 + j < M ? m0 + j : M - 1;
      rh[si][j] = *(const u32x4*)(h + r * ldh + kc);
    }
    rw[si] = *(const u32x4*)(nw + kc);
    if constexpr (LN) rb[si] = *(const u32x4*)(nb + kc);
  }
  asm volatile("" ::: "memory");
  const u32x4* const fr = (const u32x4*)a_frag + lane;  // block (step, rank tile): fr[(step * RT + tile) * 64]
  u32x4 fa[HB][NT], fb[HB][NT];
  auto load_part = [&](u32x4 (&f)[HB][NT], int s, int p) {
    asm volatile("" ::: "memory");
#pragma unroll
    for (int i = 0; i < HB; ++i)
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int st = s * STEPS + p * HB + i;
        f[i][t] = fr[((int64_t)(st < nst ? st : 0) * RT + t) * 64];
      }
    asm volatile("" ::: "memory");
  };
  if constexpr (RT > 0) load_part(fa, wave, 0), load_part(fb, wave, 1);

  // ---- pass 1, the row statistics (act_rows.h row_stats: the sum of squares, or behind a LayerNorm the two row sums, in the one fixed
  // order - lane, wave, workgroup); wave-uniform from here on
  float rs[ROWS], mn[LN ? ROWS : 1];  // rstd (and LN: the mean) of the 8 rows
  {
    float mine_rstd, mine_mean;
    row_stats<DT, NS, LN>(part, wave, lane, M - m0, K, eps, [&](int si, int j) { return rh[si][j]; }, mine_rstd, mine_mean);
#pragma unroll
    for (int j = 0; j < ROWS; ++j) {
      rs[j] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mine_rstd), j));
      if constexpr (LN) mn[j] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mine_mean), j));
    }
  }

  f32x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // ---- pass 2.  Row j of the wave's slab number si: x from the lane's 8 elements of h and of w, the block quantizer, the image store and
  // the LDS store
  auto piece = [&](auto si_c, int j) {
    constexpr int si = decltype(si_c)::value;
    const int64_t k = (int64_t)(wave + WAVES * si) * SLAB + 8 * lane;
    uint32_t w[4] = {0, 0, 0, 0};
    if (m0 + j < M) {  // (wave-uniform)
      const bool live = k < K;
      float v[8];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float h0, h1, w0, w1;
        pair_to_f32<DT>(live ? rh[si][j][i] : 0u, h0, h1);
        pair_to_f32<DT>(live ? rw[si][i] : 0u, w0, w1);
        if constexpr (LN) {  // (a chunk past K: zeros, not b)
          float b0, b1;
          pair_to_f32<DT>(rb[si][i], b0, b1);
          v[2 * i] = live ? layer_norm_x<DT>(h0, mn[j], rs[j], w0, b0) : 0.f;
          v[2 * i + 1] = live ? layer_norm_x<DT>(h1, mn[j], rs[j], w1, b1) : 0.f;
        } else {
          v[2 * i] = rms_norm_x<DT>(h0, rs[j], w0);
          v[2 * i + 1] = rms_norm_x<DT>(h1, rs[j], w1);
        }
      }
      quant_half_block<DT>(v, qx, w);
      if (k < Kp) *(u32x4*)(xq + (m0 + j) * Kp + k) = (u32x4){w[0], w[1], w[2], w[3]};  // (k past K up to the padded K: zeros)
    }
    if constexpr (RT > 0) *(u32x4*)(wb + j * PITCH + 16 * lane) = (u32x4){w[0], w[1], w[2], w[3]};
    __builtin_amdgcn_sched_barrier(0);  // (rows are not interleaved: each would keep its temporaries alive beside the fragment sets)
  };
  auto slab = [&](auto si_c) {
    constexpr int si = decltype(si_c)::value;
    const int s = wave + WAVES * si;
    if (s >= nslab) return;  // (wave-uniform)
    if constexpr (RT > 0 && si > 0) load_part(fa, s, 0), load_part(fb, s, 1);
#pragma unroll
    for (int j = 0; j < ROWS; ++j) piece(si_c, j);
    if constexpr (RT > 0) {
      wave_fence();
#pragma unroll
      for (int p = 0; p < NP; p += 2) {
        mult_part<HB, NT>(tok, fa, p, acc);
        if (p + 2 < NP) load_part(fa, s, p + 2);
        mult_part<HB, NT>(tok, fb, p + 1, acc);
        if (p + 3 < NP) load_part(fb, s, p + 3);
      }
      wave_fence();
    }
  };
  slab(std::integral_constant<int, 0>{});
  if constexpr (NS > 1) slab(std::integral_constant<int, 1>{});
  // the eight partial tiles summed in wave order, A_out, the bf16 store
  if constexpr (RT > 0) tiles_sum_aout<RT, true>(smem, acc, wave, lane, m0, M, xaq, qa, L_aout);
}

}  // namespace an

// The launch of lqer_quantize_act_xa_normed and (norm = NORM_LAYER, nb the norm bias) of lqer_quantize_act_xa_layernormed (api.hip has
// checked pointers for NULL, the stride against K and eps): everything this kernel does not serve is refused here, in words, with
// nothing launched.  r == 0: the image alone (a_b16 and xaq unused).  check_only: the refusals alone (api.hip asks before it plans the
// GEMM call).
int act_normed_dispatch(int norm, const void* h, const void* nw, const void* nb, float eps, int dtype, int64_t M, int64_t K, int64_t ldh,
                        const QP& qx, bf16_t* xq, const void* a_b16, int64_t r, const QP& qa, bf16_t* xaq, hipStream_t st, bool check_only) {
  const char* const what = norm == NORM_LAYER ? "quantize_act_xa_layernormed" : "quantize_act_xa_normed";
  auto no = [&](const char* why) {
    set_error("%s: %s", what, why);
    return LQER_E_UNSUPPORTED;
  };
  if (dtype != LQER_F16 && dtype != LQER_BF16) return no("h must be fp16 or bf16 (the two roundings of x are those of a 16-bit eager model)");
  if (qx.kind != LQER_Q_MXINT || qx.block != 16 || qx.mbits > 8 || qx.mbits < 1) return no("the x_quantizer must be block_fp in blocks of 16, width 2..9");
  if (K <= 0 || K % 16 != 0) return no("in_features must be a positive multiple of 16");
  if (K > an::MAX_K) return no("in_features above 8192 (a wave keeps the rows of at most two 512-k slabs in registers)");
  if (((uintptr_t)h % 16) != 0 || ((ldh * 2) % 16) != 0 || ((uintptr_t)nw % 16) != 0 || ((uintptr_t)xq % 16) != 0)
    return no("h, its row stride, the norm weight and the image must be 16-byte aligned");
  if (norm == NORM_LAYER && ((uintptr_t)nb % 16) != 0) return no("the norm bias must be 16-byte aligned");
  const int64_t rp = r > 0 ? lqer_padded_r(r) : 0, Kp = lqer_padded_k(K);
  int L = 0;
  if (rp) {
    if (!(rp == 16 || rp == 32 || rp == 48 || rp == 64 || rp == 96 || rp == 128))
      return no("the padded rank must be 16, 32, 48, 64, 96 or 128 (or rank 0: the image alone)");
    if (qa.kind != LQER_Q_MXINT || qa.mbits > 8) return no("the A_out_quantizer must be block_fp of width <= 9");
    if ((L = arow::aout_block(qa, rp)) == 0) return no("A_out blocks must be 4, 8, 16, 32 or 64 columns that divide the padded rank, or one block per row");
    if (((uintptr_t)a_b16 % 16) != 0 || ((uintptr_t)xaq % 16) != 0) return no("the A^T image and xaq must be 16-byte aligned");
  }
  if ((M + an::ROWS - 1) / an::ROWS > 0x7fffffff) return no("more than 2^31 - 1 groups of 8 token rows");
  if (M == 0 || check_only) return LQER_OK;
  const bf16_t* const a_frag = rp ? (const bf16_t*)a_b16 + rp * Kp : nullptr;
  const unsigned grid = (unsigned)((M + an::ROWS - 1) / an::ROWS);
  const int lds = (int)an::lds_bytes_n((int)rp, norm);
  auto run = [&](auto dt, auto ns, auto nm, auto rt) {
    constexpr int LIMIT = 160 * 1024;
    return launch_k<an::k_act_normed<decltype(dt)::value, decltype(rt)::value, decltype(ns)::value, decltype(nm)::value>, LIMIT>(
        what, grid, 512, lds, st, (const bf16_t*)h, (const bf16_t*)nw, eps, M, ldh, K, Kp, a_frag, xq, xaq, qx, qa, L, (const bf16_t*)nb);
  };
  auto by_rt = [&](auto dt, auto ns, auto nm) {  // 16-column tiles of the padded rank
    switch (rp / 16) {
      case 0: return run(dt, ns, nm, std::integral_constant<int, 0>{});
      case 1: return run(dt, ns, nm, std::integral_constant<int, 1>{});
      case 2: return run(dt, ns, nm, std::integral_constant<int, 2>{});
      case 3: return run(dt, ns, nm, std::integral_constant<int, 3>{});
      case 4: return run(dt, ns, nm, std::integral_constant<int, 4>{});
      case 6: return run(dt, ns, nm, std::integral_constant<int, 6>{});
      default: return run(dt, ns, nm, std::integral_constant<int, 8>{});
    }
  };
  auto by_norm = [&](auto dt, auto ns) {
    return norm == NORM_LAYER ? by_rt(dt, ns, std::integral_constant<int, NORM_LAYER>{}) : by_rt(dt, ns, std::integral_constant<int, NORM_RMS>{});
  };
  auto by_ns = [&](auto dt) {  // slabs a wave keeps in registers
    return Kp > 8 * an::SLAB ? by_norm(dt, std::integral_constant<int, 2>{}) : by_norm(dt, std::integral_constant<int, 1>{});
  };
  return dtype == LQER_F16 ? by_ns(std::integral_constant<int, LQER_F16>{}) : by_ns(std::integral_constant<int, LQER_BF16>{});
}

}  // namespace lqer
