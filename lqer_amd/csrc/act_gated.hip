// The activation side of a DOWN projection fed by a gated MLP, as ONE launch: h = act(gate) * up formed in registers (Llama / Mistral:
// down_proj(silu(gate_proj(x)) * up_proj(x)); OPT: fc2(relu(fc1(x))), up == NULL), then what the activation side does with an x tensor -
// x_quantizer in blocks of [1, 16] (reference quantizers/block_fp.py:55-82 through quantized_layers/linear.py:148,154) -> the bf16
// activation image, h_q A on v_mfma_f32_16x16x32_bf16 (linear.py:155) and A_out_quantizer (linear.py:156).  h never reaches HBM.
//
//   h   s = round_dt(g / (1 + exp(-g))) in fp32 with the full-precision expf and a true division, h = round_dt(float(s) * float(u)):
//       the two roundings eager F.silu(g) * u performs in dt (the product of two dt values is exact in fp32).  relu is exact.
//
// Work split.  A workgroup owns ROWS = 8 token rows over ALL of K (no partial tiles in HBM, no second launch, any M >= 1); its 8 waves
// take the slabs of 512 k in turn (slab s belongs to wave s % 8).  Inside a slab a REQUEST is one whole token row: lane l holds
// elements 8 l .. 8 l + 7 of the slab - of gate and of up alike, one 16-byte load each, 1 KiB of one row per request and tensor - so
//   - which rows exist is a wave-uniform question: a row past M costs a clamped load (row M - 1 again, a cache hit) and no arithmetic,
//     which is what a decode-size call (M = 1: seven of eight rows) is made of;
//   - a block of 16 is lanes (2 i, 2 i + 1): the block maximum crosses with one DPP quad permute;
//   - the lane's 8 quantized values are one 16-byte store to the image and one to the wave's PRIVATE LDS slab [8 rows][1040 B] - a row of
//     the slab is written by one instruction, conflict-free, and no workgroup barrier stands inside the k loop.
// Data flow of a slab: its 16 row requests were issued one slab ahead (behind the previous slab's last quantized row); the first two
// parts of its A^T fragments (the fragment-major copy of lqer_a_b16_prepare, ONE coalesced 16-byte load per lane and 16 x 32 block) are
// requested in front of the quantizer and land under it; the 8 rows are quantized; the next slab's rows are requested; then the slab's
// 16 MFMA steps run from LDS (one ds_read_b128 per step: row lane & 7, chunk 4 step + lane / 16 - the 8 rows are rows 0-7 of the 16-row
// operand) against two fragment register sets refilled in turn.  Every wave keeps ONE accumulator chain per rank tile over its slabs in
// ascending k; the 8 partial tiles meet in LDS and are summed in wave order: bit-stable from run to run, no atomics.  A_out follows
// k_act16_fused (block L as in act16_fused_dispatch).  The image is the oracle quantizer's output for h bit for bit; h_q A is inside the
// summation-order envelope (tests/_envelope.py).
//
// LDS: 8 x 8 x 1040 B slabs + 8 x 8 x rp x 4 B partial tiles = 65 KiB + 4..16 KiB.  rank 0: the image alone, no LDS.
#include "act_rows.h"

namespace lqer {
namespace ag {

using namespace arow;  // the work split and the pieces shared with act_normed.hip; gated(): one element of h (act: wave-uniform)

template <int DT, int RT, bool UP>
__global__ __launch_bounds__(512) void k_act_gated(const void* __restrict__ gate, const void* __restrict__ up, int act, int64_t M, int64_t ldg,
                                                    int64_t ldu, int64_t K, int64_t Kp, const bf16_t* __restrict__ a_frag, bf16_t* __restrict__ xq,
                                                    bf16_t* __restrict__ xaq, QP qx, QP qa, int L_aout) {
  constexpr int RP = 16 * RT, NT = RT ? RT : 1;
  constexpr int HB = part_steps(RT);                   // steps per fragment part: a register set holds HB x RT fragments = 32 registers
  constexpr int NP = STEPS / HB;                       // parts per slab; part p (steps HB p .. HB p + HB - 1) lives in set p & 1
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t m0 = (int64_t)blockIdx.x * ROWS;
  const int nslab = (int)((Kp + SLAB - 1) / SLAB), nst = (int)(Kp / 32);
  // ---- requests.  Every load is unconditional and inside its tensor: a row past M reads row M - 1, a chunk past K the row's last chunk,
  // a slab past the last one the last one, a step past the padded K fragment block 0; what is out of range is zeroed where it is used.
  u32x4 rg[ROWS], ru[UP ? ROWS : 1];
  auto load_rows = [&](int s) {
    asm volatile("" ::: "memory");
    const int64_t k = (int64_t)(s < nslab ? s : nslab - 1) * SLAB + 8 * lane, kc = k < K ? k : K - 8;
#pragma unroll
    for (int j = 0; j < ROWS; ++j) {
      const int64_t r = m0 + j < M ? m0 + j : M - 1;
      rg[j] = *(const u32x4*)((const bf16_t*)gate + r * ldg + kc);
      if constexpr (UP) ru[j] = *(const u32x4*)((const bf16_t*)up + r * ldu + kc);
    }
    asm volatile("" ::: "memory");
  };
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
  load_rows(wave);
  unsigned char* const wb = smem + (size_t)wave * ROWS * PITCH;          // this wave's slab: [ROWS][PITCH]
  const int g4 = lane >> 4;
  const unsigned char* const tok = wb + (lane & 7) * PITCH + 16 * g4;    // + 64 step: row lane & 7, chunk 4 step + g4
  f32x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // ---- row j of slab s: h from the lane's 8 gate / up elements, the block quantizer (the block's other half sits in lane ^ 1), the
  // image store and the LDS store
  auto piece = [&](int s, int j) {
    const int64_t k = (int64_t)s * SLAB + 8 * lane;
    uint32_t w[4] = {0, 0, 0, 0};
    if (m0 + j < M) {  // (wave-uniform)
      const bool live = k < K;  // (K % 8 == 0: a chunk is inside the tensors or outside them as a whole)
      float v[8];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float g0, g1, u0 = 0.f, u1 = 0.f;
        pair_to_f32<DT>(live ? rg[j][i] : 0u, g0, g1);
        if constexpr (UP) pair_to_f32<DT>(live ? ru[j][i] : 0u, u0, u1);
        v[2 * i] = gated<DT, UP>(g0, u0, act), v[2 * i + 1] = gated<DT, UP>(g1, u1, act);
      }
      quant_half_block<DT>(v, qx, w);
      if (k < Kp) *(u32x4*)(xq + (m0 + j) * Kp + k) = (u32x4){w[0], w[1], w[2], w[3]};  // (k past K up to the padded K: zeros)
    }
    if constexpr (RT > 0) *(u32x4*)(wb + j * PITCH + 16 * lane) = (u32x4){w[0], w[1], w[2], w[3]};
    __builtin_amdgcn_sched_barrier(0);  // (rows are not interleaved: each would keep its temporaries alive beside the fragment sets)
  };
  for (int s = wave; s < nslab; s += WAVES) {
    if constexpr (RT > 0) load_part(fa, s, 0), load_part(fb, s, 1);
#pragma unroll
    for (int j = 0; j < ROWS; ++j) piece(s, j);
    load_rows(s + WAVES);  // (the wave's next slab, into the registers the quantizer has just freed)
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
  }
  // the eight partial tiles summed in wave order, A_out, the bf16 store
  if constexpr (RT > 0) tiles_sum_aout<RT, false>(smem, acc, wave, lane, m0, M, xaq, qa, L_aout);
}

}  // namespace ag

// The launch of lqer_quantize_act_xa_gated (api.hip has checked pointers for NULL, the strides against K and `act`): everything this
// kernel does not serve is refused here, in words, with nothing launched.  r == 0: the image alone (a_b16 and xaq unused).
// check_only: the refusals alone (api.hip asks before it plans the GEMM call).
int act_gated_dispatch(const void* gate, const void* up, int act, int dtype, int64_t M, int64_t K, int64_t ldg, int64_t ldu, const QP& qx, bf16_t* xq,
                       const void* a_b16, int64_t r, const QP& qa, bf16_t* xaq, hipStream_t st, bool check_only) {
  auto no = [](const char* why) {
    set_error("quantize_act_xa_gated: %s", why);
    return LQER_E_UNSUPPORTED;
  };
  if (dtype != LQER_F16 && dtype != LQER_BF16) return no("gate / up must be fp16 or bf16 (the two roundings of h are those of a 16-bit eager model)");
  if (qx.kind != LQER_Q_MXINT || qx.block != 16 || qx.mbits > 8 || qx.mbits < 1) return no("the x_quantizer must be block_fp in blocks of 16, width 2..9");
  if (K <= 0 || K % 16 != 0) return no("in_features must be a positive multiple of 16");
  if (((uintptr_t)gate % 16) != 0 || ((ldg * 2) % 16) != 0 || ((uintptr_t)up % 16) != 0 || (up && (ldu * 2) % 16 != 0) || ((uintptr_t)xq % 16) != 0)
    return no("gate, up, their row strides and the image must be 16-byte aligned");
  const int64_t rp = r > 0 ? lqer_padded_r(r) : 0, Kp = lqer_padded_k(K);
  int L = 0;
  if (rp) {
    if (!(rp == 16 || rp == 32 || rp == 64)) return no("the padded rank must be 16, 32 or 64 (or rank 0: the image alone)");
    if (qa.kind != LQER_Q_MXINT || qa.mbits > 8) return no("the A_out_quantizer must be block_fp of width <= 9");
    L = (qa.block <= 0 || qa.block >= rp) ? (int)rp : qa.block;
    const int G = L / 4;
    if (rp % L != 0 || L % 4 != 0 || (G & (G - 1)) != 0 || G > 64) return no("A_out blocks must be 4, 8, 16, 32 or 64 columns that divide the padded rank");
    if (((uintptr_t)a_b16 % 16) != 0 || ((uintptr_t)xaq % 16) != 0) return no("the A^T image and xaq must be 16-byte aligned");
  }
  if ((M + ag::ROWS - 1) / ag::ROWS > 0x7fffffff) return no("more than 2^31 - 1 groups of 8 token rows");
  if (M == 0 || check_only) return LQER_OK;
  const bf16_t* const a_frag = rp ? (const bf16_t*)a_b16 + rp * Kp : nullptr;
  const unsigned grid = (unsigned)((M + ag::ROWS - 1) / ag::ROWS);
  const int lds = (int)ag::lds_bytes((int)rp);
  auto run = [&](auto dt, auto hasup) {
    constexpr int DT = decltype(dt)::value, LIMIT = 160 * 1024;
    constexpr bool UP = decltype(hasup)::value;
    const char* const what = "quantize_act_xa_gated";
    switch (rp / 16) {  // 16-column tiles of the padded rank
      case 0: return launch_k<ag::k_act_gated<DT, 0, UP>, LIMIT>(what, grid, 512, lds, st, gate, up, act, M, ldg, ldu, K, Kp, a_frag, xq, xaq, qx, qa, L);
      case 1: return launch_k<ag::k_act_gated<DT, 1, UP>, LIMIT>(what, grid, 512, lds, st, gate, up, act, M, ldg, ldu, K, Kp, a_frag, xq, xaq, qx, qa, L);
      case 2: return launch_k<ag::k_act_gated<DT, 2, UP>, LIMIT>(what, grid, 512, lds, st, gate, up, act, M, ldg, ldu, K, Kp, a_frag, xq, xaq, qx, qa, L);
      default: return launch_k<ag::k_act_gated<DT, 4, UP>, LIMIT>(what, grid, 512, lds, st, gate, up, act, M, ldg, ldu, K, Kp, a_frag, xq, xaq, qx, qa, L);
    }
  };
  auto by_up = [&](auto dt) { return up ? run(dt, std::true_type{}) : run(dt, std::false_type{}); };
  return dtype == LQER_F16 ? by_up(std::integral_constant<int, LQER_F16>{}) : by_up(std::integral_constant<int, LQER_BF16>{});
}

}  // namespace lqer
