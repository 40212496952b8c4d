// Rank-r side path, first half:  xAq = A_out_quantizer( Q_x(x) @ A )   (reference quantized_layers/linear.py:154).  [M,K] x [K,r] with
// r << K: a skinny GEMM that streams the quantized activation once, i.e. HBM/L2 bound - so it is cut into independent (row tile,
// K chunk) pieces, an fp32 partial tile in scratch each:
//   k_xa_partial (xa_partial.hip)         : ~2048 pieces of 32 or 64 rows, one wave each, operands straight from L2
//   xal::k_xa_partial_lds (xa_staged.hip) : 128-row tiles, both operands staged through LDS (M >= 512; int8 images, rank 65..128)
//   k_quant_xa16 (quant_xa16.hip), xal::k_quant_xa128 (xa_staged.hip) : the same behind the block-16 activation quantizer, one launch
//   k_xa_reduce4 / _limbs / _blk (xa_reduce.hip) : sum the chunks in a fixed order (bit-reproducible, no atomics), apply A_out, write
//                  the exact bf16 image the fused GEMM's prologue consumes.
// A comes as exact bf16 limbs (pack.hip), x as the exact bf16 image of the activation quantizer, so every product is exact in fp32;
// only the fp32 accumulation order differs from the reference's torch.matmul.  Here: the scratch size and the two dispatchers.
#include "xa_common.h"

namespace lqer {
size_t xa_scratch_bytes(int64_t m_max, int64_t K, int64_t rp) {
  // split-K plan: row_groups * nchunk <= XA_TARGET_WAVES + row_groups for every M <= m_max;
  // fused plan (k_quant_xa16): row_groups * ceil(Kp / 256) partial tiles
  const int64_t rg = (m_max + XA_ROWS - 1) / XA_ROWS;
  const int64_t split = XA_TARGET_WAVES + rg;
  const int64_t fused = rg * ((lqer_padded_k(K) + QX_K - 1) / QX_K);
  return (size_t)(split > fused ? split : fused) * XA_ROWS * rp * sizeof(float);
}
static size_t partial_bytes(const XaPlan& plan, int rp) { return (size_t)plan.nchunk * plan.row_groups * XA_ROWS * rp * sizeof(float); }

// Fused activation quantize + side path.  Returns LQER_E_UNSUPPORTED (without launching) when the shape or
// formats are outside what the fused kernels cover; the caller then runs the two separate steps.
int quant_xa_fused_dispatch(const void* x, int dtype, int64_t M, int64_t K, int64_t ldx, const QP& qx, bf16_t* xq,
                            const bf16_t* a_t, int a_limbs, int64_t r, const QP& qa, bf16_t* xaq, float* scratch,
                            size_t scratch_bytes, hipStream_t st) {
  const int64_t Kp = lqer_padded_k(K);
  const int rp = (int)lqer_padded_r(r);
  if (qx.kind != LQER_Q_MXINT || qx.block != 16 || qx.mbits > 8 || rp > 128 || qa.kind != LQER_Q_MXINT || qa.mbits > 8)
    return LQER_E_UNSUPPORTED;
  const int La = xa_out_block(qa, rp);
  if (rp % La != 0 || !xa_reduce4_block(La)) return LQER_E_UNSUPPORTED;
  if (M == 0) return LQER_OK;
  XaPlan plan;
  int rc;
  if (rp > 64) {
    // rank 65..128: 64-row tiles, both MFMA operands through LDS (xal::k_quant_xa128), the chunks of the LDS-staged side GEMM
    const int64_t ldx_b = ldx * 2;
    if (rp % 32 != 0 || a_limbs != 1 || M < 512 || dtype == LQER_F32 || K % 8 != 0 || (uintptr_t)x % 16 != 0 || ldx_b % 16 != 0 ||
        xal::ROWS * ldx_b >= 0x40000000)
      return LQER_E_UNSUPPORTED;
    plan = xa_plan(M, Kp);
    const xal::Chunks c = xal::chunks(M, xal::QROWS, Kp * 2, plan.nchunk);
    plan.nchunk = c.nch;
    if (!scratch || scratch_bytes < partial_bytes(plan, rp)) return LQER_E_UNSUPPORTED;
    rc = xal::launch_q(dtype, rp, x, M, K, ldx_b, qx, xq, Kp, a_t, plan.row_groups, c, scratch, st);
  } else {
    plan = {(int)((M + XA_ROWS - 1) / XA_ROWS), (int)((Kp + QX_K - 1) / QX_K), QX_K};  // one partial tile per row group and QX_K
    if (!scratch || scratch_bytes < partial_bytes(plan, rp)) return LQER_E_UNSUPPORTED;  // sized for the unfused plan: fall back
    rc = quant_xa16_launch(x, dtype, M, K, ldx, qx, xq, Kp, a_t, a_limbs, rp, plan, scratch, st);
  }
  if (rc || !xaq) return rc;  // (xaq == nullptr: the consumer reduces the partial tiles itself)
  xa_reduce_launch(scratch, plan, rp, qa, 0, xaq, nullptr, st);
  return check_launch("quantize_act_xa");
}

// x_limbs: the activation image holds that many bf16 limbs side by side ([Mp][x_limbs * Kp], act_limbs.hip) and a_t
// is repeated as often along k; xa_limbs: limbs of the result when A_out is a pass-through (0 otherwise).
// x_limbs = 0: xq holds fp16 bits and a_t is ONE fp16 image [rp][Kp] (pack.hip::a_f16_dispatch) - v_mfma_*_f16.
// x_limbs = -1: xq holds int8 mantissas [Mp][lqer_padded_k8(K)] with the row scales behind them (the int8 route).
int lowrank_xa_dispatch(const bf16_t* xq, int64_t M, int64_t K, int x_limbs, const bf16_t* a_t, int a_limbs, int64_t r,
                        const QP& q, int xa_limbs, bf16_t* xaq, float* scratch, size_t scratch_bytes, hipStream_t st) {
  const bool x_f16 = x_limbs == 0;
  const bool x_i8 = x_limbs == -1;
  const bool a_f16 = x_i8 && a_limbs == -1;  // int8 mantissas x ONE fp16 image of A^T (lqer_f16_prepare) on the fp16 MFMA
  if (x_f16 || a_f16) a_limbs = 1;
  if (x_f16 || x_i8) x_limbs = 1;
  const int64_t Kp = lqer_padded_k(K) * x_limbs;
  const int64_t Kx = x_i8 ? padded_k8(K) : Kp;  // row stride of the activation image (elements)
  const float* rowscale = x_i8 ? i8_row_scales(xq, M, K) : nullptr;
  const int rp = (int)lqer_padded_r(r);
  const bool pass = q.kind == LQER_Q_PASSTHROUGH;
  const bool fixed = q.kind == LQER_Q_INT;  // (integer: the reduce pass quantizes with the pinned exponent, common.h)
  const bool mf = q.kind == LQER_Q_MINIFLOAT;  // (minifloat: elementwise, k_xa_reduce4<1, true>)
  if (pass ? (xa_limbs != 2 && xa_limbs != 3)
           : !((q.kind == LQER_Q_MXINT && q.mbits <= 8) || (fixed && q.mmax <= 256.f && q.mneg <= 256.f) || (mf && q.width <= 8))) {
    set_error("A_out_quantizer must be block_fp or integer with codes up to 256 (a bf16 image), minifloat, or passthrough with 2 or 3 "
              "limbs, on the HIP path (got kind %d width %d)", q.kind, q.width);
    return LQER_E_UNSUPPORTED;
  }
  const int L = pass ? 4 : xa_out_block(q, rp);
  if (rp % L != 0 || L % 2 != 0) {
    set_error("A_out_quantizer block %d does not tile the padded rank %d", q.block, rp);
    return LQER_E_UNSUPPORTED;
  }
  if (rp > 32 * XA_MAX_TILES) {
    set_error("rank %d > %d not supported", (int)r, 32 * XA_MAX_TILES);
    return LQER_E_UNSUPPORTED;
  }
  if (M == 0) return LQER_OK;
  XaPlan plan = xa_plan(M, Kp);
  if (!scratch || scratch_bytes < partial_bytes(plan, rp)) {
    set_error("lowrank_xa: scratch %zu B < %zu B", scratch_bytes, partial_bytes(plan, rp));
    return LQER_E_WORKSPACE;
  }
  // the LDS-staged kernel (xal): the int8 route's images at any rank tile count up to 2; the bf16 image x one bf16 limb of A^T
  // for ranks beyond the fused quantizer's (rank 65..128: the OPT configurations)
  const bool lds_i8 = a_f16 && (rp == 32 || rp == 64) && Kx % xal::BKB == 0;
  const bool lds_b16 = !x_f16 && !x_i8 && x_limbs == 1 && a_limbs == 1 && rp % 32 == 0 && rp > 64 && rp <= 128;
  if ((lds_i8 || lds_b16) && M >= 512) {
    const int64_t x_ld = lds_i8 ? Kx : Kp * 2;  // bytes per activation row (both zero-padded to whole 128-byte steps)
    const xal::Chunks c = xal::chunks(M, xal::ROWS, x_ld, plan.nchunk);
    const int rc = xal::launch(lds_i8, rp, xq, x_ld, a_t, Kp, plan.row_groups, c, scratch, st);
    if (rc) return rc;
    plan.nchunk = c.nch;  // (what the reduce pass sums)
  } else {
    xa_partial_launch(xq, M, Kp, Kx, x_f16 || a_f16, x_i8, a_t, a_limbs, rp, plan, scratch, st);
  }
  xa_reduce_launch(scratch, plan, rp, q, xa_limbs, xaq, rowscale, st);
  return check_launch("lowrank_xa");
}

}  // namespace lqer
