// What the kernel families of the rank-r side path share (overview: lowrank_xa.hip): the split-K plan, the int8 -> bf16 / fp16 fragment
// converters, and each family's host launcher - a kernel is instantiated in the one file that defines it and reached through these.
#pragma once
#include <type_traits>

#include "gemm_tile.h"  // lds_void

namespace lqer {

constexpr int XA_ROWS = 32, XA_MAX_TILES = 8;  // token rows per wave; 32-column tiles of the padded rank at most (rp <= 256)
constexpr int XA_TARGET_WAVES = 2048;  // (row group, K chunk) pieces the split-K plan aims for
constexpr int QX_K = 256;              // k per workgroup of the fused quantize + side-GEMM kernel (k_quant_xa16)
constexpr int QX_WAVES = QX_K / 64;    // one wave per 64 k; QX_K threads, two 16-element blocks each

struct XaPlan {
  int row_groups, nchunk, kc;  // kc = k per chunk (multiple of 64)
};
__host__ __device__ inline XaPlan xa_plan(int64_t M, int64_t Kp) {
  XaPlan p;
  p.row_groups = (int)((M + XA_ROWS - 1) / XA_ROWS);
  const int windows = (int)(Kp / 64);
  int want = p.row_groups > 0 ? (XA_TARGET_WAVES + p.row_groups - 1) / p.row_groups : 1;
  if (want < 1) want = 1;
  if (want > windows) want = windows;
  const int wpc = (windows + want - 1) / want;  // 64-k windows per chunk
  p.kc = wpc * 64;
  p.nchunk = (windows + wpc - 1) / wpc;
  return p;
}

// columns per A_out block of a padded rank (one block per row where the format names none); k_xa_reduce4 takes 4 * 2^g <= 256 of them
inline int xa_out_block(const QP& q, int rp) { return (q.block <= 0 || q.block >= rp) ? rp : q.block; }
inline bool xa_reduce4_block(int L) { return L % 4 == 0 && ((L / 4) & (L / 4 - 1)) == 0 && L / 4 <= 64; }

// f(std::integral_constant<int, V>) for the listed V that v equals (the caller has checked that one does), in the style of with_dtype
template <int... V, class F>
int with_int(int v, F&& f) {
  int rc = LQER_E_UNSUPPORTED;
  (void)((v == V && (rc = f(std::integral_constant<int, V>{}), true)) || ...);
  return rc;
}

// 32 int8 mantissas of an activation row (a lane's bytes of one 64-k window: lo, hi) as four bf16 fragments (integers up to 127: exact)
__device__ __forceinline__ void i8x32_to_bf16(const u32x4& lo, const u32x4& hi, bf16x8 (&f)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {  // fragment i = bytes 8i .. 8i+7
    const uint32_t w0 = i < 2 ? lo[2 * i] : hi[2 * i - 4], w1 = i < 2 ? lo[2 * i + 1] : hi[2 * i - 3];
    u32x4 r;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const uint32_t w = j ? w1 : w0;
      const float f0 = (float)(int)(int8_t)(w & 0xff), f1 = (float)(int)(int8_t)((w >> 8) & 0xff);
      const float f2 = (float)(int)(int8_t)((w >> 16) & 0xff), f3 = (float)(int)(int8_t)(w >> 24);
      r[2 * j] = (__float_as_uint(f0) >> 16) | (__float_as_uint(f1) & 0xffff0000u);
      r[2 * j + 1] = (__float_as_uint(f2) >> 16) | (__float_as_uint(f3) & 0xffff0000u);
    }
    f[i] = __builtin_bit_cast(bf16x8, r);
  }
}
// the same 32 mantissas as fp16 (XI8 with an fp16 A^T image: the mantissas times an fp16-exact A on v_mfma_*_f16, ONE limb of
// A^T instead of two): byte b -> the half 0x6400 | (b ^ 0x80) = 1024 + (b + 128), minus 1152 - two bytes per v_perm_b32 and
// v_pk_add_f16 instead of three conversions per byte
__device__ __forceinline__ void i8x32_to_f16(const u32x4& lo, const u32x4& hi, bf16x8 (&f)[4]) {
  typedef __attribute__((ext_vector_type(2))) _Float16 h2;
  const h2 bias = {(_Float16)-1152.0f, (_Float16)-1152.0f};
#pragma unroll
  for (int i = 0; i < 4; ++i) {  // fragment i = bytes 8i .. 8i+7
    const uint32_t w0 = i < 2 ? lo[2 * i] : hi[2 * i - 4], w1 = i < 2 ? lo[2 * i + 1] : hi[2 * i - 3];
    u32x4 r;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const uint32_t t = (j ? w1 : w0) ^ 0x80808080u;
      const h2 a = __builtin_bit_cast(h2, __builtin_amdgcn_perm(0x64646464u, t, 0x04010400u)) + bias;  // bytes 0, 1
      const h2 b = __builtin_bit_cast(h2, __builtin_amdgcn_perm(0x64646464u, t, 0x04030402u)) + bias;  // bytes 2, 3
      r[2 * j] = __builtin_bit_cast(uint32_t, a);
      r[2 * j + 1] = __builtin_bit_cast(uint32_t, b);
    }
    f[i] = __builtin_bit_cast(bf16x8, r);
  }
}

// xa_partial.hip: one wave per (RG x 32 rows, K chunk), operands straight from L2 (no check_launch: the reduce launch follows)
void xa_partial_launch(const bf16_t* xq, int64_t M, int64_t Kp, int64_t Kx, bool x_f16, bool x_i8, const bf16_t* a_t, int a_limbs, int rp,
                       const XaPlan& plan, float* part, hipStream_t st);
// xa_staged.hip: both operands through LDS, tiles of token rows x K chunks of whole 128-byte steps
namespace xal {
constexpr int ROWS = 128, BKB = 128;  // token rows per workgroup, activation bytes per row and step
// ... of the fused quantizer: 64-row tiles x twice the K per chunk - half the partial tiles to write and to reduce (-1.3 .. -1.7 us
// per rank-96 / 128 forward at K = 4096 against 128-row tiles; +-0 at K = 16384)
constexpr int QROWS = 64;
struct Chunks { int tiles, nch, spc, steps_total; };  // row tiles, K chunks, steps per chunk, steps of a row
Chunks chunks(int64_t M, int tile_rows, int64_t row_bytes, int max_chunks);
// rp = 32 NT: NT = 1, 2 with int8 mantissas x one fp16 image of A^T (i8), NT = 3, 4 with the bf16 image x one bf16 limb
int launch(bool i8, int rp, const void* xq, int64_t x_ld, const bf16_t* a_img, int64_t Kp, int row_groups, const Chunks& c, float* part,
           hipStream_t st);
// the same with the activation quantizer in front (dtype: LQER_F16 or LQER_BF16; rp = 96 or 128)
int launch_q(int dtype, int rp, const void* x, int64_t M, int64_t K, int64_t ldx_b, const QP& q, bf16_t* xq, int64_t Kp, const bf16_t* a_img,
             int row_groups, const Chunks& c, float* part, hipStream_t st);
}  // namespace xal
// quant_xa16.hip: activation quantizer (blocks of 16) + the partial tiles of one 256-k chunk per workgroup, rp <= 64
int quant_xa16_launch(const void* x, int dtype, int64_t M, int64_t K, int64_t ldx, const QP& q, bf16_t* xq, int64_t Kp, const bf16_t* a_t,
                      int a_limbs, int rp, const XaPlan& plan, float* part, hipStream_t st);
// xa_reduce.hip: fixed-order sum of the partial tiles + A_out (xa_limbs: limbs of a pass-through's result; rowscale: the int8
// image's row scales or nullptr) -> the bf16 image the GEMM's prologue reads.  The caller checks the launch.
void xa_reduce_launch(const float* part, const XaPlan& plan, int rp, const QP& q, int xa_limbs, bf16_t* xaq, const float* rowscale,
                      hipStream_t st);

}  // namespace lqer
