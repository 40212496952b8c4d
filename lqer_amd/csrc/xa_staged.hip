// Side GEMM x A with both operands staged through LDS (prefill sizes), and the same with the activation quantizer in front.
// k_xa_partial reads both operands with one 16-byte load per lane and ROW: 32-64 different cache lines per wave instruction.
// Counters (tools/r03_sidepmc.sh, C4): the texture addresser is busy for the kernel's whole duration, stalled on the L1 tag
// lookups (TA_BUSY ~ 84 k of ~90 k cycles, TA_ADDR_STALLED_BY_TC 18.5 M summed) - 84 MB of activations move at 1.7-2.2 TB/s.
// Here a workgroup (4 waves) owns 128 token rows x one K chunk and walks it in steps of 128 BYTES of activation row: the
// step's activation tile (128 rows x 128 B) and A^T slab arrive by LDS-DMA in whole 128-byte lines, three slots, two steps
// ahead (source-side XOR swizzles: fragment reads are conflict-free); wave w multiplies rows 32 w .. 32 w + 31.  Two operand
// formats:
//   I8  (the W4A8 INT configurations): int8 mantissas (128 k per step) x ONE fp16 image of A^T (256 B per rank row and step),
//       v_mfma_f32_32x32x16_f16 after the byte -> half conversion of k_xa_partial;
//   B16 (block_fp activations, rank > 64 - the OPT configurations): the bf16 activation image (64 k per step) x one bf16
//       limb of A^T (128 B per rank row and step), v_mfma_f32_32x32x16_bf16.
// Same partial-tile layout as k_xa_partial (the reduce kernels do not change); the k order inside a step is permuted the same
// way for both operands.
#include "xa_common.h"

namespace lqer::xal {
constexpr int X_SLOT = ROWS * BKB;  // 16 KiB
constexpr int a_row_bytes(bool i8) { return i8 ? 256 : 128; }
constexpr int NS = 3, AHEAD = NS - 1;  // ring slots; steps in flight ahead of the one being multiplied (a fourth slot - 96 KB per CU
                                       // in flight - measured +-0 at C4 and C5: tools/ab_xa.py)
constexpr int lds_bytes(int nt, bool i8) { return NS * (X_SLOT + 32 * nt * a_row_bytes(i8)); }

template <int NT, bool I8>  // 32-column rank tiles: rp = 32 NT
__global__ __launch_bounds__(256) void k_xa_partial_lds(const uint8_t* __restrict__ xq, int64_t x_ld, const bf16_t* __restrict__ a_img,
                                                        int64_t Kp, int row_groups, int nchunk, int steps_per_chunk, int steps_total,
                                                        float* __restrict__ part) {
  constexpr int RP = 32 * NT, AROW = a_row_bytes(I8), A_SLOT = RP * AROW, SLOT = X_SLOT + A_SLOT;
  constexpr int APR = 1024 / AROW;        // A^T rows per 1-KiB piece (4 or 8)
  constexpr int NA = RP / APR / 4;        // A^T pieces per wave and step
  constexpr int ACH = AROW / 16;          // 16-byte chunks per A^T row and step (16 or 8)
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r31 = lane & 31, h = lane >> 5;
  const int tile = blockIdx.x / nchunk, c = blockIdx.x - tile * nchunk;
  const int s_begin = c * steps_per_chunk;
  const int s_end = s_begin + steps_per_chunk < steps_total ? s_begin + steps_per_chunk : steps_total;
  const uint32_t lds0 = (uint32_t)(uintptr_t)(lds_void*)smem;
  // staging: wave w brings rows 32 w .. 32 w + 31 of the activation tile (4 pieces of 8 rows x 128 B) and NA pieces of A^T
  // (x_ld: bytes per activation row)
  const auto x_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)(xq + (int64_t)tile * ROWS * x_ld), 0, (int)(ROWS * x_ld), 0x00020000);
  const auto a_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)a_img, 0, (int)(RP * Kp * 2), 0x00020000);
  int x_voff[4], a_voff[4];  // (NA entries used: an array sized by a template-dependent constant, captured by a lambda, makes hipcc's
                             // HOST pass drop the kernel's stub without a diagnostic - gemm_w4a8.hip has the same note)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = wave * 32 + i * 8 + (lane >> 3);
    x_voff[i] = row * (int)x_ld + (((lane & 7) ^ ((row >> 1) & 7)) << 4);
    a_voff[i] = 0;
  }
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    if constexpr (I8) {  // 4 rows x 256 B per piece, 16 chunks per row
      const int row = 4 * (wave * NA + i) + (lane >> 4);
      a_voff[i] = row * (int)Kp * 2 + (((lane & 15) ^ (row & 15)) << 4);
    } else {             // 8 rows x 128 B per piece: the activation tile's swizzle
      const int row = 8 * (wave * NA + i) + (lane >> 3);
      a_voff[i] = row * (int)Kp * 2 + (((lane & 7) ^ ((row >> 1) & 7)) << 4);
    }
  }
  auto issue = [&](int st) {
    const int slot = st % NS;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(x_rsrc, (lds_void*)(smem + slot * SLOT + (wave * 4 + i) * 1024), 16, x_voff[i], st * BKB, 0, 0);
#pragma unroll
    for (int i = 0; i < NA; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(a_rsrc, (lds_void*)(smem + slot * SLOT + X_SLOT + (wave * NA + i) * 1024), 16, a_voff[i],
                                               st * AROW, 0, 0);
  };
  // fragment addresses (slot 0): activation row 32 w + r31, 16-byte chunk 2 j + h; A^T row n = 32 t + r31: I8 chunks 4 j + 2 h (+ 1),
  // B16 chunk 2 j + h
  const int xrow = wave * 32 + r31;
  uint32_t xa[4], aa[4][4][2];  // (NT tiles, I8: two reads per (tile, j))
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    xa[j] = lds0 + xrow * 128 + (((2 * j + h) ^ ((xrow >> 1) & 7)) << 4);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int n = 32 * t + r31;
      if constexpr (I8) {
#pragma unroll
        for (int u = 0; u < 2; ++u) aa[t][j][u] = lds0 + X_SLOT + n * 256 + (((4 * j + 2 * h + u) ^ (n & 15)) << 4);
      } else {
        aa[t][j][0] = lds0 + X_SLOT + n * 128 + (((2 * j + h) ^ ((n >> 1) & 7)) << 4);
        aa[t][j][1] = 0;
      }
    }
  }
  static_assert(ACH == (I8 ? 16 : 8), "A^T chunk geometry");
  f32x16 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;
#pragma unroll
  for (int d = 0; d < AHEAD; ++d)
    if (s_begin + d < s_end) issue(s_begin + d);
  typedef __attribute__((ext_vector_type(2))) _Float16 h2;
  const h2 bias = {(_Float16)-1152.0f, (_Float16)-1152.0f};
  for (int st = s_begin; st < s_end; ++st) {
    // own loads of step st landed (the batches of the steps behind it - up to AHEAD - 1 - may stay in flight), then everybody's
    {
      const int younger = s_end - 1 - st < AHEAD - 1 ? s_end - 1 - st : AHEAD - 1;  // (workgroup-uniform)
      static_assert(AHEAD >= 2 && AHEAD <= 4, "counted waits below");
      if (younger >= 3) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * (4 + NA)) : "memory");
      else if (younger == 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * (4 + NA)) : "memory");
      else if (younger == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 + NA) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    asm volatile("s_barrier" ::: "memory");  // (also: every wave has finished its reads of step st - 1, whose slot is filled next)
    if (st + AHEAD < s_end) issue(st + AHEAD);
    const uint32_t so = (uint32_t)((st % NS) * SLOT);
    // (asm: hipcc would put vmcnt(0) in front of LDS reads it can see while an LDS-DMA is in flight; every read's result is
    // pinned behind the lgkmcnt(0) below by a "+v" operand)
    u32x4 xr[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) asm volatile("ds_read_b128 %0, %1" : "=v"(xr[j]) : "v"(xa[j] + so));
    bf16x8 ar[4][4][2];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int u = 0; u < (I8 ? 2 : 1); ++u) asm volatile("ds_read_b128 %0, %1" : "=v"(ar[t][j][u]) : "v"(aa[t][j][u] + so));
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(xr[0]), "+v"(xr[1]), "+v"(xr[2]), "+v"(xr[3]));
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int u = 0; u < (I8 ? 2 : 1); ++u) asm volatile("" : "+v"(ar[t][j][u]));
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if constexpr (I8) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {  // bytes 8 u .. 8 u + 7 of the chunk -> 8 halves (i8x32_to_f16's arithmetic)
          u32x4 f;
#pragma unroll
          for (int d = 0; d < 2; ++d) {
            const uint32_t tb = xr[j][2 * u + d] ^ 0x80808080u;
            f[2 * d] = __builtin_bit_cast(uint32_t, __builtin_bit_cast(h2, __builtin_amdgcn_perm(0x64646464u, tb, 0x04010400u)) + bias);
            f[2 * d + 1] = __builtin_bit_cast(uint32_t, __builtin_bit_cast(h2, __builtin_amdgcn_perm(0x64646464u, tb, 0x04030402u)) + bias);
          }
          const bf16x8 xf = __builtin_bit_cast(bf16x8, f);
#pragma unroll
          for (int t = 0; t < NT; ++t) acc[t] = mfma_32x32x16<true>(xf, ar[t][j][u], acc[t]);
        }
      } else {
        const bf16x8 xf = __builtin_bit_cast(bf16x8, xr[j]);
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = mfma_32x32x16<false>(xf, ar[t][j][0], acc[t]);
      }
    }
  }
  // D layout: col n = lane & 31, row m = (reg & 3) + 8 (reg >> 2) + 4 h.  part[c][rg * 32 + m][n]
  const int rg = tile * 4 + wave;
  if (rg < row_groups) {
    float* dst = part + ((int64_t)c * row_groups + rg) * XA_ROWS * RP;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int e = 0; e < 16; ++e) dst[((e & 3) + 8 * (e >> 2) + 4 * h) * RP + 32 * t + r31] = acc[t][e];
  }
}

// The B16 form of the kernel above with the ACTIVATION QUANTIZER in front of it (block_fp activations in blocks of 16, rank
// 65..128: the OPT configurations and q/k/v groups, which the 32-row fused kernel k_quant_xa16 does not cover - its waves fetch
// their own A^T fragments, 64 KB per workgroup at rank 128).  Instead of an LDS-DMA of the bf16 image, every wave loads the
// 16-bit source of its 32 rows x 64 k (four 16-byte requests per lane and step, 8 lanes per 128-byte line, two steps ahead in
// two register sets), quantizes it - a block of 16 = two neighbouring lanes, the maximum crosses with one DPP - and writes the
// bf16 words both to the step's LDS slot (where the DMA would have put them: same source-side swizzle) and to the image the
// GEMM reads.  One pass over x instead of two launches and a re-read of the image.  vmcnt counts loads, stores and LDS-DMA
// together in issue order (MI355X_MICROARCH.md): behind a step's loads lie the previous step's 4 image stores and the next
// step's 4 + NA requests.
template <int DT, int NT, int WAVES, int TROWS = ROWS>  // WAVES waves share TROWS / 32 row groups x NT rank tiles; TROWS = 128 or 64 token rows
__global__ __launch_bounds__(64 * WAVES) void k_quant_xa128(const uint8_t* __restrict__ x, int64_t M, int64_t K, int64_t ldx_b, QP q,
                                                            uint8_t* __restrict__ xq, int64_t Kp, const bf16_t* __restrict__ a_img,
                                                            int row_groups, int nchunk, int steps_per_chunk, int steps_total,
                                                            float* __restrict__ part) {
  static_assert(DT == LQER_F16 || DT == LQER_BF16, "16-bit sources");
  static_assert(WAVES == 4 || WAVES == 8, "4 or 8 waves");
  static_assert(TROWS == 128 || TROWS == 64, "128- or 64-row tiles");
  constexpr int XS = TROWS * BKB;                  // the tile's activation slot
  constexpr int RP = 32 * NT, AROW = 128, A_SLOT = RP * AROW, SLOT = XS + A_SLOT;
  constexpr int XP = (TROWS / 8) / WAVES;          // activation pieces (8 rows x 128 B of image) a wave quantizes per step
  static_assert(XP >= 1, "at most one wave per activation piece");
  constexpr int AP_ALL = RP / 8;                   // A^T pieces (8 rows x 128 B) per step
  constexpr int AP = (AP_ALL + WAVES - 1) / WAVES; // per wave (a wave without a piece of its own repeats another one: same bytes)
  constexpr int NRG = TROWS / 32;                  // 32-row groups of the tile
  constexpr int TG = WAVES / NRG;                  // waves per 32-row group
  constexpr int TW = (NT + TG - 1) / TG;           // rank tiles per wave
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r31 = lane & 31, h = lane >> 5;
  const int tile = blockIdx.x / nchunk, c = blockIdx.x - tile * nchunk;
  const int s_begin = c * steps_per_chunk;
  const int s_end = s_begin + steps_per_chunk < steps_total ? s_begin + steps_per_chunk : steps_total;
  const uint32_t lds0 = (uint32_t)(uintptr_t)(lds_void*)smem;
  const int64_t row0 = (int64_t)tile * TROWS;
  const int rows_here = (int)(M - row0 < TROWS ? M - row0 : TROWS);  // (>= 1: the grid has ceil(M / TROWS) tiles)
  auto make_rs = [](const uint8_t* base, uint32_t range) {
    const unsigned long long b64 = (unsigned long long)base;
    return (u32x4){(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)b64),
                   (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(b64 >> 32)) & 0xffffu,
                   (uint32_t)__builtin_amdgcn_readfirstlane((int)range), 0x00020000u};
  };
  // rows of the tile beyond M read as zeros through the range check; the image has its padded rows
  const u32x4 x_rs = make_rs(x + row0 * ldx_b, (uint32_t)(rows_here * ldx_b));
  const u32x4 q_rs = make_rs(xq + row0 * Kp * 2, (uint32_t)(TROWS * Kp * 2));
  const auto a_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)a_img, 0, (int)(RP * Kp * 2), 0x00020000);
  int gx_voff[4], qs_voff[4], kc[4], a_voff[4], a_piece[4];
  uint32_t ldw[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int piece = wave * XP + (i < XP ? i : 0);
    const int row = piece * 8 + (lane >> 3);
    const int cs = (lane & 7) ^ ((row >> 1) & 7);  // the source chunk this lane's LDS position holds (k_xa_partial_lds's swizzle)
    gx_voff[i] = row * (int)ldx_b + cs * 16;
    qs_voff[i] = row * (int)Kp * 2 + cs * 16;
    kc[i] = cs * 8;
    ldw[i] = lds0 + piece * 1024 + lane * 16;
    a_voff[i] = 0, a_piece[i] = 0;
  }
#pragma unroll
  for (int i = 0; i < AP; ++i) {
    a_piece[i] = (wave + i * WAVES) % AP_ALL;
    const int row = 8 * a_piece[i] + (lane >> 3);
    a_voff[i] = row * (int)Kp * 2 + (((lane & 7) ^ ((row >> 1) & 7)) << 4);
  }
  // Every step issues the requests of step st + 2 - beyond the chunk with out-of-range offsets (zeros, no traffic; the LDS-DMA
  // zero-fills a slot nobody reads) - so that ONE counted wait without a branch around it serves every step: a branch made
  // hipcc copy the destination registers of the loads in front of the wait that retires them.
  auto issue = [&](int st, u32x4& x0, u32x4& x1, u32x4& x2, u32x4& x3) {
    const int slot = st % 3;
    const int oob = st < s_end ? 0 : 0x40000000;  // (the voffset takes part in the range check)
#pragma unroll
    for (int i = 0; i < AP; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(a_rsrc, (lds_void*)(smem + slot * SLOT + XS + a_piece[i] * 1024), 16, a_voff[i] | oob,
                                               st * AROW, 0, 0);
    const int so = __builtin_amdgcn_readfirstlane(st * BKB);
    if constexpr (XP == 4)
      asm volatile("buffer_load_dwordx4 %0, %4, %8, %9 offen\n\tbuffer_load_dwordx4 %1, %5, %8, %9 offen\n\t"
                   "buffer_load_dwordx4 %2, %6, %8, %9 offen\n\tbuffer_load_dwordx4 %3, %7, %8, %9 offen"
                   : "=&v"(x0), "=&v"(x1), "=&v"(x2), "=&v"(x3)
                   : "v"(gx_voff[0] | oob), "v"(gx_voff[1] | oob), "v"(gx_voff[2] | oob), "v"(gx_voff[3] | oob), "s"(x_rs), "s"(so)
                   : "memory");
    else if constexpr (XP == 2)
      asm volatile("buffer_load_dwordx4 %0, %2, %4, %5 offen\n\tbuffer_load_dwordx4 %1, %3, %4, %5 offen"
                   : "=&v"(x0), "=&v"(x1)
                   : "v"(gx_voff[0] | oob), "v"(gx_voff[1] | oob), "s"(x_rs), "s"(so)
                   : "memory");
    else
      asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen" : "=&v"(x0) : "v"(gx_voff[0] | oob), "s"(x_rs), "s"(so) : "memory");
  };
  // fragment reads: activation rows of this wave's 32-row group, rank tiles th * TW .. of the A^T slab
  const int rgi = wave % NRG, th = wave / NRG;
  const int xrow = rgi * 32 + r31;
  uint32_t xa[4], aa[4][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    xa[j] = lds0 + xrow * 128 + (((2 * j + h) ^ ((xrow >> 1) & 7)) << 4);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int tt = th * TW + t < NT ? th * TW + t : NT - 1;  // (a tile slot beyond the rank: re-reads the last one, never stored)
      const int n = 32 * tt + r31;
      aa[t][j] = lds0 + XS + n * 128 + (((2 * j + h) ^ ((n >> 1) & 7)) << 4);
    }
  }
  f32x16 acc[4];  // (TW used; fixed sizes: an array sized by a template constant and captured by a lambda loses the kernel's host stub)
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;
  typedef __attribute__((ext_vector_type(2))) float f2;
  // quantize the lane's 8 values of piece i (step st), write LDS + image
  auto quant_piece = [&](int st, int i, u32x4 wd) {
    const bool valid = st * 64 + kc[i] < K;  // (k beyond K inside the padded step: zeros)
    float v[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t u = valid ? wd[j] : 0u;
      pair_to_f32<DT>(u, v[2 * j], v[2 * j + 1]);
    }
    float amax = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(v[j]));
    // the block's other half lies in lane ^ 1 (chunks 2b, 2b + 1: the swizzle keeps the pair together)
    amax = fmaxf(amax, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(amax), 0xB1, 0xf, 0xf, true)));
    const bool any = amax > 0.f;
    const int e = block_exponent_u(any ? amax : 1.0f, q);
    uint32_t w[4];
    if (__builtin_expect(mxint16_fast_ok(e, q), 1)) {  // (per block, like the standalone quantizer: the two routes differ in the sign of a zero)
      const float sc = __uint_as_float((uint32_t)(127 + q.mbits - e) << 23);
      const float inv = __uint_as_float((uint32_t)(127 + e - q.mbits) << 23);
      const float es = 1e-9f * sc, lo = -q.mneg, hi = q.mmax;
      const f2 magic = {12582912.0f, 12582912.0f};
#pragma unroll
      for (int j = 0; j < 4; ++j) {  // (mxint16_bf16_fast's arithmetic, common.h)
        const f2 xv = {v[2 * j], v[2 * j + 1]};
        const f2 cc = {copysignf(es, xv[0]), copysignf(es, xv[1])};
        f2 r = (__builtin_elementwise_fma(xv, (f2){sc, sc}, cc) + magic) - magic;
        r[0] = __builtin_amdgcn_fmed3f(r[0], lo, hi);
        r[1] = __builtin_amdgcn_fmed3f(r[1], lo, hi);
        const f2 val = r * (f2){inv, inv};
        uint32_t b0 = __float_as_uint(val[0]), b1 = __float_as_uint(val[1]);
        if constexpr (DT != LQER_F16) {  // (fp16 cannot hold a non-zero |x| <= 1e-8)
          b0 = fabsf(xv[0]) <= 1e-8f ? 0u : b0;
          b1 = fabsf(xv[1]) <= 1e-8f ? 0u : b1;
        }
        w[j] = any ? __builtin_amdgcn_perm(b1, b0, 0x07060302u) : 0u;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t b0 = exact_bf16_bits(ldexpf(mxint_mantissa(v[2 * j], e, q), e - q.mbits));
        const uint32_t b1 = exact_bf16_bits(ldexpf(mxint_mantissa(v[2 * j + 1], e, q), e - q.mbits));
        w[j] = any ? (b0 | (b1 << 16)) : 0u;
      }
    }
    const u32x4 wv = {w[0], w[1], w[2], w[3]};
    const int so = __builtin_amdgcn_readfirstlane(st * BKB);
    // (s_nop: a VALU write of the data registers of a > 64-bit store needs a wait state the hazard recogniser cannot add here)
    asm volatile("ds_write_b128 %0, %1\n\tbuffer_store_dwordx4 %1, %2, %3, %4 offen\n\ts_nop 1"
                 :: "v"(ldw[i] + (uint32_t)((st % 3) * SLOT)), "v"(wv), "v"(qs_voff[i]), "s"(q_rs), "s"(so) : "memory");
  };
  auto body = [&](int st, u32x4& x0, u32x4& x1, u32x4& x2, u32x4& x3) {
    // the step's own requests have landed: behind them lie at most the previous step's XP image stores (waited for as well)
    // and the next step's XP + AP requests
    if constexpr (XP == 4) {
      asm volatile("s_waitcnt vmcnt(%[n])" : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3) : [n] "n"(XP + AP) : "memory");
      quant_piece(st, 0, x0), quant_piece(st, 1, x1), quant_piece(st, 2, x2), quant_piece(st, 3, x3);
    } else if constexpr (XP == 2) {
      asm volatile("s_waitcnt vmcnt(%[n])" : "+v"(x0), "+v"(x1) : [n] "n"(XP + AP) : "memory");
      quant_piece(st, 0, x0), quant_piece(st, 1, x1);
    } else {
      asm volatile("s_waitcnt vmcnt(%[n])" : "+v"(x0) : [n] "n"(XP + AP) : "memory");
      quant_piece(st, 0, x0);
    }
    // everybody's words of step st are in the slot (and every wave is past its reads of step st - 1, whose slot is filled next)
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    issue(st + 2, x0, x1, x2, x3);
    const uint32_t so = (uint32_t)((st % 3) * SLOT);
    u32x4 xr[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) asm volatile("ds_read_b128 %0, %1" : "=v"(xr[j]) : "v"(xa[j] + so));
    bf16x8 ar[4][4];
#pragma unroll
    for (int t = 0; t < TW; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j) asm volatile("ds_read_b128 %0, %1" : "=v"(ar[t][j]) : "v"(aa[t][j] + so));
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(xr[0]), "+v"(xr[1]), "+v"(xr[2]), "+v"(xr[3]));
#pragma unroll
    for (int t = 0; t < TW; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j) asm volatile("" : "+v"(ar[t][j]));
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bf16x8 xf = __builtin_bit_cast(bf16x8, xr[j]);
#pragma unroll
      for (int t = 0; t < TW; ++t) acc[t] = mfma_32x32x16<false>(xf, ar[t][j], acc[t]);
    }
  };
  u32x4 p0, p1, p2, p3, q0, q1, q2, q3;  // the two register sets of source chunks in flight (XP of each used)
  issue(s_begin, p0, p1, p2, p3);
  issue(s_begin + 1, q0, q1, q2, q3);
  for (int st = s_begin; st < s_end; st += 2) {
    body(st, p0, p1, p2, p3);
    if (st + 1 < s_end) body(st + 1, q0, q1, q2, q3);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the last image stores and the requests past the chunk)
  const int rg = tile * NRG + rgi;
  if (rg < row_groups) {
    float* dst = part + ((int64_t)c * row_groups + rg) * XA_ROWS * RP;
#pragma unroll
    for (int t = 0; t < TW; ++t) {
      const int tt = th * TW + t;
      if (tt < NT) {
#pragma unroll
        for (int e = 0; e < 16; ++e) dst[((e & 3) + 8 * (e >> 2) + 4 * h) * RP + 32 * tt + r31] = acc[t][e];
      }
    }
  }
}

// K chunks of whole steps for ceil(M / tile_rows) row tiles: about one workgroup per CU (256; 512 measured 10-25 % slower), at most the
// split-K plan's chunks (max_chunks) - fewer, longer chunks than one wave per chunk: less for the reduce pass to read
Chunks chunks(int64_t M, int tile_rows, int64_t row_bytes, int max_chunks) {
  Chunks c;
  c.steps_total = (int)(row_bytes / BKB), c.tiles = (int)((M + tile_rows - 1) / tile_rows);
  int nch = 256 / c.tiles;
  nch = nch < 1 ? 1 : (nch > max_chunks ? max_chunks : nch);
  nch = nch < c.steps_total ? nch : c.steps_total;
  c.spc = (c.steps_total + nch - 1) / nch;
  c.nch = (c.steps_total + c.spc - 1) / c.spc;
  return c;
}

int launch(bool i8, int rp, const void* xq, int64_t x_ld, const bf16_t* a_img, int64_t Kp, int row_groups, const Chunks& c, float* part,
           hipStream_t st) {
  auto run = [&](auto nt, auto i8_c) {
    constexpr int NT = decltype(nt)::value;
    constexpr bool I8 = decltype(i8_c)::value;
    return launch_k<k_xa_partial_lds<NT, I8>>("lowrank_xa", (unsigned)(c.tiles * c.nch), 256, lds_bytes(NT, I8), st, (const uint8_t*)xq, x_ld,
                                              a_img, Kp, row_groups, c.nch, c.spc, c.steps_total, part);
  };
  if (i8) return with_int<1, 2>(rp / 32, [&](auto nt) { return run(nt, std::true_type{}); });
  return with_int<3, 4>(rp / 32, [&](auto nt) { return run(nt, std::false_type{}); });
}

int launch_q(int dtype, int rp, const void* x, int64_t M, int64_t K, int64_t ldx_b, const QP& q, bf16_t* xq, int64_t Kp, const bf16_t* a_img,
             int row_groups, const Chunks& c, float* part, hipStream_t st) {
  return with_int<LQER_F16, LQER_BF16>(dtype, [&](auto dt) {
    return with_int<3, 4>(rp / 32, [&](auto nt) {
      constexpr int DT = decltype(dt)::value, NT = decltype(nt)::value, W = 8;  // (W: waves per workgroup)
      return launch_k<k_quant_xa128<DT, NT, W, QROWS>>("quantize_act_xa", (unsigned)(c.tiles * c.nch), 64 * W, 3 * (QROWS * BKB + 32 * NT * 128), st,
                                                       (const uint8_t*)x, M, K, ldx_b, q, (uint8_t*)xq, Kp, a_img, row_groups, c.nch, c.spc,
                                                       c.steps_total, part);
    });
  });
}

}  // namespace lqer::xal
