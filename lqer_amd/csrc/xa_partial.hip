// Side GEMM x A, split over K, one wave per piece, operands straight from L2: every size the staged and fused kernels do not take.
#include "xa_common.h"

namespace lqer {
// One wave = RG x 32 token rows x one K chunk.  Within a 64-k window lane (r = lane & 31, h = lane >> 5) owns the
// 32 consecutive k at 32h of its rows - one 64-byte load per row - and feeds them to 4 MFMAs in the order it holds
// them (the k order inside a window is a free permutation as long as both operands use the same one).  Every A^T
// fragment (fetched from L2) feeds RG MFMAs: with one row group per wave the A^T stream, rp/32 times the activation
// stream, is the bound.
// XF16: fp16 activation image and fp16 A^T (LQER_Q_PASSTHROUGH_F16).  AFPF: the A^T fragments of the next window are
// requested one window ahead as well (a_limbs * NT <= 4 fragment sets = 64 registers; used for rank <= 64): without it
// every 64-k window waits one L2 latency for them, which - not the activation stream - bounds the kernel at large M
// (16384 x 13824, rank 64, two limbs: 358 -> 326 us for quantizer + side GEMM; no gain at rank 128, where it is off).
// XI8: the activation image holds int8 mantissas ([Mp][Kx] bytes, Kx = the image's row stride; one exponent per row, applied
// to the row's sum by the reduce pass): the lane's 32 bytes of a window are converted to bf16 (integers up to 127: exact).
// PF2 (XI8 with AFPF): the activation loads run TWO windows ahead (two named register stages, the loop unrolled by two) - at
// M = 16384 a wave holds 64 rows x 64 bytes per window, 4 waves per CU: one window ahead leaves 16 KB per CU in flight and the
// HBM latency, not the bandwidth, sets the pace (84 MB in 49 us = 1.7 TB/s).
template <int NT, int RG, bool XF16 = false, bool AFPF = false, bool XI8 = false, bool PF2 = false>
__global__ __launch_bounds__(256) void k_xa_partial(const bf16_t* __restrict__ xq, int64_t M, int64_t Kp, int64_t Kx,
                                                    const bf16_t* __restrict__ a_t, int a_limbs, int rp, XaPlan plan,
                                                    float* __restrict__ part) {
  const int lane = threadIdx.x & 63;
  const int wid = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int wave_rows = (plan.row_groups + RG - 1) / RG;
  if (wid >= wave_rows * plan.nchunk) return;
  const int wr = wid / plan.nchunk, c = wid - wr * plan.nchunk;
  const int r = lane & 31, h = lane >> 5;
  const int64_t k_begin = (int64_t)c * plan.kc;
  const int64_t k_end = k_begin + plan.kc < Kp ? k_begin + plan.kc : Kp;
  f32x16 acc[RG][NT];
#pragma unroll
  for (int u = 0; u < RG; ++u)
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int j = 0; j < 16; ++j) acc[u][t][j] = 0.f;
  const bf16_t* xrow[RG];  // (XI8: a byte pointer - the lane's 32 consecutive k of a window are 32 bytes)
#pragma unroll
  for (int u = 0; u < RG; ++u) {
    const int rg = wr * RG + u < plan.row_groups ? wr * RG + u : plan.row_groups - 1;  // a clamped duplicate is not stored
    const int64_t row = (int64_t)rg * XA_ROWS + r;  // rows past M repeat the last one (never read beyond the tensor: the
    if constexpr (XI8)                              // image may be the caller's own fp16 tensor); their results are unused
      xrow[u] = (const bf16_t*)((const uint8_t*)xq + (row < M ? row : M - 1) * Kx + 32 * h);
    else
      xrow[u] = xq + (row < M ? row : M - 1) * Kx + 32 * h;
  }
  // the next window's activation loads are issued before this window's MFMAs (the stream from HBM is the bound)
  constexpr int NST = PF2 ? 2 : 1;  // register stages of the activation prefetch
  bf16x8 xn[NST][RG][XI8 ? 2 : 4];  // XI8: the raw 32 bytes
  auto load_x = [&](int64_t k0, auto st_c) {
    constexpr int ST = decltype(st_c)::value;
#pragma unroll
    for (int u = 0; u < RG; ++u) {
      if constexpr (XI8) {
#pragma unroll
        for (int i = 0; i < 2; ++i) xn[ST][u][i] = *(const bf16x8*)((const uint8_t*)xrow[u] + k0 + 16 * i);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) xn[ST][u][i] = *(const bf16x8*)(xrow[u] + k0 + 8 * i);
      }
    }
  };
  using std::integral_constant;
  load_x(k_begin, integral_constant<int, 0>{});
  if constexpr (PF2) {
    if (k_begin + 64 < k_end) load_x(k_begin + 64, integral_constant<int, 1>{});
  }
  // (limb, tile) fragment sets held one window ahead; the fp16 image of the int8 route is ONE limb: half the registers
  constexpr int LMAX = AFPF ? ((XF16 && XI8) ? 1 : 4 / NT) : 1;
  constexpr int PAIRS = AFPF ? LMAX * NT : 1;
  bf16x8 afn[PAIRS][4];
  auto load_af = [&](int64_t k0) {
    if constexpr (AFPF) {
#pragma unroll
      for (int l = 0; l < LMAX; ++l)
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const int n = t * 32 + r;
          if (l < a_limbs && n < rp) {
            const bf16_t* arow = a_t + ((int64_t)l * rp + n) * Kp + k0 + 32 * h;
#pragma unroll
            for (int i = 0; i < 4; ++i) afn[l * NT + t][i] = *(const bf16x8*)(arow + 8 * i);
          } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) afn[l * NT + t][i] = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
          }
        }
    }
  };
  load_af(k_begin);
  // one 64-k window out of register stage ST; its stage is refilled NST windows ahead
  auto window = [&](int64_t k0, auto st_c) {
    constexpr int ST = decltype(st_c)::value;
    bf16x8 xf[RG][4];
#pragma unroll
    for (int u = 0; u < RG; ++u) {
      if constexpr (XI8 && XF16) {
        i8x32_to_f16(__builtin_bit_cast(u32x4, xn[ST][u][0]), __builtin_bit_cast(u32x4, xn[ST][u][1]), xf[u]);
      } else if constexpr (XI8) {
        i8x32_to_bf16(__builtin_bit_cast(u32x4, xn[ST][u][0]), __builtin_bit_cast(u32x4, xn[ST][u][1]), xf[u]);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) xf[u][i] = xn[ST][u][i];
      }
    }
    if (k0 + 64 * NST < k_end) load_x(k0 + 64 * NST, st_c);
    if constexpr (AFPF) {
      bf16x8 afc[PAIRS][4];
#pragma unroll
      for (int p = 0; p < PAIRS; ++p)
#pragma unroll
        for (int i = 0; i < 4; ++i) afc[p][i] = afn[p][i];
      if (k0 + 64 < k_end) load_af(k0 + 64);
#pragma unroll
      for (int l = 0; l < LMAX; ++l)
#pragma unroll
        for (int t = 0; t < NT; ++t)
          if (l < a_limbs) {
#pragma unroll
            for (int u = 0; u < RG; ++u)
#pragma unroll
              for (int i = 0; i < 4; ++i) acc[u][t] = mfma_32x32x16<XF16>(xf[u][i], afc[l * NT + t][i], acc[u][t]);
          }
      return;
    }
    for (int l = 0; l < a_limbs; ++l) {
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int n = t * 32 + r;
        bf16x8 af[4];
        if (n < rp) {
          const bf16_t* arow = a_t + ((int64_t)l * rp + n) * Kp + k0 + 32 * h;
#pragma unroll
          for (int i = 0; i < 4; ++i) af[i] = *(const bf16x8*)(arow + 8 * i);
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) af[i] = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
        }
#pragma unroll
        for (int u = 0; u < RG; ++u)
#pragma unroll
          for (int i = 0; i < 4; ++i) acc[u][t] = mfma_32x32x16<XF16>(xf[u][i], af[i], acc[u][t]);
      }
    }
  };
  for (int64_t k0 = k_begin; k0 < k_end; k0 += 64 * NST) {
    window(k0, integral_constant<int, 0>{});
    if constexpr (PF2) {
      if (k0 + 64 < k_end) window(k0 + 64, integral_constant<int, 1>{});
    }
  }
  // D layout: col n = lane & 31, row m = (reg & 3) + 8 (reg >> 2) + 4 h.  part[c][rg*32 + m][n]
#pragma unroll
  for (int u = 0; u < RG; ++u) {
    const int rg = wr * RG + u;
    if (rg < plan.row_groups) {
      float* dst = part + ((int64_t)c * plan.row_groups + rg) * XA_ROWS * rp;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int n = t * 32 + r;
        if (n < rp) {
#pragma unroll
          for (int j = 0; j < 16; ++j) dst[((j & 3) + 8 * (j >> 2) + 4 * h) * rp + n] = acc[u][t][j];
        }
      }
    }
  }
}

// f16: fp16 operands on v_mfma_*_f16 - the fp16 activation image, or int8 mantissas (i8) with ONE fp16 image of A^T
void xa_partial_launch(const bf16_t* xq, int64_t M, int64_t Kp, int64_t Kx, bool f16, bool i8, const bf16_t* a_t, int a_limbs, int rp,
                       const XaPlan& plan, float* part, hipStream_t st) {
  const int nt = (rp + 31) / 32;
  const int rgw = nt <= 4 ? 2 : 1;  // row groups per wave: two while RG x NT accumulator tiles + two activation windows fit the register file
  const int wave_rows = (plan.row_groups + rgw - 1) / rgw;
  const unsigned grid = (unsigned)((wave_rows * plan.nchunk + 3) / 4);
  auto run = [&](auto f16_c, auto i8_c) {
    with_int<1, 2, 3, 4, 5, 6, 7, 8>(nt, [&](auto nt_c) {
      constexpr int NT = decltype(nt_c)::value, RG = NT <= 4 ? 2 : 1;
      constexpr bool XF16 = decltype(f16_c)::value, XI8 = decltype(i8_c)::value;
      if (NT <= 2 && a_limbs * NT <= 4 && plan.kc > 64)  // A^T fragments one window ahead, int8 activations two
        k_xa_partial<NT, RG, XF16, (NT <= 2), XI8, XI8><<<grid, 256, 0, st>>>(xq, M, Kp, Kx, a_t, a_limbs, rp, plan, part);
      else
        k_xa_partial<NT, RG, XF16, false, XI8, false><<<grid, 256, 0, st>>>(xq, M, Kp, Kx, a_t, a_limbs, rp, plan, part);
      return 0;
    });
  };
  if (f16) i8 ? run(std::true_type{}, std::true_type{}) : run(std::true_type{}, std::false_type{});
  else i8 ? run(std::false_type{}, std::true_type{}) : run(std::false_type{}, std::false_type{});
}

}  // namespace lqer
