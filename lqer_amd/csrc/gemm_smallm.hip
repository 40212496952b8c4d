// Small-M (decode) variant of the fused W4 x A8 Linear kernel, M <= 64 tokens:
//
//   y[m,n] = sum_k xq[m,k] * Wq[n,k]  +  bq[n]  +  Q_Bout( sum_j xAq[m,j] * B[j,n] )
//
// (reference quantized_layers/linear.py:155-156, same arithmetic as gemm_w4a8.hip).  At these sizes the
// packed weight (0.56 B per element) is the only large operand and the kernel is HBM-bound on it, so the
// tile kernel's 128-row tiles would leave all but N/256 CUs idle.  Here ONE workgroup owns one panel row =
// 16 output columns x all of K: nk panels of 576 B that are contiguous in the packed image, streamed straight
// into registers (no LDS staging: nothing is reused across waves) by 8 waves that take every 8th panel;
// N/16 workgroups (256 for N = 4096) put every CU on the stream.
//
// Arithmetic: v_mfma_f32_16x16x32_bf16, A operand = 16 weight rows x 32 k (lane: row l & 15, k 8 (l >> 4) ..+8 =
// exactly one 32-bit word of 4-bit codes -> one expand per MFMA), B operand = 16 tokens x 32 k from the bf16
// activation image (L2-resident: M x K x 2 B), D = 16 (n) x 16 (token) fp32, lane: token l & 15, n 4 (l >> 4) + j.
// A B_out block (16 consecutive n of a token) is the 4 registers of the 4 lanes l, l^16, l^32, l^48.
// The 8 waves' partial sums are added in a fixed order through LDS (bit-reproducible); wave 0 adds the side
// path (MFMA straight from global memory, re-quantized in registers), the bias, and stores.
// SmPanel, SmLane (the lane's place in a panel), sm_expand and quad16_max come from smallm_tile.h, shared with decode1.hip.
#include "gemm_plan.h"
#include "smallm_tile.h"

namespace lqer {

constexpr int SM_NW = 8;       // waves per workgroup: wave w takes panels w, w + 8, ...
template <int MT> struct SmUnr { static constexpr int v = MT <= 2 ? 4 : 2; };  // panels per register buffer (two buffers)

// W: 0 - the standard 4-bit image; 2, 3 - the compact image of a weight of that width (w_narrow.h), read directly: other loads and
// another expand, the same panels on the same waves in the same order, so the same sums.
// The kernel's body, inlined into both kernels below (the standard image's keeps its name and its four template arguments).
template <int DT, bool LOWRANK, int BOUT, int MT, int W>
__device__ __forceinline__ void smallm_body(const GemmArgs& g) {
  constexpr bool XF16 = DT == LQER_F16X;  // fp16 activation image and fp16 weight fragments in the main loop (gemm_w4a8.hip)
  __shared__ __attribute__((aligned(16))) float red[(SM_NW - 1) * MT * 4 * 64];
  __shared__ __attribute__((aligned(16))) bf16_t xaq_l[LOWRANK ? MT * 16 * 64 : 8];  // [token][rp <= 64]: x A after A_out (partials mode)
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const SmLaneT<W> ln(lane, g.w_narrow & 0xff);
  const int row = ln.row, q = ln.q;  // weight row / token within the tile; k group
  const int n0 = blockIdx.x * 16;
  const int nk = g.Kp / 64;
  const uint8_t* prow = g.wp + (int64_t)blockIdx.x * nk * ln.panel_bytes;

  f32x4 acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  // wave 0 fetches the first side-path fragments (limb 0, rank entries 0..31) now, under the weight stream
  const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  bf16x8 sp_b = zero8, sp_x[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) sp_x[t] = zero8;
  const bool from_partials = LOWRANK && g.xa_part != nullptr;
  if (LOWRANK && wave == 0 && g.b_limbs > 0 && 8 * q < g.rp) {
    sp_b = *(const bf16x8*)(g.bt + (int64_t)(n0 + row) * g.rp + 8 * q);
    if (!from_partials) {
#pragma unroll
      for (int t = 0; t < MT; ++t)
        if (t * 16 + row < g.M) sp_x[t] = *(const bf16x8*)(g.xaq + (int64_t)(t * 16 + row) * g.xaq_ld + 8 * q);
    }
  }
  auto load_panel = [&](int kt, SmPanelT<W>& p, bf16x8 (&x)[MT][2]) {
    const uint8_t* pp = prow + (int64_t)kt * ln.panel_bytes;
    if constexpr (W == 0) {
      p.cw = *(const u32x4*)(pp + ln.codes_off);
    } else {
      p.cw = *(const uint32_t*)(pp + ln.codes_off);
      if constexpr (W == 3) p.sg = *(const uint32_t*)(pp + ln.signs_off);
    }
    p.ex = *(const uint32_t*)(pp + ln.exps_off);
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      // token rows beyond M load nothing: the activation image (M x K x 2 B, read by every workgroup from L2) is
      // the larger stream of this kernel; their output columns are never stored
      x[t][0] = x[t][1] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
      if (t * 16 + row < g.M) {
        const bf16_t* xr = g.xq + (int64_t)(t * 16 + row) * g.Kp + kt * 64 + 8 * q;
        x[t][0] = *(const bf16x8*)xr;
        x[t][1] = *(const bf16x8*)(xr + 32);
      }
    }
  };
  auto compute_panel = [&](const SmPanelT<W>& p, const bf16x8 (&x)[MT][2]) {
    bf16x8 wb0, wb1;
    sm_expand<XF16, W>(p, ln, wb0, wb1);
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      acc[t] = mfma_16x16x32<XF16>(wb0, x[t][0], acc[t]);
      acc[t] = mfma_16x16x32<XF16>(wb1, x[t][1], acc[t]);
    }
  };

  // wave w takes panels w, w + SM_NW, ...; two register buffers of SM_UNR panels keep 2 x SM_UNR panels of loads in flight
  constexpr int SM_UNR = SmUnr<MT>::v;
  SmPanelT<W> pa[SM_UNR], pb[SM_UNR];
  bf16x8 xa[SM_UNR][MT][2], xb[SM_UNR][MT][2];
  const int per_wave = (nk - wave + SM_NW - 1) / SM_NW;  // panels of this wave
  auto kt_of = [&](int i) { return wave + SM_NW * i; };
  int i = 0;
#pragma unroll
  for (int u = 0; u < SM_UNR; ++u)
    if (u < per_wave) load_panel(kt_of(u), pa[u], xa[u]);
  if constexpr (LOWRANK) {
    if (from_partials) {
      // (after the first weight panels have been requested: the partial tiles' round trip passes under the weight stream's)
      // x A = sum over the split-K chunks, ascending (the order of k_xa_reduce4: same bits as the three-launch route),
      // then A_out in blocks of 16 = 4 consecutive lanes (decode1.hip has the same text, written out in both: as a function it changes device code - profiles/shared_pieces_codeobj.txt, "not taken"); the bf16 image goes to LDS for wave 0's epilogue (it is read
      // after the combine barrier below).  One lane per 4 rank entries; M * rp / 4 <= 1024 items on 512 lanes.
      const int total = g.M * g.rp / 4;
      for (int base = 0; base < total; base += 64 * SM_NW) {
        const int item = base + (int)threadIdx.x;
        const bool live = item < total;
        float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
        if (live) {
          const float* src = g.xa_part + (int64_t)item * 4;
          int c = 0;
          for (; c + 8 <= g.xa_nchunk; c += 8) {
            float4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = *(const float4*)(src + (c + u) * g.xa_cstride);
#pragma unroll
            for (int u = 0; u < 8; ++u) sum.x += v[u].x, sum.y += v[u].y, sum.z += v[u].z, sum.w += v[u].w;
          }
          for (; c < g.xa_nchunk; ++c) {
            const float4 v = *(const float4*)(src + c * g.xa_cstride);
            sum.x += v.x, sum.y += v.y, sum.z += v.z, sum.w += v.w;
          }
        }
        float amax = fmaxf(fmaxf(fabsf(sum.x), fabsf(sum.y)), fmaxf(fabsf(sum.z), fabsf(sum.w)));
        amax = fmaxf(amax, __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(amax), 0xB1, 0xf, 0xf, true)));  // quad_perm [1,0,3,2]
        amax = fmaxf(amax, __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(amax), 0x4E, 0xf, 0xf, true)));  // quad_perm [2,3,0,1]
        if (live) {
          const bool any = amax > 0.f;
          const int e = any ? block_exponent(amax, g.aout) : 0;
          const float v[4] = {sum.x, sum.y, sum.z, sum.w};
          uint32_t w[2];
#pragma unroll
          for (int i = 0; i < 2; ++i) {
            const float q0 = any && fabsf(v[2 * i]) > g.aout.tiny ? mxint_value(v[2 * i], e, g.aout) : 0.f;
            const float q1 = any && fabsf(v[2 * i + 1]) > g.aout.tiny ? mxint_value(v[2 * i + 1], e, g.aout) : 0.f;
            w[i] = exact_bf16_bits(q0) | (exact_bf16_bits(q1) << 16);
          }
          *(uint2*)(xaq_l + item * 4) = make_uint2(w[0], w[1]);
        }
      }
    }
  }

  for (; i < per_wave; i += 2 * SM_UNR) {
#pragma unroll
    for (int u = 0; u < SM_UNR; ++u)
      if (i + SM_UNR + u < per_wave) load_panel(kt_of(i + SM_UNR + u), pb[u], xb[u]);
#pragma unroll
    for (int u = 0; u < SM_UNR; ++u)
      if (i + u < per_wave) compute_panel(pa[u], xa[u]);
#pragma unroll
    for (int u = 0; u < SM_UNR; ++u)
      if (i + 2 * SM_UNR + u < per_wave) load_panel(kt_of(i + 2 * SM_UNR + u), pa[u], xa[u]);
#pragma unroll
    for (int u = 0; u < SM_UNR; ++u)
      if (i + SM_UNR + u < per_wave) compute_panel(pb[u], xb[u]);
  }

  // fixed-order combine: (((w0 + w1) + w2) + ...) + w7
  if (wave > 0) {
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j) red[(((wave - 1) * MT + t) * 4 + j) * 64 + lane] = acc[t][j];
  }
  __syncthreads();
  if (wave != 0) return;
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int w2 = 0; w2 < SM_NW - 1; ++w2) acc[t][j] += red[((w2 * MT + t) * 4 + j) * 64 + lane];

  // ---- side path + bias + store (wave 0): lane = token 16 t + row, output columns n0 + 4 q + j
  const int nq = n0 + 4 * q;
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    if constexpr (LOWRANK) {
      const bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
      if (from_partials && 8 * q < g.rp && t * 16 + row < g.M) sp_x[t] = *(const bf16x8*)(xaq_l + (t * 16 + row) * g.rp + 8 * q);
      if (g.b_limbs > 0) s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(sp_b, sp_x[t], s, 0, 0, 0);  // prefetched
      for (int l = 0; l < g.b_limbs; ++l)
        for (int ks = (l == 0 ? 1 : 0); ks * 32 < g.rp; ++ks) {
          const int j0 = ks * 32 + 8 * q;  // rp is a multiple of 16: the upper half of the last 32 may lie beyond it
          bf16x8 bb = zero, xv = zero;
          if (j0 < g.rp) {
            bb = *(const bf16x8*)(g.bt + ((int64_t)l * g.Np + n0 + row) * g.rp + j0);
            if (t * 16 + row < g.M)
              xv = from_partials ? *(const bf16x8*)(xaq_l + (t * 16 + row) * g.rp + j0)
                                 : *(const bf16x8*)(g.xaq + (int64_t)(t * 16 + row) * g.xaq_ld + j0);
          }
          s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bb, xv, s, 0, 0, 0);
        }
      if constexpr (BOUT == 1) {  // (the same text as decode1.hip's epilogue, written out in both: as a function it changes device code - profiles/shared_pieces_codeobj.txt, "not taken")
        float amax = fmaxf(fmaxf(fabsf(s[0]), fabsf(s[1])), fmaxf(fabsf(s[2]), fabsf(s[3])));
        amax = quad16_max(amax);
        const int e = block_exponent(amax, g.bout);  // amax = 0: every element takes the pass-through
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] = fabsf(s[j]) <= 1e-8f ? s[j] : mxint_value(s[j], e, g.bout);
      }
    }
    // same association as the tile kernel: the side path and the bias form the initial accumulator
    float out[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) out[j] = (s[j] + (g.bias ? g.bias[nq + j] : 0.f)) + acc[t][j];
    const int m = t * 16 + row;
    if (m < g.M) store_row4<DT>(g.y, (int64_t)m * g.ldy + nq, nq, g.N, out);
  }
}

template <int DT, bool LOWRANK, int BOUT, int MT>
__global__ __launch_bounds__(64 * SM_NW) void k_lqer_gemm_smallm(GemmArgs g) {
  smallm_body<DT, LOWRANK, BOUT, MT, 0>(g);
}
// ... reading the compact image of a weight of W = 2 or 3 bits
template <int DT, bool LOWRANK, int BOUT, int MT, int W>
__global__ __launch_bounds__(64 * SM_NW) void k_lqer_gemm_smallm_narrow(GemmArgs g) {
  smallm_body<DT, LOWRANK, BOUT, MT, W>(g);
}

template <int DT, bool LR, int BO, int MT, int W>
static int run_smallm_mt(const GemmPlan& p, const GemmArgs& g, hipStream_t st) {
  if constexpr (W == 0) return launch_k<k_lqer_gemm_smallm<DT, LR, BO, MT>>("lqer_gemm_smallm", p.grid, 64 * SM_NW, 0, st, g);
  else return launch_k<k_lqer_gemm_smallm_narrow<DT, LR, BO, MT, W>>("lqer_gemm_smallm (compact image)", p.grid, 64 * SM_NW, 0, st, g);
}

template <int DT, bool LR, int BO, int W>
static int run_smallm(const GemmPlan& p, const GemmArgs& g, hipStream_t st) {
  switch (p.mt) {  // 16-row token tiles
    case 1: return run_smallm_mt<DT, LR, BO, 1, W>(p, g, st);
    case 2: return run_smallm_mt<DT, LR, BO, 2, W>(p, g, st);
    case 3: return run_smallm_mt<DT, LR, BO, 3, W>(p, g, st);
    default: return run_smallm_mt<DT, LR, BO, 4, W>(p, g, st);
  }
}

template <int DT, int W>
static int launch_smallm_w(const GemmPlan& p, const GemmArgs& g, hipStream_t st) {
  if (!p.lowrank) return run_smallm<DT, false, 0, W>(p, g, st);
  return p.bout == 1 ? run_smallm<DT, true, 1, W>(p, g, st) : run_smallm<DT, true, 0, W>(p, g, st);
}

template <int DT>
static int launch_smallm(const GemmPlan& p, const GemmArgs& g, hipStream_t st) {
  switch (p.w_img) {  // the image the kernel reads: the plan's (0: standard; 2, 3: compact, of that width)
    case 0: return launch_smallm_w<DT, 0>(p, g, st);
    case 2: return launch_smallm_w<DT, 2>(p, g, st);
    case 3: return launch_smallm_w<DT, 3>(p, g, st);
  }
  set_error("lqer_gemm_smallm: no instantiation for a compact image of width %d", p.w_img);
  return LQER_E_UNSUPPORTED;
}

int smallm_launch(const GemmPlan& p, const GemmArgs& g, int dtype, hipStream_t st) {
  return with_dtype(dtype, [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    if constexpr (DT == LQER_F16)
      if (p.f16x) return launch_smallm<LQER_F16X>(p, g, st);
    return launch_smallm<DT>(p, g, st);
  });
}

}  // namespace lqer
