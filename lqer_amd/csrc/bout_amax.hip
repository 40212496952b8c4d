// The B_out pre-pass of the fused GEMM: the row-block maxima that the tile kernels' BOUT 2 and the int8 kernel read as bout_amax.
// Two kernels (B^T fragments from registers / through LDS), the zero fill of their cells, the scratch size, and launch_amax,
// which gemm_launch.hip calls.
#include <utility>

#include "gemm_plan.h"
#include "gemm_tile.h"

namespace lqer {

// Pre-pass for B_out blocks other than 16 columns: max |xAq @ B| over every (token row, block of L columns),
// L a multiple of 16.  One wave = one 32 x 32 tile of the product (same MFMA orientation as the GEMM
// prologue); the per-16-column maxima are folded into amax[m][n / L] with atomicMax on the fp32 bit pattern
// (non-negative floats order like unsigned integers; max is order-independent, so the result is
// reproducible).  The buffer is zeroed on the stream before this kernel.
// RG 32-row groups per wave (every B^T fragment feeds RG MFMAs), NKS 16-deep slices of the padded rank (exact: no per-slice branch).
// Round 3: the kernel was a chain of load -> vmcnt(0) -> 4 MFMAs per slice (a branch per slice kept hipcc from batching the
// loads; 228 registers: two waves per SIMD) - a third of its MFMA time.  Now a (column tile, limb) BATCH of NKS fragments is
// requested one batch ahead of the MFMAs that consume it (two named register sets), the first MFMA of a tile takes a literal
// zero accumulator, and a lane keeps one running maximum per row group (every register of its accumulator is the same token
// row), folded with v_max3_f32; the lane pair is combined once, at the commit.
template <int RG, int NKS>
__global__ __launch_bounds__(256) void k_bout_amax(GemmArgs g, int tiles_n32, int seg_tiles) {
  // One wave = 32 RG token rows x a run of `seg_tiles` 32-column tiles: the rows' xAq fragments stay in registers, the
  // running maximum of the current B_out block stays in a register and is committed (one atomicMax per row) when
  // the run leaves the block - a handful of atomics per row instead of one per 16 columns.
  const int lane = threadIdx.x & 63;
  const int64_t wid = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t groups = ((g.M + 31) / 32 + RG - 1) / RG;
  const int nseg = (tiles_n32 + seg_tiles - 1) / seg_tiles;
  if (wid >= groups * nseg) return;
  const int tg = (int)(wid / nseg), sg = (int)(wid - (int64_t)tg * nseg);
  const int l31 = lane & 31, lh = lane >> 5;
  const int Mp = (g.M + LQER_M_ALIGN - 1) / LQER_M_ALIGN * LQER_M_ALIGN;  // rows of xaq / bout_amax that exist
  bf16x8 xa[RG][NKS];
  int rowv[RG];
#pragma unroll
  for (int u = 0; u < RG; ++u) {
    const int row = (tg * RG + u) * 32 + l31;
    rowv[u] = row < Mp ? row : -1;
    const int rc = row < Mp ? row : Mp - 1;  // (a clamped duplicate: computed, never committed)
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) xa[u][ks] = *(const bf16x8*)(g.xaq + (int64_t)rc * g.xaq_ld + ks * 16 + 8 * lh);
  }
  const int t_begin = sg * seg_tiles;
  const int t_end = t_begin + seg_tiles < tiles_n32 ? t_begin + seg_tiles : tiles_n32;
  int cur_blk = (t_begin * 32) / g.bout_L;
  float cur[RG];
#pragma unroll
  for (int u = 0; u < RG; ++u) cur[u] = 0.f;
  auto commit = [&]() {
#pragma unroll
    for (int u = 0; u < RG; ++u) {
      const float m = pair32_max(cur[u]);  // lanes l and l ^ 32 hold the two column halves of the same token row
      if (lh == 0 && rowv[u] >= 0) {
        if (g.bout_nseg > 0) g.bout_amax[(int64_t)sg * Mp + rowv[u]] = m;  // one block per row: this segment's partial (plain store)
        else atomicMax((unsigned int*)g.bout_amax + (int64_t)rowv[u] * g.bout_nblk + cur_blk, __float_as_uint(m));
      }
    }
  };
  const f32x16 zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  const int nb = (t_end - t_begin) * g.b_limbs;  // batches: (tile, limb), limb fastest - the GEMM kernels' summation order
  const int64_t limb_stride = (int64_t)g.Np * g.rp;
  const bf16_t* const b_lane = g.bt + (int64_t)l31 * g.rp + 8 * lh;
  bf16x8 ba[NKS], bb[NKS];
  auto load = [&](int i, bf16x8 (&dst)[NKS]) {  // batch i (past the end: the last one again - never used)
    const int ii = i < nb ? i : nb - 1;
    const int tn = t_begin + ii / g.b_limbs, l = ii - (ii / g.b_limbs) * g.b_limbs;
    const bf16_t* p = b_lane + l * limb_stride + (int64_t)tn * 32 * g.rp;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) dst[ks] = *(const bf16x8*)(p + ks * 16);
  };
  f32x16 acc[RG];
  int tn = t_begin, l = 0;
  auto consume = [&](const bf16x8 (&src)[NKS]) {
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      if (l == 0 && ks == 0) {
#pragma unroll
        for (int u = 0; u < RG; ++u) acc[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(src[0], xa[u][0], zero, 0, 0, 0);
      } else {
#pragma unroll
        for (int u = 0; u < RG; ++u) acc[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(src[ks], xa[u][ks], acc[u], 0, 0, 0);
      }
    }
    if (++l == g.b_limbs) {  // the tile's product is complete: fold it into the running maxima
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int blk = (tn * 32 + 16 * b) / g.bout_L;  // wave-uniform
        if (blk != cur_blk) {
          commit();
          cur_blk = blk;
#pragma unroll
          for (int u = 0; u < RG; ++u) cur[u] = 0.f;
        }
#pragma unroll
        for (int u = 0; u < RG; ++u) {
          float m = cur[u];
#pragma unroll
          for (int k = 0; k < 8; k += 2) m = fmaxf(fmaxf(m, fabsf(acc[u][8 * b + k])), fabsf(acc[u][8 * b + k + 1]));  // v_max3_f32 |.|
          cur[u] = m;
        }
      }
      l = 0, ++tn;
    }
  };
  if (nb > 0) load(0, ba);
  for (int i = 0; i < nb; i += 2) {
    load(i + 1, bb);
    consume(ba);
    if (i + 1 >= nb) break;
    load(i + 2, ba);
    consume(bb);
  }
  commit();
}

// The same pre-pass with the B^T fragments through LDS, for rank 64 (the W4A8 INT configurations).  Counters of k_bout_amax<4, 4>
// at C4 (tools/r03_sidepmc.sh): the texture addresser is busy 62 % of the kernel, the MFMA pipe 30 % - every wave fetches its own
// copy of the B^T run, 32 lanes x 128-byte rows per request.  Here the four waves of a workgroup take four different groups of
// 128 token rows over the SAME run of column tiles: a stage of AMX_SB (tile, limb) batches - 4 KB each, contiguous in the B^T
// image - is read once per workgroup with one 16-byte request per thread and batch (16 lanes per 256-byte line), swizzled into
// LDS (two stage buffers, one barrier per stage), and every wave reads its fragments from there.  Same maxima (max is
// order-independent), same commit.
constexpr int AMX_SB = 4;
__global__ __launch_bounds__(256) void k_bout_amax_lds(GemmArgs g, int tiles_n32, int seg_tiles) {
  constexpr int RG = 4, NKS = 4;
  __shared__ __attribute__((aligned(16))) unsigned char sbuf[2][AMX_SB][4096];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, lh = lane >> 5;
  const int64_t groups = ((g.M + 31) / 32 + RG - 1) / RG;
  const int nseg = (tiles_n32 + seg_tiles - 1) / seg_tiles;
  const int wgr = (int)(blockIdx.x / nseg), sg = (int)(blockIdx.x - (int64_t)wgr * nseg);
  const int64_t tg_raw = (int64_t)wgr * 4 + wave;
  const bool live = tg_raw < groups;               // (a wave past the last row group still stages and meets the barriers)
  const int tg = (int)(live ? tg_raw : groups - 1);
  const int Mp = (g.M + LQER_M_ALIGN - 1) / LQER_M_ALIGN * LQER_M_ALIGN;
  bf16x8 xa[RG][NKS];
  int rowv[RG];
#pragma unroll
  for (int u = 0; u < RG; ++u) {
    const int row = (tg * RG + u) * 32 + l31;
    rowv[u] = live && row < Mp ? row : -1;
    const int rc = row < Mp ? row : Mp - 1;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) xa[u][ks] = *(const bf16x8*)(g.xaq + (int64_t)rc * g.xaq_ld + ks * 16 + 8 * lh);
  }
  const int t_begin = sg * seg_tiles;
  const int t_end = t_begin + seg_tiles < tiles_n32 ? t_begin + seg_tiles : tiles_n32;
  int cur_blk = (t_begin * 32) / g.bout_L;
  float cur[RG];
#pragma unroll
  for (int u = 0; u < RG; ++u) cur[u] = 0.f;
  auto commit = [&]() {
#pragma unroll
    for (int u = 0; u < RG; ++u) {
      const float m = pair32_max(cur[u]);
      if (lh == 0 && rowv[u] >= 0) {
        if (g.bout_nseg > 0) g.bout_amax[(int64_t)sg * Mp + rowv[u]] = m;
        else atomicMax((unsigned int*)g.bout_amax + (int64_t)rowv[u] * g.bout_nblk + cur_blk, __float_as_uint(m));
      }
    }
  };
  const f32x16 zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  const int nb = (t_end - t_begin) * g.b_limbs;  // batches (tile, limb), limb fastest
  const int nst = (nb + AMX_SB - 1) / AMX_SB;
  const int64_t limb_stride = (int64_t)g.Np * g.rp;
  // staging: thread t moves 16-byte chunk t of a batch's 4 KB (row t / 8 of the tile, chunk t % 8 of its 128 B) to the swizzled slot
  const int srow = tid >> 3, sch = tid & 7;
  const int sdst = srow * 128 + ((sch ^ (srow & 7)) << 4);
  u32x4 st[AMX_SB];
  auto gload = [&](int s) {
#pragma unroll
    for (int u = 0; u < AMX_SB; ++u) {
      const int i = s * AMX_SB + u, ii = i < nb ? i : nb - 1;  // (past the end: the last batch again, never consumed)
      const int tn = t_begin + ii / g.b_limbs, l = ii - (ii / g.b_limbs) * g.b_limbs;
      st[u] = *(const u32x4*)(g.bt + l * limb_stride + (int64_t)tn * 32 * g.rp + tid * 8);
    }
  };
  auto lwrite = [&](int buf) {
#pragma unroll
    for (int u = 0; u < AMX_SB; ++u) *(u32x4*)(&sbuf[buf][u][sdst]) = st[u];
  };
  int fo[NKS];  // fragment offsets inside a batch: row l31, chunk 2 ks + lh
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) fo[ks] = l31 * 128 + (((2 * ks + lh) ^ (l31 & 7)) << 4);
  f32x16 acc[RG];
  int tn = t_begin, l = 0;
  gload(0);
  lwrite(0);
  __syncthreads();
  for (int s = 0; s < nst; ++s) {
    if (s + 1 < nst) gload(s + 1);
    const int buf = s & 1;
#pragma unroll
    for (int u2 = 0; u2 < AMX_SB; ++u2) {
      if (s * AMX_SB + u2 < nb) {
        bf16x8 fr[NKS];
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) fr[ks] = *(const bf16x8*)(&sbuf[buf][u2][fo[ks]]);
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
          if (l == 0 && ks == 0) {
#pragma unroll
            for (int u = 0; u < RG; ++u) acc[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[0], xa[u][0], zero, 0, 0, 0);
          } else {
#pragma unroll
            for (int u = 0; u < RG; ++u) acc[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[ks], xa[u][ks], acc[u], 0, 0, 0);
          }
        }
        if (++l == g.b_limbs) {
#pragma unroll
          for (int b = 0; b < 2; ++b) {
            const int blk = (tn * 32 + 16 * b) / g.bout_L;  // wave-uniform
            if (blk != cur_blk) {
              commit();
              cur_blk = blk;
#pragma unroll
              for (int u = 0; u < RG; ++u) cur[u] = 0.f;
            }
#pragma unroll
            for (int u = 0; u < RG; ++u) {
              float m = cur[u];
#pragma unroll
              for (int k = 0; k < 8; k += 2) m = fmaxf(fmaxf(m, fabsf(acc[u][8 * b + k])), fabsf(acc[u][8 * b + k + 1]));
              cur[u] = m;
            }
          }
          l = 0, ++tn;
        }
      }
    }
    if (s + 1 < nst) lwrite(buf ^ 1);  // (everybody left that buffer before the previous barrier)
    __syncthreads();
  }
  commit();
}

size_t gemm_scratch_bytes(int64_t m_max, int64_t N, const QP& bout) {
  if (bout.kind != LQER_Q_MXINT || bout.block == 16) return 0;
  const int64_t Np = lqer_padded_n(N);
  const int64_t L = (bout.block <= 0 || bout.block >= N) ? Np : bout.block;
  const int64_t nblk = (Np + L - 1) / L;
  // (one block per row on the int8 route: up to LQER_AMAX_NSEG column-segment partials per row instead of one atomic cell - or as
  // many {value, tag} granules of 8 bytes when the GEMM exchanges the maxima itself)
  return (size_t)lqer_padded_m(m_max) * (nblk == 1 ? 2 * LQER_AMAX_NSEG : nblk) * sizeof(float);
}

__global__ void k_zero_cells(uint32_t* p, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = 0u;
}

// k_bout_amax<RG, LO + I> for every I of the sequence: launches the one the plan asks for (rc: its result), or says that it is not among them
template <int RG, int LO, int... I>
static bool run_amax(const GemmPlan& p, const GemmArgs& g, hipStream_t st, int& rc, std::integer_sequence<int, I...>) {
  return p.pre.rg == RG && ((p.pre.nks == LO + I && (rc = launch_k<k_bout_amax<RG, LO + I>>("lqer_gemm (B_out pre-pass)", p.pre.grid, 256, 0, st, g,
                                                                                             p.pre.tiles_n32, p.pre.seg_tiles), true)) || ...);
}

// the zero fill of the cells, where the plan wants one, and the pre-pass of the plan
int launch_amax(const GemmPlan& p, const GemmArgs& g, bool amax_zeroed, hipStream_t st) {
  // (amax_zeroed: the activation kernel of the same forward did it.  A kernel, not hipMemsetAsync: as a memset NODE of a captured graph
  // the fill left two of every four cells untouched on replay - ROCm 7.2, tools/graph_replay_gemm.py - while the eager call was fine)
  if (p.zero_bytes && !amax_zeroed) {
    const int rc = launch_k<k_zero_cells>("lqer_gemm (zero fill)", (unsigned)((p.zero_bytes / 4 + 255) / 256), 256, 0, st, (uint32_t*)g.bout_amax,
                                          (int64_t)(p.zero_bytes / 4));
    if (rc) return rc;
  }
  if (p.pre.lds)
    return launch_k<k_bout_amax_lds>("lqer_gemm (B_out pre-pass)", p.pre.grid, 256, 0, st, g, p.pre.tiles_n32, p.pre.seg_tiles);
  // row groups per wave x 16-deep slices of the padded rank (only the pairs listed here exist): up to 4 slices with 1, 2 or 4 row groups,
  // 5 .. 8 with 2, 9 .. 16 with 1 - what a wave's registers hold beside the accumulators (plan_prepass)
  using std::make_integer_sequence;
  int rc;
  if (run_amax<4, 1>(p, g, st, rc, make_integer_sequence<int, 4>{}) || run_amax<2, 1>(p, g, st, rc, make_integer_sequence<int, 8>{}) ||
      run_amax<1, 1>(p, g, st, rc, make_integer_sequence<int, 4>{}) || run_amax<1, 9>(p, g, st, rc, make_integer_sequence<int, 8>{}))
    return rc;
  set_error("%s", p.msg);  // (plan_prepass refused: more slices than any instantiation has)
  return p.launch_err;
}

}  // namespace lqer
