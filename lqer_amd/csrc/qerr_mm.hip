// lqer_qerr_matmul: products of the quantization-error operator E_s = diag(s) (W - Q_w(W))^T  [K, N] with skinny fp32 matrices, E never
// in memory - the O(N K) step of the subspace-iteration approximator (lqer_amd/approximate.py, method="subspace").
//   trans = 0:  Y [N, L] = E_s^T X [K, L] = (W - Q_w(W)) (s . X)        contraction over K (W's contiguous dim)
//   trans = 1:  Y [K, L] = E_s   X [N, L] = s . ((W - Q_w(W))^T X)      contraction over N
// W [N, K] fp32 / fp16 / bf16 with row stride ldw, 1 <= L <= 256, s [K] fp32 or absent.
//
// Traffic model: one read of W in its own dtype per product (2 B per fp16 element), plus the split-contraction partials written and
// read once (below).  The reference route reads W, writes Q_w(W) and E^T in fp32 and hands E^T to a full SVD.
//
// ONE kernel body (k_qerr_mm), two sources of the E fragment (template FUSED, the idiom of attn_decode.hip's SRC):
//   fused : the workgroup's 32 x 128 tile of W is loaded in the caller's dtype, lane t holding the run of 16 consecutive k
//           (row t / 8, run t % 8) - a wave's request is 8 rows x 256 contiguous bytes of fp16.  max|run| is an in-lane reduction; blocks
//           of 32 / 64 / 128 combine 2 / 4 / 8 ADJACENT lanes with __shfl_xor (a tile starts at a multiple of 128, so no block straddles
//           two tiles).  Then the library's block rule word for word - block_exponent, mxint_mantissa, ldexpf, the |w| <= 1e-8 keep-as-is
//           rule (quantize.hip emit16's `deq`) - and e = w - deq in fp32.  A partial last block reads zeros behind K, as the
//           quantizer kernels do (zeros raise no maximum).
//   dense : the same lane reads the same 16 elements of a caller-provided fp32 E [N, K] (every other weight quantizer: whole-row blocks,
//           2-D tiles, integer, minifloat - Python computes E with the quantizer kernel that serves the format).
// Both leave float e[16] per lane; everything from there on is written once.
//
// The E tile goes through LDS, not straight from registers into the matrix pipe.  The fp32 MFMA takes ONE A element per lane and step,
// so a register-fed multiply needs a different lane layout per orientation (a row's consecutive k across lanes for trans = 1, a whole
// block per lane for trans = 0) - two quantizers, two reductions.  Through LDS one producer layout (the library's own "a lane holds 16
// consecutive k", k_quant_seg16) serves both: the tile [32 n][128 k] (row pitch 132 floats: 16-byte rows for the producer's
// ds_write_b128) is read as A[n][k] for trans = 0 and as A[k][n] for trans = 1, one ds_read_b32 per lane and MFMA step, at most
// two lanes per bank in either orientation.  Cost: 4 B written + 4 B read per element against 2 B from HBM - at HBM speed 20 B per
// clock and CU of the 128 B/clk the LDS moves.
//
// Arithmetic: v_mfma_f32_32x32x2_f32 - both operands enter the matrix pipe as fp32, fp32 accumulation; no limb splits.
// Wave w of the four owns the k slab [32 w, 32 w + 32) of every tile in BOTH orientations:
//   trans = 0: 16 steps over its 32 k (A = tile[n = lane % 32][k = 32 w + 2 step + lane / 32]) into 32 n x L - the four waves' sums are
//              added at the end through LDS in wave order;
//   trans = 1: 16 steps over the tile's 32 n (A = tile[n = 2 step + lane / 32][k = 32 w + lane % 32]) into its own 32 k x L.
// The accumulators are NT tiles of 32 columns (NT = ceil(L / 32) is one of 1, 2, 3, 5, 8: 48 -> 2, 80 -> 3, 144 -> 5).
//
// Skinny operand: the B element of a step is X[row][32 t + lane % 32] - 128 contiguous bytes per half wave - read straight from
// global memory (trans = 0: times s[row], so the product is (W - Q)(s . X) as the header states it).  X is L x 4 B per contraction index and
// at most 4.5 MB in all: it lives in L2.  It is NOT staged in LDS: with the slab split above the four waves of a workgroup multiply
// four different row ranges of X for trans = 0 (nothing to share), and for trans = 1 the three re-reads hit L1; an LDS copy of
// 128 rows x 256 columns would be 128 KB and leave one workgroup per CU.  trans = 1 applies s at the store (in the reduce kernel).
//
// Work split: the output is only N x L (K x L), so the contraction is cut into `splits` runs of whole tiles such that the grid has about
// two workgroups per CU (qerr_plan: a function of N, K, trans alone); workgroup (row tile, split) writes its partial sums to
// workspace [splits][rows][L], and k_qerr_reduce adds them IN SPLIT ORDER, one thread per output.  No float atomics, no counters: the
// order of every sum is fixed by the shape, two calls give the same bits; every partial a reduce thread reads was written by the first
// kernel of the same call (workspace contents are never assumed).  Partials are splits x rows x L x 4 B: at 4096 x 4096, L = 48,
// 3 MB (trans = 0, 4 splits) and 12.6 MB (trans = 1, 16 splits) beside 33.5 MB of fp16 W.
//
// Bounds: rows behind N and columns behind K enter the tile as zeros (no load is issued for them); B elements of a row behind the
// contraction length or a column >= L are zeros (no load); stores are guarded by row < rows and column < L, Y is written at
// row * ldy + column only.  Rows of W whose base or pitch is not 16-byte aligned take element loads (common.h load16: same values).
#include "common.h"

namespace lqer {

constexpr int QE_TN = 32, QE_TK = 128, QE_PITCH = QE_TK + 4;
constexpr int QE_TARGET_BLOCKS = 512, QE_MAX_SPLITS = 32;

// launch geometry: a function of (N, K, trans) alone
struct QerrPlan {
  int64_t rows;       // rows of Y: N (trans = 0) or K
  int64_t out_tiles;  // workgroups along the rows of Y: 32 n, or 128 k (four waves x 32)
  int64_t ctiles;     // tiles along the contraction: 128 k, or 32 n
  int64_t per;        // contraction tiles per split
  int64_t splits;
};
QerrPlan qerr_plan(int64_t N, int64_t K, int trans) {
  const int64_t nt = (N + QE_TN - 1) / QE_TN, kt = (K + QE_TK - 1) / QE_TK;
  QerrPlan p;
  p.rows = trans ? K : N;
  p.out_tiles = trans ? kt : nt;
  p.ctiles = trans ? nt : kt;
  int64_t want = (QE_TARGET_BLOCKS + p.out_tiles - 1) / p.out_tiles;
  want = want > QE_MAX_SPLITS ? QE_MAX_SPLITS : want;
  want = want > p.ctiles ? p.ctiles : want;
  p.per = (p.ctiles + want - 1) / want;
  p.splits = (p.ctiles + p.per - 1) / p.per;
  return p;
}
size_t qerr_workspace(int64_t N, int64_t K, int64_t L, int trans) {
  const QerrPlan p = qerr_plan(N, K, trans);
  return (size_t)p.splits * (size_t)p.rows * (size_t)L * sizeof(float);
}

// The E fragment of lane (row n, 16 k from k): e = w - Q_w(w) from W (FUSED) or the caller's E itself.
template <int DT, bool FUSED>
__device__ __forceinline__ void qerr_fragment(const void* __restrict__ W, int64_t N, int64_t K, int64_t ldw, bool vec, int64_t n, int64_t k,
                                              const QP& q, float (&e)[16]) {
  float v[16];
  load16<DT>(W, n * ldw + k, n < N ? K - k : 0, vec, v);
  if constexpr (!FUSED) {
#pragma unroll
    for (int i = 0; i < 16; ++i) e[i] = v[i];
  } else {
    float amax = 0.0f;
#pragma unroll
    for (int i = 0; i < 16; ++i) amax = fmaxf(amax, fabsf(v[i]));
    for (int m = 1; m < q.block / 16; m <<= 1) amax = fmaxf(amax, __shfl_xor(amax, m, 64));  // (the lanes of one block are adjacent)
    const bool any = amax > 0.0f;
    const int ex = any ? block_exponent(amax, q) : 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const float m = any ? mxint_mantissa(v[i], ex, q) : 0.0f;
      const float deq = fabsf(v[i]) <= 1e-8f ? v[i] : ldexpf(m, ex - q.mbits);  // (quantize.hip emit16: what lqer_quantize_mxint stores)
      e[i] = v[i] - deq;
    }
  }
}

template <int DT, bool FUSED, int TRANS, int NT>
__global__ __launch_bounds__(256) void k_qerr_mm(const void* __restrict__ W, int64_t N, int64_t K, int64_t ldw, int vec, QP q,
                                                 const float* __restrict__ scale, const float* __restrict__ X, int64_t ldx, int L,
                                                 int64_t ctiles, int64_t per, float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float tile[QE_TN * QE_PITCH];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int pr = t >> 3, pc = (t & 7) * 16;  // the producer's row and first k inside the tile
  const int lo = lane & 31, hi = lane >> 5;
  const int64_t ot = blockIdx.x, split = blockIdx.y;
  const int64_t c0 = split * per, c1 = c0 + per < ctiles ? c0 + per : ctiles;
  const int64_t rows = TRANS ? K : N, clen = TRANS ? N : K;

  f32x16 acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.0f;

  for (int64_t c = c0; c < c1; ++c) {
    const int64_t n0 = (TRANS ? c : ot) * QE_TN, k0 = (TRANS ? ot : c) * QE_TK;
    float e[16];
    qerr_fragment<DT, FUSED>(W, N, K, ldw, vec != 0, n0 + pr, k0 + pc, q, e);
    __syncthreads();  // the previous tile's reads are done
#pragma unroll
    for (int i = 0; i < 4; ++i)
      *(f32x4*)&tile[pr * QE_PITCH + pc + 4 * i] = (f32x4){e[4 * i], e[4 * i + 1], e[4 * i + 2], e[4 * i + 3]};
    __syncthreads();
#pragma unroll 4
    for (int s = 0; s < 16; ++s) {
      const float a = TRANS ? tile[(2 * s + hi) * QE_PITCH + 32 * w + lo] : tile[lo * QE_PITCH + 32 * w + 2 * s + hi];
      const int64_t brow = TRANS ? n0 + 2 * s + hi : k0 + 32 * w + 2 * s + hi;  // the contraction index of this lane's B element
      const bool rok = brow < clen;
      const float sc = (!TRANS && scale && rok) ? scale[brow] : 1.0f;
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int col = 32 * j + lo;
        const float b = (rok && col < L) ? X[brow * ldx + col] * sc : 0.0f;
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[j], 0, 0, 0);
      }
    }
  }

  // accumulator element r of a lane: row 8 (r / 4) + 4 hi + r % 4, column lo of its 32 x 32 tile
  if constexpr (!TRANS) {
    // the four waves hold sums over their k slabs of the same 32 n x L: added in wave order through LDS, one column tile at a time
    float* const red = tile;  // 3 x 1024 floats of the 4224
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      __syncthreads();
      if (w > 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) red[(w - 1) * 1024 + r * 64 + lane] = acc[j][r];
      }
      __syncthreads();
      if (w == 0) {
#pragma unroll
        for (int u = 0; u < 3; ++u)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[j][r] += red[u * 1024 + r * 64 + lane];
      }
    }
    if (w != 0) return;
  }
  const int64_t r0 = TRANS ? ot * QE_TK + 32 * w : ot * QE_TN;
  float* const dst = part + (size_t)split * (size_t)rows * (size_t)L;
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int col = 32 * j + lo;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t row = r0 + 8 * (r >> 2) + 4 * hi + (r & 3);
      if (row < rows && col < L) dst[row * L + col] = acc[j][r];
    }
  }
}

// Y[row][col] = (s[row]) sum over the splits, in split order
__global__ __launch_bounds__(256) void k_qerr_reduce(const float* __restrict__ part, int splits, int64_t rows, int L,
                                                     const float* __restrict__ row_scale, float* __restrict__ Y, int64_t ldy) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * L) return;
  const int64_t row = i / L;
  const int col = (int)(i - row * L);
  float s = part[i];
  for (int p = 1; p < splits; ++p) s += part[(size_t)p * (size_t)rows * (size_t)L + i];
  Y[row * ldy + col] = row_scale ? row_scale[row] * s : s;
}

template <int DT, bool FUSED, int TRANS>
static void qerr_launch_nt(int nt, dim3 grid, hipStream_t st, const void* W, int64_t N, int64_t K, int64_t ldw, int vec, const QP& q,
                           const float* scale, const float* X, int64_t ldx, int L, const QerrPlan& p, float* part) {
  switch (nt) {
#define QE_CASE(NT_) \
  case NT_: k_qerr_mm<DT, FUSED, TRANS, NT_><<<grid, 256, 0, st>>>(W, N, K, ldw, vec, q, scale, X, ldx, L, p.ctiles, p.per, part); break;
    QE_CASE(1) QE_CASE(2) QE_CASE(3) QE_CASE(5) QE_CASE(8)
#undef QE_CASE
  }
}

// `fused`: W is the weight and q its block_fp format with blocks of 16 / 32 / 64 / 128; else W is E itself (fp32).  Arguments are checked
// by the entry point (api.hip).
int qerr_mm_dispatch(const void* W, int dtype, int64_t N, int64_t K, int64_t ldw, bool fused, const QP& q, const float* scale, int trans,
                     const float* X, int64_t ldx, int64_t L, float* Y, int64_t ldy, void* workspace, hipStream_t st) {
  const QerrPlan p = qerr_plan(N, K, trans);
  const int es = dtype == LQER_F32 ? 4 : 2;
  const int vec = (((uintptr_t)W & 15) == 0 && (ldw * es) % 16 == 0) ? 1 : 0;
  const int tiles = (int)((L + 31) / 32);
  const int nt = tiles <= 3 ? tiles : (tiles <= 5 ? 5 : 8);
  const dim3 grid((unsigned)p.out_tiles, (unsigned)p.splits);
  float* part = (float*)workspace;
  auto go = [&](auto dt, auto fz) {
    constexpr int DT = decltype(dt)::value;
    constexpr bool FZ = decltype(fz)::value;
    if (trans) qerr_launch_nt<DT, FZ, 1>(nt, grid, st, W, N, K, ldw, vec, q, scale, X, ldx, (int)L, p, part);
    else qerr_launch_nt<DT, FZ, 0>(nt, grid, st, W, N, K, ldw, vec, q, scale, X, ldx, (int)L, p, part);
    return LQER_OK;
  };
  if (fused) with_dtype(dtype, [&](auto dt) { return go(dt, std::true_type{}); });
  else go(std::integral_constant<int, LQER_F32>{}, std::false_type{});
  const int rc = check_launch("qerr_matmul (partials)");
  if (rc != LQER_OK) return rc;
  const int64_t total = p.rows * L;
  k_qerr_reduce<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(part, (int)p.splits, p.rows, (int)L, trans ? scale : nullptr, Y, ldy);
  return check_launch("qerr_matmul (reduce)");
}

}  // namespace lqer
