// lqer_col_abs_stats: per-column sum|x| and max|x| of an activation x [M, K] in ONE pass over x - the calibration statistics of
// L2QER (reference src/lqer/statistic_profiler/scale.py:32-38: x.float().abs().view(-1, K).mean(0), torch.maximum into the running
// scale) and of the outlier-column count (statistic_profiler/threshold.py:39-40: x.abs().ge(threshold) ... .any(dim=0).sum()).
//
// Traffic model: x is read once in its own dtype (2 B per fp16 / bf16 element, 4 B per fp32 element); the reference's hook body
// moves 18 B per fp16 element (fp32 copy, abs copy, column mean) and 12 B per fp32 element.  On top come the partials of stage 1,
// written and read once: 2 x 2 x 4 B x row_chunks x K with row_chunks <= 64 - at M = 8192 that is 6 % of an fp16 x at K = 4096
// (64 chunks) and 2.3 % at K = 11008 (24 chunks).
//
// Stage 1 (k_col_stats_partial): grid = (column strips, row chunks).  A workgroup of 256 threads is 32 column lanes x 8 row groups; a
// lane owns V adjacent columns (one 16-byte load: 8 elements of a 16-bit dtype, 4 of fp32), so a wave reads two row segments of
// 512 contiguous bytes per load instruction.  Row group g walks rows r0 + g, r0 + g + 8, ... of the chunk, four loads in flight,
// adding |x| (upcast to fp32) to one accumulator per column IN ROW ORDER and folding max|x|; the 8 row groups combine through LDS in
// group order and the workgroup stores one fp32 {sum, max} per column to psum / pmax [row_chunks][K].  Columns beyond the last full
// 16-byte group, and every column of an input whose base or row pitch is not 16-byte aligned, take the SAME lane layout with
// element loads (a scalar variant of the load only: one accumulator per column, the same order of additions - the same bits).
// Stage 2 (k_col_stats_final): one thread per column adds the partials in chunk order, divides by M, and writes the outputs.
// No floating-point atomics anywhere: the order of every sum is fixed by (M, K, dtype), two calls on one input agree bit for bit.
// The count of columns with max|x| >= threshold is an integer atomicAdd per wave into a cell that stage 1 zeroes.
//
// NaN as torch has it: |NaN| poisons the column's sum, torch.maximum keeps it (run = NaN), torch's amax gives NaN (col_absmax = NaN);
// fmaxf drops NaNs, so pmax holds the maximum of the column's OTHER elements - which is what x.abs().ge(t).any(0) asks about (a NaN
// compares false, a finite neighbour in the same column still counts).
#include "common.h"

namespace lqer {

constexpr int CS_COL_LANES = 32, CS_ROW_GROUPS = 8, CS_UNROLL = 4;
constexpr int CS_MAX_CHUNKS = 64;        // row chunks (partials: 2 x 4 B x chunks x K)
constexpr int CS_MIN_CHUNK_ROWS = 64;    // ... of at least this many rows: 8 per row group
constexpr int CS_TARGET_BLOCKS = 1024;   // four workgroups per CU on 256 CUs: 16 waves x 4 loads x 1 KiB in flight per CU

template <int DT>
struct ColVec {
  static constexpr int V = DT == LQER_F32 ? 4 : 8;
};

// the V values of one 16-byte load, upcast to fp32
template <int DT>
__device__ __forceinline__ void unpack16(const u32x4 rawv, float (&v)[ColVec<DT>::V]) {
  // (plain words first: indexing the vector with the unrolled j directly made hipcc reuse word 0 for all four pairs - common.h row8_chunk)
  const uint32_t raw[4] = {rawv[0], rawv[1], rawv[2], rawv[3]};
  if constexpr (DT == LQER_F32) {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = __uint_as_float(raw[j]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) pair_to_f32<DT>(raw[j], v[2 * j], v[2 * j + 1]);
  }
}

template <int DT>
__global__ __launch_bounds__(CS_COL_LANES* CS_ROW_GROUPS) void k_col_stats_partial(const void* __restrict__ x, int64_t M, int64_t K,
                                                                                    int64_t ldx, int chunk_rows, int aligned,
                                                                                    float* __restrict__ psum, float* __restrict__ pmax,
                                                                                    int32_t* __restrict__ count_cell) {
  constexpr int V = ColVec<DT>::V, ES = DT == LQER_F32 ? 4 : 2, W = CS_COL_LANES * V;
  __shared__ float lsum[CS_ROW_GROUPS][W + 4], lmax[CS_ROW_GROUPS][W + 4];
  const int cl = threadIdx.x % CS_COL_LANES, rg = threadIdx.x / CS_COL_LANES;
  const int64_t c0 = ((int64_t)blockIdx.x * CS_COL_LANES + cl) * V;
  const int64_t r0 = (int64_t)blockIdx.y * chunk_rows;
  const int64_t r1 = r0 + chunk_rows < M ? r0 + chunk_rows : M;
  if (count_cell && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *count_cell = 0;  // (stage 2 runs behind this kernel)

  float s[V], m[V];
#pragma unroll
  for (int j = 0; j < V; ++j) s[j] = 0.0f, m[j] = 0.0f;
  if (c0 < K) {
    if (aligned && c0 + V <= K) {
      const char* base = (const char*)x + c0 * ES;
      for (int64_t r = r0 + rg; r < r1; r += CS_ROW_GROUPS * CS_UNROLL) {
        u32x4 raw[CS_UNROLL];
#pragma unroll
        for (int u = 0; u < CS_UNROLL; ++u) {
          const int64_t rr = r + u * CS_ROW_GROUPS;
          raw[u] = rr < r1 ? *(const u32x4*)(base + rr * ldx * ES) : (u32x4){0u, 0u, 0u, 0u};  // (+0 changes neither sum nor max)
        }
#pragma unroll
        for (int u = 0; u < CS_UNROLL; ++u) {
          float v[V];
          unpack16<DT>(raw[u], v);
#pragma unroll
          for (int j = 0; j < V; ++j) s[j] += fabsf(v[j]), m[j] = __builtin_fmaxf(m[j], fabsf(v[j]));
        }
      }
    } else {
      // the scalar variant: the tail group of a K that is no multiple of V, or an input without 16-byte alignment
      const int nv = K - c0 < V ? (int)(K - c0) : V;
      for (int64_t r = r0 + rg; r < r1; r += CS_ROW_GROUPS) {
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const float v = j < nv ? load_elem<DT>(x, r * ldx + c0 + j) : 0.0f;
          s[j] += fabsf(v), m[j] = __builtin_fmaxf(m[j], fabsf(v));
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < V; ++j) lsum[rg][cl * V + j] = s[j], lmax[rg][cl * V + j] = m[j];
  __syncthreads();
  const int64_t col = (int64_t)blockIdx.x * W + threadIdx.x;
  if ((int)threadIdx.x < W && col < K) {
    float ts = lsum[0][threadIdx.x], tm = lmax[0][threadIdx.x];
#pragma unroll
    for (int g = 1; g < CS_ROW_GROUPS; ++g) ts += lsum[g][threadIdx.x], tm = __builtin_fmaxf(tm, lmax[g][threadIdx.x]);
    psum[(int64_t)blockIdx.y * K + col] = ts;
    pmax[(int64_t)blockIdx.y * K + col] = tm;
  }
}

__global__ __launch_bounds__(256) void k_col_stats_final(const float* __restrict__ psum, const float* __restrict__ pmax, int chunks,
                                                          int64_t K, float rows, float* __restrict__ run, float* __restrict__ absmax,
                                                          float threshold, int32_t* __restrict__ count_cell) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool ge = false;
  if (k < K) {
    float s = 0.0f, m = 0.0f;
    for (int c = 0; c < chunks; ++c) s += psum[(int64_t)c * K + k], m = __builtin_fmaxf(m, pmax[(int64_t)c * K + k]);
    const float mean = s / rows;
    if (run) {
      const float old = run[k];
      run[k] = (mean > old || mean != mean) ? mean : old;  // torch.maximum: a NaN on either side stays
    }
    if (absmax) absmax[k] = s != s ? s : m;  // (a NaN in the column: torch's amax gives NaN)
    ge = m >= threshold;
  }
  if (count_cell) {
    const int n = __builtin_popcountll(__builtin_amdgcn_ballot_w64(ge));
    if (n && (threadIdx.x & 63) == 0) atomicAdd(count_cell, n);
  }
}

// launch geometry of stage 1: a function of (M, K, dtype) alone
static void col_stats_plan(int dtype, int64_t M, int64_t K, int* strips, int* chunks, int* chunk_rows) {
  const int W = CS_COL_LANES * (dtype == LQER_F32 ? 4 : 8);
  const int64_t ns = (K + W - 1) / W;
  int64_t nc = (CS_TARGET_BLOCKS + ns - 1) / ns;
  const int64_t cap = (M + CS_MIN_CHUNK_ROWS - 1) / CS_MIN_CHUNK_ROWS;
  nc = nc > CS_MAX_CHUNKS ? CS_MAX_CHUNKS : nc;
  nc = nc > cap ? cap : nc;
  const int64_t cr = (M + nc - 1) / nc;
  *strips = (int)ns, *chunk_rows = (int)cr, *chunks = (int)((M + cr - 1) / cr);
}

// (sized for the most chunks any dtype's plan takes at this M: the caller's buffer does not depend on the dtype)
static size_t col_stats_workspace(int64_t M, int64_t K) {
  int64_t nc = (M + CS_MIN_CHUNK_ROWS - 1) / CS_MIN_CHUNK_ROWS;
  nc = nc > CS_MAX_CHUNKS ? CS_MAX_CHUNKS : nc;
  return (size_t)2 * nc * K * sizeof(float);
}

}  // namespace lqer

extern "C" size_t lqer_col_abs_stats_workspace_bytes(int64_t M, int64_t K) {
  if (M <= 0 || K <= 0) return 0;
  return lqer::col_stats_workspace(M, K);
}

extern "C" int lqer_col_abs_stats(const void* x, int dtype, int64_t M, int64_t K, int64_t ldx, float* run_absmean_max, float* col_absmax,
                                  float threshold, int32_t* n_cols_ge, void* workspace, size_t workspace_bytes, void* stream) {
  using namespace lqer;
  if (!x || M <= 0 || K <= 0 || ldx < K || M > ((int64_t)1 << 30) || K > ((int64_t)1 << 30)) {
    set_error("col_abs_stats: bad argument (x %p, M %lld, K %lld, ldx %lld)", x, (long long)M, (long long)K, (long long)ldx);
    return LQER_E_INVALID;
  }
  if (dtype != LQER_F32 && dtype != LQER_F16 && dtype != LQER_BF16) {
    set_error("col_abs_stats: unknown dtype %d", dtype);
    return LQER_E_INVALID;
  }
  if (!run_absmean_max && !col_absmax && !n_cols_ge) {
    set_error("col_abs_stats: no output requested (run_absmean_max, col_absmax and n_cols_ge are all null)");
    return LQER_E_INVALID;
  }
  const size_t need = col_stats_workspace(M, K);
  if (workspace_bytes < need) {
    set_error("col_abs_stats: workspace %zu B < %zu B (lqer_col_abs_stats_workspace_bytes)", workspace_bytes, need);
    return LQER_E_WORKSPACE;
  }
  if (!workspace || ((uintptr_t)workspace & 3)) {
    set_error("col_abs_stats: workspace null or not 4-byte aligned");
    return LQER_E_INVALID;
  }
  int strips, chunks, chunk_rows;
  col_stats_plan(dtype, M, K, &strips, &chunks, &chunk_rows);
  float* psum = (float*)workspace;
  float* pmax = psum + (size_t)chunks * K;
  const int es = dtype == LQER_F32 ? 4 : 2;
  const int aligned = (((uintptr_t)x & 15) == 0 && (ldx * es) % 16 == 0) ? 1 : 0;
  const hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)strips, (unsigned)chunks);
  const int nt = CS_COL_LANES * CS_ROW_GROUPS;
  if (dtype == LQER_F32) k_col_stats_partial<LQER_F32><<<grid, nt, 0, st>>>(x, M, K, ldx, chunk_rows, aligned, psum, pmax, n_cols_ge);
  else if (dtype == LQER_F16) k_col_stats_partial<LQER_F16><<<grid, nt, 0, st>>>(x, M, K, ldx, chunk_rows, aligned, psum, pmax, n_cols_ge);
  else k_col_stats_partial<LQER_BF16><<<grid, nt, 0, st>>>(x, M, K, ldx, chunk_rows, aligned, psum, pmax, n_cols_ge);
  const int rc = check_launch("col_abs_stats (partials)");
  if (rc != LQER_OK) return rc;
  k_col_stats_final<<<(unsigned)((K + 255) / 256), 256, 0, st>>>(psum, pmax, chunks, K, (float)M, run_absmean_max, col_absmax, threshold,
                                                                n_cols_ge);
  return check_launch("col_abs_stats (final)");
}
