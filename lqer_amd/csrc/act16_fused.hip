// The block-16 MXINT activation side as ONE launch (round 6): x_quantizer in blocks of [1, 16] (reference quantizers/block_fp.py:55-82
// through quantized_layers/linear.py:154, llama-7b.toml:78-105) + x_q A (linear.py:155) + A_out_quantizer (linear.py:156) - what
// k_quant_xa16 (quantizer + split-K partial tiles of x A) + k_xa_reduce4 (fixed-order sum + A_out) did in two launches: the reduce is a
// 4.9-us launch-floor kernel beside a 56-us GEMM at BASELINE configs[1] and resisted three fusions into its neighbours (NOTEBOOK 7-9).
//
// A workgroup owns ROWS = 8 token rows over ALL of K (no partial tiles in HBM, no reduce launch, no cross-workgroup protocol), and inside
// it every WAVE is a pipeline of its own over slabs of 512 k (slab s belongs to wave s % 8), each slab in four QUARTERS of 128 k - a
// block's exponent needs nothing outside its 16 elements, so nothing waits for a whole row, and a 32-k MFMA step needs all 8 rows of its
// k only:
//   load     one 16-byte request per lane covers 4 rows x 256 B of a quarter (two whole 128-byte lines per row), two requests a quarter
//            of all 8 rows; the slab's eight requests go out in front of everything else the kernel does, quarter 0 first, from
//            arguments that arrive preloaded in SGPRs (Makefile: A16_FLAGS);
//   quantize a block of 16 = two neighbouring lanes (the maximum crosses with one DPP); k_quant_xa16's arithmetic (mxint16_bf16_fast or,
//            at extreme exponents, the element routine) on the lane's 8 values -> 8 bf16 = 16 bytes, stored to the activation image
//            and to the wave's PRIVATE LDS slab [8 rows][1040 B] - no workgroup barrier;
//   multiply as soon as a quarter of all 8 rows is quantized, its 4 steps of v_mfma_f32_16x16x32_bf16 while the later quarters are still
//            arriving: the 8 rows as rows 0-7 of the 16-row operand (one ds_read_b128 per step: row lane & 7, chunk 4 t + lane / 16; the
//            pitch of 1040 B keeps a 16-lane group on 16 distinct bank quads), A^T fragments as ONE coalesced 16-byte load per lane from
//            the fragment-major copy behind the bf16 image (lqer_a_b16_prepare), in two register sets; steps ascending in one
//            accumulator chain per rank tile, whatever the order of the loads;
//   finally  the 8 waves' partial tiles through LDS, summed in wave order (fixed: run-to-run bit-stable), A_out exactly as k_xa_reduce4.
// The image is bit for bit k_quant_xa16's; x A is summed in another order (xAq inside the summation-order envelope, tests/_envelope.py).
// Both are bit for bit what the row-major body of round 6 wrote (tests/test_gpu_act16_golden.py).
#include "common.h"

namespace lqer {
namespace a16f {

constexpr int ROWS = 8, WAVES = 8, SLAB = 512, PITCH = 1040;

__host__ inline size_t lds_bytes(int rp) { return (size_t)WAVES * ROWS * PITCH + (size_t)WAVES * ROWS * rp * sizeof(float); }

typedef __attribute__((ext_vector_type(8))) __bf16 bf16v8;

#ifdef LQER_CLOCKPROBE
__device__ unsigned long long* g_a16_stamp_buf = nullptr;  // diagnostic build: shader cycles at the phase boundaries of a wave's FIRST slab
#define A16_STAMP(i) asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(cp[i])::"memory")
#else
#define A16_STAMP(i)
#endif

template <int DT, int RT>
__global__ __launch_bounds__(512) void k_act16_fused(const void* __restrict__ x, int64_t M, int64_t ld, int64_t K, int64_t Kp,
                                                      const bf16_t* __restrict__ a_frag, bf16_t* __restrict__ xq, bf16_t* __restrict__ xaq, QP qx, QP qa,
                                                      int L_aout) {
  constexpr int RP = 16 * RT;
  constexpr int QK = SLAB / 4, QS = QK / 32;  // a quarter of a slab: 128 k = 4 MFMA steps
  constexpr int HB = RT == 4 ? 2 : 4;         // steps per fragment part: two register sets of HB x RT fragments (<= 32 registers each)
  constexpr int NP = QS / HB;                 // parts per quarter; part p of a slab (steps HB p .. HB p + HB - 1) lives in set p & 1
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t m0 = (int64_t)blockIdx.x * ROWS;
#ifdef LQER_CLOCKPROBE
  unsigned long long cp[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  A16_STAMP(0);
#endif
  // ---- the first slab's requests, in front of every other piece of setup.  Request j = 2 q + h of a slab: quarter q, rows 4 h .. 4 h + 3;
  // the lane's row is 4 h + lane / 16, its 8 elements the chunk lane % 16 of the quarter.  Every load is unconditional (a row past M reads
  // row M - 1, a chunk past K the row's last chunk, a step past the padded K fragment block 0; what is out of range is zeroed or multiplies
  // zeros where it is used): straight-line code, so each wait counts exactly the requests behind the one it needs.
  const int rl = lane >> 4, cl = lane & 15;
  const int nslab = (int)((Kp + SLAB - 1) / SLAB), nst = (int)(Kp / 32);
  const bool row_ok[2] = {m0 + rl < M, m0 + 4 + rl < M};
  const bf16_t* const xr[2] = {(const bf16_t*)x + (row_ok[0] ? m0 + rl : M - 1) * ld, (const bf16_t*)x + (row_ok[1] ? m0 + 4 + rl : M - 1) * ld};
  const u32x4* const fr = (const u32x4*)a_frag + lane;  // block (step, rank tile): fr[(step * RT + tile) * 64]
  u32x4 raw[ROWS], fa[HB][RT], fb[HB][RT];
  auto load_rows = [&](int s, auto j0, auto j1) {
    asm volatile("" ::: "memory");
#pragma unroll
    for (int j = decltype(j0)::value; j < decltype(j1)::value; ++j) {
      const int64_t k = (int64_t)s * SLAB + (j >> 1) * QK + 8 * cl;
      raw[j] = *(const u32x4*)(xr[j & 1] + (k < K ? k : K - 8));
    }
    asm volatile("" ::: "memory");
  };
  // (part p of slab s: HB steps x RT tiles of A^T fragments, ONE coalesced 16-byte load per lane and block)
  auto load_part = [&](u32x4 (&f)[HB][RT], int s, int p) {
    asm volatile("" ::: "memory");
#pragma unroll
    for (int i = 0; i < HB; ++i)
#pragma unroll
      for (int t = 0; t < RT; ++t) {
        const int st = s * (SLAB / 32) + p * HB + i;
        f[i][t] = fr[((int64_t)(st < nst ? st : 0) * RT + t) * 64];
      }
    asm volatile("" ::: "memory");
  };
  using I0 = std::integral_constant<int, 0>;
  using I2 = std::integral_constant<int, 2>;
  using I4 = std::integral_constant<int, 4>;
  using I8 = std::integral_constant<int, 8>;
  // Loads complete in the order they were issued, so a fragment part lands behind every row requested in front of it: parts 0 and 1 go out
  // between the rows of the quarters they belong to (the rows of quarter 0 keep the memory busy meanwhile), the later parts from inside the
  // slab, each into the register set that a multiplied part has freed.
  auto front = [&](int s) {
    load_rows(s, I0{}, I2{});
    load_part(fa, s, 0);
    if constexpr (NP == 1) load_rows(s, I2{}, I4{});
    load_part(fb, s, 1);
    if constexpr (NP == 1) load_rows(s, I4{}, I8{});
    else load_rows(s, I2{}, I8{});
  };
  if (wave < nslab) front(wave);
  A16_STAMP(1);  // the first slab's requests are out
  unsigned char* const wb = smem + (size_t)wave * ROWS * PITCH;                 // this wave's slab: [ROWS][PITCH]
  float* const red = (float*)(smem + (size_t)WAVES * ROWS * PITCH);             // [WAVES][ROWS][RP] partial tiles
  const int g = lane >> 4;
  const unsigned char* const tok = wb + (lane & 7) * PITCH + 16 * g;  // + 64 t: row lane & 7, chunk 4 t + g
  unsigned char* const wr[2] = {wb + rl * PITCH + 16 * cl, wb + (4 + rl) * PITCH + 16 * cl};  // + 256 q: the lane's chunk of quarter q
  bf16_t* const xqr[2] = {xq + (m0 + rl) * Kp + 8 * cl, xq + (m0 + 4 + rl) * Kp + 8 * cl};    // + the quarter's first k
  f32x4 acc[RT];
#pragma unroll
  for (int t = 0; t < RT; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // ---- quantize request j of slab s: the lane's 8 values of its row; the block's other half sits in lane ^ 1.  FULL: the slab lies inside K
  auto piece = [&](int s, int j, auto full) {
    constexpr bool FULL = decltype(full)::value;
    const int64_t kq = (int64_t)s * SLAB + (j >> 1) * QK, k = kq + 8 * cl;
    const bool live = row_ok[j & 1] && (FULL || k < K);  // (K % 8 == 0: a chunk is inside x or outside it as a whole)
    float v[8];
    const uint32_t wd[4] = {live ? raw[j][0] : 0u, live ? raw[j][1] : 0u, live ? raw[j][2] : 0u, live ? raw[j][3] : 0u};
#pragma unroll
    for (int i = 0; i < 4; ++i) pair_to_f32<DT>(wd[i], v[2 * i], v[2 * i + 1]);
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) amax = fmaxf(amax, fabsf(v[i]));
    amax = fmaxf(amax, __shfl_xor(amax, 1, 64));
    uint32_t w[4] = {0, 0, 0, 0};
    if (amax > 0.f) {
      const int e = block_exponent_u(amax, qx);
      // (mxint_bf16_image's text, common.h: called as the function, the three bf16 kernels come out in another instruction order)
      if (mxint16_fast_ok(e, qx)) {
        mxint16_bf16_fast<DT != LQER_F16, 8>(v, e, qx, w);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const uint32_t lo = exact_bf16_bits(ldexpf(mxint_mantissa(v[2 * i], e, qx), e - qx.mbits));
          const uint32_t hi = exact_bf16_bits(ldexpf(mxint_mantissa(v[2 * i + 1], e, qx), e - qx.mbits));
          w[i] = lo | (hi << 16);
        }
      }
    }
    const u32x4 wv = {w[0], w[1], w[2], w[3]};
    if (FULL || k < Kp) *(u32x4*)(xqr[j & 1] + kq) = wv;  // (rows up to the padded M are allocated; rows past M and k past K: zeros)
    *(u32x4*)(wr[j & 1] + 256 * (j >> 1)) = wv;
    __builtin_amdgcn_sched_barrier(0);  // (pieces are not interleaved: each would keep its temporaries alive beside the fragment sets)
  };
  // ---- multiply part p: HB steps of 32 k
  auto mult = [&](const u32x4 (&f)[HB][RT], int p) {
    // (the wave reads back what it wrote itself: LDS executes a wave's accesses in order - no workgroup barrier; the fences keep the
    // compiler from moving the reads up, or the next quarter's writes in front of them)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    __builtin_amdgcn_sched_barrier(0);
    u32x4 tk[HB];
#pragma unroll
    for (int i = 0; i < HB; ++i) tk[i] = *(const u32x4*)(tok + 64 * (HB * p + i));
#pragma unroll
    for (int i = 0; i < HB; ++i)
#pragma unroll
      for (int t = 0; t < RT; ++t)
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16v8, tk[i]), __builtin_bit_cast(bf16v8, f[i][t]), acc[t], 0, 0, 0);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_sched_barrier(0);
  };
  // ---- a slab, quarter by quarter: quantize the quarter of all 8 rows as soon as it has landed, multiply its 4 steps while the later
  // quarters are still arriving; behind the last quarter 4 steps remain.  FULL: the slab lies inside K.
  // (Four rank tiles: a set holds half a quarter, so only quarter 0's parts can be requested in front of the later rows; the other
  // parts would land behind the last row wherever they were multiplied, and are multiplied behind it - 12 steps.)
  auto slab = [&](int s, auto full) {
    [[maybe_unused]] const bool first = s == wave;
    piece(s, 0, full), piece(s, 1, full);
    if (first) A16_STAMP(2);  // quarter 0 landed and quantized
    if constexpr (NP == 1) {
      mult(fa, 0);
      load_part(fa, s, 2);
      piece(s, 2, full), piece(s, 3, full);
      mult(fb, 1);
      load_part(fb, s, 3);
      piece(s, 4, full), piece(s, 5, full);
      mult(fa, 2);
      piece(s, 6, full), piece(s, 7, full);
      if (first) A16_STAMP(3);  // the last quarter quantized, image stores issued
      mult(fb, 3);
    } else {
      mult(fa, 0);
      load_part(fa, s, 2);
      mult(fb, 1);
      load_part(fb, s, 3);
#pragma unroll
      for (int j = 2; j < 8; ++j) piece(s, j, full);
      if (first) A16_STAMP(3);
#pragma unroll
      for (int p = 2; p < 4 * NP; p += 2) {
        mult(fa, p);
        if (p + 2 < 4 * NP) load_part(fa, s, p + 2);
        mult(fb, p + 1);
        if (p + 3 < 4 * NP) load_part(fb, s, p + 3);
      }
    }
  };
  for (int s = wave; s < nslab; s += WAVES) {
    if ((int64_t)(s + 1) * SLAB <= K) slab(s, std::true_type{});
    else slab(s, std::false_type{});
#ifdef LQER_CLOCKPROBE
    if (s == wave) {
      asm volatile("" ::"v"(acc[0]));
      A16_STAMP(4);  // the slab's last step multiplied
    }
#endif
    // (the wave's next slab: its requests go out as soon as the last part's registers are free.  Inside the branches above they would
    // cost more than they gain: a wait behind the join of a taken and a not-taken path counts for the path with fewer requests, so the
    // last quarter's multiply would wait for the next slab's rows)
    if (s + WAVES < nslab) front(s + WAVES);
  }
  // D layout: column n = lane & 15, rows 4 g + j: token rows 0-7 live in g = 0, 1
  if (g < 2) {
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j) red[(wave * ROWS + 4 * g + j) * RP + 16 * t + (lane & 15)] = acc[t][j];
  }
  __syncthreads();
#ifdef LQER_CLOCKPROBE
  A16_STAMP(5);  // every wave's partial tile is in LDS
  if (g_a16_stamp_buf && lane == 0) {
    unsigned long long* o = g_a16_stamp_buf + ((size_t)blockIdx.x * WAVES + wave) * 8;
    for (int i = 1; i < 6; ++i) o[i] = cp[i] - cp[0];
    unsigned long long rt;
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(rt)::"memory");
    o[0] = cp[0], o[6] = rt;
  }
#endif
  // ---- fixed-order sum of the 8 partial tiles, A_out (k_xa_reduce4's arithmetic), bf16 store
  const int tid = threadIdx.x;
  const bool live = tid < ROWS * RP / 4;
  const int r = tid / (RP / 4), c4 = tid - r * (RP / 4);
  float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
  if (live) {
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
      const float4 v = *(const float4*)(red + (w * ROWS + r) * RP + 4 * c4);
      sum.x += v.x, sum.y += v.y, sum.z += v.z, sum.w += v.w;
    }
  }
  if (tid >= 64 * ((ROWS * RP / 4 + 63) / 64)) return;  // (whole waves only: the shuffles below need their partners)
  float bmax = fmaxf(fmaxf(fabsf(sum.x), fabsf(sum.y)), fmaxf(fabsf(sum.z), fabsf(sum.w)));
  const int G = L_aout / 4;
  for (int d = 1; d < G; d <<= 1) bmax = fmaxf(bmax, __shfl_xor(bmax, d, 64));
  if (!live || m0 + r >= M) return;
  const bool anyb = bmax > 0.f;
  const int eb = anyb ? block_exponent(bmax, qa) : 0;
  const float v[4] = {sum.x, sum.y, sum.z, sum.w};
  uint32_t w2[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const float m0v = anyb ? mxint_mantissa(v[2 * i], eb, qa) : 0.f;
    const float m1v = anyb ? mxint_mantissa(v[2 * i + 1], eb, qa) : 0.f;
    w2[i] = exact_bf16_bits(ldexpf(m0v, eb - qa.mbits)) | (exact_bf16_bits(ldexpf(m1v, eb - qa.mbits)) << 16);
  }
  *(uint2*)(xaq + ((m0 + r) * RP + 4 * c4)) = make_uint2(w2[0], w2[1]);
}

// the bf16 image [rp][Kp] (limb 0 of lqer_pack_lowrank's a_t) and, behind it, its fragment-major copy: block (s = 32-k step, t = 16-rank
// tile) at ((s * RT + t) * 64 + lane) * 8 elements; lane (n = lane & 15, g = lane >> 4) holds A^T[16 t + n][32 s + 8 g .. + 8)
__global__ __launch_bounds__(256) void k_a_b16(const bf16_t* __restrict__ limb0, int64_t Kp, int rp, bf16_t* __restrict__ out) {
  const int RT = rp / 16;
  const int64_t n_img = (int64_t)rp * Kp / 8, total = 2 * n_img;  // 16-byte pieces: the image, then the fragments (same count)
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    if (idx < n_img) {
      ((u32x4*)out)[idx] = ((const u32x4*)limb0)[idx];
    } else {
      const int64_t f = idx - n_img;
      const int lane = (int)(f & 63);
      const int64_t blk = f >> 6;
      const int t = (int)(blk % RT);
      const int64_t s = blk / RT;
      ((u32x4*)out)[idx] = *(const u32x4*)(limb0 + (int64_t)(16 * t + (lane & 15)) * Kp + 32 * s + 8 * (lane >> 4));
    }
  }
}

}  // namespace a16f

#ifdef LQER_CLOCKPROBE
extern "C" int lqer_debug_set_a16_stamp_buffer(void* p) { return (int)hipMemcpyToSymbol(HIP_SYMBOL(a16f::g_a16_stamp_buf), &p, sizeof(p)); }
#endif

size_t a_b16_image_bytes(int64_t K, int64_t r) { return (size_t)2 * lqer_padded_r(r) * lqer_padded_k(K) * sizeof(bf16_t); }

int a_b16_prepare_dispatch(const void* a_t_limbs, int64_t K, int64_t r, void* out, hipStream_t st) {
  const int64_t rp = lqer_padded_r(r), Kp = lqer_padded_k(K);
  if (rp % 16 != 0 || Kp % 32 != 0) {
    set_error("a_b16_prepare: padded rank %d / padded K %d", (int)rp, (int)Kp);
    return LQER_E_UNSUPPORTED;
  }
  const int64_t total = 2 * rp * Kp / 8;
  a16f::k_a_b16<<<(unsigned)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096), 256, 0, st>>>((const bf16_t*)a_t_limbs, Kp, (int)rp, (bf16_t*)out);
  return check_launch("a_b16_prepare");
}

// LQER_E_UNSUPPORTED: not this kernel's case (the caller takes k_quant_xa16 + k_xa_reduce4 on the image's first part)
int act16_fused_dispatch(const void* x, int dtype, int64_t M, int64_t K, int64_t ldx, const QP& qx, bf16_t* xq, const void* a_b16, int64_t r,
                         const QP& qa, bf16_t* xaq, int tuning, hipStream_t st) {
  if (tuning & LQER_TUNE_ACT16_SPLIT) return LQER_E_UNSUPPORTED;
  const int64_t rp = lqer_padded_r(r), Kp = lqer_padded_k(K);
  if (dtype == LQER_F32 || !a_b16 || !xaq || !xq || r <= 0 || M <= 0) return LQER_E_UNSUPPORTED;
  // (rank 128 - RT = 8, eight parts of two steps - was built and measured in round 6: c5 1049 against 1129 with k_quant_xa128 + k_xa_reduce4:
  // every 8-row workgroup streams 1-4 MB of A^T fragments; not instantiated)
  if (!(rp == 16 || rp == 32 || rp == 64)) return LQER_E_UNSUPPORTED;
  if (qx.kind != LQER_Q_MXINT || qx.block != 16 || qx.mbits > 8) return LQER_E_UNSUPPORTED;
  if (((uintptr_t)x % 16) != 0 || ((ldx * 2) % 16) != 0 || K % 16 != 0) return LQER_E_UNSUPPORTED;
  if (qa.kind != LQER_Q_MXINT || qa.mbits > 8) return LQER_E_UNSUPPORTED;
  const int L = (qa.block <= 0 || qa.block >= rp) ? (int)rp : qa.block;
  const int G = L / 4;
  if (rp % L != 0 || L % 4 != 0 || (G & (G - 1)) != 0 || G > 64) return LQER_E_UNSUPPORTED;
  // every workgroup of 8 rows streams the whole A^T image: worth it while the token count is small (see act8_fused.hip)
  if (!(tuning & LQER_TUNE_ACT16_FUSED) && (M > LQER_ACT8_FUSED_MAX_M || M < LQER_ACT8_FUSED_MIN_M)) return LQER_E_UNSUPPORTED;
  const bf16_t* const a_frag = (const bf16_t*)a_b16 + rp * Kp;
  const unsigned grid = (unsigned)((M + a16f::ROWS - 1) / a16f::ROWS);
  const int lds = (int)a16f::lds_bytes((int)rp);
  auto run = [&](auto dt) {
    constexpr int DT = decltype(dt)::value, LIMIT = 160 * 1024;
    const char* const what = "quantize_act_xa (fused block-16 route)";
    switch (rp / 16) {  // 16-column tiles of the padded rank
      case 1: return launch_k<a16f::k_act16_fused<DT, 1>, LIMIT>(what, grid, 512, lds, st, x, M, ldx, K, Kp, a_frag, xq, xaq, qx, qa, L);
      case 2: return launch_k<a16f::k_act16_fused<DT, 2>, LIMIT>(what, grid, 512, lds, st, x, M, ldx, K, Kp, a_frag, xq, xaq, qx, qa, L);
      default: return launch_k<a16f::k_act16_fused<DT, 4>, LIMIT>(what, grid, 512, lds, st, x, M, ldx, K, Kp, a_frag, xq, xaq, qx, qa, L);
    }
  };
  return dtype == LQER_F16 ? run(std::integral_constant<int, LQER_F16>{}) : run(std::integral_constant<int, LQER_BF16>{});
}

}  // namespace lqer
