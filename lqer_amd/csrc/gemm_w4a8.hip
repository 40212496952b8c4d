// The fused W4 x A8 Linear kernel:
//
//   y[m,n] = sum_k xq[m,k] * Wq[n,k]  +  bq[n]  +  Q_Bout( sum_j xAq[m,j] * B[j,n] )
//
// replaces reference quantized_layers/linear.py:155-156 (torch.matmul(xA, B), B_out_quantizer,
// F.linear, add).  One workgroup = one 128(m) x 256(n) output tile (wide in n: a weight costs 0.56 B
// of L2->LDS traffic per element, an activation 2 B), 8 waves side by side along n, each
// wave 128 x 32 = 4 x 1 tiles of v_mfma_f32_32x32x16_bf16 (bf16 holds every MXINT value
// m * 2^e, |m| < 256, exactly; fp32 accumulation - SURVEY.md §7 H1 strategy S1).
//
// The MFMA is issued "transposed" (A operand = weight rows, B operand = token rows), so a lane owns
// one token row m and, per accumulator quad, 4 consecutive output columns n:
//   acc reg k of a 32x32 tile:  m = lane & 31,  n = (k & 3) + 8 (k >> 2) + 4 (lane >> 5).
// A B_out block (16 consecutive n of one token) is then 8 registers of lane l and 8 of lane l^32:
// 7 in-lane max + one v_permlane32_swap; and the output leaves as 16-byte stores.
//
//  * prologue: the rank-r product xAq @ B runs on the MFMA straight from global memory, is
//    re-quantized in registers, the bias is added, and the result is the INITIAL accumulator of the
//    main loop - there is no epilogue pass over the tile.
//  * main loop, BK = 64: every global access is an LDS-DMA (buffer_load ... lds, 16 B/lane) into a
//    4-slot ring, three k-steps ahead, retired with a COUNTED s_waitcnt vmcnt so that loads stay in
//    flight across barriers.  The activation tile is staged as bf16 (XOR swizzle on the source
//    address); the weights stay PACKED in LDS (4-bit codes + block exponents, 0.56 B per weight) and
//    each wave expands the fragments it needs in registers, in the shadow of its MFMAs - sign-magnitude nibbles
//    on the bf16 main loop without a table (common.h expand_frag_lin: 11 vector instructions per fragment with
//    its scale, 45 per wave and k-step in all; with the table 55).
//  * the two waves of a SIMD run half a k-step apart (LOAD / COMPUTE ping-pong, see the main loop).
//  * tiles are numbered so that each of the 8 XCDs works on a contiguous run of tiles (same token
//    rows -> the activation slab stays in that XCD's L2).
//
// This file holds the 128- and 64-row kernel and its launch.  What it shares with the other tile kernels is in gemm_tile.h; the
// pre-pass for B_out blocks other than 16 in bout_amax.hip; the dispatcher of all four routes in gemm_launch.hip.
#include <type_traits>
#include <utility>

#include "gemm_plan.h"
#include "gemm_tile.h"

namespace lqer {

#ifndef LQER_DEPTH
#define LQER_DEPTH 3
#endif
constexpr int DEPTH = LQER_DEPTH;                     // k-steps of prefetch in flight
constexpr int NSLOT = DEPTH + 1;                      // LDS ring slots
constexpr int R_SLOT = (BN / 16) * LQER_PANEL_BYTES;  // 9216 B  packed weight panels (4-bit codes + exponents)
constexpr int OFF_A = 0;
// per tile height (MT 32-row tiles): activation slot 16 KiB (128 rows) or 8 KiB (64 rows), bf16; the panels behind the ring
constexpr int a_slot_bytes(int mt) { return 32 * mt * BK * 2; }
constexpr int gemm_lds_bytes(int mt) { return NSLOT * a_slot_bytes(mt) + NSLOT * R_SLOT; }  // 102400 B / 69632 B (two workgroups per CU)
// KSPLIT: the stash of the side product's late operands is static LDS of the kernel, beside the ring's dynamic bytes (4 KiB of xAq
// fragments, then 2 KiB of B^T fragments per wave); behind the main loop the drained ring is the exchange of the wave pairs' partial
// sums, two m tiles = 8 KiB per wave at a time
constexpr int KS_STASH_B = 4096, KS_STASH_BYTES = KS_STASH_B + 8 * 2048, KS_XCH = 8192;
static_assert(8 * KS_XCH <= gemm_lds_bytes(4), "the exchange lies inside the ring");

// ---- LDS access in inline asm -------------------------------------------------------------------
// hipcc's waitcnt pass treats every global_load_lds in flight as a pending LDS write and puts
// s_waitcnt vmcnt(0) in front of any LDS access it can see, which would drain the prefetch ring every
// k-step.  Inside the main loop all LDS reads/writes are therefore asm statements the pass cannot
// see; completion is waited for explicitly (cdna_hip_programming.md §5.7 form (ii): the wait
// statement names every destination register "+v", so no consumer can be scheduled above it).
template <int OFF>
__device__ __forceinline__ bf16x8 lds_read128(uint32_t addr) {
  bf16x8 v;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "i"(OFF));
  return v;
}
__device__ __forceinline__ u32x4 lds_read128u(uint32_t addr) {
  u32x4 v;
  asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(addr));
  return v;
}
__device__ __forceinline__ uint32_t lds_read32_512(uint32_t addr) {
  uint32_t v;
  asm volatile("ds_read_b32 %0, %1 offset:512" : "=v"(v) : "v"(addr));
  return v;
}
__device__ __forceinline__ u32x2 lds_read64(uint32_t addr) {
  u32x2 v;
  asm volatile("ds_read_b64 %0, %1" : "=v"(v) : "v"(addr));
  return v;
}
__device__ __forceinline__ int lds_read_i8_512(uint32_t addr) {
  int v;
  asm volatile("ds_read_i8 %0, %1 offset:512" : "=v"(v) : "v"(addr));
  return v;
}
__device__ __forceinline__ void lds_write128(uint32_t addr, u32x4 v) {
  asm volatile("ds_write_b128 %0, %1" ::"v"(addr), "v"(v) : "memory");
}
template <int OFF>
__device__ __forceinline__ void lds_write128_at(uint32_t addr, f32x4 v) {
  asm volatile("ds_write_b128 %0, %1 offset:%2" ::"v"(addr), "v"(v), "i"(OFF) : "memory");
}
__device__ __forceinline__ void lds_wait(bf16x8& a, bf16x8& b, bf16x8& c, bf16x8& d) {
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
}
__device__ __forceinline__ void lds_wait(bf16x8& a, bf16x8& b) {
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a), "+v"(b));
}
__device__ __forceinline__ void lds_wait(u32x2& a, int& b) {
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a), "+v"(b));
}

#ifdef LQER_STAMPS
#define LQER_LOAD_BARRIER ""  // the diagnostic build stamps between the waits and the barrier
#else
#define LQER_LOAD_BARRIER "\n\ts_barrier"
#endif
#if defined(LQER_STAMPS) || defined(LQER_CLOCKPROBE)
__device__ unsigned long long* g_stamp_buf = nullptr;  // diagnostic builds only
#endif
#ifdef LQER_STAMPS
// Diagnostic build only: per-section cycle sums (s_memtime) of the main loop, written to a buffer that
// nothing else reads.  Never quote this build's run time (the stamps serialise the sections).
#define STAMP(i)                                                                        \
  do {                                                                                  \
    unsigned long long t_;                                                              \
    __builtin_amdgcn_sched_barrier(0);                                                  \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");         \
    __builtin_amdgcn_sched_barrier(0);                                                  \
    st_sum[i] += t_ - st_prev;                                                          \
    st_prev = t_;                                                                       \
  } while (0)
#else
#define STAMP(i)
#endif

// BOUT: 0 pass-through, 1 blocks of 16 (max in registers), 2 any block (max from the pre-pass).  STAGED: the side product's
// operands go through LDS (below) - a separate instantiation, so that the direct route keeps its own register allocation.
// MT: 32-row tiles per wave = tile height / 32.  4: the 128 x 256 tile.  2: a 64 x 256 tile for token counts whose 128-row
// grid leaves most of the chip idle (half the MFMA work per expanded weight fragment, twice the workgroups).
// WTWOS: the packed weight holds two's-complement nibbles (w_quantizer = integer, codes -8 .. 7): the second expand of common.h
// (128-row tiles, staged side path and 16-bit / fp32 tensors only: a format no template configuration uses gets a working
// kernel, not a tuned one).
// DEFER (round 6): the B_out re-quantization of the side product leaves the prologue.  There it was ~800 vector instructions per wave
// between the side product's MFMAs and the first k-step with nothing to hide behind: 3.5 of the 5.4 us in front of the main loop at
// 2048 x 4096 x 4096 (tools/clock_probe.py, "prologue split").  Here the side product stays in registers of its own (sp), the main
// loop opens on bias alone, its first 16 k-steps each carry one sixteenth of the re-quantization in the vector slots between their
// MFMAs (even piece: a block's maximum, exponent and scale factors; odd piece: its eight values), and sp is added behind the last
// k-step - as gemm_smallm.hip and decode1.hip always did.  Same formula (the scale exponent clamped to normal floats, exact while
// |x| <= 1e-8 passes through: gemm_w4a8_i8.hip's epilogue); blocks of 16, clamps up to 2^22 and K >= 1024 (launch_gemm).
// WMF: the packed weight holds minifloat codes (w_quantizer = minifloat, 2..4 bits): the magnitude code indexes the format's e4m3 table
// (g.w_lut, expand_frag_lut) instead of the integer one.  BOUT 3: a minifloat B_out, elementwise (minifloat_value) in the prologue.
// KSPLIT: the two waves of a SIMD (w and w + 4) share 128 rows x 64 columns and split the k-step between them: each reads the
// activation fragments of two of its four 16-deep slices (8 x 16 B instead of 16: half the LDS activation reads of the workgroup),
// expands the weight fragments of those slices for both 32-column halves (4 per step, as before) and issues the same 16 MFMAs, into
// acc (the half it will store) and acc_o (its partner's half).  Behind the main loop the pairs exchange acc_o through LDS, over the
// drained ring (two m tiles at a time), and each wave adds its partner's partial to its own.  Registers: acc + acc_o are 128, the fragments 32, so the
// deferred side product is held 64 rows at a time: m tiles 0 and 1 from the prologue (pieces 0-7, added behind step 7), m tiles
// 2 and 3 from operands the prologue stashes in static LDS and step 8 reads back (pieces 8-15, added behind step 15).
// DEFER with the direct side path and the table-free expand only (the instantiation of 2048 x 4096 -> 4096 at rank 32).
// (the body of both kernels below: the k split is k_lqer_gemm's deferred, direct instantiation; k_lqer_gemm_nks is that instantiation
// with every wave on all four slices, the geometry of the other instantiations)
template <int DT, bool LOWRANK, int BOUT, bool STAGED, int MT, bool WTWOS, bool DEFER, bool WMF, bool KSPLIT>
__device__ __forceinline__ void gemm_tile_body(const GemmArgs& g) {
  static_assert(MT == 4 || MT == 2, "128- or 64-row tiles");
  static_assert(!DEFER || (LOWRANK && BOUT == 1 && MT == 4), "deferred B_out: blocks of 16 on 128-row tiles");
  static_assert(!WTWOS || DT != LQER_F16X, "integer weights: no fp16 main loop");
  static_assert(!KSPLIT || (DEFER && !STAGED && !WTWOS && !WMF && DT != LQER_F16X), "k split: deferred B_out, direct side path, plain nibbles, bf16");
  constexpr int BMk = 32 * MT;   // tile rows
  constexpr int AP = MT / 2;     // 8-row LDS-DMA pieces of the activation tile per wave and k-step
  constexpr bool XF16 = DT == LQER_F16X;  // fp16 activation image, weights expanded to fp16, v_mfma_f32_32x32x16_f16
  constexpr int A_SLOT = a_slot_bytes(MT), OFF_R = NSLOT * A_SLOT;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // 8 waves side by side along n: each owns (KSPLIT: stores) all 128 token rows x 32 output columns.  KSPLIT: waves w and w + 4
  // hold columns 64 (w % 4) .. + 64 - the lower wave stores the first half - and kh is the wave's pair of k slices (2 kh, 2 kh + 1)
  const int kh = KSPLIT ? wave >> 2 : 0;
  const int wn = KSPLIT ? 2 * (wave & 3) + kh : wave;
  const int l31 = lane & 31, lh = lane >> 5;
#ifdef LQER_CLOCKPROBE
  unsigned long long cp_rin, cp_rq = 0;  // diagnostic build: the chip-wide 100 MHz counter at the wave's entry / in front of the B_out re-quantization
  asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(cp_rin)::"memory");
#endif

  const int tile = xcd_tile(blockIdx.x, g.tiles_m * g.tiles_n);
  const int tm = tile / g.tiles_n, tn = tile - tm * g.tiles_n;
  const int m0 = tm * BMk, n0 = tn * BN;
  const int nk = g.Kp / BK;

  // ---- staging ------------------------------------------------------------------------------
  // activation: wave w stages tile rows [16w, 16w+16): 2 x LDS-DMA of 8 rows x 128 B.  Buffer
  // addressing: wave-uniform descriptor + per-lane byte offset fixed for the whole kernel + the
  // k-step as scalar offset, so a prefetch costs no vector ALU work.
  const auto a_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)(g.xq + (int64_t)m0 * g.Kp), 0, BMk * g.Kp * 2, 0x00020000);
  int a_voff[2] = {0, 0};  // (AP entries used; a dependent-size array here makes hipcc's HOST pass drop the kernel's stub silently)
#pragma unroll
  for (int i = 0; i < AP; ++i) {
    const int row = wave * (8 * AP) + i * 8 + (lane >> 3);
    const int chunk = (lane & 7) ^ ((row >> 1) & 7);
    a_voff[i] = (row * g.Kp + chunk * 8) * 2;
  }
  // weights: nine 1-KiB pieces per k-step (gemm_tile.h w_piece_voff): wave w issues piece w, wave 0 also piece 8 -
  // 25 LDS-DMA instructions per k-step and workgroup, all with full EXEC.
  const uint8_t* w_base = g.wp + ((int64_t)(n0 / 16) * nk) * LQER_PANEL_BYTES;
  const auto w_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)w_base, 0, 16 * nk * LQER_PANEL_BYTES, 0x00020000);
  const int w_voff = w_piece_voff(wave, lane, nk), w_voff8 = w_piece_voff(8, lane, nk);
  unsigned char* const a_dst0 = smem + OFF_A + wave * (8 * AP) * 128;  // + slot * A_SLOT + piece * 1024
  unsigned char* const w_dst0 = smem + OFF_R + wave * 1024;      // + slot * R_SLOT
  auto issue_loads = [&](int kt, int slot) {  // 3 LDS-DMA instructions per wave (wave 0: 4)
#pragma unroll
    for (int i = 0; i < AP; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(a_rsrc, (lds_void*)(a_dst0 + slot * A_SLOT + i * 1024), 16, a_voff[i],
                                               kt * (BK * 2), 0, 0);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(w_rsrc, (lds_void*)(w_dst0 + slot * R_SLOT), 16, w_voff, kt * LQER_PANEL_BYTES, 0, 0);
    if (wave == 0)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(w_rsrc, (lds_void*)(smem + OFF_R + 8192 + slot * R_SLOT), 16, w_voff8,
                                               kt * LQER_PANEL_BYTES, 0, 0);
  };
  // fragment read addresses (slot 0).  Activation: row = wave tile row + lane & 31, chunk 2 ks + (lane >> 5),
  // swizzled; the second m tile is +32 rows = +4096 B (row + 32 keeps (row >> 1) & 7).
  const uint32_t lds0 = (uint32_t)(uintptr_t)(lds_void*)smem;
  uint32_t stash0 = 0;  // KSPLIT: the stash of the side product's late operands
  if constexpr (KSPLIT) {
    __shared__ __attribute__((aligned(16))) unsigned char ks_stash[KS_STASH_BYTES];
    stash0 = (uint32_t)(uintptr_t)(lds_void*)ks_stash;
  }
  uint32_t fa_addr[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) fa_addr[ks] = lds0 + OFF_A + swz(l31, 2 * (KSPLIT ? (2 * kh + ks) & 3 : ks) + lh);  // m tile i: + i * 4096 (KSPLIT: [0], [1] are the wave's two slices)
  // Packed weights: weight row n = wave tile column + lane & 31 lives in panel n / 16 at row n % 16; its
  // 32 B of codes hold the words of chunks {0,2,4,6} then {1,3,5,7}, so the lane's 4 words (chunk
  // 2 ks + (lane >> 5), ks = 0..3) are one 16-byte read; its 4 biased block exponents are one 4-byte read.
  const int nw = wn * 32 + l31;
  const uint32_t fw_addr = lds0 + OFF_R + (nw >> 4) * LQER_PANEL_BYTES + (nw & 15) * 32 + lh * 16;
  const uint32_t fe_addr = lds0 + OFF_R + (nw >> 4) * LQER_PANEL_BYTES + (nw & 15) * 4;  // + 512
  // KSPLIT: the wave's two slices are 8 of those 16 bytes of codes and 2 of the 4 exponent bytes, for its own column half and (+-
  // two panels) for its partner's
  const uint32_t ks_fw = fw_addr + 8 * kh, ks_fe = fe_addr + 2 * kh;
  const uint32_t ks_fw_o = kh ? ks_fw - 2 * LQER_PANEL_BYTES : ks_fw + 2 * LQER_PANEL_BYTES;
  const uint32_t ks_fe_o = kh ? ks_fe - 2 * LQER_PANEL_BYTES : ks_fe + 2 * LQER_PANEL_BYTES;

  // ---- side path, first half: fetch before the ring prefetch -----------------------------------------------------
  // acc = Q_Bout(xAq @ B) + bias opens the accumulators.  The tile's rows of xAq are staged through LDS - 64 rank
  // entries per pass, in the ring slot that is not yet a prefetch target (slot DEPTH), in the activation tile's own
  // swizzled layout - and this wave's B^T fragments of a pass are fetched in one batch: one memory latency per pass
  // instead of one per 16-deep slice, no 8-fold refetch of xAq by the 8 waves.  The loads of pass 0 are issued BEFORE
  // the ring prefetch (loads return in order: their results can then be awaited while the prefetch is in flight), and
  // the staging writes / fragment reads are asm statements, invisible to the waitcnt pass (see above).
  constexpr int STG = STAGED ? BMk * 8 / 512 : 1;  // staged 16-byte chunks per thread and pass
  u32x4 stg[STG];
  bf16x8 sb[STAGED ? 2 : 1][STAGED ? 4 : 1];  // B^T fragments of one limb of the pass, double-buffered
  const uint32_t stage = lds0 + OFF_A + (NSLOT - 1) * A_SLOT;
  const bf16_t* const bt_row = STAGED ? g.bt + (int64_t)(n0 + wn * 32 + l31) * g.rp + 8 * lh : nullptr;
  auto side_fetch_b = [&](int p0, int l, auto buf_c) {  // limb l of this wave's B^T fragments -> sb[buf]
    constexpr int BUF = decltype(buf_c)::value;
    if constexpr (STAGED) {
      const int cols = g.rp - p0 < 64 ? g.rp - p0 : 64;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
        if (l < g.b_limbs && ks * 16 < cols) sb[BUF][ks] = *(const bf16x8*)(bt_row + (int64_t)l * g.Np * g.rp + p0 + ks * 16);
    }
  };
  auto side_fetch = [&](int p0) {
    if constexpr (!STAGED) return;
    const int cols = g.rp - p0 < 64 ? g.rp - p0 : 64;  // a multiple of 16
    const int cpr = cols >> 3;                          // 16-byte chunks per row
#pragma unroll
    for (int j = 0; j < STG; ++j) {
      const int c = tid + 512 * j;
      if (c < BMk * cpr) {
        const int row = c / cpr, ch = c - row * cpr;
        stg[j] = *(const u32x4*)(g.xaq + (int64_t)(m0 + row) * g.xaq_ld + p0 + 8 * ch);
      }
    }
    side_fetch_b(p0, 0, std::integral_constant<int, 0>{});
  };
  // (a side product of at most two 16-deep slices - rank <= 32 with one limb - is cheaper fetched directly: the two
  // barriers of the staged route cost more than they save there; launch_gemm picks the instantiation)
  constexpr bool side_staged = LOWRANK && STAGED;
  if constexpr (side_staged) side_fetch(0);
  // direct route (at most two 16-deep slices: rank <= 32 with one limb, or rank 16 with two): both slices' operands
  // are requested here, ahead of the ring prefetch, instead of one slice at a time behind it
  constexpr bool side_direct = LOWRANK && !STAGED;
  bf16x8 db[side_direct ? 2 : 1], dx[side_direct ? 2 : 1][side_direct ? MT : 1];
  const bool two_limbs = g.b_limbs > 1;  // (then rank 16: slice s = limb s; else slice s = rank entries 16 s ..)
  if constexpr (side_direct) {
#pragma unroll
    for (int sl = 0; sl < 2; ++sl) {
      const int l = two_limbs ? sl : 0, ks = two_limbs ? 0 : sl;
      if constexpr (KSPLIT) {  // (a slice that does not exist is stashed as zeros: step 8 multiplies both without a branch)
        db[sl] = bf16x8{};
        dx[sl][2] = dx[sl][3] = bf16x8{};
      }
      if (l < g.b_limbs && ks * 16 < g.rp) {
        db[sl] = *(const bf16x8*)(g.bt + ((int64_t)l * g.Np + n0 + wn * 32 + l31) * g.rp + ks * 16 + 8 * lh);
#pragma unroll
        for (int i = 0; i < MT; ++i) dx[sl][i] = *(const bf16x8*)(g.xaq + (int64_t)(m0 + i * 32 + l31) * g.xaq_ld + ks * 16 + 8 * lh);
      }
    }
  }

  // prologue loads: steps 0 .. DEPTH-1
#pragma unroll
  for (int d = 0; d < DEPTH; ++d) issue_loads(d, d);  // (past the end of K: dropped by the buffer range check)

  f32x16 acc[MT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int k = 0; k < 16; ++k) acc[i][k] = 0.f;
  constexpr int SPT = KSPLIT ? 2 : MT;  // m tiles of the side product held at a time
  f32x16 sp[DEFER ? SPT : 1];  // DEFER: the side product, re-quantized in place during the first k-steps
  if constexpr (DEFER) {
#pragma unroll
    for (int i = 0; i < SPT; ++i)
#pragma unroll
      for (int k = 0; k < 16; ++k) sp[i][k] = 0.f;
  }
  f32x16 acc_o[KSPLIT ? MT : 1];  // KSPLIT: the partial sums of the partner's column half
  if constexpr (KSPLIT) {
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int k = 0; k < 16; ++k) acc_o[i][k] = 0.f;
  }
  auto side_acc = [&](int i) -> f32x16& {
    if constexpr (DEFER) return sp[i];
    else return acc[i];
  };

  // ---- low-rank prologue: acc = Q_Bout(xAq @ B) + bias ----------------------------------------
  if constexpr (LOWRANK) {
    if constexpr (side_direct) {
#pragma unroll
      for (int sl = 0; sl < 2; ++sl) {
        const int l = two_limbs ? sl : 0, ks = two_limbs ? 0 : sl;
        if (l < g.b_limbs && ks * 16 < g.rp) {
#pragma unroll
          for (int i = 0; i < SPT; ++i) side_acc(i) = __builtin_amdgcn_mfma_f32_32x32x16_bf16(db[sl], dx[sl][i], side_acc(i), 0, 0, 0);
        }
      }
      if constexpr (KSPLIT) {
        // the operands of m tiles 2 and 3 wait in LDS for step 8: the activation side's fragments are the same in every wave
        // (wave 0 writes them), the B^T fragments are the wave's own
        const uint32_t st_b = stash0 + KS_STASH_B + wave * 2048 + lane * 16, st_x = stash0 + lane * 16;
#pragma unroll
        for (int sl = 0; sl < 2; ++sl) {
          lds_write128(st_b + sl * 1024, __builtin_bit_cast(u32x4, db[sl]));
          if (wave == 0) {
            lds_write128(st_x + (2 * sl) * 1024, __builtin_bit_cast(u32x4, dx[sl][2]));
            lds_write128(st_x + (2 * sl + 1) * 1024, __builtin_bit_cast(u32x4, dx[sl][3]));
          }
        }
      }
    }
    if constexpr (side_staged)
    for (int p0 = 0; p0 < g.rp; p0 += 64) {
      const int cols = g.rp - p0 < 64 ? g.rp - p0 : 64;
      const int cpr = cols >> 3;
      if (p0) {
        asm volatile("s_barrier" ::: "memory");  // the previous pass's fragment reads are done (lgkmcnt(0) below)
        side_fetch(p0);
      }
#pragma unroll
      for (int j = 0; j < STG; ++j) {
        const int c = tid + 512 * j;
        if (c < BMk * cpr) {
          const int row = c / cpr, ch = c - row * cpr;
          lds_write128(stage + swz(row, ch), stg[j]);
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      auto limb = [&](int l, auto buf_c) {
        constexpr int BUF = decltype(buf_c)::value;
        if (l >= g.b_limbs) return;
        side_fetch_b(p0, l + 1, std::integral_constant<int, BUF ^ 1>{});  // the next limb's fragments, under this limb's MFMAs
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
          if (ks * 16 < cols) {
            const uint32_t fa = stage + swz(l31, 2 * ks + lh);  // m tile i: + i * 4096 (row + 32 keeps the swizzle)
            if constexpr (MT == 4) {
              bf16x8 x0 = lds_read128<0>(fa), x1 = lds_read128<4096>(fa), x2 = lds_read128<8192>(fa), x3 = lds_read128<12288>(fa);
              lds_wait(x0, x1, x2, x3);
              side_acc(0) = __builtin_amdgcn_mfma_f32_32x32x16_bf16(sb[BUF][ks], x0, side_acc(0), 0, 0, 0);
              side_acc(1) = __builtin_amdgcn_mfma_f32_32x32x16_bf16(sb[BUF][ks], x1, side_acc(1), 0, 0, 0);
              side_acc(2) = __builtin_amdgcn_mfma_f32_32x32x16_bf16(sb[BUF][ks], x2, side_acc(2), 0, 0, 0);
              side_acc(3) = __builtin_amdgcn_mfma_f32_32x32x16_bf16(sb[BUF][ks], x3, side_acc(3), 0, 0, 0);
            } else {
              bf16x8 x0 = lds_read128<0>(fa), x1 = lds_read128<4096>(fa);
              lds_wait(x0, x1);
              acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(sb[BUF][ks], x0, acc[0], 0, 0, 0);
              acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(sb[BUF][ks], x1, acc[1], 0, 0, 0);
            }
          }
      };
      limb(0, std::integral_constant<int, 0>{});
      limb(1, std::integral_constant<int, 1>{});
      limb(2, std::integral_constant<int, 0>{});
    }
#ifdef LQER_CLOCKPROBE
    asm volatile("s_waitcnt vmcnt(6)\n\ts_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(cp_rq)::"memory");  // side operands landed, MFMAs issued
#endif
    if constexpr (BOUT == 3) {  // minifloat: per element, no maxima
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int k = 0; k < 16; ++k) acc[i][k] = minifloat_value(acc[i][k], g.bout);
    } else if constexpr (BOUT != 0 && !DEFER) {
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          float amax;
          if constexpr (BOUT == 1) {
            amax = 0.f;
#pragma unroll
            for (int k = 0; k < 8; ++k) amax = fmaxf(amax, fabsf(acc[i][8 * b + k]));
            amax = pair32_max(amax);
          } else {
            // block of L columns (L a multiple of 16): its max was reduced by k_bout_amax.  (No buffer: the integer
            // quantizer - fixed point, its "exponent" is pinned to 0 by the QP's clamp whatever amax says)
            amax = g.bout_amax ? g.bout_amax[(int64_t)(m0 + i * 32 + l31) * g.bout_nblk + (n0 + wn * 32 + 16 * b) / g.bout_L] : 1.0f;
          }
          const int e = block_exponent(amax, g.bout);  // amax = 0: every element takes the pass-through
          float blk[8];
#pragma unroll
          for (int k = 0; k < 8; ++k) blk[k] = acc[i][8 * b + k];
          mxint_requant_fast(blk, e, g.bout);  // two elements per packed fp32 instruction (common.h)
#pragma unroll
          for (int k = 0; k < 8; ++k) acc[i][8 * b + k] = blk[k];
        }
    }
  }
  if (g.bias) {
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const float bv = g.bias[acc_col(n0 + wn * 32, k, lh)];
#pragma unroll
      for (int i = 0; i < MT; ++i) acc[i][k] += bv;
    }
  }

  // ---- main loop ------------------------------------------------------------------------------
  // Ping-pong: the two waves that share a SIMD (w and w+4) run one barrier apart.  A k-step is
  //   LOAD(kt):    read this wave's operands of step kt from ring slot kt % 4 into registers (8 x 16 B of
  //                activation fragments, 2 x 16 B of weight codes, 2 x 4 B of block exponents), issue the
  //                loads of step kt+3 into slot (kt+3) % 4, wait, barrier;
  //   COMPUTE(kt): per 16-deep k slice expand two weight fragments (VALU) and issue 4 MFMAs; barrier.
  // While waves 0-3 compute, waves 4-7 load, and vice versa:
  //   barrier index      2kt-1        2kt          2kt+1         2kt+2
  //   waves 0-3:    ... | LOAD(kt)  | COMPUTE(kt) | LOAD(kt+1)  | ...
  //   waves 4-7:    ... | COMP(kt-1)| LOAD(kt)    | COMPUTE(kt) | ...
  // RAW: every wave ends LOAD(kt-1) with a counted vmcnt that retires its own loads of step kt (the
  // DEPTH-1 younger batches of 3 stay in flight) and then passes a barrier (2kt-2 or 2kt-1) before
  // anyone starts LOAD(kt).  WAR: slot (kt+3) % 4 held step kt-1, last read in LOAD(kt-1) of waves 4-7,
  // which ends (lgkmcnt(0)) before barrier 2kt-1; the overwriting loads are issued after it.
  const bool late = wave >= 4;
  // loads(0) landed; two batches of AP + 1 (3, or 2 with 64-row tiles) may stay in flight
  if constexpr (KSPLIT) asm volatile("s_waitcnt vmcnt(6) lgkmcnt(0)\n\ts_barrier" ::: "memory");  // (and the stash is written)
  else if constexpr (MT == 4) asm volatile("s_waitcnt vmcnt(6)\n\ts_barrier" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(4)\n\ts_barrier" ::: "memory");
  if (late) asm volatile("s_barrier" ::: "memory");
#ifdef LQER_CLOCKPROBE
  // diagnostic build: shader cycles (s_memtime) and 100 MHz ticks (s_memrealtime) around the whole main loop
  unsigned long long cp_c0, cp_r0;
  asm volatile("s_memtime %0\n\ts_memrealtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(cp_c0), "=s"(cp_r0)::"memory");
#endif
#ifdef LQER_STAMPS
  unsigned long long st_sum[8] = {0, 0, 0, 0, 0, 0, 0, 0}, st_prev;
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(st_prev)::"memory");
#endif
  // hand-built buffer descriptors for the in-asm LDS-DMA (gemm_tile.h ring_rsrc_base): the tile's rows of xq, the column tile's panels
  const u32x2 a_rs01 = ring_rsrc_base(g.xq + (int64_t)m0 * g.Kp);
  const u32x4 a_rs = {a_rs01[0], a_rs01[1], (uint32_t)(BMk * g.Kp * 2), 0x00020000u};
  const u32x2 w_rs01 = ring_rsrc_base(w_base);
  const u32x4 w_rs = {w_rs01[0], w_rs01[1], (uint32_t)(16 * nk * LQER_PANEL_BYTES), 0x00020000u};
  const uint32_t m0_a = lds0 + OFF_A + wave * (8 * AP) * 128;  // + slot * A_SLOT (+ 1024: second piece)
  const uint32_t m0_w = lds0 + OFF_R + wave * 1024;      // + slot * R_SLOT
  const uint32_t m0_w8 = lds0 + OFF_R + 8192;            // + slot * R_SLOT (piece 8, wave 0)
  // One k-step.  The ring slot is a compile-time constant (the loop below is unrolled by the ring size), so every
  // LDS address is a per-lane base register + an immediate offset and the LDS-DMA destinations are constants.
  // LOAD(kt) is ONE asm statement (a compiler-visible gap between LDS reads and their wait lets hipcc copy registers
  // that have not landed): the 18 LDS reads first, then the LDS-DMA prefetch of step kt+3 - the reads' latency passes
  // while the DMA instructions issue -, then the counted waits.  The step's first weight fragment is expanded in the
  // slack left before the barrier, so that COMPUTE opens with an MFMA.  The loading wave has issue priority over
  // its computing SIMD partner (whose MFMAs only need an issue slot every 32 cycles).
  // DEFER piece P of k-step P (0..15): block j = P / 2 = (m tile j / 2, column half j % 2) of the side product.  Straight-line vector
  // code only (no branch: it has to share the COMPUTE section's scheduling region with the MFMAs it hides behind).
  float dq_s = 1.f, dq_inv = 1.f;  // scale factors 2^(mbits - e), 2^(e - mbits) of the block between its two pieces
  auto defer_piece = [&](auto piece_c) {
    constexpr int P = decltype(piece_c)::value;
    if constexpr (DEFER && P >= 0) {
      typedef __attribute__((ext_vector_type(2))) float f2;
      constexpr int J = P >> 1, I = (J >> 1) % SPT, B8 = 8 * (J & 1);  // (KSPLIT: sp holds m tiles 0, 1, from step 8 on m tiles 2, 3)
      if constexpr ((P & 1) == 0) {
        float amax = 0.f;
#pragma unroll
        for (int k = 0; k < 8; k += 2) amax = fmaxf(fmaxf(amax, fabsf(sp[I][B8 + k])), fabsf(sp[I][B8 + k + 1]));
        amax = pair32_max(amax);
        // (mbits - e clamped to the exponents of normal floats: beyond, every element of the block is below 1e-8 and passes through)
        int up = g.bout.mbits - block_exponent(amax, g.bout);
        up = up > 126 ? 126 : (up < -126 ? -126 : up);
        dq_s = __uint_as_float((uint32_t)(127 + up) << 23);
        dq_inv = __uint_as_float((uint32_t)(127 - up) << 23);
      } else {
        const float es = g.bout.eps * dq_s, hi = g.bout.mmax, lo = -g.bout.mneg, tiny = g.bout.tiny;
        const f2 magic = {12582912.0f, 12582912.0f};
#pragma unroll
        for (int k = 0; k < 8; k += 2) {
          const f2 x = {sp[I][B8 + k], sp[I][B8 + k + 1]};
          const f2 c = {copysignf(es, x[0]), copysignf(es, x[1])};
          f2 r = (__builtin_elementwise_fma(x, (f2){dq_s, dq_s}, c) + magic) - magic;
          r[0] = __builtin_amdgcn_fmed3f(r[0], lo, hi);
          r[1] = __builtin_amdgcn_fmed3f(r[1], lo, hi);
          const f2 val = r * (f2){dq_inv, dq_inv};
          sp[I][B8 + k] = fabsf(x[0]) <= tiny ? x[0] : val[0];
          sp[I][B8 + k + 1] = fabsf(x[1]) <= tiny ? x[1] : val[1];
        }
      }
    }
  };
  // (the piece's results are needed a k-step later, or behind the loop: without a use inside the section hipcc sinks the whole
  // computation to that use - all sixteen pieces ended up behind the main loop.  An empty asm that "modifies" them pins them here)
  auto defer_pin = [&](auto piece_c) {
    constexpr int P = decltype(piece_c)::value;
    (void)dq_s, (void)dq_inv, (void)sp;  // (captured here: operands of an asm statement inside a dependent branch do not make a capture)
    if constexpr (DEFER && P >= 0) {
      constexpr int J = P >> 1, I = (J >> 1) % SPT, B8 = 8 * (J & 1);  // (KSPLIT: sp holds m tiles 0, 1, from step 8 on m tiles 2, 3)
      if constexpr ((P & 1) == 0) asm volatile("" : "+v"(dq_s), "+v"(dq_inv));
      else
        asm volatile("" : "+v"(sp[I][B8]), "+v"(sp[I][B8 + 1]), "+v"(sp[I][B8 + 2]), "+v"(sp[I][B8 + 3]), "+v"(sp[I][B8 + 4]), "+v"(sp[I][B8 + 5]),
                     "+v"(sp[I][B8 + 6]), "+v"(sp[I][B8 + 7]));
    }
  };
  auto step = [&](int kt, auto slot_c, auto piece_c) {
    constexpr int SLOT = decltype(slot_c)::value;
    constexpr int slot_new = SLOT == 0 ? NSLOT - 1 : SLOT - 1;  // (slot + DEPTH) % NSLOT
    STAMP(7);
    __builtin_amdgcn_s_setprio(1);
    const int ktn = __builtin_amdgcn_readfirstlane(kt + DEPTH);
    const int a_soff = ktn * (BK * 2), w_soff = ktn * LQER_PANEL_BYTES;
    const uint32_t m0a0 = m0_a + slot_new * A_SLOT, m0a1 = m0a0 + 1024;
    const uint32_t m0w = m0_w + slot_new * R_SLOT, m0w8 = m0_w8 + slot_new * R_SLOT;
    bf16x8 xa[4][MT];  // [ks][m tile]
    u32x4 wr;
    uint32_t we;
    constexpr int P = decltype(piece_c)::value;
    u32x2 wr2[2];      // KSPLIT: the code words of the wave's two slices, [own half, partner's half]
    uint32_t we2[2];   // ... and their two exponent bytes
    bf16x8 sdb[2], sdx[2][2];  // KSPLIT, step 8: the stashed side operands of m tiles 2 and 3
    if constexpr (KSPLIT) {
      if constexpr (P == 8) {
        const uint32_t st_b = stash0 + KS_STASH_B + wave * 2048 + lane * 16, st_x = stash0 + lane * 16;
        asm volatile(
            "ds_read_b128 %0, %6\n\tds_read_b128 %1, %6 offset:1024\n\t"
            "ds_read_b128 %2, %7\n\tds_read_b128 %3, %7 offset:1024\n\tds_read_b128 %4, %7 offset:2048\n\tds_read_b128 %5, %7 offset:3072\n\t"
            "s_waitcnt lgkmcnt(0)"
            : "=&v"(sdb[0]), "=&v"(sdb[1]), "=&v"(sdx[0][0]), "=&v"(sdx[0][1]), "=&v"(sdx[1][0]), "=&v"(sdx[1][1])
            : "v"(st_b), "v"(st_x)
            : "memory");
      }
      asm volatile(
          "ds_read_b64 %[w0], %[fw] offset:%c[ro]\n\tds_read_b64 %[w1], %[fwo] offset:%c[ro]\n\t"
          "ds_read_u16 %[e0], %[fe] offset:%c[ro]+512\n\tds_read_u16 %[e1], %[feo] offset:%c[ro]+512\n\t"
          LQER_READ_X2("%[x00]", "%[x01]", "%[fa0]", "%c[ao]") LQER_READ_X2("%[x02]", "%[x03]", "%[fa0]", "%c[ao]+8192")
          LQER_READ_X2("%[x10]", "%[x11]", "%[fa1]", "%c[ao]") LQER_READ_X2("%[x12]", "%[x13]", "%[fa1]", "%c[ao]+8192")
          LQER_LDS_DMA("%[ma0]", "%[av0]", "%[ars]", "%[aso]") LQER_LDS_DMA("%[ma1]", "%[av1]", "%[ars]", "%[aso]")
          LQER_LDS_DMA("%[mw]", "%[wv]", "%[wrs]", "%[wso]")
          "s_cmp_lg_u32 %[wv0], 0\n\ts_cbranch_scc1 1f\n\t"
          LQER_LDS_DMA("%[mw8]", "%[wv8]", "%[wrs]", "%[wso]")
          "1:\n\ts_waitcnt vmcnt(6) lgkmcnt(0)"  // (as below)
          : [w0] "=&v"(wr2[0]), [w1] "=&v"(wr2[1]), [e0] "=&v"(we2[0]), [e1] "=&v"(we2[1]), [x00] "=&v"(xa[0][0]), [x01] "=&v"(xa[0][1]),
            [x02] "=&v"(xa[0][2]), [x03] "=&v"(xa[0][3]), [x10] "=&v"(xa[1][0]), [x11] "=&v"(xa[1][1]), [x12] "=&v"(xa[1][2]),
            [x13] "=&v"(xa[1][3])
          : [fw] "v"(ks_fw), [fwo] "v"(ks_fw_o), [fe] "v"(ks_fe), [feo] "v"(ks_fe_o), [fa0] "v"(fa_addr[0]), [fa1] "v"(fa_addr[1]),
            [ao] "i"(SLOT * A_SLOT), [ro] "i"(SLOT * R_SLOT), [av0] "v"(a_voff[0]), [av1] "v"(a_voff[1]), [wv] "v"(w_voff),
            [wv8] "v"(w_voff8), [ars] "s"(a_rs), [wrs] "s"(w_rs), [ma0] "s"(m0a0), [ma1] "s"(m0a1), [mw] "s"(m0w), [mw8] "s"(m0w8),
            [aso] "s"(a_soff), [wso] "s"(w_soff), [wv0] "s"(wave)
          : "memory", "scc");
    } else if constexpr (MT == 4) {
      asm volatile(
          "ds_read_b128 %0, %18 offset:%c25\n\tds_read_b32 %1, %19 offset:%c25+512\n\t"
          LQER_READ_X2("%2", "%3", "%20", "%c24") LQER_READ_X2("%4", "%5", "%20", "%c24+8192")
          LQER_READ_X2("%6", "%7", "%21", "%c24") LQER_READ_X2("%8", "%9", "%21", "%c24+8192")
          LQER_READ_X2("%10", "%11", "%22", "%c24") LQER_READ_X2("%12", "%13", "%22", "%c24+8192")
          LQER_READ_X2("%14", "%15", "%23", "%c24") LQER_READ_X2("%16", "%17", "%23", "%c24+8192")
          LQER_LDS_DMA("%32", "%26", "%30", "%36") LQER_LDS_DMA("%33", "%27", "%30", "%36") LQER_LDS_DMA("%34", "%28", "%31", "%37")
          "s_cmp_lg_u32 %38, 0\n\ts_cbranch_scc1 1f\n\t"
          LQER_LDS_DMA("%35", "%29", "%31", "%37")
          // own loads of step kt+1 landed: the batches of kt+2 and kt+3 (3 loads each, wave 0: 4 - it waits a little
          // more than it must) may stay in flight
          "1:\n\ts_waitcnt vmcnt(6) lgkmcnt(0)"
          : "=&v"(wr), "=&v"(we), "=&v"(xa[0][0]), "=&v"(xa[0][1]), "=&v"(xa[0][2]), "=&v"(xa[0][3]), "=&v"(xa[1][0]),
            "=&v"(xa[1][1]), "=&v"(xa[1][2]), "=&v"(xa[1][3]), "=&v"(xa[2][0]), "=&v"(xa[2][1]), "=&v"(xa[2][2]),
            "=&v"(xa[2][3]), "=&v"(xa[3][0]), "=&v"(xa[3][1]), "=&v"(xa[3][2]), "=&v"(xa[3][3])
          : "v"(fw_addr), "v"(fe_addr), "v"(fa_addr[0]), "v"(fa_addr[1]), "v"(fa_addr[2]), "v"(fa_addr[3]),  // 18..23
            "i"(SLOT * A_SLOT), "i"(SLOT * R_SLOT),                                                         // 24, 25
            "v"(a_voff[0]), "v"(a_voff[1]), "v"(w_voff), "v"(w_voff8),                                       // 26..29
            "s"(a_rs), "s"(w_rs), "s"(m0a0), "s"(m0a1), "s"(m0w), "s"(m0w8), "s"(a_soff), "s"(w_soff), "s"(wave)  // 30..38
          : "memory", "scc");  // (s_cmp inside)
    } else {  // 64-row tile: two m tiles per k slice, one activation piece per wave
      asm volatile(
          "ds_read_b128 %0, %10 offset:%c17\n\tds_read_b32 %1, %11 offset:%c17+512\n\t"
          LQER_READ_X2("%2", "%3", "%12", "%c16") LQER_READ_X2("%4", "%5", "%13", "%c16")
          LQER_READ_X2("%6", "%7", "%14", "%c16") LQER_READ_X2("%8", "%9", "%15", "%c16")
          LQER_LDS_DMA("%23", "%18", "%21", "%26") LQER_LDS_DMA("%24", "%19", "%22", "%27")
          "s_cmp_lg_u32 %28, 0\n\ts_cbranch_scc1 1f\n\t"
          LQER_LDS_DMA("%25", "%20", "%22", "%27")
          "1:\n\ts_waitcnt vmcnt(4) lgkmcnt(0)"
          : "=&v"(wr), "=&v"(we), "=&v"(xa[0][0]), "=&v"(xa[0][1]), "=&v"(xa[1][0]), "=&v"(xa[1][1]), "=&v"(xa[2][0]),
            "=&v"(xa[2][1]), "=&v"(xa[3][0]), "=&v"(xa[3][1])
          : "v"(fw_addr), "v"(fe_addr), "v"(fa_addr[0]), "v"(fa_addr[1]), "v"(fa_addr[2]), "v"(fa_addr[3]),  // 10..15
            "i"(SLOT * A_SLOT), "i"(SLOT * R_SLOT),                                                         // 16, 17
            "v"(a_voff[0]), "v"(w_voff), "v"(w_voff8),                                                       // 18..20
            "s"(a_rs), "s"(w_rs), "s"(m0a0), "s"(m0w), "s"(m0w8), "s"(a_soff), "s"(w_soff), "s"(wave)         // 21..28
          : "memory", "scc");
    }
    STAMP(1);  // LDS reads + DMA issue + waits
    // sign-magnitude nibbles on the bf16 main loop: the table-free expand (expand_frag_lin), its 2^9 added to the step's four
    // exponent bytes at once (no carry: the plan sends an image with a byte beyond LIN_EXP_BYTE_MAX to the WMF instantiation)
    constexpr bool WLIN = !WMF && !WTWOS && !XF16;
    if constexpr (WLIN && !KSPLIT) we += 0x09090909u;
    auto expand = [&](uint32_t word, uint32_t scale_bits) {
      if constexpr (WMF) return expand_frag_lut(word, scale_bits, g.w_lut[0], g.w_lut[1]);
      else if constexpr (WTWOS) return expand_frag_twos(word, scale_bits);
      else if constexpr (WLIN) return expand_frag_lin(word, scale_bits);
      else return expand_frag_t<XF16>(word, scale_bits);
    };
    if constexpr (KSPLIT) {
      we2[0] += 0x0909u, we2[1] += 0x0909u;
      wr[0] = wr2[0][0], we = we2[0];
    }
    bf16x8 wb_first = expand(wr[0], exp_byte_bits<0>(we));
    asm volatile("s_barrier" : "+v"(wb_first)::"memory");
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
    STAMP(4);  // expand of the first fragment + barrier
    // ---- COMPUTE(kt)
    if constexpr (KSPLIT && P == 8) {  // m tiles 0 and 1 of the side product are done: add them, and multiply m tiles 2 and 3
#pragma unroll
      for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int k = 0; k < 16; ++k) acc[i][k] += sp[i][k], sp[i][k] = 0.f;
#pragma unroll
        for (int sl = 0; sl < 2; ++sl) sp[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(sdb[sl], sdx[sl][i], sp[i], 0, 0, 0);
      }
    }
    defer_piece(piece_c);
    if constexpr (KSPLIT) {
      // [column half][slice] -> fp32 bits of the block scale 2^(e - mbits + 9)
      const uint32_t sc[2][2] = {{0u, exp_byte_bits<1>(we2[0])}, {exp_byte_bits<0>(we2[1]), exp_byte_bits<1>(we2[1])}};  // ([0][0]: wb_first has it)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const bf16x8 wb = j + h == 0 ? wb_first : expand(wr2[h][j], sc[h][j]);
#pragma unroll
          for (int i = 0; i < MT; ++i) {
            if (h) acc_o[i] = mfma_32x32x16<XF16>(wb, xa[j][i], acc_o[i]);
            else acc[i] = mfma_32x32x16<XF16>(wb, xa[j][i], acc[i]);
          }
        }
      // one wave feeds the SIMD's MFMA pipe during COMPUTE: the next fragment's 11 vector instructions go three at a time into the
      // shadows of the four MFMAs of this one (a clump of 11 between two MFMAs leaves the pipe idle)
      if constexpr (P < 0) {
#pragma unroll
        for (int n = 0; n < 16; ++n) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);
        }
      }
    } else {
      // biased exponent byte ks -> fp32 bits of the block scale 2^(e - mbits)
      const uint32_t sc[4] = {0u, exp_byte_bits<1>(we), exp_byte_bits<2>(we), exp_byte_bits<3>(we)};  // ([0]: wb_first has it)
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const bf16x8 wb = ks == 0 ? wb_first : expand(wr[ks], sc[ks]);
#pragma unroll
        for (int i = 0; i < MT; ++i) acc[i] = mfma_32x32x16<XF16>(wb, xa[ks][i], acc[i]);
      }
    }
    defer_pin(piece_c);
    __builtin_amdgcn_sched_barrier(0);
    STAMP(5);  // COMPUTE section issue
    asm volatile("s_barrier" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    STAMP(6);  // barrier after COMPUTE
  };
  using std::integral_constant;
  constexpr integral_constant<int, -1> no_piece{};
  int kt0 = 0;
  if constexpr (DEFER) {  // the first 16 k-steps (launch_gemm: nk >= 16), each with its piece of the re-quantization
#define LQER_DSTEP(KT) step(KT, integral_constant<int, (KT) % NSLOT>{}, integral_constant<int, KT>{})
    LQER_DSTEP(0); LQER_DSTEP(1); LQER_DSTEP(2); LQER_DSTEP(3); LQER_DSTEP(4); LQER_DSTEP(5); LQER_DSTEP(6); LQER_DSTEP(7);
    LQER_DSTEP(8); LQER_DSTEP(9); LQER_DSTEP(10); LQER_DSTEP(11); LQER_DSTEP(12); LQER_DSTEP(13); LQER_DSTEP(14); LQER_DSTEP(15);
#undef LQER_DSTEP
    kt0 = 16;
  }
  if (kt0 < nk)
  for (int kt = kt0;; kt += NSLOT) {  // 4 steps per trip, slots 0..3; every step is the same branch-free stream
    step(kt, integral_constant<int, 0>{}, no_piece);
    if (kt + 1 >= nk) break;
    step(kt + 1, integral_constant<int, 1>{}, no_piece);
    if (kt + 2 >= nk) break;
    step(kt + 2, integral_constant<int, 2>{}, no_piece);
    if (kt + 3 >= nk) break;
    step(kt + 3, integral_constant<int, 3>{}, no_piece);
    if (kt + 4 >= nk) break;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the prefetches issued past the end of K have drained
  if (!late) asm volatile("s_barrier" ::: "memory");
#ifdef LQER_CLOCKPROBE
  {
    unsigned long long cp_c1, cp_r1;
    asm volatile("s_memtime %0\n\ts_memrealtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(cp_c1), "=s"(cp_r1)::"memory");
    if (g_stamp_buf && lane == 0) {
      g_stamp_buf[(blockIdx.x * 8 + wave) * 8 + 0] = cp_c1 - cp_c0;
      g_stamp_buf[(blockIdx.x * 8 + wave) * 8 + 1] = cp_r1 - cp_r0;
      g_stamp_buf[(blockIdx.x * 8 + wave) * 8 + 2] = cp_rin;  // absolute ticks: entry, main loop start, main loop end
      g_stamp_buf[(blockIdx.x * 8 + wave) * 8 + 3] = cp_r0;
      g_stamp_buf[(blockIdx.x * 8 + wave) * 8 + 4] = cp_r1;
      g_stamp_buf[(blockIdx.x * 8 + wave) * 8 + 7] = cp_rq;
    }
  }
#endif
#ifdef LQER_STAMPS
  if (g_stamp_buf && lane == 0)
    for (int i = 0; i < 8; ++i) g_stamp_buf[(blockIdx.x * 8 + wave) * 8 + i] = st_sum[i];
#endif

  if constexpr (DEFER) {
#pragma unroll
    for (int i = 0; i < SPT; ++i)
#pragma unroll
      for (int k = 0; k < 16; ++k) acc[MT - SPT + i][k] += sp[i][k];  // (KSPLIT: m tiles 2 and 3; step 8 added 0 and 1)
  }
  if constexpr (KSPLIT) {
    // every wave's LDS-DMA has landed (vmcnt(0) above); behind this barrier every ring read is done too: the ring is free
    asm volatile("s_barrier" ::: "memory");
  }
  // KSPLIT, at the head of the stores of m tile i: the waves leave their partials of the partner's column half, two m tiles at a
  // time, each in its own 8 KiB (16 B per lane and quad: conflict-free) - in front of tile 2 a barrier first, behind which everyone
  // has read tiles 0 and 1 -, and each wave adds what its partner left for tile i (the stores of tile i - 1 are then in flight)
  auto add_partner = [&](int i) {
    if constexpr (KSPLIT) {
      if (i == 0 || i == 2) {
        const uint32_t x_out = lds0 + wave * KS_XCH + lane * 16;
        if (i == 2) asm volatile("s_barrier" ::: "memory");
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          lds_write128_at<0>(x_out + j * 4096, __builtin_shufflevector(acc_o[i + j], acc_o[i + j], 0, 1, 2, 3));
          lds_write128_at<1024>(x_out + j * 4096, __builtin_shufflevector(acc_o[i + j], acc_o[i + j], 4, 5, 6, 7));
          lds_write128_at<2048>(x_out + j * 4096, __builtin_shufflevector(acc_o[i + j], acc_o[i + j], 8, 9, 10, 11));
          lds_write128_at<3072>(x_out + j * 4096, __builtin_shufflevector(acc_o[i + j], acc_o[i + j], 12, 13, 14, 15));
        }
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      }
      const uint32_t x_in = lds0 + (wave ^ 4) * KS_XCH + lane * 16 + (i & 1) * 4096;
      f32x4 q0, q1, q2, q3;
      asm volatile(
          "ds_read_b128 %0, %4\n\tds_read_b128 %1, %4 offset:1024\n\tds_read_b128 %2, %4 offset:2048\n\t"
          "ds_read_b128 %3, %4 offset:3072\n\ts_waitcnt lgkmcnt(0)"
          : "=&v"(q0), "=&v"(q1), "=&v"(q2), "=&v"(q3)
          : "v"(x_in)
          : "memory");
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[i][t] += q0[t], acc[i][4 + t] += q1[t], acc[i][8 + t] += q2[t], acc[i][12 + t] += q3[t];
    }
  };
  // ---- store ----------------------------------------------------------------------------------
  // per 32x32 tile and quad q: regs 4q..4q+3 = columns n = nb + 8q + 4 lh + (0..3) of token row m
  const bool aligned16 = (((uintptr_t)g.y) & 15) == 0;
  const int nb = n0 + wn * 32;
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    add_partner(i);
    const int m = m0 + i * 32 + l31;
    if constexpr (DT == LQER_F32) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int n = nb + 8 * q + 4 * lh;
        if (m < g.M) {
          float* dst = (float*)g.y + (int64_t)m * g.ldy + n;
          if (n + 3 < g.N && (g.ldy & 3) == 0 && aligned16) {
            *(float4*)dst = make_float4(acc[i][4 * q], acc[i][4 * q + 1], acc[i][4 * q + 2], acc[i][4 * q + 3]);
          } else {
#pragma unroll
            for (int t = 0; t < 4; ++t)
              if (n + t < g.N) dst[t] = acc[i][4 * q + t];
          }
        }
      }
    } else {
      // 16-bit outputs: pack 4 columns into 8 B, then merge quads (q, q+1) of lanes l / l^32 into one
      // 16-B store: lanes 0-31 get columns 16p .. 16p+7, lanes 32-63 columns 16p+8 .. 16p+15
      uint32_t pk[4][2];
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const float v0 = acc[i][4 * q + 2 * h], v1 = acc[i][4 * q + 2 * h + 1];
          if constexpr (DT == LQER_F16 || DT == LQER_F16X) {
            typedef __attribute__((ext_vector_type(2))) _Float16 h2;
            h2 hv = {(_Float16)v0, (_Float16)v1};
            pk[q][h] = __builtin_bit_cast(uint32_t, hv);
          } else {
            pk[q][h] = (uint32_t)f32_to_bf16_rne(v0) | ((uint32_t)f32_to_bf16_rne(v1) << 16);
          }
        }
      const bool wide = (g.ldy & 7) == 0 && nb + 32 <= g.N && aligned16;  // wave-uniform
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const uint32_t a0 = pk[2 * p][0], a1 = pk[2 * p][1], b0 = pk[2 * p + 1][0], b1 = pk[2 * p + 1][1];
        if (wide) {
          auto r0 = __builtin_amdgcn_permlane32_swap(a0, b0, false, false);
          auto r1 = __builtin_amdgcn_permlane32_swap(a1, b1, false, false);
          // lanes 0-31: {own quad 2p, upper lane's quad 2p}; lanes 32-63: {lower lane's quad 2p+1, own quad 2p+1}
          if (m < g.M) {
            bf16_t* dst = (bf16_t*)g.y + (int64_t)m * g.ldy + nb + 16 * p + 8 * lh;
            *(uint4*)dst = make_uint4(r0[0], r1[0], r0[1], r1[1]);
          }
        } else if (m < g.M) {
#pragma unroll
          for (int qq = 0; qq < 2; ++qq) {
            const int n = nb + 8 * (2 * p + qq) + 4 * lh;
            const uint32_t lo = qq ? b0 : a0, hi = qq ? b1 : a1;
            bf16_t* dst = (bf16_t*)g.y + (int64_t)m * g.ldy + n;
            if (n < g.N) dst[0] = (bf16_t)(lo & 0xffff);
            if (n + 1 < g.N) dst[1] = (bf16_t)(lo >> 16);
            if (n + 2 < g.N) dst[2] = (bf16_t)(hi & 0xffff);
            if (n + 3 < g.N) dst[3] = (bf16_t)(hi >> 16);
          }
        }
      }
    }
  }
#ifdef LQER_CLOCKPROBE
  {
    unsigned long long cp_r2, cp_r3;  // stores issued; stores acknowledged
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(cp_r2)::"memory");
    asm volatile("s_waitcnt vmcnt(0)\n\ts_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(cp_r3)::"memory");
    if (g_stamp_buf && lane == 0) {
      g_stamp_buf[(blockIdx.x * 8 + wave) * 8 + 5] = cp_r2;
      g_stamp_buf[(blockIdx.x * 8 + wave) * 8 + 6] = cp_r3;
    }
  }
#endif
}

template <int DT, bool LOWRANK, int BOUT, bool STAGED = false, int MT = 4, bool WTWOS = false, bool DEFER = false, bool WMF = false>
__global__ __launch_bounds__(512) void k_lqer_gemm(GemmArgs g) {
  // the deferred kernel with the direct side path and the table-free expand on the bf16 main loop: the k split
  constexpr bool KSPLIT = DEFER && !STAGED && !WTWOS && !WMF && DT != LQER_F16X;
  gemm_tile_body<DT, LOWRANK, BOUT, STAGED, MT, WTWOS, DEFER, WMF, KSPLIT>(g);
}
template <int DT>
__global__ __launch_bounds__(512) void k_lqer_gemm_nks(GemmArgs g) {  // (LQER_TUNE_NO_KSPLIT)
  gemm_tile_body<DT, true, 1, false, 4, false, true, false, false>(g);
}

// The instantiations of the tile kernel that exist - the variants the plan can ask for (gemm_plan.hip), per element type:
template <int DT, bool LR, int BO, bool ST, int MT, bool WTWOS, bool DEFER, bool WMF, bool NKS>
constexpr bool tile_variant_exists() {
  constexpr bool nibbles = WTWOS || WMF;
  if (WTWOS && WMF) return false;
  if (NKS && !(LR && BO == 1 && DEFER && !ST && MT == 4 && !nibbles && DT != LQER_F16X)) return false;  // the pin against the k split: where the k split exists
  // integer / minifloat nibbles, minifloat B_out: 128-row tiles, and no fp16 main loop beside them (the plan refuses)
  if ((nibbles || BO == 3) && (MT != 4 || DT == LQER_F16X)) return false;
  if (!LR) return BO == 0 && !ST && !DEFER;  // no side path: nothing of it to choose
  if (nibbles) return ST && !DEFER;          // beside integer / minifloat nibbles the side path is always staged
  if (DEFER) return BO == 1 && MT == 4;      // blocks of 16 under the main loop of the 128-row tile
  return true;                               // B_out 0 .. 3, direct or staged, 128- or 64-row tiles
}

// variant I, its bits as in launch_tile's key: launched if it exists and is the plan's
template <int DT, int I>
static bool run_tile(int key, const GemmPlan& p, const GemmArgs& g, hipStream_t st, int& rc) {
  constexpr bool LR = I & 1, ST = I & 2, WTWOS = I & 8, DEFER = I & 16, WMF = I & 32;
  constexpr bool NKS = I & 256;
  constexpr int MT = I & 4 ? 2 : 4, BO = (I >> 6) & 3;
  if constexpr (tile_variant_exists<DT, LR, BO, ST, MT, WTWOS, DEFER, WMF, NKS>()) {
    if (key == I) {
      if constexpr (NKS) rc = launch_k<k_lqer_gemm_nks<DT>>("lqer_gemm", p.grid, 512, gemm_lds_bytes(MT), st, g);
      else rc = launch_k<k_lqer_gemm<DT, LR, BO, ST, MT, WTWOS, DEFER, WMF>>("lqer_gemm", p.grid, 512, gemm_lds_bytes(MT), st, g);
      return true;
    }
  }
  return false;
}

// the plan's variant -> the instantiation
template <int DT, int... I>
static int launch_tile(const GemmPlan& p, const GemmArgs& g, hipStream_t st, std::integer_sequence<int, I...>) {
  const int key = p.lowrank | p.staged << 1 | (p.tile_rows == 64) << 2 | p.w_twos << 3 | p.defer << 4 | p.w_mf << 5 | p.bout << 6 |
                  (p.defer && !p.staged && !p.f16x && !p.ksplit) << 8;  // (bit 8: the k split exists for the variant and is pinned off)
  int rc;
  if ((run_tile<DT, I>(key, p, g, st, rc) || ...)) return rc;
  set_error("linear_gemm: the plan asks for a tile kernel variant that does not exist (%#x)", key);
  return LQER_E_UNSUPPORTED;
}

int tile128_launch(const GemmPlan& p, const GemmArgs& g, int dtype, hipStream_t st) {
  constexpr std::make_integer_sequence<int, 8 << 6> variants{};
  return with_dtype(dtype, [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    if constexpr (DT == LQER_F16)
      if (p.f16x) return launch_tile<LQER_F16X>(p, g, st, variants);
    return launch_tile<DT>(p, g, st, variants);
  });
}

#if defined(LQER_STAMPS) || defined(LQER_CLOCKPROBE)
extern "C" int lqer_debug_set_stamp_buffer(void* p) {
  return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_stamp_buf), &p, sizeof(p));
}
#endif

}  // namespace lqer
