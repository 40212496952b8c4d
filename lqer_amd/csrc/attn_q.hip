// Fused quantized attention (reference models/llama_decoder.py:259-297, opt_decoder.py:125,190, as lqer_amd/attention.py runs it):
//     S  = Q_x0(Q) Q_w0(K^T) ->DT;  S1 = S scaling ->DT;  S2 = S1 + mask ->DT;  P = softmax_fp32(S2) ->DT;  O = Q_x1(P) Q_w1(V) ->DT
// with the four block_fp quantizers of the two products (width <= 8, blocks of 16 along the last dim of each operand) and every
// ->DT a rounding to the element type where the unfused route materialises a tensor.  The [s, t] scores never leave the chip.
//
// P is divided by the whole row's sum BEFORE it is rounded and quantized and the quantizer is not linear, so the output accumulator
// cannot be rescaled afterwards (no online softmax): every query tile sweeps the key tiles twice,
//   sweep 1: Q K^T -> S2 -> running row maximum and row sum (rescaled as the maximum grows - that is exact enough for a SUM);
//   sweep 2: Q K^T again -> S2 -> P = exp(S2 - max) / sum ->DT -> Q_x1 in registers -> P V.
// 6 s t d flops instead of 4 s t d, all on v_mfma_f32_32x32x16_bf16 (every 8-bit MXINT value is an exact bf16 number).
//
//   k_attn_kimage / k_attn_vimage   K, V -> bf16 images [b kv_heads][t][d] of Q_w0(K^T) (blocks of 16 along t) and [b kv_heads][d][t]
//                                   of Q_w1(V) (blocks along d): the tile bodies of matmul_q.hip's image kernels (qmm_image.h) with
//                                   a stride each for batch and kv head; grouped-query heads share an image.
//   k_attn_q                        one workgroup = 128 queries of one head = 4 waves x 32 queries.  The product is issued
//                                   TRANSPOSED, S^T = Kq Qq^T (key image rows as the A operand, the quantized query rows - in
//                                   registers for the tile's life - as B): a lane owns ONE query and 16 of a 32-key subtile's scores,
//                                   keys (r & 3) + 8 (r >> 2) + 4 (lane >> 5).  Registers 0-7 of lanes l and l ^ 32 are one block of
//                                   16 along t, registers 8-15 the next: the block maximum of Q_x1 needs one v_permlane32_swap, and the
//                                   8 quantized values of a register octet ARE the B fragment of one k-step of O^T = Vq^T P^T (the
//                                   image rows of V as A, read from LDS in the accumulator's key order) - P never moves between lanes
//                                   and never touches LDS.  O^T leaves a lane with its query's d values, 4 consecutive per store.
//                                   Key tiles of 64 go through LDS (rows padded against bank conflicts), the next tile's loads are
//                                   requested before the current tile's MFMAs (register staging; one buffer, two barriers per tile).
//                                   A second instantiation (PSL) reads each sequence's number of keys from the device: one call over
//                                   the sequences of a paged pool (lqer_attention_q_paged).  A third (RAG) also reads each sequence's
//                                   number of query rows, and where they start in a packed [total][heads][D] tensor, from the device:
//                                   a scheduler step of decoders and prompt chunks in one call (lqer_attention_q_paged_ragged).
//                                   WIN, on either paged form, adds the sliding-window rule at compile time: query p sees keys
//                                   p - W < j <= p, and the sweeps start at the first key tile the workgroup can see
//                                   (lqer_attention_q_paged_window, lqer_attention_q_paged_ragged_window).
//                                   TREE, on the RAG form without WIN, adds the rule of a draft-tree verify (k_attn_q_tree,
//                                   lqer_attention_q_paged_tree): a sequence's S_b <= 64 query rows are the nodes of a draft tree,
//                                   its last S_b keys theirs, and a lane selects by its own row's uint64 word as well (tree_sees,
//                                   attn_math.h) - the causal rule with holes, every tile, subtile and lane bound the causal one.
//                                   The body is written once (attn_q_body); the kernels that existed keep their symbols and record.
// Written once: the fold of the lane pair's (max, sum) behind sweep 1 (fold_lane_pair, attn_math.h); the skip of a subtile no key of
// which the wave sees, for both sweeps (`unseen`); which instantiations exist (attn_variant_exists) - attn::launch folds over
// (PSL, RAG, WIN, TREE) behind it.
#include "attn_math.h"  // rnd<DT>, exp_neg, quant8of16_bf16, fold_lane_pair: shared with attn_decode.hip

namespace lqer {

namespace attn {

constexpr int NW = 4, BQ = 32 * NW, BT = 64;  // waves, queries per workgroup, keys per LDS tile
constexpr int VD = ATTN_V_ROWS;              // rows of the V image per (batch, kv head): D padded to the image kernel's 128

struct Args {
  const void* q;
  const bf16_t* kimg;  // [batch kv_heads][Tp][Dp]
  const bf16_t* vimg;  // [batch kv_heads][VD][Tv]
  const void* mask;
  void* out;
  float* stats;
  int64_t S, T, D, Tp, Dp, Tv;
  int64_t q_bs, q_hs, q_rs, m_bs, m_hs, m_rs, o_bs, o_hs, o_rs;
  int heads, kv_heads, mode;  // mode: 0 no mask, 1 additive mask tensor, 2 causal rule
  float scaling;
  QP q0, q1;  // Q_x0 (queries), Q_x1 (probabilities)
  bool qvec, mvec;
  const int32_t* lens;  // PSL: [batch] keys of the b-th sequence (device); T above is then the bound max_len the images' strides come from
  const int32_t* q_starts;  // RAG: [batch + 1] (device) - sequence b's query rows are tokens q_starts[b] .. q_starts[b + 1] - 1 of q / out
                            // [total][heads][D] (q_bs = o_bs = 0, q_rs / o_rs the token strides) and of stats [total][heads][2]; S above
                            // is then the bound max_s the grid's x comes from
  int64_t window;  // WIN: W >= 1 - query i sees key j iff i + off - W < j <= i + off (read by no other instantiation)
};

// the argument record of the kernel with TREE: the rows' masks behind the record of the others, which stays what it was
struct ArgsTree : Args {
  const uint64_t* tree;  // (device, [total]) one word per packed query token - bit j: draft node j is the token's node or an ancestor of it
};

template <int DT>
__global__ __launch_bounds__(256) void k_attn_kimage(const void* __restrict__ k, int64_t D, int64_t T, int64_t k_bs, int64_t k_hs, int64_t k_rs,
                                                      int kv_heads, QP q, bf16_t* __restrict__ img, int64_t Tp, int64_t Dp, bool vec) {
  const int64_t z = blockIdx.z;  // y = K^T [d][t], d contiguous: blocks of 16 along t
  qmm::bimage_k_tile<DT>(k, (z / kv_heads) * k_bs + (z % kv_heads) * k_hs, D, T, k_rs, q, img + z * Tp * Dp, Tp, Dp, vec, (int64_t)blockIdx.x * 64,
                         (int64_t)blockIdx.y * 64);
}

template <int DT>
__global__ __launch_bounds__(256) void k_attn_vimage(const void* __restrict__ v, int64_t D, int64_t T, int64_t v_bs, int64_t v_hs, int64_t v_rs,
                                                      int kv_heads, QP q, bf16_t* __restrict__ img, int64_t Tv, bool vec) {
  const int64_t z = blockIdx.z;  // y = V [t][d], d contiguous: blocks of 16 along d, transposed through LDS
  qmm::bimage_j_tile<DT, false>(v, (z / kv_heads) * v_bs + (z % kv_heads) * v_hs, T, D, v_rs, q, img + z * VD * Tv, VD, Tv, vec, (int64_t)blockIdx.y * 64,
                                (int64_t)blockIdx.x * 64);
}

// PSL (per-sequence lengths, the paged pool): a workgroup takes T = lens[b] - and with it the causal offset and every key bound below -
// from the device; Tp and Tv stay those of the bound.  A sequence of no keys gets zeros and no statistics.
// RAG (per-sequence query counts, with PSL): a workgroup also takes S = q_starts[b + 1] - q_starts[b] - and with it the causal offset
// T - S, its sequence's own number of query tiles and their order - from the device, and finds its rows of q, out and the statistics
// at token q_starts[b] + (row in the sequence).  The grid's x covers the bound max_s: a workgroup whose tile lies beyond its
// sequence's S - every one of a sequence with S = 0 - leaves before any barrier, load or store.
// WIN (the sliding window, with PSL; the call is causal): the causal rule's three levels once more at the LOW end.  The workgroup's
// sweeps start at key tile it0 = max(0, q0 + off - W + 1) / BT - no image tile below it is loaded, and the image kernels
// (kv_cache.hip) have written none -, a wave skips a 32-key subtile that ends at or below w_begin = max(0, q0 + 32 wave + off - W + 1),
// and a lane's register is visible iff its key is at or above tmin = max(0, qi + off - W + 1) as well: a SELECT wherever the causal
// limit is tested - never a product with a mask, the image rows of dead keys may hold anything.
// TREE (a draft tree, with RAG and without WIN; the call is causal): sequence b's rows are the S_b nodes of its tree and its last S_b
// keys - at and above off = T - S - theirs, in the same order.  The lane reads its row's word once and sees key off + j iff j <= its
// own row and bit j is set: one more SELECT in `vis`.  t_end, w_end, tmax and `unseen` are the causal ones - the rule only takes keys away.
// The body of k_attn_q and k_attn_q_tree, on the record A of the kernel.
template <int DT, int DK, bool PSL, bool RAG, bool WIN, bool TREE, class A>  // DK: 32-wide tiles of the head dim (D <= 32 DK)
__device__ __forceinline__ void attn_q_body(const A a) {
  static_assert(!RAG || PSL, "per-sequence query counts come with per-sequence lengths");
  static_assert(!WIN || PSL, "the window rule runs on the paged forms");
  static_assert(!TREE || (RAG && !WIN), "the tree rule comes with the per-sequence counts, without a window");
  constexpr int KS = 64 * DK + 16;  // bytes of a key row in LDS (+16: the 16-byte fragment reads of 16 consecutive rows hit 16 bank groups)
  constexpr int VS = 128 + 8;       // bytes of a V^T row (64 keys) in LDS (+8: the 8-byte reads of 32 rows hit 32 bank pairs)
  __shared__ __attribute__((aligned(16))) unsigned char sK[BT * KS];
  __shared__ __attribute__((aligned(16))) unsigned char sV[32 * DK * VS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lh = lane >> 5;
  const int64_t h = blockIdx.y, b = blockIdx.z, z = b * a.kv_heads + h / (a.heads / a.kv_heads);
  int64_t S = a.S, row0 = 0;  // this sequence's query rows, and the token of its first (RAG; else row 0 of batch b)
  if constexpr (RAG) {
    row0 = a.q_starts[b], S = a.q_starts[b + 1] - row0;
    if ((int64_t)blockIdx.x * BQ >= S) return;  // (uniform over the workgroup, before any barrier)
  }
  const int64_t nq = (S + BQ - 1) / BQ;
  const int64_t qt = a.mode == 2 ? nq - 1 - (int64_t)blockIdx.x : (int64_t)blockIdx.x;  // causal: the long tiles first
  const int64_t q0 = qt * BQ, qi = q0 + wave * 32 + l31;
  int64_t T = a.T;
  if constexpr (PSL) {
    T = a.lens[b];
    if (T == 0) {  // (uniform over the workgroup, before any barrier)
      if (qi < S) {
        const float o4[4] = {0.f, 0.f, 0.f, 0.f};
        for (int d = 4 * lh; d < (int)a.D; d += 8) store_row4<DT>(a.out, b * a.o_bs + h * a.o_hs + (row0 + qi) * a.o_rs + d, d, (int)a.D, o4);
      }
      return;
    }
  }
  const int64_t off = T - S;  // causal: key j is visible to query i iff j <= i + off
  const float NEG_INF = -__builtin_inff();

  // ---- this lane's query row, quantized: fragment ks holds d = 16 ks + 8 lh .. + 7
  bf16x8 qf[2 * DK];
#pragma unroll
  for (int ks = 0; ks < 2 * DK; ++ks) {
    uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (qi < S && ks * 16 < a.D) {
      float v[16];
      load16<DT>(a.q, b * a.q_bs + h * a.q_hs + (row0 + qi) * a.q_rs + ks * 16, 16, a.qvec, v);
      quant16_bf16<DT != LQER_F16>(v, a.q0, w);
    }
    const u32x4 f = {lh ? w[4] : w[0], lh ? w[5] : w[1], lh ? w[6] : w[2], lh ? w[7] : w[3]};
    qf[ks] = __builtin_bit_cast(bf16x8, f);
  }

  // ---- key tiles this workgroup / wave / lane looks at
  const int64_t q_last = (q0 + BQ < S ? q0 + BQ : S) - 1;
  int64_t t_end = T;  // keys [0, t_end) are visible to some query of the workgroup
  if (a.mode == 2) {
    const int64_t e = q_last + off + 1;
    t_end = e < 0 ? 0 : (e < T ? e : T);
  }
  const int nt = (int)((t_end + BT - 1) / BT);
  int64_t w_end = T;  // ... of this wave
  if (a.mode == 2) {
    const int64_t e = q0 + wave * 32 + 31 + off + 1;
    w_end = e < 0 ? 0 : (e < T ? e : T);
  }
  int64_t tmax = T - 1;  // the last key visible to this lane's query
  if (a.mode == 2) tmax = qi + off < tmax ? qi + off : tmax;
  int it0 = 0;                   // WIN: the first key tile some query of the workgroup sees
  int64_t w_begin = 0, tmin = 0;  // ... the first key visible to the wave, to this lane's query
  if constexpr (WIN) {
    const int64_t g = q0 + off - a.window + 1, wb = g + wave * 32, lb = qi + off - a.window + 1;
    it0 = g > 0 ? (int)(g / BT) : 0;
    w_begin = wb > 0 ? wb : 0;
    tmin = lb > 0 ? lb : 0;
  }
  const int64_t qic = qi < S ? qi : S - 1;
  uint64_t tmask = 0;  // TREE: this lane's row of the tree
  if constexpr (TREE) tmask = a.tree[row0 + qic];
  // register r of the subtile at tb holds key tb + 4 lh + (r & 3) + 8 (r >> 2): visible iff that offset is <= lim (and, WIN, >= lim_lo;
  // TREE: the key is draft node jb + offset, jb = tb + 4 lh - off, or - below node 0 - one of the committed context)
  auto vis = [](int r, int64_t lim_lo, int64_t lim, uint64_t tm, int64_t jb) {
    const int kr = (r & 3) + 8 * (r >> 2);
    if constexpr (TREE) return kr <= lim && tree_sees(tm, jb + kr);
    else if constexpr (WIN) return lim_lo <= kr && kr <= lim;
    else return kr <= lim;
  };
  const int64_t moff = a.mode == 1 ? b * a.m_bs + h * a.m_hs + qic * a.m_rs : 0;

  // (the staged pieces travel BY VALUE: arrays captured by reference in these lambdas ended up in scratch memory)
  struct Stage {
    uint4 r[DK];
  };
  auto fetch_k = [&](int it) {
    Stage st;
    const bf16_t* base = a.kimg + (z * a.Tp + (int64_t)it * BT) * a.Dp;
#pragma unroll
    for (int u = 0; u < DK; ++u) {
      const int p = tid + 256 * u, row = p / (4 * DK), ch = p % (4 * DK);
      st.r[u] = *(const uint4*)(base + (int64_t)row * a.Dp + ch * 8);
    }
    return st;
  };
  auto put_k = [&](const Stage st) {
#pragma unroll
    for (int u = 0; u < DK; ++u) {
      const int p = tid + 256 * u, row = p / (4 * DK), ch = p % (4 * DK);
      *(uint4*)(sK + row * KS + ch * 16) = st.r[u];
    }
  };
  auto fetch_v = [&](int it) {
    Stage st;
    const bf16_t* base = a.vimg + z * VD * a.Tv + (int64_t)it * BT;
#pragma unroll
    for (int u = 0; u < DK; ++u) {
      const int p = tid + 256 * u, row = p >> 3, ch = p & 7;
      st.r[u] = *(const uint4*)(base + (int64_t)row * a.Tv + ch * 8);
    }
    return st;
  };
  auto put_v = [&](const Stage st) {
#pragma unroll
    for (int u = 0; u < DK; ++u) {
      const int p = tid + 256 * u, row = p >> 3, ch = p & 7;
      *(uint2*)(sV + row * VS + ch * 16) = make_uint2(st.r[u].x, st.r[u].y);
      *(uint2*)(sV + row * VS + ch * 16 + 8) = make_uint2(st.r[u].z, st.r[u].w);
    }
  };

  // S2 of the 32-key subtile at tb for this lane's query: s2[r] is key tb + (r & 3) + 8 (r >> 2) + 4 lh
  auto scores = [&](int64_t tb, int u, float (&s2)[16]) {
    float mk[16];
    if (a.mode == 1) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int64_t t = tb + 8 * g + 4 * lh;
        if (a.mvec) {  // (T a multiple of 4: a group of four lies inside the row or behind it - read from a clamped address, unused then)
          const int64_t tc = t < T ? t : T - 4;
          if constexpr (DT == LQER_F32) {
            const float4 m4 = *(const float4*)((const float*)a.mask + moff + tc);
            mk[4 * g] = m4.x, mk[4 * g + 1] = m4.y, mk[4 * g + 2] = m4.z, mk[4 * g + 3] = m4.w;
          } else {
            const uint2 m2 = *(const uint2*)((const bf16_t*)a.mask + moff + tc);
            const uint32_t wd[2] = {m2.x, m2.y};
#pragma unroll
            for (int j = 0; j < 2; ++j) pair_to_f32<DT>(wd[j], mk[4 * g + 2 * j], mk[4 * g + 2 * j + 1]);
          }
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) mk[4 * g + j] = t + j < T ? load_elem<DT>(a.mask, moff + t + j) : 0.f;
        }
      }
    }
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < 2 * DK; ++ks) {
      const bf16x8 kf = *(const bf16x8*)(sK + (32 * u + l31) * KS + (2 * ks + lh) * 16);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float s = rnd<DT>(rnd<DT>(acc[r]) * a.scaling);
      if (a.mode == 1) s = rnd<DT>(s + mk[r]);
      s2[r] = s;
    }
  };

  // the 32-key subtile at tb, in either sweep: no key of it is visible to the wave (wave-uniform) - beyond the causal limit or, WIN, below
  // the window's low end
  auto unseen = [&](int64_t tb) {
    if (tb >= w_end) return true;
    if constexpr (WIN)
      if (tb + 32 <= w_begin) return true;
    return false;
  };

  // ---- sweep 1: row maximum and row sum of exp(S2 - maximum), per lane over its own keys, then across the lane pair
  float m = NEG_INF, l = 0.f;
  Stage kr = fetch_k(it0), vr;  // (nt = 0: rows 0-63 of the image exist)
  for (int it = it0; it < nt; ++it) {
    __syncthreads();  // the previous tile's fragment reads are done
    put_k(kr);
    __syncthreads();
    kr = fetch_k(it + 1 < nt ? it + 1 : it);  // the next tile's loads travel under this tile's work (past the end: a re-read, unused)
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int64_t tb = (int64_t)it * BT + 32 * u;
      if (unseen(tb)) continue;
      float s2[16];
      scores(tb, u, s2);
      const int64_t lim = tmax - tb - 4 * lh, lim_lo = tmin - tb - 4 * lh;  // register r is visible iff (WIN: lim_lo <=) (r & 3) + 8 (r >> 2) <= lim
      const int64_t jb = tb + 4 * lh - off;
      float tm = NEG_INF;
#pragma unroll
      for (int r = 0; r < 16; ++r) tm = vis(r, lim_lo, lim, tmask, jb) ? fmaxf(tm, s2[r]) : tm;
      const float mn = fmaxf(m, tm), mref = mn == NEG_INF ? 0.f : mn;
      float ls = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) ls += vis(r, lim_lo, lim, tmask, jb) ? exp_neg(s2[r] - mref) : 0.f;
      l = l * exp_neg(m - mref) + ls;
      m = mn;
    }
  }
  float M, L;
  fold_lane_pair(m, l, M, L);
  if (a.stats && lh == 0 && qi < S) {
    float* st = a.stats + (RAG ? (row0 + qi) * a.heads + h : (b * a.heads + h) * S + qi) * 2;  // RAG: [total][heads][2]
    st[0] = M, st[1] = L;
  }

  // ---- sweep 2: S2 again -> P ->DT -> Q_x1 -> O^T += Vq^T P^T
  f32x16 o[DK];
#pragma unroll
  for (int dt = 0; dt < DK; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
  kr = fetch_k(it0), vr = fetch_v(it0);
  for (int it = it0; it < nt; ++it) {
    __syncthreads();
    put_k(kr);
    put_v(vr);
    __syncthreads();
    kr = fetch_k(it + 1 < nt ? it + 1 : it);
    vr = fetch_v(it + 1 < nt ? it + 1 : it);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int64_t tb = (int64_t)it * BT + 32 * u;
      if (unseen(tb)) continue;
      float s2[16];
      scores(tb, u, s2);
      const int64_t lim = tmax - tb - 4 * lh, lim_lo = tmin - tb - 4 * lh, jb = tb + 4 * lh - off;
#pragma unroll
      for (int r = 0; r < 16; ++r) s2[r] = vis(r, lim_lo, lim, tmask, jb) ? rnd<DT>(exp_neg(s2[r] - M) / L) : 0.f;  // (S2 = max = -inf: NaN, as the unfused route)
#pragma unroll
      for (int s = 0; s < 2; ++s) {  // registers 8 s .. 8 s + 7: keys tb + 16 s + {0-3, 8-11} + 4 lh - half a block of 16, one k-step of P V
        const float v8[8] = {s2[8 * s], s2[8 * s + 1], s2[8 * s + 2], s2[8 * s + 3], s2[8 * s + 4], s2[8 * s + 5], s2[8 * s + 6], s2[8 * s + 7]};
        uint32_t w[4];
        quant8of16_bf16<DT != LQER_F16>(v8, a.q1, w);
        const u32x4 pw = {w[0], w[1], w[2], w[3]};
        const bf16x8 pf = __builtin_bit_cast(bf16x8, pw);
#pragma unroll
        for (int dt = 0; dt < DK; ++dt) {
          const unsigned char* vp = sV + (32 * dt + l31) * VS + (32 * u + 16 * s + 4 * lh) * 2;
          const uint2 v0 = *(const uint2*)vp, v1 = *(const uint2*)(vp + 16);
          const u32x4 vw = {v0.x, v0.y, v1.x, v1.y};
          o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, vw), pf, o[dt], 0, 0, 0);
        }
      }
    }
  }

  // ---- O^T: this lane's query, d = 32 dt + 8 (r >> 2) + 4 lh + (r & 3)
  if (qi < S) {
    const int64_t at0 = b * a.o_bs + h * a.o_hs + (row0 + qi) * a.o_rs;
#pragma unroll
    for (int dt = 0; dt < DK; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int d = 32 * dt + 8 * g + 4 * lh;
        if (d < a.D) {
          const float o4[4] = {o[dt][4 * g], o[dt][4 * g + 1], o[dt][4 * g + 2], o[dt][4 * g + 3]};
          store_row4<DT>(a.out, at0 + d, d, (int)a.D, o4);
        }
      }
  }
}

template <int DT, int DK, bool PSL = false, bool RAG = false, bool WIN = false>
__global__ __launch_bounds__(64 * NW, 2) void k_attn_q(const Args a) {
  attn_q_body<DT, DK, PSL, RAG, WIN, false>(a);
}
template <int DT, int DK>
__global__ __launch_bounds__(64 * NW, 2) void k_attn_q_tree(const ArgsTree a) {
  attn_q_body<DT, DK, true, true, false, true>(a);
}

// The instantiations of the attention kernel that exist, stated once: the per-sequence query counts and the window run on the paged
// forms (PSL), the tree rule on the form with per-sequence counts and no window
template <bool PSL, bool RAG, bool WIN, bool TREE = false>
constexpr bool attn_variant_exists() {
  if (TREE) return PSL && RAG && !WIN;
  return PSL || !(RAG || WIN);
}

// with a cache the two images are already on their way on c.st (kv_cache_images_dispatch: written from the packed KV cache)
template <int DT>
static int launch(const AttnCall& c, Args a) {
  const int esz = DT == LQER_F32 ? 4 : 2;
  if (!c.packed) {
    const unsigned nz = (unsigned)(c.batch * a.kv_heads);
    k_attn_kimage<DT><<<dim3((unsigned)(a.Dp / 64), (unsigned)(a.Tp / 64), nz), 256, 0, c.st>>>(
        c.k, a.D, a.T, c.ks[0], c.ks[1], c.ks[2], a.kv_heads, make_qp(*c.k_fmt), (bf16_t*)a.kimg, a.Tp, a.Dp, al16(c.k, c.ks, esz));
    k_attn_vimage<DT><<<dim3((unsigned)(VD / 64), (unsigned)(a.Tv / 64), nz), 256, 0, c.st>>>(
        c.v, a.D, a.T, c.vs[0], c.vs[1], c.vs[2], a.kv_heads, make_qp(*c.v_fmt), (bf16_t*)a.vimg, a.Tv, al16(c.v, c.vs, esz));
  }
  a.qvec = al16(c.q, c.qs, esz);
  // the mask is read in groups of four elements: rows and pointer aligned to that, and T a multiple of four
  a.mvec = a.mode == 1 && a.T % 4 == 0 && (uintptr_t)a.mask % (4 * esz) == 0 && a.m_bs % 4 == 0 && a.m_hs % 4 == 0 && a.m_rs % 4 == 0;
  const dim3 grid((unsigned)((a.S + BQ - 1) / BQ), (unsigned)a.heads, (unsigned)c.batch);
  const int dk = (int)((a.D + 31) / 32);
  const bool ragged = c.paged && c.pool.ragged;  // (a.S: the bound max_s - the grid's x; the kernel takes S from q_starts)
  const bool win = c.paged && c.windowed;        // (the two _window entries: causal, W >= 1 - the check's)
  const bool tree = ragged && c.treed;           // (lqer_attention_q_paged_tree: causal, max_s <= 64 - the check's)
  with_flags(
      [&](auto psl, auto rag, auto w, auto tr) {
        if constexpr (attn_variant_exists<psl, rag, w, tr>()) {
          const auto run = [&](auto k) {
            if constexpr (tr) k_attn_q_tree<DT, k><<<grid, 64 * NW, 0, c.st>>>(ArgsTree{a, c.tree});
            else k_attn_q<DT, k, psl, rag, w><<<grid, 64 * NW, 0, c.st>>>(a);
          };
          switch (dk) {
            case 1: run(std::integral_constant<int, 1>{}); break;
            case 2: run(std::integral_constant<int, 2>{}); break;
            case 3: run(std::integral_constant<int, 3>{}); break;
            default: run(std::integral_constant<int, 4>{}); break;
          }
        }
        return 0;
      },
      c.paged, ragged, win, tree);
  if (tree) return check_launch("lqer_attention_q_paged_tree");
  return check_launch(ragged ? (win ? "lqer_attention_q_paged_ragged_window" : "lqer_attention_q_paged_ragged")
                      : c.paged ? (win ? "lqer_attention_q_paged_window" : "lqer_attention_q_paged")
                                : (c.packed ? "lqer_attention_q_kv" : "lqer_attention_q"));
}

}  // namespace attn

static size_t attn_align(size_t v) { return (v + 255) / 256 * 256; }
static void attn_dims(int64_t T, int64_t D, int64_t* Tp, int64_t* Dp, int64_t* Tv) {
  *Tp = (T + 127) / 128 * 128, *Dp = (D + 63) / 64 * 64, *Tv = (T + 63) / 64 * 64;
}
// [K image: batch kv_heads x Tp x Dp bf16][V image: batch kv_heads x 128 x Tv bf16], each rounded up to 256 bytes
size_t attention_q_workspace_bytes(int64_t batch, int64_t kv_heads, int64_t T, int64_t D) {
  int64_t Tp, Dp, Tv;
  attn_dims(T, D, &Tp, &Dp, &Tv);
  return attn_align((size_t)(batch * kv_heads * Tp * Dp) * sizeof(bf16_t)) + attn_align((size_t)(batch * kv_heads * attn::VD * Tv) * sizeof(bf16_t));
}

// the two images at their places in the workspace - from the raw K and V (attn::launch) or from the codes of the packed KV cache or
// of the paged pool (kv_cache.hip) - then k_attn_q on them
int attention_q_dispatch(const AttnCall& c) {
  attn::Args a;
  a.q = c.q, a.mask = c.mask, a.out = c.out, a.stats = c.row_stats;
  a.S = c.S, a.T = c.T, a.D = c.D;
  attn_dims(c.T, c.D, &a.Tp, &a.Dp, &a.Tv);
  a.kimg = (const bf16_t*)c.workspace;
  a.vimg = (const bf16_t*)((const unsigned char*)c.workspace + attn_align((size_t)(c.batch * c.kv_heads * a.Tp * a.Dp) * sizeof(bf16_t)));
  a.q_bs = c.qs[0], a.q_hs = c.qs[1], a.q_rs = c.qs[2];
  a.m_bs = c.mask ? c.ms[0] : 0, a.m_hs = c.mask ? c.ms[1] : 0, a.m_rs = c.mask ? c.ms[2] : 0;
  a.o_bs = c.os[0], a.o_hs = c.os[1], a.o_rs = c.os[2];
  a.heads = (int)c.heads, a.kv_heads = (int)c.kv_heads, a.mode = c.causal ? 2 : (c.mask ? 1 : 0);
  a.scaling = c.scaling;
  a.q0 = make_qp(*c.q_fmt), a.q1 = make_qp(*c.p_fmt);
  a.qvec = a.mvec = false;  // (attn::launch sets them)
  a.lens = c.paged ? c.pool.lens : nullptr;  // (paged: c.T is the bound max_len - the images' strides; the kernels take T from lens[b])
  a.q_starts = c.paged && c.pool.ragged ? c.pool.starts : nullptr;  // (ragged: c.S is the bound max_s, qs / os hold {0, head, token})
  a.window = c.paged && c.windowed ? c.window : 0;
  if (c.packed) kv_cache_images_dispatch(c, (bf16_t*)a.kimg, a.Tp, a.Dp, (bf16_t*)a.vimg, a.Tv);
  return with_dtype(c.dtype, [&](auto dt) { return attn::launch<decltype(dt)::value>(c, a); });
}

}  // namespace lqer
