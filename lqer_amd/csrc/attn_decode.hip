// Fused quantized attention for decode steps: 1 <= S <= 8 query rows against T keys, split over the KEYS (reference
// models/llama_decoder.py:259-297, opt_decoder.py:125,190 - the arithmetic of attn_q.hip's header, unchanged):
//     S  = Q_x0(Q) Q_w0(K^T) ->DT;  S1 = S scaling ->DT;  S2 = S1 + mask ->DT;  P = softmax_fp32(S2) ->DT;  O = Q_x1(P) Q_w1(V) ->DT
// attn_q.hip gives a lane one query and a workgroup 128 of them: at S = 1 that is one live lane in 32, heads x batch workgroups, and
// two bf16 images of the whole K and V written and read back.  Here a workgroup owns one CHUNK of keys for all R = (heads / kv_heads) S
// query rows of its kv head; K and V are read once, in DT, straight from the caller's tensors (grouped-query K / V once per kv head).
//
// P is divided by the whole row's sum BEFORE it is rounded and quantized, so partial outputs over chunks cannot be rescaled afterwards
// (no online softmax, no flash-decoding merge): the row's maximum and sum must be complete before any P exists.  Three launches:
//   k_attn_dec_scores  grid (chunks, kv heads, batch).  The chunk's K rows -> registers with the lanes along d (a lane: 4 consecutive d
//                      x 16 keys = four blocks of Q_w0, no cross-lane step for the block maximum) -> quant16_bf16 -> LDS [key][d] ->
//                      S^T = Kq Qq^T on v_mfma_f32_32x32x16_bf16 (a wave: 32 keys x 32 query rows, the fragment layout of k_attn_q) ->
//                      S2 to the workspace, {max, sum exp(S2 - max)} of the chunk per row next to it.
//   k_attn_dec_pv      same grid.  Folds the row's chunk statistics IN CHUNK ORDER, P = exp(S2 - max) / sum ->DT, Q_x1 over 16 keys in a
//                      lane pair (quant8of16_bf16), the chunk's V rows -> quant16_bf16 along d -> LDS [key][d], O^T += Vq^T Pq^T, the
//                      R x D fp32 partial of the chunk to the workspace.  Chunk 0 (with a window: the first live chunk) writes row_stats.
//   k_attn_dec_sum     adds the partials IN CHUNK ORDER, rounds ->DT, stores through the output strides.
// The chunk length depends on T alone (dec_chunk), a row's arithmetic on that row alone: no floating-point atomics, no counters, the
// same bits run to run, for a batch slice and for a slice of a kv group's heads.
//
// Both kernels take their K / V from one of three sources (template parameter SRC): the caller's tensors in DT, quantized here; the
// packed KV cache (kv_pack.h: the codes and block exponents of Q_w0(K^T) and Q_w1(V), written by kv_cache.hip) - 16-byte loads of
// codes, a convert and a scale; or the paged pool - the same codes, a block of 16 keys found through the sequence's row of a page
// table.  Every source writes the SAME bf16 image to LDS; everything after the first barrier is one body.
// With the paged pool the sequences of a batch have lengths of their own, read from the device: a workgroup takes T = lens[b], and with
// it the chunk length, the chunk count and the causal offset of ITS sequence; the grid and the workspace strides come from the bound
// max_len (dec_max_chunks), and a workgroup whose chunk its sequence does not have leaves before the first barrier.  A sequence's
// results are those of a call of batch 1 at T = lens[b]: nothing it computes depends on max_len or on the rest of the batch.
//
// A sliding window (template parameter WIN, DArgs::win = W keys, with the causal rule): the query at position p sees keys p - W < j <= p.
// A key outside the window gives P = +0 on the mask-tensor route (exp_neg underflows, Q_x1 of zeros is zero, a chunk whose keys are
// all masked folds into the row's sum with factor 0), so applying the window as a RULE gives that route's bits and lets the kernels
// skip what no row of the call can see: with lo = max(0, T - S - W + 1), chunks below lo / C leave before the first barrier and are
// left out of both folds (their workspace cells are never written and never read; chunk lo / C writes row_stats), and keys below the
// page boundary 16 (lo / 16) are zero rows in LDS whose table entries and pages are never dereferenced - a released page may hold
// anything.  A page is one block of Q_w0 along t and one group of Q_w1's exponents, so the live pages' codes do not depend on the rest.
//
// Per-sequence query counts (template parameter RAG, the paged source only: lqer_attention_q_decode_paged_ragged): a speculative
// decoder's verify step, a scheduler step of one-token decoders beside sequences that take a few.  q and out are packed
// [total][heads][D] tensors through a token and a head stride, and a workgroup (chunk, kv head, b) takes S_b = q_starts[b + 1] -
// q_starts[b] from the device as it takes T_b: its row count R_b = rep S_b, the causal offset T_b - S_b, the window's first key
// lo = max(0, T_b - S_b - W + 1) and with it the first live chunk, the page boundary and the chunk that writes row_stats, and the
// token q_starts[b] at which its rows of q, out and row_stats begin.  S_b = 0: the workgroup leaves before the first barrier.  The
// workspace rows are indexed by PACKED TOKEN: sequence b owns rows q_starts[b] heads .. q_starts[b + 1] heads - 1, row g R_b + r of
// that range for row r of kv head g (a bijection), so the workspace follows total x heads and not batch x max_s.  The host bound
// max_s sizes k_attn_dec_sum's grid alone.  Everything a row computes - chunks, folds, fragments, quantizers, rounding points - is
// the uniform kernels' at S = S_b: the rows of a sequence are those of a call of batch 1 with S = S_b, whatever else is in the batch.
//
// A prefix on shared pages read ONCE PER GROUP (template parameter GRP, the paged source without WIN and RAG:
// lqer_attention_q_decode_paged_shared): beams, samples of one prompt, requests behind one system prompt hold their first P keys on
// the same pages (lqer_kv_pool_fork).  The caller names the groups (DArgsGrp: grp_of, and grp_starts / grp_members in CSR form, the
// first member of a group its leader) and P per group, a multiple of 16.  Grid, workspace and k_attn_dec_sum are the plain paged
// call's.  Workgroup (c, g, b) takes T_b, C and nch from lens[b] as ever; chunk c is SHARED when b's group has more than one member
// and (c + 1) C <= P.  Of a shared chunk the leader's workgroup loads the keys (the V rows) once, through its own table row - every
// key lies below P <= every member's length - and runs the row loop over n_members R rows: row r is row r % R of member r / R, and
// that member's call index, length, causal offset, q / row_stats offset and workspace rows are per-LANE values; the 32-row groups run
// straight through the member boundaries.  The other members' workgroups of that chunk leave before the first barrier.  A lane still
// owns one query row, an MFMA output column depends on that lane's operand alone, and in k_attn_dec_pv a lane folds the chunk
// statistics of its own member's chunks 0 .. nch_j - 1 in chunk order: every row has the bits of the plain call.  Every workspace cell
// is still written by exactly one workgroup (a member's cells of a shared chunk by the leader's, all others by its own) - no atomics,
// no counters, three launches.  All members of a group with P > 0 have one chunk length (the caller's contract): the leader's C is
// the C of every row it computes.  P is a licence - a smaller P than the members really share gives the same bits.
//
// A draft tree (template parameter TREE of the two bodies, the paged source with RAG, without WIN and GRP:
// lqer_attention_q_decode_paged_tree): the verify step of a speculative decoder that drafts a TREE of up to 8 nodes per sequence.  The
// last S_b keys of a sequence are its draft nodes in append order (parents before children), and every packed query token has one
// uint64 word on the device (DArgsTree::tree, read once per row at sr.tok + si): bit j set iff node j is the row's node or one of
// its ancestors.  Row i sees the committed context - the keys below off = T_b - S_b - and key off + j iff j <= i and bit j is set
// (tree_sees, attn_math.h): the causal rule with holes, as a SELECT wherever the causal limit is tested.  A hidden key is left out
// of the row's maximum and sum and gives P = +0 - what the additive mask tensor gives it (its exponential underflows to 0, and a
// chunk none of whose keys a row sees folds with factor 0) - so the rows have the bits of the uniform kernels under that mask.
// Chunks, grid, workspace and k_attn_dec_sum are the RAG ones.  The kernels' names are k_attn_dec_scores_tree / k_attn_dec_pv_tree:
// the two bodies are written once (dec_scores, dec_pv), and the kernels that existed keep their symbols and argument records.
//
// Nibble codes in the paged pool (template parameter N4 of the two kernels, the paged source without GRP: k_fmt / v_fmt of kind
// LQER_Q_MXINT_C4, kv_pack.h): the packed stage loads 8 bytes per 16 codes and widens them to the byte codes (kvc::load_codes16) in
// front of the same codes16_to_bf16 - the scores kernel's flag is K's storage, the PV kernel's V's.  Nothing else differs.
//
// Written once: a key's 16 quantized values to its LDS row (put_key16: the packed stage of both kernels, the raw V stage); the fold of
// the lane pair's (max, sum) (fold_lane_pair, attn_math.h); which instantiations exist (decode_variant_exists) -
// attention_q_decode_dispatch is one fold over (element type, source, WIN, RAG, GRP, K4, V4, TREE) behind it.
#include "attn_math.h"
#include "kv_pack.h"

namespace lqer {

namespace attn {

constexpr int DEC_MAX_S = 8;     // query rows per head
constexpr int DEC_CMAX = 128;    // keys per chunk at most
constexpr int DEC_LS = 256 + 16; // bytes of an LDS row of 128 bf16 (+16: the 16-byte fragment reads of 16 consecutive rows hit 16 bank groups)

// keys per chunk: 16 ceil(T / 256) clamped to [16, 128] - T / 16 chunks up to T = 256, then 16, from T = 2048 on chunks of 128.
// Llama-7B's step (32 heads, T = 2048): 16 x 32 = 512 workgroups of 4 waves, two per CU on 256 CUs.
__host__ __device__ inline int dec_chunk(int64_t T, int64_t D) {
  (void)D;
  const int64_t n = (T + 255) / 256;
  return 16 * (int)(n < 1 ? 1 : (n > 8 ? 8 : n));
}

// the most chunks any T <= max_len has - the grid's x and the workspace's chunk stride with per-sequence lengths.  nch is not monotonic
// in T (256 keys: 16 chunks of 16; 257: 9 of 32; 2049: 17 of 128): up to 256 keys it is ceil(T / 16), from 257 to 2048 at most 16
// (reached at every multiple of 256), beyond 2048 ceil(T / 128) >= 17.
__host__ inline int dec_max_chunks(int64_t max_len) {
  return (int)(max_len <= 256 ? (max_len + 15) / 16 : (max_len <= 2048 ? 16 : (max_len + 127) / 128));
}

struct DArgs {
  const void *q, *k, *v, *mask;
  void* out;
  float* stats;
  float *s2, *cst, *part;  // workspace: S2 [rows][Tp], chunk statistics [rows][nch][2], partial outputs [rows][nch][D]
  int64_t S, T, D, R, Tp, rows;
  int64_t q_bs, q_hs, q_rs, k_bs, k_hs, k_rs, v_bs, v_hs, v_rs, m_bs, m_hs, m_rs, o_bs, o_hs, o_rs;
  int C, nch, heads, kv_heads, rep, mode;  // mode: 0 no mask, 1 additive mask tensor, 2 causal rule
  float scaling;
  QP q0, qk, q1, qv;
  bool qvec, kvec, vvec;
  int nchs;  // chunks the workspace has room for per row (its stride over rows): nch, or dec_max_chunks(max_len) with the paged source
  kvc::KvSrc<const unsigned char> src;  // the packed and the paged source (kv_pack.h)
  int64_t win;  // the window W of the kernels with WIN (mode 2 only); 0: none.  (Last: the members above keep their kernarg offsets)
};
// the argument record of the kernels with RAG: the token starts behind it, so the other kernels' record is what it was
struct DArgsRag : DArgs {
  const int32_t* q_starts;  // (device, [batch + 1]) sequence b owns tokens q_starts[b] .. q_starts[b + 1] - 1
};
// the argument record of the kernels with GRP: the groups of sequences that hold a prefix on the same pages, behind the same record
struct DArgsGrp : DArgs {
  const int32_t* grp_of;       // (device, [batch]) the group of the call's b-th sequence
  const int32_t* grp_starts;   // (device, [groups + 1]) group i owns entries grp_starts[i] .. grp_starts[i + 1] - 1 of grp_members
  const int32_t* grp_members;  // (device, [batch]) call indices, group by group; a group's first member is its leader
  const int32_t* grp_keys;     // (device, [groups]) P: the leading keys a group's members hold on the same pages, a multiple of 16
};
// the argument record of the kernels with TREE: the rows' masks behind the RAG record
struct DArgsTree : DArgsRag {
  const uint64_t* tree;  // (device, [total]) one word per packed query token - bit j: draft node j is the token's node or an ancestor of it
};
template <bool RAG, bool GRP = false>
using DArgsOf = std::conditional_t<GRP, DArgsGrp, std::conditional_t<RAG, DArgsRag, DArgs>>;

// the paged source: chunk length and chunk count of a sequence of T = lens[b] keys
__device__ __forceinline__ void paged_chunks(const DArgs& a, int64_t T, int& C, int& nch) {
  C = dec_chunk(T, a.D);
  nch = (int)((T + C - 1) / C);
}

// GRP: what workgroup (chunk c, sequence b) does with a chunk of C keys.  The chunk is SHARED when b's group has more than one member
// and the chunk lies wholly below the group's P keys: the group's leader then loads it once and runs the rows of all n members
// (`mem`: their call indices), every other member leaves (n = 0).  Any other chunk is the workgroup's own: n = 1, mem = nullptr.
// Uniform over the workgroup (scalars), decided before the first barrier.
struct GrpChunk {
  int n;
  const int32_t* mem;
};
__device__ __forceinline__ GrpChunk grp_chunk(const DArgsGrp& a, int64_t b, int64_t c, int C) {
  const int gi = __builtin_amdgcn_readfirstlane(a.grp_of[b]);
  const int m0 = __builtin_amdgcn_readfirstlane(a.grp_starts[gi]), m1 = __builtin_amdgcn_readfirstlane(a.grp_starts[gi + 1]);
  const int P = __builtin_amdgcn_readfirstlane(a.grp_keys[gi]);
  if (m1 - m0 < 2 || (c + 1) * C > P) return {1, nullptr};
  if (__builtin_amdgcn_readfirstlane(a.grp_members[m0]) != b) return {0, nullptr};
  return {m1 - m0, a.grp_members + m0};
}

// WIN: the first key that any of the S rows of a sequence of T keys sees
__device__ __forceinline__ int64_t win_first(const DArgs& a, int64_t T, int64_t S) {
  const int64_t lo = T - S - a.win + 1;
  return lo > 0 ? lo : 0;
}

// The query rows of the call's b-th sequence: S rows per head and R = rep S per kv head, `tok` the token at which they begin in q,
// out and row_stats (0 without RAG: those are addressed through a batch stride), `wrow` the workspace row of row 0 of kv head g.
// RAG: S from q_starts, the same for every lane (made a scalar: the row loops and the divisions by S stay uniform).
struct SeqRows {
  int64_t S, R, tok, wrow;
};
template <bool RAG>
__device__ __forceinline__ SeqRows seq_rows(const DArgsOf<RAG>& a, int64_t b, int64_t g) {
  if constexpr (RAG) {
    const int t0 = __builtin_amdgcn_readfirstlane(a.q_starts[b]), t1 = __builtin_amdgcn_readfirstlane(a.q_starts[b + 1]);
    const int64_t S = t1 - t0, R = a.rep * S;
    return {S, R, t0, (int64_t)t0 * a.heads + g * R};
  } else {
    return {a.S, a.R, 0, (b * a.kv_heads + g) * a.R};
  }
}

// 16 quantized values of one key (the 8 words of quant16_bf16 / codes16_to_bf16) -> their 32 bytes of the key's row of the LDS image
__device__ __forceinline__ void put_key16(unsigned char* at, const uint32_t (&w)[8]) {
  uint4* dst = (uint4*)at;
  dst[0] = make_uint4(w[0], w[1], w[2], w[3]);
  dst[1] = make_uint4(w[4], w[5], w[6], w[7]);
}

// the body of k_attn_dec_scores and k_attn_dec_scores_tree, on the record A of the kernel
template <int DT, int SRC, bool WIN, bool RAG, bool GRP, bool N4, bool TREE, class A>
__device__ __forceinline__ void dec_scores(const A a) {
  static_assert(!N4 || (SRC == SRC_PAGED && !GRP), "nibble K codes: the paged pool, no grouped instantiation");
  static_assert(!TREE || (SRC == SRC_PAGED && RAG && !WIN && !GRP), "the tree rule: the paged pool with per-sequence counts, no window, no groups");
  __shared__ __attribute__((aligned(16))) unsigned char sK[DEC_CMAX * DEC_LS];
  __shared__ float sSt[4][32][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lh = lane >> 5;
  const int64_t c = blockIdx.x, g = blockIdx.y, b = blockIdx.z, z = b * a.kv_heads + g;
  const SeqRows sr = seq_rows<RAG>(a, b, g);
  if constexpr (RAG) {
    if (sr.S <= 0) return;  // (a sequence without query rows: uniform over the workgroup, before any barrier; nothing is written)
  }
  const int64_t S = sr.S, R = sr.R;
  const int32_t* prow;  // the slot's row of the page table
  const int64_t T = kvc::seq<SRC>(a.src, b, a.T, prow);
  int C = a.C, nch = a.nch;
  if constexpr (SRC == SRC_PAGED) {
    paged_chunks(a, T, C, nch);
    if (c >= nch) return;  // (none of this sequence's chunks; uniform over the workgroup, before any barrier)
  }
  int64_t Rt = R;  // GRP: the rows of the row loop - a shared chunk's leader runs those of every member
  const int32_t* mem = nullptr;
  if constexpr (GRP) {
    const GrpChunk gc = grp_chunk(a, b, c, C);
    if (gc.n == 0) return;  // (the leader's workgroup computes this chunk for this sequence's rows)
    Rt = gc.n * R, mem = gc.mem;
  }
  int64_t plo = 0;  // WIN: keys below plo lie on pages wholly outside every row's window - zero rows, their table entries and pages unread
  if constexpr (WIN) {
    const int64_t lo = win_first(a, T, S);
    if (c < lo / C) return;  // (a dead chunk: nothing written, and nothing reads its workspace cells)
    plo = lo / 16 * 16;
  }
  const auto dead = [&](int64_t t) {
    if constexpr (WIN) return t < plo;
    else return false;
  };
  const int64_t t0 = c * C;
  const int D = (int)a.D;
  const float NEG_INF = -__builtin_inff();

  if constexpr (SRC != SRC_RAW) {
    // ---- the chunk's keys from the packed cache: a thread owns 16 consecutive d of 4 consecutive keys - four 16-byte loads of codes and
    // the 16 exponents of their block (one per d); keys at and beyond T are zero rows and are not read
    const int dg_n = D / 16, items = (C / 4) * dg_n;
    for (int it = tid; it < items; it += 256) {
      const int kq = it / dg_n, dg = it % dg_n;
      const int64_t tq = t0 + 4 * kq;
      uint4 e4 = make_uint4(0, 0, 0, 0), c[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) c[j] = make_uint4(0, 0, 0, 0);
      const bool gone = dead(tq);  // (four keys of one page: all of them or none)
      if (tq < T && !gone) {  // (paged: the one table entry first, the five loads one round trip behind it)
        const int64_t blk = kvc::block<SRC>(a.src, prow, z, g, tq / 16);
        e4 = *(const uint4*)(a.src.ke + blk * D + 16 * dg);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (tq + j < T) c[j] = kvc::load_codes16<N4>(a.src.kc, blk, tq % 16 + j, D, dg);
      }
      const uint32_t eb[4] = {e4.x, e4.y, e4.z, e4.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (tq + j < T && !gone) kvc::codes16_to_bf16(c[j], eb, a.qk, w);
        put_key16(sK + (4 * kq + j) * DEC_LS + dg * 32, w);
      }
    }
  } else {
    // ---- the chunk's keys: a thread owns 4 consecutive d of 16 consecutive keys = four blocks of Q_w0 (blocks of 16 along t)
    const int dq = D / 4, ncol = (C / 16) * dq;
    for (int col = tid; col < ncol; col += 256) {
      const int kb = col / dq, d0 = 4 * (col % dq);
      float x[4][16];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int64_t t = t0 + 16 * kb + i;
        float v4[4] = {0.f, 0.f, 0.f, 0.f};
        if (t < T && !dead(t)) load4<DT>(a.k, b * a.k_bs + g * a.k_hs + t * a.k_rs + d0, a.kvec, v4);
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j][i] = v4[j];
      }
      uint32_t w[4][8];
#pragma unroll
      for (int j = 0; j < 4; ++j) quant16_bf16<DT != LQER_F16>(x[j], a.qk, w[j]);
#pragma unroll
      for (int i = 0; i < 16; ++i) {  // key 16 kb + i: the four d as one 8-byte store
        const int sh = 16 * (i & 1);
        const uint32_t lo = ((w[0][i >> 1] >> sh) & 0xffffu) | ((w[1][i >> 1] >> sh) << 16);
        const uint32_t hi = ((w[2][i >> 1] >> sh) & 0xffffu) | ((w[3][i >> 1] >> sh) << 16);
        *(uint2*)(sK + (16 * kb + i) * DEC_LS + d0 * 2) = make_uint2(lo, hi);
      }
    }
  }
  __syncthreads();

  // ---- S^T = Kq Qq^T: wave w takes keys 32 w .. 32 w + 31 of the chunk, a lane ONE query row and 16 of those keys,
  // (r & 3) + 8 (r >> 2) + 4 lh (rows of sK at and beyond C hold whatever LDS held: their scores are never used)
  const int nsub = (C + 31) / 32;
  for (int64_t rg = 0; rg < Rt; rg += 32) {
    int64_t row = rg + l31;
    const bool live = row < Rt;
    int64_t rowc = live ? row : Rt - 1;
    int64_t bq = b, Tq = T, wrow = sr.wrow;  // the sequence of this lane's row: its call index, its length, its workspace row 0
    if constexpr (GRP) {
      if (mem) {  // a shared chunk: row r is row r % R of member r / R - the 32-row groups run straight through the members
        const int64_t j = rowc / R;
        bq = mem[j], Tq = a.src.lens[bq], wrow = (bq * a.kv_heads + g) * R;
        row = rowc = rowc - j * R;  // (a lane that is not live stores nothing)
      }
    }
    const int64_t off = Tq - S;
    const int64_t h = g * a.rep + rowc / S, si = rowc % S;
    float m = NEG_INF, l = 0.f;
    if (wave < nsub) {
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) {
        if (ks * 16 < D) {
          uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
          if (live) {
            float v[16];
            load16<DT>(a.q, bq * a.q_bs + h * a.q_hs + (sr.tok + si) * a.q_rs + ks * 16, 16, a.qvec, v);
            quant16_bf16<DT != LQER_F16>(v, a.q0, w);
          }
          const u32x4 f = {lh ? w[4] : w[0], lh ? w[5] : w[1], lh ? w[6] : w[2], lh ? w[7] : w[3]};
          const bf16x8 kf = *(const bf16x8*)(sK + (32 * wave + l31) * DEC_LS + (2 * ks + lh) * 16);
          acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, __builtin_bit_cast(bf16x8, f), acc, 0, 0, 0);
        }
      }
      int64_t tvis = Tq - 1;  // the last key visible to this lane's query
      if (a.mode == 2) tvis = si + off < tvis ? si + off : tvis;
      int64_t tlo = 0;  // WIN: the first key this lane's query sees (negative: all of them)
      if constexpr (WIN) tlo = si + off - a.win + 1;
      const int64_t moff = a.mode == 1 ? bq * a.m_bs + h * a.m_hs + si * a.m_rs : 0;
      uint64_t tmask = 0;  // TREE: this lane's row of the tree
      if constexpr (TREE) tmask = a.tree[sr.tok + si];
      float s2[16];
      bool vis[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int kk = 32 * wave + (r & 3) + 8 * (r >> 2) + 4 * lh;
        const int64_t t = t0 + kk;
        float s = rnd<DT>(rnd<DT>(acc[r]) * a.scaling);
        if (a.mode == 1) s = rnd<DT>(s + (t < Tq ? load_elem<DT>(a.mask, moff + t) : 0.f));
        s2[r] = s;
        vis[r] = kk < C && t <= tvis && (!WIN || t >= tlo) && (!TREE || tree_sees(tmask, t - off));
      }
      float tm = NEG_INF;
#pragma unroll
      for (int r = 0; r < 16; ++r) tm = vis[r] ? fmaxf(tm, s2[r]) : tm;
      const float mref = tm == NEG_INF ? 0.f : tm;
      float ls = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) ls += vis[r] ? exp_neg(s2[r] - mref) : 0.f;
      if (live) {
        float* dst = a.s2 + (wrow + row) * a.Tp + t0 + 32 * wave + 4 * lh;
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4)
          if (32 * wave + 8 * q4 + 4 * lh < C) *(float4*)(dst + 8 * q4) = make_float4(s2[4 * q4], s2[4 * q4 + 1], s2[4 * q4 + 2], s2[4 * q4 + 3]);
      }
      fold_lane_pair(tm, ls, m, l);  // the lane pair (l, l ^ 32): lower lane's keys first in both lanes
      if (lh == 0) sSt[wave][l31][0] = m, sSt[wave][l31][1] = l;
    }
    __syncthreads();
    if (wave == 0 && lh == 0 && live) {  // the chunk's subtiles in key order
      float M = NEG_INF;
      for (int u = 0; u < nsub; ++u) M = fmaxf(M, sSt[u][l31][0]);
      const float mr = M == NEG_INF ? 0.f : M;
      float L = 0.f;
      for (int u = 0; u < nsub; ++u) L += sSt[u][l31][1] * exp_neg(sSt[u][l31][0] - mr);
      float* cs = a.cst + ((wrow + row) * a.nchs + c) * 2;
      cs[0] = M, cs[1] = L;
    }
    __syncthreads();
  }
}

template <int DT, int SRC, bool WIN, bool RAG, bool GRP, bool N4 = false>
__global__ __launch_bounds__(256, 2) void k_attn_dec_scores(const DArgsOf<RAG, GRP> a) {
  dec_scores<DT, SRC, WIN, RAG, GRP, N4, false>(a);
}
template <int DT, bool N4>
__global__ __launch_bounds__(256, 2) void k_attn_dec_scores_tree(const DArgsTree a) {
  dec_scores<DT, SRC_PAGED, false, true, false, N4, true>(a);
}

// the body of k_attn_dec_pv and k_attn_dec_pv_tree, on the record A of the kernel
template <int DT, int SRC, bool WIN, bool RAG, bool GRP, bool N4, bool TREE, class A>
__device__ __forceinline__ void dec_pv(const A a) {
  static_assert(!N4 || (SRC == SRC_PAGED && !GRP), "nibble V codes: the paged pool, no grouped instantiation");
  static_assert(!TREE || (SRC == SRC_PAGED && RAG && !WIN && !GRP), "the tree rule: the paged pool with per-sequence counts, no window, no groups");
  __shared__ __attribute__((aligned(16))) unsigned char sV[DEC_CMAX * DEC_LS];  // [key][d] bf16
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lh = lane >> 5;
  const int64_t c = blockIdx.x, g = blockIdx.y, b = blockIdx.z, z = b * a.kv_heads + g;
  const SeqRows sr = seq_rows<RAG>(a, b, g);
  if constexpr (RAG) {
    if (sr.S <= 0) return;
  }
  const int64_t S = sr.S, R = sr.R;
  const int32_t* prow;
  const int64_t T = kvc::seq<SRC>(a.src, b, a.T, prow);
  int C = a.C, nch = a.nch;
  if constexpr (SRC == SRC_PAGED) {
    paged_chunks(a, T, C, nch);
    if (c >= nch) return;
  }
  int64_t Rt = R;
  const int32_t* mem = nullptr;
  if constexpr (GRP) {
    const GrpChunk gc = grp_chunk(a, b, c, C);
    if (gc.n == 0) return;
    Rt = gc.n * R, mem = gc.mem;
  }
  int64_t plo = 0;
  int c_lo = 0;  // WIN: the first chunk that holds a visible key
  if constexpr (WIN) {
    const int64_t lo = win_first(a, T, S);
    c_lo = (int)(lo / C);
    if (c < c_lo) return;
    plo = lo / 16 * 16;
  }
  const auto dead = [&](int64_t t) {
    if constexpr (WIN) return t < plo;
    else return false;
  };
  const int64_t t0 = c * C;
  const int D = (int)a.D;
  const float NEG_INF = -__builtin_inff();

  if constexpr (SRC != SRC_RAW) {
    // ---- the chunk's V rows from the packed cache: a thread owns 16 consecutive d (one block of Q_w1) of 4 consecutive keys - four
    // 16-byte loads of codes, one dword of their four exponents; keys at and beyond T are zero rows and are not read
    const int db_n = D / 16, items = (C / 4) * db_n;
    for (int it = tid; it < items; it += 256) {
      const int kq = it / db_n, db = it % db_n;
      const int64_t tq = t0 + 4 * kq;
      uint32_t e4 = 0;
      uint4 c[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) c[j] = make_uint4(0, 0, 0, 0);
      const bool gone = dead(tq);
      if (tq < T && !gone) e4 = kvc::load_v4<N4>(a.src, kvc::block<SRC>(a.src, prow, z, g, tq / 16), tq, T, D, db, c);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const uint32_t e1 = ((e4 >> (8 * j)) & 0xffu) * 0x01010101u;
        const uint32_t eb[4] = {e1, e1, e1, e1};
        if (tq + j < T && !gone) kvc::codes16_to_bf16(c[j], eb, a.qv, w);
        put_key16(sV + (4 * kq + j) * DEC_LS + db * 32, w);
      }
    }
  } else {
    // ---- the chunk's V rows: a thread quantizes 16 consecutive d of one key (blocks of 16 along d); keys beyond T are zero rows
    const int db_n = D / 16, items = C * db_n;
    for (int it = tid; it < items; it += 256) {
      const int key = it / db_n, db = it % db_n;
      const int64_t t = t0 + key;
      uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      if (t < T && !dead(t)) {
        float x[16];
        load16<DT>(a.v, b * a.v_bs + g * a.v_hs + t * a.v_rs + 16 * db, 16, a.vvec, x);
        quant16_bf16<DT != LQER_F16>(x, a.qv, w);
      }
      put_key16(sV + key * DEC_LS + db * 32, w);
    }
  }
  __syncthreads();
  if (wave * 32 >= D) return;  // wave w owns d = 32 w .. 32 w + 31 (no barrier follows)

  for (int64_t rg = 0; rg < Rt; rg += 32) {
    int64_t row = rg + l31;
    const bool live = row < Rt;
    int64_t rowc = live ? row : Rt - 1;
    int64_t Tq = T, wrow = sr.wrow;  // the sequence of this lane's row: its length, its workspace row 0 - and its chunk count
    int nchq = nch;
    if constexpr (GRP) {
      if (mem) {  // a shared chunk: row r is row r % R of member r / R, which folds the statistics of ITS chunks 0 .. nch_j - 1
        const int64_t j = rowc / R, bq = mem[j];
        Tq = a.src.lens[bq], wrow = (bq * a.kv_heads + g) * R, nchq = (int)((Tq + C - 1) / C);
        row = rowc = rowc - j * R;  // (a lane that is not live stores nothing)
      }
    }
    const int64_t off = Tq - S;
    const int64_t si = rowc % S;
    // ---- the row's maximum and sum from the chunk statistics, in chunk order
    const float* cs = a.cst + (wrow + rowc) * a.nchs * 2;
    float M = NEG_INF;
    for (int cc = c_lo; cc < nchq; ++cc) M = fmaxf(M, cs[2 * cc]);
    const float mr = M == NEG_INF ? 0.f : M;
    float L = 0.f;
    for (int cc = c_lo; cc < nchq; ++cc) L += cs[2 * cc + 1] * exp_neg(cs[2 * cc] - mr);
    if (a.stats && c == (WIN ? c_lo : 0) && wave == 0 && lh == 0 && live) {
      // (RAG: row_stats is [total][heads][2] - by token, then head; else [batch][heads][S][2], the workspace's row order)
      float* st = a.stats + (RAG ? (sr.tok + si) * a.heads + g * a.rep + row / S : wrow + row) * 2;
      st[0] = M, st[1] = L;
    }
    int64_t tvis = Tq - 1;
    if (a.mode == 2) tvis = si + off < tvis ? si + off : tvis;
    if (!live) tvis = -1;
    int64_t tlo = 0;
    if constexpr (WIN) tlo = si + off - a.win + 1;
    uint64_t tmask = 0;  // TREE: this lane's row of the tree
    if constexpr (TREE) tmask = a.tree[sr.tok + si];

    // ---- O^T += Vq^T Pq^T: a k-step is one block of 16 keys of Q_x1, this lane's half of it keys 8 lh .. 8 lh + 7
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const float* srow = a.s2 + (wrow + rowc) * a.Tp;
    for (int kst = 0; kst < C / 16; ++kst) {
      const int64_t tb = t0 + 16 * kst + 8 * lh;
      const float4 sa = *(const float4*)(srow + tb), sb = *(const float4*)(srow + tb + 4);
      const float s8[8] = {sa.x, sa.y, sa.z, sa.w, sb.x, sb.y, sb.z, sb.w};
      float p[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) p[i] = tb + i <= tvis && (!WIN || tb + i >= tlo) && (!TREE || tree_sees(tmask, tb + i - off)) ? rnd<DT>(exp_neg(s8[i] - M) / L) : 0.f;  // (S2 = max = -inf: NaN, as the unfused route)
      uint32_t w[4];
      quant8of16_bf16<DT != LQER_F16>(p, a.q1, w);
      const u32x4 pw = {w[0], w[1], w[2], w[3]};
      const unsigned short* vp = (const unsigned short*)(sV + (16 * kst + 8 * lh) * DEC_LS) + 32 * wave + l31;
      uint32_t e[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) e[i] = vp[i * (DEC_LS / 2)];
      const u32x4 vw = {e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16)};
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, vw), __builtin_bit_cast(bf16x8, pw), acc, 0, 0, 0);
    }
    if (live) {  // d = 32 wave + 8 q4 + 4 lh + (0..3)
      float* dst = a.part + ((wrow + row) * a.nchs + c) * a.D + 32 * wave + 4 * lh;
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4)
        if (32 * wave + 8 * q4 + 4 * lh < D) *(float4*)(dst + 8 * q4) = make_float4(acc[4 * q4], acc[4 * q4 + 1], acc[4 * q4 + 2], acc[4 * q4 + 3]);
    }
  }
}

template <int DT, int SRC, bool WIN, bool RAG, bool GRP, bool N4 = false>
__global__ __launch_bounds__(256, 2) void k_attn_dec_pv(const DArgsOf<RAG, GRP> a) {
  dec_pv<DT, SRC, WIN, RAG, GRP, N4, false>(a);
}
template <int DT, bool N4>
__global__ __launch_bounds__(256, 2) void k_attn_dec_pv_tree(const DArgsTree a) {
  dec_pv<DT, SRC_PAGED, false, true, false, N4, true>(a);
}

// one thread = four consecutive d of one output row (PAGED: the chunks of the row's own sequence).  RAG: the grid's y is the
// sequence and its x covers the max_s heads rows a sequence has at most - a thread beyond the S_b heads rows of ITS sequence leaves
// (no barrier in this kernel); the row's sequence costs the two loads of its starts, not a search of q_starts.
template <int DT, bool PAGED, bool WIN, bool RAG>
__global__ __launch_bounds__(256) void k_attn_dec_sum(const DArgsOf<RAG> a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int dq = (int)a.D / 4;
  const int d = 4 * (int)(i % dq);
  int64_t grow = i / dq, b, h, si, S = a.S;  // the workspace row; the sequence, head and row - RAG: token - of out
  if constexpr (RAG) {
    b = blockIdx.y;
    const int64_t tok = a.q_starts[b];
    S = a.q_starts[b + 1] - tok;
    if (grow >= S * a.heads) return;  // (also S_b = 0)
    h = grow / S, si = tok + grow % S, grow += tok * a.heads;
  } else {
    if (i >= a.rows * dq) return;
    b = grow / (a.heads * a.S), h = (grow / a.S) % a.heads, si = grow % a.S;
  }
  int64_t T = a.T;
  int C = a.C, nch = a.nch, c_lo = 0;
  if constexpr (PAGED) {
    T = a.src.lens[b];
    paged_chunks(a, T, C, nch);
  }
  if constexpr (WIN) c_lo = (int)(win_first(a, T, S) / C);  // (the partials of the chunks below were never written)
  const float* p = a.part + grow * a.nchs * a.D + d;
  float o[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
  for (int cc = c_lo; cc < nch; ++cc) {
    const float4 t = *(const float4*)(p + (int64_t)cc * a.D);
    o[0] += t.x, o[1] += t.y, o[2] += t.z, o[3] += t.w;
  }
  store_row4<DT>(a.out, b * a.o_bs + h * a.o_hs + si * a.o_rs + d, d, (int)a.D, o);
}

// The instantiations of the decode kernels that exist, stated once: the window, the per-sequence counts, the groups and the nibble codes
// have public entries on the paged source only, and the grouped kernels take none of the other three; the tree rule comes with the
// per-sequence counts, without a window and without groups.
template <int SRC, bool WIN, bool RAG, bool GRP, bool K4, bool V4, bool TREE = false>
constexpr bool decode_variant_exists() {
  if (TREE) return SRC == SRC_PAGED && RAG && !WIN && !GRP;
  if (SRC != SRC_PAGED) return !(WIN || RAG || GRP || K4 || V4);
  return !GRP || !(WIN || RAG || K4 || V4);
}

// K4 / V4 (the paged pool): the scores kernel reads K alone and the PV kernel V alone - one flag each
template <int DT, int SRC, bool WIN = false, bool RAG = false, bool GRP = false, bool K4 = false, bool V4 = false, bool TREE = false>
static int launch_decode(const std::conditional_t<TREE, DArgsTree, DArgsOf<RAG, GRP>>& a, int64_t batch, hipStream_t st) {
  const dim3 grid((unsigned)a.nchs, (unsigned)a.kv_heads, (unsigned)batch);
  if constexpr (TREE) {
    k_attn_dec_scores_tree<DT, K4><<<grid, 256, 0, st>>>(a);
    k_attn_dec_pv_tree<DT, V4><<<grid, 256, 0, st>>>(a);
  } else {
    k_attn_dec_scores<DT, SRC, WIN, RAG, GRP, K4><<<grid, 256, 0, st>>>(a);
    k_attn_dec_pv<DT, SRC, WIN, RAG, GRP, V4><<<grid, 256, 0, st>>>(a);
  }
  // (RAG: a.S is the bound max_s - x over the rows a sequence has at most, y the sequence)
  const dim3 sgrid((unsigned)(((RAG ? a.S * a.heads : a.rows) * (a.D / 4) + 255) / 256), RAG ? (unsigned)batch : 1u);
  k_attn_dec_sum<DT, SRC == SRC_PAGED, WIN, RAG><<<sgrid, 256, 0, st>>>(a);  // (GRP, TREE: the plain / RAG call's kernel, on the record's base)
  if (TREE) return check_launch("lqer_attention_q_decode_paged_tree");
  if (GRP) return check_launch("lqer_attention_q_decode_paged_shared");
  if (RAG) return check_launch("lqer_attention_q_decode_paged_ragged");
  if (WIN) return check_launch("lqer_attention_q_decode_paged_window");
  return check_launch(SRC == SRC_PAGED ? "lqer_attention_q_decode_paged" : (SRC == SRC_PACKED ? "lqer_attention_q_decode_kv" : "lqer_attention_q_decode"));
}

}  // namespace attn

static size_t dec_align(size_t v) { return (v + 255) / 256 * 256; }

int attention_q_decode_max_s() { return attn::DEC_MAX_S; }
int attention_q_decode_chunk(int64_t T, int64_t D) { return attn::dec_chunk(T, D); }

// rows = batch heads S, C = dec_chunk(T, D), nch = ceil(T / C):
// [S2: rows x nch C fp32][chunk statistics: rows x nch x 2 fp32][partial outputs: rows x nch x D fp32], each rounded up to 256 bytes
size_t attention_q_decode_workspace_bytes(int64_t batch, int64_t heads, int64_t S, int64_t T, int64_t D) {
  const int64_t C = attn::dec_chunk(T, D), nch = (T + C - 1) / C, rows = batch * heads * S;
  return dec_align((size_t)(rows * nch * C) * 4) + dec_align((size_t)(rows * nch * 2) * 4) + dec_align((size_t)(rows * nch * D) * 4);
}

// the paged source: the same three parts with strides fixed by the bound max_len - S2 rows of max_len rounded up to 128 (every T <= max_len
// rounded up to its chunk fits), dec_max_chunks(max_len) chunks per row
size_t attention_q_decode_paged_workspace_bytes(int64_t batch, int64_t heads, int64_t S, int64_t max_len, int64_t D) {
  const int64_t Tp = (max_len + 127) / 128 * 128, nchs = attn::dec_max_chunks(max_len), rows = batch * heads * S;
  return dec_align((size_t)(rows * Tp) * 4) + dec_align((size_t)(rows * nchs * 2) * 4) + dec_align((size_t)(rows * nchs * D) * 4);
}

// per-sequence counts: the same three parts over rows = total heads - a row per packed token and head, whatever the counts are
size_t attention_q_decode_paged_ragged_workspace_bytes(int64_t total, int64_t heads, int64_t max_len, int64_t D) {
  return attention_q_decode_paged_workspace_bytes(1, heads, total, max_len, D);
}

int attention_q_decode_dispatch(const AttnCall& c) {
  attn::DArgsRag a;  // (the kernels without per-sequence counts take its base)
  a.q = c.q, a.k = c.k, a.v = c.v, a.mask = c.mask, a.out = c.out, a.stats = c.row_stats;
  a.S = c.S, a.T = c.T, a.D = c.D;
  a.C = attn::dec_chunk(c.T, c.D), a.nch = a.nchs = (int)((c.T + a.C - 1) / a.C), a.Tp = (int64_t)a.nch * a.C;
  if (c.paged) a.nchs = attn::dec_max_chunks(c.T), a.Tp = (c.T + 127) / 128 * 128;  // (T = max_len; the kernels take T, C, nch from lens[b])
  a.rep = (int)(c.heads / c.kv_heads), a.R = a.rep * c.S, a.rows = c.batch * c.heads * c.S;
  const bool ragged = c.paged && c.pool.ragged;  // (S: the bound max_s; the workspace rows follow the packed tokens)
  a.q_starts = ragged ? c.pool.starts : nullptr;
  if (ragged) a.rows = c.pool.total * c.heads;
  unsigned char* ws = (unsigned char*)c.workspace;
  a.s2 = (float*)ws;
  ws += dec_align((size_t)(a.rows * a.Tp) * 4);
  a.cst = (float*)ws;
  ws += dec_align((size_t)(a.rows * a.nchs * 2) * 4);
  a.part = (float*)ws;
  const int esz = c.dtype == LQER_F32 ? 4 : 2;
  a.q_bs = c.qs[0], a.q_hs = c.qs[1], a.q_rs = c.qs[2];
  a.m_bs = c.mask ? c.ms[0] : 0, a.m_hs = c.mask ? c.ms[1] : 0, a.m_rs = c.mask ? c.ms[2] : 0;
  a.o_bs = c.os[0], a.o_hs = c.os[1], a.o_rs = c.os[2];
  a.heads = (int)c.heads, a.kv_heads = (int)c.kv_heads, a.mode = c.causal ? 2 : (c.mask ? 1 : 0);
  a.win = c.windowed ? (c.window < ((int64_t)1 << 31) ? c.window : (int64_t)1 << 31) : 0;  // (beyond every T <= 2^30 the rule is plain causal)
  a.scaling = c.scaling;
  a.q0 = make_qp(*c.q_fmt), a.qk = make_qp(*c.k_fmt), a.q1 = make_qp(*c.p_fmt), a.qv = make_qp(*c.v_fmt);
  a.qvec = al16(c.q, c.qs, esz);
  a.k_bs = a.k_hs = a.k_rs = a.v_bs = a.v_hs = a.v_rs = 0, a.kvec = a.vvec = false, a.src = {};
  if (c.packed) {  // the codes of a cache or a pool: no k, v (null in c) or their strides
    a.src = kvc::src_of(c);
  } else {
    a.k_bs = c.ks[0], a.k_hs = c.ks[1], a.k_rs = c.ks[2], a.v_bs = c.vs[0], a.v_hs = c.vs[1], a.v_rs = c.vs[2];
    a.kvec = al16(c.k, c.ks, esz), a.vvec = al16(c.v, c.vs, esz);
  }
  attn::DArgsGrp ag;  // (the plain paged call's record and, behind it, the groups)
  if (c.paged && c.grouped) {
    (attn::DArgs&)ag = a;
    ag.grp_of = c.grp_of, ag.grp_starts = c.grp_starts, ag.grp_members = c.grp_members, ag.grp_keys = c.grp_keys;
  }
  attn::DArgsTree at;  // (the record with per-sequence counts and, behind it, the rows' tree masks)
  const bool tree = ragged && c.treed;
  if (tree) {
    (attn::DArgsRag&)at = a;
    at.tree = c.tree;
  }
  return with_dtype(c.dtype, [&](auto dt) {
    return with_flags(
        [&](auto packed, auto paged, auto win, auto rag, auto grp, auto k4, auto v4, auto tr) {
          constexpr int SRC = paged ? attn::SRC_PAGED : (packed ? attn::SRC_PACKED : attn::SRC_RAW);
          if constexpr ((packed || !paged) && attn::decode_variant_exists<SRC, win, rag, grp, k4, v4, tr>()) {
            if constexpr (tr) return attn::launch_decode<dt, SRC, win, rag, grp, k4, v4, tr>(at, c.batch, c.st);
            else if constexpr (grp) return attn::launch_decode<dt, SRC, win, rag, grp, k4, v4>(ag, c.batch, c.st);
            else return attn::launch_decode<dt, SRC, win, rag, grp, k4, v4>(a, c.batch, c.st);
          } else {  // (the checks of api.hip let no such call through)
            set_error("attention_q_decode: no kernel for this combination of source, window, per-sequence counts, groups, nibble codes and tree");
            return (int)LQER_E_UNSUPPORTED;
          }
        },
        c.packed, c.paged, c.paged && c.windowed, ragged, c.paged && c.grouped, c.paged && c.pool.k4, c.paged && c.pool.v4, tree);
  });
}

}  // namespace lqer
