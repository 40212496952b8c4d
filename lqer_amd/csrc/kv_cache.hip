// The packed KV cache's writer and its test hook (layout and codes: kv_pack.h, include/lqer_hip.h "packed KV cache").
//   k_kv_append  new V rows: quantized along d and stored at once (a thread: 16 d of one key - 16 bytes of codes, one exponent byte).
//                new K rows: every block of 16 keys they touch is quantized along t from the staging rows (the raw keys of the open
//                block that were there before) plus the new keys, zero-padded on the right, and stored whole - codes of all 16 rows,
//                the exponents of the block (a thread: 4 d of the 16 keys, as k_attn_dec_scores reads raw keys).  The raw keys of the
//                block left open go to the staging rows.
// One launch when the staging rows read and the staging rows written cannot meet (the new keys stay inside the open block, or the
// cache ended on a block boundary); otherwise the staging rows are written by a second launch of the same kernel.
//   k_kv_unpack  code x 2^(e - mbits) as fp32, one element per thread.
//   k_kv_pool_append / k_kv_pool_gather   the same append into the paged pool (a page = 16 keys of all kv heads; per-sequence lengths
//                and a block table on the device), in one launch (see the kernel), and one sequence's bytes out of the pool into a dense cache.
//   k_kv_kimage / k_kv_vimage   the cache -> the two bf16 images k_attn_q reads (attn_q.hip; what k_attn_kimage / k_attn_vimage write from
//                the raw K and V): codes16_to_bf16 on 16 codes per 16-byte load, zeros wherever the raw image kernels write their
//                padding - every key at or beyond T, every d at or beyond D.  Nothing of the cache at or beyond key T reaches an image.
//                Templated on the source as attn_decode.hip's kernels: the dense cache, or the paged pool - a block of 16 keys found
//                through the page table, T = lens[b] per sequence of the call (lqer_attention_q_paged).
#include "kv_pack.h"

namespace lqer {

namespace kvc {

struct AArgs {
  unsigned char *kc, *ke, *vc, *ve;
  void* stage;
  const void *kn, *vn;
  int64_t Z, kvh, cap, D, len, n;
  int64_t k_bs, k_hs, k_rs, v_bs, v_hs, v_rs;
  int64_t kb0, nkb;  // the blocks of 16 keys the new keys touch
  int64_t s0, ns;    // keys s0 .. s0 + ns - 1 (of the block left open) go to staging rows t % 16
  int phase;         // 1: quantize K blocks and V rows, 2: write the staging rows, 3: both
  QP qk, qv;
  bool kvec, vvec;
};

// 4 d of one block of 16 keys (x[j][r]: d0 + j of key r) -> the codes of the 16 rows (row pitch D bytes, the four d as one dword) and
// the four exponent bytes of the block: the K side of an append, dense or paged
template <int DT>
__device__ __forceinline__ void store_kblock4(const float (&x)[4][16], const QP& qk, unsigned char* kc, int64_t D, unsigned char* ke) {
  uint32_t cw[4][4], eb = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) eb |= quant16_codes<DT != LQER_F16>(x[j], qk, cw[j]) << (8 * j);
#pragma unroll
  for (int r = 0; r < 16; ++r) {  // key r of the block: the four d as one dword
    const int sh = 8 * (r & 3);
    *(uint32_t*)(kc + r * D) = ((cw[0][r >> 2] >> sh) & 0xffu) | (((cw[1][r >> 2] >> sh) & 0xffu) << 8) |
                               (((cw[2][r >> 2] >> sh) & 0xffu) << 16) | (((cw[3][r >> 2] >> sh) & 0xffu) << 24);
  }
  *(uint32_t*)ke = eb;
}

// 16 d of one new V row -> its 16 codes and its exponent byte: the V side of an append, dense or paged
template <int DT>
__device__ __forceinline__ void store_vrow16(const void* vn, int64_t off, bool vec, const QP& qv, unsigned char* vc, unsigned char* ve) {
  float x[16];
  qmm::load16<DT>(vn, off, 16, vec, x);
  uint32_t cw[4];
  const uint32_t eb = quant16_codes<DT != LQER_F16>(x, qv, cw);
  *(uint4*)vc = make_uint4(cw[0], cw[1], cw[2], cw[3]);
  *ve = (unsigned char)eb;
}

// 4 d of one raw key -> a staging row, bits as they are (dst 16- / 8-byte aligned: d0 a multiple of 4 of a row of D elements)
template <int DT>
__device__ __forceinline__ void copy_raw4(const void* kn, int64_t src, bool vec, void* stage, int64_t dst) {
  if constexpr (DT == LQER_F32) {
    const uint32_t* s = (const uint32_t*)kn + src;
    *(uint4*)((uint32_t*)stage + dst) = vec ? *(const uint4*)s : make_uint4(s[0], s[1], s[2], s[3]);
  } else {
    const unsigned short* s = (const unsigned short*)kn + src;
    *(uint2*)((unsigned short*)stage + dst) =
        vec ? *(const uint2*)s : make_uint2((uint32_t)s[0] | ((uint32_t)s[1] << 16), (uint32_t)s[2] | ((uint32_t)s[3] << 16));
  }
}

template <int DT>
__global__ __launch_bounds__(256) void k_kv_append(const AArgs a) {
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int D = (int)a.D, dq = D / 4, db_n = D / 16;
  if (a.phase & 1) {
    const int64_t nK = a.Z * a.nkb * dq, nV = a.Z * a.n * db_n;
    if (i < nK) {  // ---- 4 d of one block of 16 keys
      const int64_t z = i / (a.nkb * dq), rem = i % (a.nkb * dq);
      const int64_t kb = a.kb0 + rem / dq, b = z / a.kvh, g = z % a.kvh;
      const int d0 = 4 * (int)(rem % dq);
      float x[4][16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t t = 16 * kb + r;
        float v4[4] = {0.f, 0.f, 0.f, 0.f};
        if (t < a.len) attn::load4<DT>(a.stage, (z * 16 + r) * a.D + d0, true, v4);
        else if (t < a.len + a.n) attn::load4<DT>(a.kn, b * a.k_bs + g * a.k_hs + (t - a.len) * a.k_rs + d0, a.kvec, v4);
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j][r] = v4[j];
      }
      store_kblock4<DT>(x, a.qk, a.kc + (z * a.cap + 16 * kb) * a.D + d0, a.D, a.ke + (z * (a.cap / 16) + kb) * a.D + d0);
      return;
    }
    i -= nK;
    if (i < nV) {  // ---- 16 d of one new key
      const int64_t z = i / (a.n * db_n), rem = i % (a.n * db_n);
      const int64_t j = rem / db_n, b = z / a.kvh, g = z % a.kvh, t = a.len + j;
      const int db = (int)(rem % db_n);
      store_vrow16<DT>(a.vn, b * a.v_bs + g * a.v_hs + j * a.v_rs + 16 * db, a.vvec, a.qv, a.vc + (z * a.cap + t) * a.D + 16 * db,
                       a.ve + ((z * (a.cap / 16) + t / 16) * db_n + db) * 16 + t % 16);
      return;
    }
    i -= nV;
  }
  if ((a.phase & 2) && i < a.Z * a.ns * dq) {  // ---- 4 d of one raw key of the open block, bits as they are
    const int64_t z = i / (a.ns * dq), rem = i % (a.ns * dq);
    const int64_t t = a.s0 + rem / dq, b = z / a.kvh, g = z % a.kvh;
    const int d0 = 4 * (int)(rem % dq);
    const int64_t src = b * a.k_bs + g * a.k_hs + (t - a.len) * a.k_rs + d0, dst = (z * 16 + t % 16) * a.D + d0;
    copy_raw4<DT>(a.kn, src, a.kvec, a.stage, dst);
  }
}

// ---- the paged pool (kv_pack.h: PoolLayout; include/lqer_hip.h "paged KV pool") --------------------------------------------------------
struct PArgs {
  unsigned char *kc, *ke, *vc, *ve;
  void* stage;
  const void *kn, *vn;
  const int32_t *tbl, *slots, *lens;  // device: [slots][tstride] pages, [batch] slot of the call's b-th sequence, [batch] its length before the call
  int64_t batch, kvh, D, n, tstride;
  int64_t nkbm;  // blocks of 16 keys that n new keys can touch at most (from len % 16 = 15): (n + 14) / 16 + 1
  int64_t k_bs, k_hs, k_rs, v_bs, v_hs, v_rs;
  QP qk, qv;
  bool kvec, vvec;
};

// lqer_kv_cache_append's semantics per sequence, the length read from the device and the blocks found through the slot's table row.
// ONE launch, whatever len % 16 is: the dense append needs a second launch where the staging rows read (0 .. len % 16 - 1) and the
// staging rows written (the open block left behind) can meet, because there different threads read and write them.  Here the thread
// that quantizes 4 d of the FIRST block a sequence's new keys touch - the only thread of the launch that reads the staging column
// (slot, kv head, d0 .. d0 + 3) - also writes that column's new rows, after its reads in program order; no other thread of the launch
// touches the column (a slot is named once per call: the caller's contract), so there is no race and nothing to order between launches.
template <int DT>
__global__ __launch_bounds__(256) void k_kv_pool_append(const PArgs a) {
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int D = (int)a.D, dq = D / 4, db_n = D / 16;
  const int64_t Z = a.batch * a.kvh, nK = Z * a.nkbm * dq, nV = Z * a.n * db_n;
  if (i < nK) {  // ---- 4 d of one block of 16 keys
    const int64_t z = i / (a.nkbm * dq), rem = i % (a.nkbm * dq);
    const int64_t j = rem / dq, b = z / a.kvh, g = z % a.kvh;
    const int d0 = 4 * (int)(rem % dq);
    const int64_t len = a.lens[b], end = len + a.n, kb = len / 16 + j;
    if (kb > (end - 1) / 16) return;  // this sequence's new keys touch fewer blocks
    const int64_t slot = a.slots[b], zs = slot * a.kvh + g;
    const int64_t blk = (int64_t)a.tbl[slot * a.tstride + kb] * a.kvh + g;
    const int64_t kn0 = b * a.k_bs + g * a.k_hs + d0;
    float x[4][16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t t = 16 * kb + r;
      float v4[4] = {0.f, 0.f, 0.f, 0.f};
      if (t < len) attn::load4<DT>(a.stage, (zs * 16 + r) * a.D + d0, true, v4);  // (only j == 0 meets keys below len)
      else if (t < end) attn::load4<DT>(a.kn, kn0 + (t - len) * a.k_rs, a.kvec, v4);
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) x[jj][r] = v4[jj];
    }
    store_kblock4<DT>(x, a.qk, a.kc + blk * 16 * a.D + d0, a.D, a.ke + blk * a.D + d0);
    if (j == 0) {  // the raw keys of the block left open -> staging rows t % 16 of this thread's column
      const int64_t open0 = end / 16 * 16, s0 = open0 > len ? open0 : len;
      for (int64_t t = s0; t < end; ++t) copy_raw4<DT>(a.kn, kn0 + (t - len) * a.k_rs, a.kvec, a.stage, (zs * 16 + t % 16) * a.D + d0);
    }
    return;
  }
  i -= nK;
  if (i < nV) {  // ---- 16 d of one new key
    const int64_t z = i / (a.n * db_n), rem = i % (a.n * db_n);
    const int64_t j = rem / db_n, b = z / a.kvh, g = z % a.kvh, t = a.lens[b] + j;
    const int db = (int)(rem % db_n);
    const int64_t blk = (int64_t)a.tbl[(int64_t)a.slots[b] * a.tstride + t / 16] * a.kvh + g;
    store_vrow16<DT>(a.vn, b * a.v_bs + g * a.v_hs + j * a.v_rs + 16 * db, a.vvec, a.qv, a.vc + (blk * 16 + t % 16) * a.D + 16 * db,
                     a.ve + (blk * db_n + db) * 16 + t % 16);
  }
}

struct GArgs {
  const unsigned char* src[5];  // the pool's sections
  unsigned char* dst[5];        // the dense cache's (batch 1)
  const int32_t* row;           // the slot's table row (device)
  int64_t slot, kvh, D, nblk, capb, stage16;  // blocks of 16 keys copied, cap / 16 of the dense cache, 16-byte pieces of a kv head's staging rows
};

// One sequence out of the pool into a dense cache of batch 1: bytes as they are, in 16-byte pieces.  A thread: one piece of one
// (kv head, block) - D pieces of K codes, D / 16 of K exponents, D of V codes, D / 16 of V exponents - or one piece of the staging rows.
__global__ __launch_bounds__(256) void k_kv_pool_gather(const GArgs a) {
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t e16 = a.D / 16, per = 2 * (a.D + e16), nB = a.kvh * a.nblk * per;
  if (i < nB) {
    const int64_t g = i / (a.nblk * per), kb = (i / per) % a.nblk;
    int64_t u = i % per;
    const int64_t sblk = (int64_t)a.row[kb] * a.kvh + g, dblk = g * a.capb + kb;
    int sec = 0;
    if (u >= a.D) u -= a.D, sec = 1;
    if (sec == 1 && u >= e16) u -= e16, sec = 2;
    if (sec == 2 && u >= a.D) u -= a.D, sec = 3;
    const int64_t item = (sec & 1) ? e16 : a.D;  // 16-byte pieces of a block in this section
    ((uint4*)a.dst[sec])[dblk * item + u] = ((const uint4*)a.src[sec])[sblk * item + u];
    return;
  }
  i -= nB;
  if (i < a.kvh * a.stage16) ((uint4*)a.dst[4])[i] = ((const uint4*)a.src[4])[a.slot * a.kvh * a.stage16 + i];
}

struct UArgs {
  const unsigned char *kc, *ke, *vc, *ve;
  float *kf, *vf;
  int64_t Z, cap, T, D;
  QP qk, qv;
};

__global__ __launch_bounds__(256) void k_kv_unpack(const UArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.Z * a.T * a.D) return;
  const int64_t z = i / (a.T * a.D), t = (i / a.D) % a.T, d = i % a.D;
  const int64_t at = (z * a.cap + t) * a.D + d, blk = z * (a.cap / 16) + t / 16;
  if (a.kf) a.kf[i] = code_value(a.kc[at], a.ke[blk * a.D + d], a.qk);
  if (a.vf) a.vf[i] = code_value(a.vc[at], a.ve[(blk * (a.D / 16) + d / 16) * 16 + t % 16], a.qv);
}

struct IArgs {
  const unsigned char *kc, *ke, *vc, *ve;
  bf16_t *kimg, *vimg;  // [Z][Tp][Dp], [Z][ATTN_V_ROWS][Tv]
  int64_t cap, D, T, Tp, Dp, Tv;
  QP qk, qv;
};
// the paged source (SRC_PAGED): the sections are the pool's, z runs over (sequence of the call, kv head), T, Tp and Tv come from the
// bound max_len and a workgroup takes its sequence's own T from lens (device) - cap and T above are unused
struct PIArgs : IArgs {
  const int32_t *tbl, *slots, *lens;  // [slots][tstride] pages, [batch] slot and length of the b-th sequence
  int64_t kvh, tstride;
};
template <int SRC>
using ImgArgs = std::conditional_t<SRC == attn::SRC_PAGED, PIArgs, IArgs>;

// the paged source's sizes for image z = b kv_heads + g: the sequence's length, its row of the page table and its kv head
__device__ __forceinline__ int64_t paged_seq(const PIArgs& a, int64_t z, const int32_t*& row, int64_t& g) {
  const int64_t b = z / a.kvh;
  g = z % a.kvh;
  row = a.tbl + (int64_t)a.slots[b] * a.tstride;
  return a.lens[b];
}

// K image: the codes' own layout, no transpose.  A thread: 16 d of one key - 16 code bytes, the 16 exponent bytes of (block of keys, d),
// 32 bytes of the image row; consecutive threads, consecutive pieces of the row.  grid.x covers Tp (Dp / 16) exactly (a multiple of 512).
// SRC_PAGED: the block of 16 keys is found through the sequence's row of the page table - one entry per thread, the two loads one round
// trip behind it - and keys at and beyond lens[b] are zeros up to the end of the 64-key tile k_attn_q reads last; a workgroup (32 or 64
// keys) that starts beyond that tile writes nothing and leaves at once: a short sequence of a ragged batch costs its own keys.
template <int SRC>
__global__ __launch_bounds__(256) void k_kv_kimage(const ImgArgs<SRC> a) {
  const int64_t z = blockIdx.y, i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int dq = (int)(a.Dp / 16);
  const int64_t t = i / dq;
  const int d0 = 16 * (int)(i % dq);
  int64_t T = a.T;
  const int32_t* prow = nullptr;
  int64_t g = 0;
  if constexpr (SRC == attn::SRC_PAGED) {
    T = paged_seq(a, z, prow, g);
    if ((int64_t)blockIdx.x * (256 / dq) >= (T + 63) / 64 * 64) return;  // (uniform over the workgroup; the kernel has no barrier)
  }
  (void)prow, (void)g;
  uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (t < T && d0 < a.D) {
    uint4 c, e;
    if constexpr (SRC == attn::SRC_PAGED) {
      const int64_t blk = (int64_t)prow[t / 16] * a.kvh + g;
      c = *(const uint4*)(a.kc + (blk * 16 + t % 16) * a.D + d0);
      e = *(const uint4*)(a.ke + blk * a.D + d0);
    } else {
      c = *(const uint4*)(a.kc + (z * a.cap + t) * a.D + d0);
      e = *(const uint4*)(a.ke + (z * (a.cap / 16) + t / 16) * a.D + d0);
    }
    const uint32_t eb[4] = {e.x, e.y, e.z, e.w};
    codes16_to_bf16(c, eb, a.qk, w);
  }
  uint4* dst = (uint4*)(a.kimg + (z * a.Tp + t) * a.Dp + d0);
  dst[0] = make_uint4(w[0], w[1], w[2], w[3]);
  dst[1] = make_uint4(w[4], w[5], w[6], w[7]);
}

// V image: V^T, rows d, t contiguous - a transpose through LDS.  One workgroup = 64 keys x all ATTN_V_ROWS image rows.
// In: thread (db = tid & 7, tg = tid >> 3) takes 16 d of the four keys t0 + 4 tg ..: four 16-byte code loads and ONE dword of
// exponents (the cache keeps the bytes of four consecutive keys of a d block together), and stores, per d, the four keys' bf16 as
// 8 bytes of the tile row d.  Out: thread (c = tid & 7) moves 16 bytes (8 keys) of the rows tid >> 3 + 16 u: eight consecutive
// lanes write the 128 contiguous bytes of an image row.
// Tile: [128 d][64 t] bf16 in 128-byte rows; the 8-byte group g of row d lives at group (g + 2 (d >> 4)) & 15.  The 8-byte stores are
// served in groups of 16 consecutive lanes on 32 banks - lanes (db 0-7, tg 2 j, 2 j + 1) at one i: without the rotation eight rows 16
// apart put all eight db on the same two groups (8-way); with it the 16 lanes hit the 16 groups of a 128-byte bank row once each.
// The rotation is even, so a 16-byte pair of groups stays a pair: the reads - per group of 16 lanes two even and two odd rows (256-byte
// bank row: the odd rows are the upper half), chunks 0-3 of one row and 4-7 of the other, all rotated by the same d >> 4 - stay
// conflict-free.
// SRC_PAGED: T = lens[b]; the four keys of a thread lie in one page - one table entry, the five loads one round trip behind it; a
// workgroup whose 64 keys start at or beyond T (a tile k_attn_q does not read for this sequence) leaves before the barrier.
template <int SRC>
__global__ __launch_bounds__(128) void k_kv_vimage(const ImgArgs<SRC> a) {
  __shared__ __attribute__((aligned(16))) unsigned char tile[ATTN_V_ROWS * 128];
  static_assert(ATTN_V_ROWS == 128, "the thread maps below cover 8 blocks of 16 d");
  const int tid = threadIdx.x;
  const int64_t z = blockIdx.y, t0 = (int64_t)blockIdx.x * 64;
  int64_t T = a.T;
  const int32_t* prow = nullptr;
  int64_t g = 0;
  if constexpr (SRC == attn::SRC_PAGED) {
    T = paged_seq(a, z, prow, g);
    if (t0 >= T) return;  // (uniform over the workgroup)
  }
  (void)prow, (void)g;
  {
    const int db = tid & 7, tg = tid >> 3;
    const int64_t t = t0 + 4 * tg;
    uint32_t w[4][8];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int j = 0; j < 8; ++j) w[r][j] = 0;
    if (16 * db < a.D && t < T) {  // (t < T <= cap, t a multiple of 4: the dword of exponents lies inside the section)
      int64_t blk = 0;  // the block of 16 keys
      if constexpr (SRC == attn::SRC_PAGED) blk = (int64_t)prow[t / 16] * a.kvh + g;
      else blk = z * (a.cap / 16) + t / 16;
      const uint32_t e4 = *(const uint32_t*)(a.ve + (blk * (a.D / 16) + db) * 16 + t % 16);
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (t + r < T) {
          const unsigned char* cp;
          if constexpr (SRC == attn::SRC_PAGED) cp = a.vc + (blk * 16 + t % 16 + r) * a.D + 16 * db;
          else cp = a.vc + (z * a.cap + t + r) * a.D + 16 * db;
          const uint4 c = *(const uint4*)cp;
          const uint32_t e = ((e4 >> (8 * r)) & 0xffu) * 0x01010101u;  // one exponent for the 16 d
          const uint32_t eb[4] = {e, e, e, e};
          codes16_to_bf16(c, eb, a.qv, w[r]);
        }
    }
    unsigned char* row = tile + (16 * db) * 128 + 8 * ((tg + 2 * db) & 15);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int sh = 16 * (i & 1);
      *(uint2*)(row + i * 128) = make_uint2(((w[0][i >> 1] >> sh) & 0xffffu) | (((w[1][i >> 1] >> sh) & 0xffffu) << 16),
                                            ((w[2][i >> 1] >> sh) & 0xffffu) | (((w[3][i >> 1] >> sh) & 0xffffu) << 16));
    }
  }
  __syncthreads();
  {
    const int c = tid & 7;
#pragma unroll
    for (int u = 0; u < ATTN_V_ROWS / 16; ++u) {
      const int d = (tid >> 3) + 16 * u;  // d >> 4 == u
      *(uint4*)(a.vimg + (z * ATTN_V_ROWS + d) * a.Tv + t0 + 8 * c) = *(const uint4*)(tile + d * 128 + 16 * ((c + u) & 7));
    }
  }
}

}  // namespace kvc

size_t kv_cache_bytes(int dtype, int64_t batch, int64_t kv_heads, int64_t capacity, int64_t D) {
  return kvc::layout(dtype, batch, kv_heads, capacity, D).total;
}

int kv_cache_append_dispatch(void* cache, const void* k_new, const void* v_new, const int64_t* ks, const int64_t* vs, int dtype, int64_t batch,
                             int64_t kv_heads, int64_t capacity, int64_t D, int64_t len, int64_t n, const QP& qk, const QP& qv, hipStream_t st) {
  const kvc::Layout l = kvc::layout(dtype, batch, kv_heads, capacity, D);
  const auto s = kvc::sections((unsigned char*)cache, l);
  kvc::AArgs a;
  a.kc = s.kc, a.ke = s.ke, a.vc = s.vc, a.ve = s.ve, a.stage = (unsigned char*)cache + l.k_stage;
  a.kn = k_new, a.vn = v_new;
  a.Z = batch * kv_heads, a.kvh = kv_heads, a.cap = s.cap, a.D = D, a.len = len, a.n = n;
  a.k_bs = ks[0], a.k_hs = ks[1], a.k_rs = ks[2], a.v_bs = vs[0], a.v_hs = vs[1], a.v_rs = vs[2];
  a.kb0 = len / 16, a.nkb = (len + n - 1) / 16 - a.kb0 + 1;
  const int64_t open0 = (len + n) / 16 * 16;  // first key of the block left open
  a.s0 = open0 > len ? open0 : len, a.ns = len + n - a.s0;
  a.qk = qk, a.qv = qv;
  const int esz = dtype == LQER_F32 ? 4 : 2;
  a.kvec = al16(k_new, ks, esz), a.vvec = al16(v_new, vs, esz);
  // staging rows read: 0 .. len % 16 - 1; written: (t % 16) of keys s0 .. len + n - 1 - apart when the new keys stay in the open block
  const bool one = len % 16 == 0 || a.s0 == len || a.ns == 0;
  const int64_t n1 = a.Z * (a.nkb * (D / 4) + n * (D / 16)), n2 = a.Z * a.ns * (D / 4);
  return with_dtype(dtype, [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    a.phase = one ? 3 : 1;
    const int64_t items = n1 + (one ? n2 : 0);
    kvc::k_kv_append<DT><<<dim3((unsigned)((items + 255) / 256)), 256, 0, st>>>(a);
    if (!one) {
      a.phase = 2;
      kvc::k_kv_append<DT><<<dim3((unsigned)((n2 + 255) / 256)), 256, 0, st>>>(a);
    }
    return check_launch("lqer_kv_cache_append");
  });
}

size_t kv_pool_bytes(int dtype, int64_t pages, int64_t slots, int64_t kv_heads, int64_t D) {
  return kvc::pool_layout(dtype, pages, slots, kv_heads, D).total;
}

int kv_pool_append_dispatch(const KvPool& p, const void* k_new, const void* v_new, const int64_t* ks, const int64_t* vs, int64_t batch, int64_t n,
                            const QP& qk, const QP& qv, hipStream_t st) {
  const kvc::PoolLayout l = kvc::pool_layout(p.dtype, p.pages, p.slots, p.kv_heads, p.D);
  unsigned char* base = (unsigned char*)p.pool;
  kvc::PArgs a;
  a.kc = base + l.k_codes, a.ke = base + l.k_exps, a.vc = base + l.v_codes, a.ve = base + l.v_exps, a.stage = base + l.k_stage;
  a.kn = k_new, a.vn = v_new, a.tbl = p.block_table, a.slots = p.seq_slots, a.lens = p.lens;
  a.batch = batch, a.kvh = p.kv_heads, a.D = p.D, a.n = n, a.tstride = p.table_stride, a.nkbm = (n + 14) / 16 + 1;
  a.k_bs = ks[0], a.k_hs = ks[1], a.k_rs = ks[2], a.v_bs = vs[0], a.v_hs = vs[1], a.v_rs = vs[2];
  a.qk = qk, a.qv = qv;
  const int esz = p.dtype == LQER_F32 ? 4 : 2;
  a.kvec = al16(k_new, ks, esz), a.vvec = al16(v_new, vs, esz);
  const int64_t items = batch * p.kv_heads * (a.nkbm * (p.D / 4) + n * (p.D / 16));
  return with_dtype(p.dtype, [&](auto dt) {
    kvc::k_kv_pool_append<decltype(dt)::value><<<dim3((unsigned)((items + 255) / 256)), 256, 0, st>>>(a);
    return check_launch("lqer_kv_pool_append");
  });
}

int kv_pool_gather_dispatch(const KvPool& p, int64_t slot, int64_t T, void* cache, int64_t capacity, hipStream_t st) {
  const kvc::PoolLayout pl = kvc::pool_layout(p.dtype, p.pages, p.slots, p.kv_heads, p.D);
  const kvc::Layout dl = kvc::layout(p.dtype, 1, p.kv_heads, capacity, p.D);
  const unsigned char* sb = (const unsigned char*)p.pool;
  unsigned char* db = (unsigned char*)cache;
  kvc::GArgs a;
  const size_t so[5] = {pl.k_codes, pl.k_exps, pl.v_codes, pl.v_exps, pl.k_stage}, dof[5] = {dl.k_codes, dl.k_exps, dl.v_codes, dl.v_exps, dl.k_stage};
  for (int i = 0; i < 5; ++i) a.src[i] = sb + so[i], a.dst[i] = db + dof[i];
  a.row = p.block_table + slot * p.table_stride, a.slot = slot, a.kvh = p.kv_heads, a.D = p.D;
  a.nblk = (T + 15) / 16, a.capb = dl.cap / 16, a.stage16 = p.D * (p.dtype == LQER_F32 ? 4 : 2);  // 16 rows x D x esz / 16
  const int64_t items = p.kv_heads * (a.nblk * 2 * (p.D + p.D / 16) + a.stage16);
  kvc::k_kv_pool_gather<<<dim3((unsigned)((items + 255) / 256)), 256, 0, st>>>(a);
  return check_launch("lqer_kv_pool_gather");
}

int kv_cache_unpack_dispatch(const void* cache, int dtype, int64_t batch, int64_t kv_heads, int64_t capacity, int64_t D, int64_t T, const QP& qk,
                             const QP& qv, float* k_f32, float* v_f32, hipStream_t st) {
  const auto s = kvc::sections((const unsigned char*)cache, kvc::layout(dtype, batch, kv_heads, capacity, D));
  kvc::UArgs a;
  a.kc = s.kc, a.ke = s.ke, a.vc = s.vc, a.ve = s.ve;
  a.kf = k_f32, a.vf = v_f32, a.Z = batch * kv_heads, a.cap = s.cap, a.T = T, a.D = D, a.qk = qk, a.qv = qv;
  kvc::k_kv_unpack<<<dim3((unsigned)((a.Z * T * D + 255) / 256)), 256, 0, st>>>(a);
  return check_launch("lqer_kv_cache_unpack");
}

// the two images of lqer_attention_q's workspace from the cache's first T keys - or, from the paged pool, from every sequence's first
// lens[b] keys, the images' strides those of T = max_len; the caller (attn_q.hip) checks the launches
void kv_cache_images_dispatch(const AttnCall& c, bf16_t* kimg, int64_t Tp, int64_t Dp, bf16_t* vimg, int64_t Tv) {
  kvc::PIArgs a;
  a.kimg = kimg, a.vimg = vimg, a.D = c.D, a.T = c.T, a.Tp = Tp, a.Dp = Dp, a.Tv = Tv;
  a.qk = make_qp(*c.k_fmt), a.qv = make_qp(*c.v_fmt);
  const dim3 kgrid((unsigned)(Tp * (Dp / 16) / 256), (unsigned)(c.batch * c.kv_heads)), vgrid((unsigned)(Tv / 64), (unsigned)(c.batch * c.kv_heads));
  if (c.paged) {
    const kvc::PoolLayout l = kvc::pool_layout(c.dtype, c.pool.pages, c.pool.slots, c.kv_heads, c.D);
    const unsigned char* base = (const unsigned char*)c.pool.pool;
    a.kc = base + l.k_codes, a.ke = base + l.k_exps, a.vc = base + l.v_codes, a.ve = base + l.v_exps, a.cap = 0;
    a.tbl = c.pool.block_table, a.slots = c.pool.seq_slots, a.lens = c.pool.lens, a.kvh = c.kv_heads, a.tstride = c.pool.table_stride;
    kvc::k_kv_kimage<attn::SRC_PAGED><<<kgrid, 256, 0, c.st>>>(a);
    kvc::k_kv_vimage<attn::SRC_PAGED><<<vgrid, 128, 0, c.st>>>(a);
    return;
  }
  const auto s = kvc::sections((const unsigned char*)c.cache, kvc::layout(c.dtype, c.batch, c.kv_heads, c.capacity, c.D));
  a.kc = s.kc, a.ke = s.ke, a.vc = s.vc, a.ve = s.ve, a.cap = s.cap;
  kvc::k_kv_kimage<attn::SRC_PACKED><<<kgrid, 256, 0, c.st>>>((const kvc::IArgs&)a);
  kvc::k_kv_vimage<attn::SRC_PACKED><<<vgrid, 128, 0, c.st>>>((const kvc::IArgs&)a);
}

}  // namespace lqer
