// The packed KV cache's writer and its test hook (layout, codes and the source record kvc::KvSrc every kernel here addresses a block of
// 16 keys through: kv_pack.h; include/lqer_hip.h "packed KV cache", "paged KV pool").  The kernels are templated on the source as
// attn_decode.hip's: the dense cache, or the paged pool (a page = 16 keys of all kv heads; per-sequence lengths and a block table on
// the device).
//   k_kv_append  new V rows: quantized along d and stored at once (a thread: 16 d of one key - 16 bytes of codes, one exponent byte).
//                new K rows: every block of 16 keys they touch is quantized along t from the staging rows (the raw keys of the open
//                block that were there before) plus the new keys, zero-padded on the right, and stored whole - codes of all 16 rows,
//                the exponents of the block (a thread: 4 d of the 16 keys, as k_attn_dec_scores reads raw keys).  The raw keys of the
//                block left open go to the staging rows.  One launch, whatever the length was (see the kernel).  A third instantiation
//                (RAG) takes every sequence's own number of new keys from the device (lqer_kv_pool_append_ragged).
//   k_kv_unpack  code x 2^(e - mbits) as fp32, one element per thread.
//   k_kv_pool_gather   one sequence's bytes out of the pool into a dense cache.
//   k_kv_pool_fork     children that share their parents' full pages: the open block's item and the staging rows, copied per child.
//   k_kv_pool_copy     pages and slots' staging rows from one pool to another (or within one), by id lists: fork's section walk.
//   k_kv_kimage / k_kv_vimage   the cache -> the two bf16 images k_attn_q reads (attn_q.hip; what k_attn_kimage / k_attn_vimage write from
//                the raw K and V): codes16_to_bf16 on 16 codes per 16-byte load, zeros wherever the raw image kernels write their
//                padding - every key at or beyond T, every d at or beyond D.  Nothing of the cache at or beyond key T reaches an image.
//                From the pool: T = lens[b] per sequence of the call (lqer_attention_q_paged).  With the window rule (WIN:
//                lqer_attention_q_paged_window, lqer_attention_q_paged_ragged_window) nothing of the pool below the page of the first
//                key the call's first query row sees is read either: tiles wholly below it are not written, the rest of its tile is zeros.
// NIBBLE codes (the paged pool, per operand - kv_pack.h; template parameters K4 / V4 / N4): the append's store stage packs two codes
// per byte, every byte written whole by one thread; the readers load 8 bytes where they loaded 16 and widen them in front of the same
// conversion; gather widens into the dense cache's byte codes; fork copies the smaller item.  Byte pools run the instantiations they ran.
#include "kv_pack.h"

namespace lqer {

namespace kvc {

struct AArgs {
  KvSrc<unsigned char> src;
  const void *kn, *vn;
  int64_t batch, D, n;
  int64_t len;  // SRC_PACKED: the length before the call (SRC_PAGED: lens[b], on the device)
  int64_t nkb;  // blocks of 16 keys per (sequence, kv head) the grid covers: those the n new keys touch, or (lengths on the device) can
                // touch at most - from len % 16 = 15: (n + 14) / 16 + 1
  int64_t k_bs, k_hs, k_rs, v_bs, v_hs, v_rs;
  QP qk, qv;
  bool kvec, vvec;
  const int32_t* starts;  // RAG: [batch + 1] (device) - sequence b's new keys are tokens starts[b] .. starts[b + 1] - 1 of kn / vn
                          // [total][kv heads][D] (k_bs = v_bs = 0, k_rs / v_rs the token strides); n and nkb above are then those of the
                          // bound max_n, which sizes the grid
};

// 4 d of one block of 16 keys (x[j][r]: d0 + j of key r) -> the codes of the 16 rows (kc: the block's first row at d0; row pitch D bytes,
// the four d as one dword) and the four exponent bytes of the block: the K side of an append, dense or paged.  N4 (nibble codes, kc at
// d0 / 2, row pitch D / 2): the four d are the two WHOLE bytes d0 / 2, d0 / 2 + 1 of every row - one 2-byte store, no byte shared with
// another thread and none read back, so a dirty page leaves no stale neighbour nibble
template <int DT, bool N4>
__device__ __forceinline__ void store_kblock4(const float (&x)[4][16], const QP& qk, unsigned char* kc, int64_t D, unsigned char* ke) {
  uint32_t cw[4][4], eb = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) eb |= quant16_codes<DT != LQER_F16>(x[j], qk, cw[j]) << (8 * j);
#pragma unroll
  for (int r = 0; r < 16; ++r) {  // key r of the block: the four d as one dword
    const int sh = 8 * (r & 3);
    const uint32_t c4 = ((cw[0][r >> 2] >> sh) & 0xffu) | (((cw[1][r >> 2] >> sh) & 0xffu) << 8) |
                        (((cw[2][r >> 2] >> sh) & 0xffu) << 16) | (((cw[3][r >> 2] >> sh) & 0xffu) << 24);
    if constexpr (N4) *(unsigned short*)(kc + r * code_pitch<true>(D)) = (unsigned short)narrow8(c4, 0);
    else *(uint32_t*)(kc + r * D) = c4;
  }
  *(uint32_t*)ke = eb;
}

// 16 d of one new V row -> its 16 codes (16 bytes, or with N4 the 8 bytes of their nibbles) and its exponent byte: the V side of an
// append, dense or paged
template <int DT, bool N4>
__device__ __forceinline__ void store_vrow16(const void* vn, int64_t off, bool vec, const QP& qv, unsigned char* vc, unsigned char* ve) {
  float x[16];
  load16<DT>(vn, off, 16, vec, x);
  uint32_t cw[4];
  const uint32_t eb = quant16_codes<DT != LQER_F16>(x, qv, cw);
  if constexpr (N4) *(uint2*)vc = make_uint2(narrow8(cw[0], cw[1]), narrow8(cw[2], cw[3]));
  else *(uint4*)vc = make_uint4(cw[0], cw[1], cw[2], cw[3]);
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

// lqer_kv_cache_append's semantics per sequence; with the pool the length is read from the device and the blocks are found through the
// slot's table row.  ONE launch, whatever len % 16 is, although the staging rows read (0 .. len % 16 - 1) and the staging rows written
// (the open block left behind) can meet: the thread that quantizes 4 d of the FIRST block a sequence's new keys touch - the only thread
// of the launch that reads the staging column (slot, kv head, d0 .. d0 + 3), every later block starts beyond len - also writes that
// column's new rows, after its reads in program order; no other thread of the launch touches the column (a slot - with the dense cache
// the batch index - is named once per call: the pool's caller's contract), so there is no race and nothing to order between launches.
// RAG (per-sequence counts, the paged pool): the grid is laid out for the bound a.n = max_n and sequence b takes n_b = starts[b + 1] -
// starts[b] from the device; its threads at a block or a key beyond n_b - all of them with n_b = 0 - leave at once, before any load
// or store.  The argument above holds per sequence as it stands: block j = 0 of (sequence, kv head, d0) exists for every n_b >= 1, its
// one thread is the only reader of the staging column and the only writer of it, reads first; the later blocks start beyond len.
// K4 / V4 (the paged pool): the K / V code section holds nibbles - the store stage alone differs (store_kblock4, store_vrow16).
template <int DT, int SRC, bool RAG = false, bool K4 = false, bool V4 = false>
__global__ __launch_bounds__(256) void k_kv_append(const AArgs a) {
  static_assert(!RAG || SRC == attn::SRC_PAGED, "per-sequence counts come with per-sequence lengths");
  static_assert(!(K4 || V4) || SRC == attn::SRC_PAGED, "nibble codes are a storage of the paged pool");
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int D = (int)a.D, dq = D / 4, db_n = D / 16;
  const int64_t kvh = a.src.kvh, Z = a.batch * kvh, nK = Z * a.nkb * dq, nV = Z * a.n * db_n;
  const int32_t* row;
  if (i < nK) {  // ---- 4 d of one block of 16 keys
    const int64_t z = i / (a.nkb * dq), rem = i % (a.nkb * dq);
    const int64_t j = rem / dq, b = z / kvh, g = z % kvh;
    const int d0 = 4 * (int)(rem % dq);
    int64_t n = a.n, tok0 = 0;  // this sequence's new keys and the first one's token
    if constexpr (RAG) {
      tok0 = a.starts[b], n = a.starts[b + 1] - tok0;
      if (n < 1) return;
    }
    const int64_t len = seq<SRC>(a.src, b, a.len, row), end = len + n, kb = len / 16 + j;
    if (kb > (end - 1) / 16) return;  // this sequence's new keys touch fewer blocks
    int64_t slot = b;
    if constexpr (SRC == attn::SRC_PAGED) slot = a.src.slots[b];
    const int64_t zs = slot * kvh + g, blk = block<SRC>(a.src, row, z, g, kb);
    const int64_t kn0 = b * a.k_bs + tok0 * a.k_rs + g * a.k_hs + d0;
    float x[4][16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t t = 16 * kb + r;
      float v4[4] = {0.f, 0.f, 0.f, 0.f};
      if (t < len) attn::load4<DT>(a.src.stage, (zs * 16 + r) * a.D + d0, true, v4);  // (only j == 0 meets keys below len)
      else if (t < end) attn::load4<DT>(a.kn, kn0 + (t - len) * a.k_rs, a.kvec, v4);
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) x[jj][r] = v4[jj];
    }
    store_kblock4<DT, K4>(x, a.qk, a.src.kc + blk * 16 * code_pitch<K4>(a.D) + (K4 ? d0 / 2 : d0), a.D, a.src.ke + blk * a.D + d0);
    if (j == 0) {  // the raw keys of the block left open -> staging rows t % 16 of this thread's column
      const int64_t open0 = end / 16 * 16, s0 = open0 > len ? open0 : len;
      for (int64_t t = s0; t < end; ++t) copy_raw4<DT>(a.kn, kn0 + (t - len) * a.k_rs, a.kvec, a.src.stage, (zs * 16 + t % 16) * a.D + d0);
    }
    return;
  }
  i -= nK;
  if (i < nV) {  // ---- 16 d of one new key
    const int64_t z = i / (a.n * db_n), rem = i % (a.n * db_n);
    const int64_t j = rem / db_n, b = z / kvh, g = z % kvh;
    int64_t tok0 = 0;
    if constexpr (RAG) {
      tok0 = a.starts[b];
      if (j >= a.starts[b + 1] - tok0) return;  // a key beyond this sequence's count
    }
    const int64_t t = seq<SRC>(a.src, b, a.len, row) + j;
    const int db = (int)(rem % db_n);
    const int64_t blk = block<SRC>(a.src, row, z, g, t / 16);
    store_vrow16<DT, V4>(a.vn, b * a.v_bs + g * a.v_hs + (tok0 + j) * a.v_rs + 16 * db, a.vvec, a.qv,
                         a.src.vc + (blk * 16 + t % 16) * code_pitch<V4>(a.D) + (V4 ? 8 : 16) * db, a.src.ve + (blk * db_n + db) * 16 + t % 16);
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
// K4 / V4: the pool's K / V codes are nibbles and the dense cache's are bytes, as ever - a 16-byte piece of the cache is then the 8-byte
// piece of the pool at the same index, widened (16 codes of one block of 16 d: the pieces of an item number alike on both sides).
template <bool K4 = false, bool V4 = false>
__global__ __launch_bounds__(256) void k_kv_pool_gather(const GArgs a) {
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t e16 = a.D / 16, per = 2 * (a.D + e16), nB = a.kvh * a.nblk * per;
  if (i < nB) {
    const int64_t g = i / (a.nblk * per), kb = (i / per) % a.nblk;
    int64_t u = i % per;
    const int64_t sblk = page_block(a.row, a.kvh, g, kb), dblk = g * a.capb + kb;
    int sec = 0;
    if (u >= a.D) u -= a.D, sec = 1;
    if (sec == 1 && u >= e16) u -= e16, sec = 2;
    if (sec == 2 && u >= a.D) u -= a.D, sec = 3;
    const int64_t item = (sec & 1) ? e16 : a.D;  // 16-byte pieces of a block in this section
    if ((K4 && sec == 0) || (V4 && sec == 2)) ((uint4*)a.dst[sec])[dblk * item + u] = widen16(((const uint2*)a.src[sec])[sblk * item + u]);
    else ((uint4*)a.dst[sec])[dblk * item + u] = ((const uint4*)a.src[sec])[sblk * item + u];
    return;
  }
  i -= nB;
  if (i < a.kvh * a.stage16) ((uint4*)a.dst[4])[i] = ((const uint4*)a.src[4])[a.slot * a.kvh * a.stage16 + i];
}

// The section walk of fork and copy: item sblk of `s` to item dblk of `d` in the four code and exponent sections - kc16 / e16 / vc16 /
// e16 16-byte pieces -, bytes as they are, over the 256 threads of a workgroup (at D = 128 with byte codes 272 pieces: more than one
// round).  s and d may be one pool; the caller keeps the two items apart.
template <class S, class T>
__device__ __forceinline__ void copy_item(const KvSrc<S>& s, const KvSrc<T>& d, int64_t sblk, int64_t dblk, int64_t kc16, int64_t vc16,
                                          int64_t e16) {
  const int64_t per = kc16 + vc16 + 2 * e16;
  for (int64_t p = threadIdx.x; p < per; p += 256) {
    int64_t u = p;
    int sec = 0;
    if (u >= kc16) u -= kc16, sec = 1;
    if (sec == 1 && u >= e16) u -= e16, sec = 2;
    if (sec == 2 && u >= vc16) u -= vc16, sec = 3;
    const int64_t item = sec == 0 ? kc16 : sec == 2 ? vc16 : e16;  // 16-byte pieces of a block in this section
    const uint4* from = (const uint4*)(sec == 0 ? s.kc : sec == 1 ? s.ke : sec == 2 ? s.vc : s.ve);
    uint4* to = (uint4*)(sec == 0 ? d.kc : sec == 1 ? d.ke : sec == 2 ? d.vc : d.ve);
    to[dblk * item + u] = from[sblk * item + u];
  }
}

// the staging rows of (slot sslot, kv head g) of `s` to (slot dslot, kv head g) of `d`: stage16 16-byte pieces
template <class S, class T>
__device__ __forceinline__ void copy_stage(const KvSrc<S>& s, const KvSrc<T>& d, int64_t sslot, int64_t dslot, int64_t g, int64_t stage16) {
  const uint4* from = (const uint4*)s.stage + (sslot * s.kvh + g) * stage16;
  uint4* to = (uint4*)d.stage + (dslot * d.kvh + g) * stage16;
  for (int64_t u = threadIdx.x; u < stage16; u += 256) to[u] = from[u];
}

struct FArgs {
  KvSrc<unsigned char> src;  // the pool; src.slots / src.lens: the CHILD's slot and the length forked at, per pair (device)
  const int32_t* from;       // the parent's slot, per pair (device)
  int64_t D, stage16;        // 16-byte pieces of a kv head's staging rows
  int64_t kc16, vc16;        // 16-byte pieces of an item's K / V codes: D with byte codes, D / 2 with nibbles
};

// Fork: pair i makes the sequence in slot src.slots[i] a copy of the first L = src.lens[i] keys of the one in slot from[i], whose full
// pages the child's table row already names - they are shared, not copied.  What is copied, bytes as they are, in 16-byte pieces: the
// parent's staging rows, and with L % 16 != 0 the item of the open block L / 16 - K codes, K exponents, V codes, V exponents - from the
// parent's page to the child's own.  grid (pairs x kv heads, 2): y = 0 the staging rows, y = 1 the item; a workgroup of y = 1 whose pair
// has no open block leaves at once.  Nothing here is read by another workgroup of the launch (a child is named once and is no parent).
__global__ __launch_bounds__(256) void k_kv_pool_fork(const FArgs a) {
  const int64_t kvh = a.src.kvh, i = blockIdx.x / kvh, g = blockIdx.x % kvh;
  const int32_t* drow;
  const int64_t L = seq<attn::SRC_PAGED>(a.src, i, 0, drow), from = a.from[i];
  if (blockIdx.y == 0) {
    copy_stage(a.src, a.src, from, (int64_t)a.src.slots[i], g, a.stage16);
    return;
  }
  if (L % 16 == 0) return;  // (uniform over the workgroup)
  copy_item(a.src, a.src, page_block(slot_row(a.src, from), kvh, g, L / 16), page_block(drow, kvh, g, L / 16), a.kc16, a.vc16, a.D / 16);
}

struct CArgs {
  KvSrc<const unsigned char> src;  // two pools of one dtype, kv_heads, D and code storage - or one pool twice
  KvSrc<unsigned char> dst;
  const int32_t *src_pages, *dst_pages, *src_slots, *dst_slots;  // the pairs (device)
  int64_t n_pages, D, stage16, kc16, vc16;                      // FArgs' piece counts
};

// Copy: a workgroup per (pair, kv head), the page pairs first - pair i < n_pages copies the item (src_pages[i], g) to (dst_pages[i], g)
// in all four code and exponent sections, pair n_pages + j the staging rows of slot src_slots[j] to slot dst_slots[j].  Bytes as they
// are; no table, no length: what a page means is the caller's books'.  Nothing here is read by another workgroup of the launch (a
// destination is named once and is no source).
__global__ __launch_bounds__(256) void k_kv_pool_copy(const CArgs a) {
  const int64_t kvh = a.src.kvh, i = blockIdx.x / kvh, g = blockIdx.x % kvh;
  if (i < a.n_pages) copy_item(a.src, a.dst, (int64_t)a.src_pages[i] * kvh + g, (int64_t)a.dst_pages[i] * kvh + g, a.kc16, a.vc16, a.D / 16);
  else copy_stage(a.src, a.dst, (int64_t)a.src_slots[i - a.n_pages], (int64_t)a.dst_slots[i - a.n_pages], g, a.stage16);
}

struct UArgs {
  KvSrc<const unsigned char> src;
  float *kf, *vf;
  int64_t Z, T, D;
  QP qk, qv;
};

__global__ __launch_bounds__(256) void k_kv_unpack(const UArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.Z * a.T * a.D) return;
  const int64_t z = i / (a.T * a.D), t = (i / a.D) % a.T, d = i % a.D;
  const int64_t blk = block<attn::SRC_PACKED>(a.src, nullptr, z, 0, t / 16), at = (blk * 16 + t % 16) * a.D + d;
  if (a.kf) a.kf[i] = code_value(a.src.kc[at], a.src.ke[blk * a.D + d], a.qk);
  if (a.vf) a.vf[i] = code_value(a.src.vc[at], a.src.ve[(blk * (a.D / 16) + d / 16) * 16 + t % 16], a.qv);
}

// z runs over (sequence of the call, kv head).  From the pool T, Tp and Tv come from the bound max_len and a workgroup takes its
// sequence's own T from lens (device)
struct IArgs {
  KvSrc<const unsigned char> src;
  bf16_t *kimg, *vimg;  // [Z][Tp][Dp], [Z][ATTN_V_ROWS][Tv]
  int64_t D, T, Tp, Dp, Tv;
  QP qk, qv;
  // WIN (the paged pool under the sliding window): W, and the query rows of a sequence - S, or (per-sequence counts) q_starts on the device
  int64_t window, S;
  const int32_t* q_starts;
};

// WIN: the first key sequence b's first query row sees, lo = max(0, T - S_b - W + 1) - no query of the call sees a key below it.  The
// images are written from the 64-key tile that holds lo on (k_attn_q's first tile of the sequence): zeros below 16 (lo / 16) - WITH NO
// TABLE ENTRY AND NO PAGE READ, those pages may have been released and serve another sequence; zeros and not nothing, because 0 x stale
// in the P V product must be 0 and not NaN -, the converted codes from there on.
__device__ __forceinline__ int64_t window_lo(const IArgs& a, int64_t b, int64_t T) {
  const int64_t S = a.q_starts ? (int64_t)(a.q_starts[b + 1] - a.q_starts[b]) : a.S, lo = T - S - a.window + 1;
  return lo > 0 ? lo : 0;
}

// K image: the codes' own layout, no transpose.  A thread: 16 d of one key - 16 code bytes, the 16 exponent bytes of (block of keys, d),
// 32 bytes of the image row; consecutive threads, consecutive pieces of the row.  grid.x covers Tp (Dp / 16) exactly (a multiple of 512).
// SRC_PAGED: the block of 16 keys is found through the sequence's row of the page table - one entry per thread, the two loads one round
// trip behind it - and keys at and beyond lens[b] are zeros up to the end of the 64-key tile k_attn_q reads last; a workgroup (32 or 64
// keys) that starts beyond that tile writes nothing and leaves at once: a short sequence of a ragged batch costs its own keys.
// WIN: a workgroup whose keys all lie below the tile of lo (window_lo) leaves too, and keys below lo's page are zeros, unread.
// N4: the pool's K codes are nibbles - an 8-byte load, widened in front of the same conversion.
template <int SRC, bool WIN = false, bool N4 = false>
__global__ __launch_bounds__(256) void k_kv_kimage(const IArgs a) {
  static_assert(!WIN || SRC == attn::SRC_PAGED, "the window rule runs on the paged pool");
  const int64_t z = blockIdx.y, i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int dq = (int)(a.Dp / 16);
  const int64_t t = i / dq;
  const int d0 = 16 * (int)(i % dq);
  const int64_t g = z % a.src.kvh;
  const int32_t* prow;
  const int64_t T = seq<SRC>(a.src, z / a.src.kvh, a.T, prow);
  if constexpr (SRC == attn::SRC_PAGED)
    if ((int64_t)blockIdx.x * (256 / dq) >= (T + 63) / 64 * 64) return;  // (uniform over the workgroup; the kernel has no barrier)
  int64_t live = 0;  // WIN: the first key read - the start of lo's page
  if constexpr (WIN) {
    const int64_t lo = window_lo(a, z / a.src.kvh, T);
    if ((int64_t)(blockIdx.x + 1) * (256 / dq) <= lo / 64 * 64) return;  // (uniform over the workgroup)
    live = lo / 16 * 16;
  }
  uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (t < T && d0 < a.D && (!WIN || t >= live)) {
    const int64_t blk = block<SRC>(a.src, prow, z, g, t / 16);
    const uint4 c = load_codes16<N4>(a.src.kc, blk, t % 16, a.D, d0 / 16), e = *(const uint4*)(a.src.ke + blk * a.D + d0);
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
// WIN: so does a workgroup whose 64 keys lie below the tile of lo (window_lo); the four keys of a thread lie in one page, below lo's -
// zeros, nothing read - or not.
// N4: the pool's V codes are nibbles (load_v4).
template <int SRC, bool WIN = false, bool N4 = false>
__global__ __launch_bounds__(128) void k_kv_vimage(const IArgs a) {
  static_assert(!WIN || SRC == attn::SRC_PAGED, "the window rule runs on the paged pool");
  __shared__ __attribute__((aligned(16))) unsigned char tile[ATTN_V_ROWS * 128];
  static_assert(ATTN_V_ROWS == 128, "the thread maps below cover 8 blocks of 16 d");
  const int tid = threadIdx.x;
  const int64_t z = blockIdx.y, t0 = (int64_t)blockIdx.x * 64;
  const int64_t g = z % a.src.kvh;
  const int32_t* prow;
  const int64_t T = seq<SRC>(a.src, z / a.src.kvh, a.T, prow);
  if constexpr (SRC == attn::SRC_PAGED)
    if (t0 >= T) return;  // (uniform over the workgroup)
  int64_t live = 0;  // WIN: the first key read - the start of lo's page
  if constexpr (WIN) {
    const int64_t lo = window_lo(a, z / a.src.kvh, T);
    if (t0 + 64 <= lo / 64 * 64) return;  // (uniform over the workgroup, before the barrier)
    live = lo / 16 * 16;
  }
  {
    const int db = tid & 7, tg = tid >> 3;
    const int64_t t = t0 + 4 * tg;
    uint32_t w[4][8];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int j = 0; j < 8; ++j) w[r][j] = 0;
    if (16 * db < a.D && t < T && (!WIN || t >= live)) {  // (t < T <= cap, t a multiple of 4: the dword of exponents lies inside the section)
      uint4 c[4];
      const uint32_t e4 = load_v4<N4>(a.src, block<SRC>(a.src, prow, z, g, t / 16), t, T, (int)a.D, db, c);
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (t + r < T) {
          const uint32_t e = ((e4 >> (8 * r)) & 0xffu) * 0x01010101u;  // one exponent for the 16 d
          const uint32_t eb[4] = {e, e, e, e};
          codes16_to_bf16(c[r], eb, a.qv, w[r]);
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

// the one append: nkb blocks of 16 keys per (sequence, kv head) on the grid (kvc::AArgs); starts: the per-sequence counts' (RAG), else null;
// K4 / V4: the pool's code sections that hold nibbles
template <int SRC, bool RAG = false, bool K4 = false, bool V4 = false>
static int kv_append(const kvc::KvSrc<unsigned char>& src, int dtype, const void* k_new, const void* v_new, const int64_t* ks, const int64_t* vs,
                     int64_t batch, int64_t D, int64_t len, int64_t n, int64_t nkb, const QP& qk, const QP& qv, hipStream_t st, const char* who,
                     const int32_t* starts = nullptr) {
  kvc::AArgs a;
  a.src = src, a.kn = k_new, a.vn = v_new, a.starts = starts;
  a.batch = batch, a.D = D, a.n = n, a.len = len, a.nkb = nkb;
  a.k_bs = ks[0], a.k_hs = ks[1], a.k_rs = ks[2], a.v_bs = vs[0], a.v_hs = vs[1], a.v_rs = vs[2];
  a.qk = qk, a.qv = qv;
  const int esz = dtype == LQER_F32 ? 4 : 2;
  a.kvec = al16(k_new, ks, esz), a.vvec = al16(v_new, vs, esz);
  const int64_t items = batch * src.kvh * (nkb * (D / 4) + n * (D / 16));
  return with_dtype(dtype, [&](auto dt) {
    kvc::k_kv_append<decltype(dt)::value, SRC, RAG, K4, V4><<<dim3((unsigned)((items + 255) / 256)), 256, 0, st>>>(a);
    return check_launch(who);
  });
}

int kv_cache_append_dispatch(void* cache, const void* k_new, const void* v_new, const int64_t* ks, const int64_t* vs, int dtype, int64_t batch,
                             int64_t kv_heads, int64_t capacity, int64_t D, int64_t len, int64_t n, const QP& qk, const QP& qv, hipStream_t st) {
  const auto src = kvc::src_of((unsigned char*)cache, kvc::layout(dtype, batch, kv_heads, capacity, D));
  return kv_append<attn::SRC_PACKED>(src, dtype, k_new, v_new, ks, vs, batch, D, len, n, (len + n - 1) / 16 - len / 16 + 1, qk, qv, st,
                                     "lqer_kv_cache_append");
}

size_t kv_pool_bytes(int dtype, int64_t pages, int64_t slots, int64_t kv_heads, int64_t D, bool k4, bool v4) {
  return kvc::pool_layout(dtype, pages, slots, kv_heads, D, k4, v4).total;
}

// the pool's append, uniform or with per-sequence counts, on the instantiation of the pool's code storage (p.k4, p.v4)
template <bool RAG>
static int kv_pool_append(const KvPool& p, const void* k_new, const void* v_new, const int64_t* ks, const int64_t* vs, int64_t batch, int64_t n,
                          const QP& qk, const QP& qv, hipStream_t st, const char* who) {
  return with_flag(p.k4, [&](auto k4) {
    return with_flag(p.v4, [&](auto v4) {
      return kv_append<attn::SRC_PAGED, RAG, decltype(k4)::value, decltype(v4)::value>(kvc::src_of<unsigned char>(p), p.dtype, k_new, v_new, ks, vs, batch,
                                                                                       p.D, 0, n, (n + 14) / 16 + 1, qk, qv, st, who,
                                                                                       RAG ? p.starts : nullptr);
    });
  });
}

int kv_pool_append_dispatch(const KvPool& p, const void* k_new, const void* v_new, const int64_t* ks, const int64_t* vs, int64_t batch, int64_t n,
                            const QP& qk, const QP& qv, hipStream_t st) {
  return kv_pool_append<false>(p, k_new, v_new, ks, vs, batch, n, qk, qv, st, "lqer_kv_pool_append");
}

// p.starts: [batch + 1] token starts (device); ks2 / vs2: elements over token / kv head of [total][kv_heads][D]; the grid follows max_n
int kv_pool_append_ragged_dispatch(const KvPool& p, const void* k_new, const void* v_new, const int64_t* ks2, const int64_t* vs2, int64_t batch,
                                   int64_t max_n, const QP& qk, const QP& qv, hipStream_t st) {
  const int64_t ks[3] = {0, ks2[1], ks2[0]}, vs[3] = {0, vs2[1], vs2[0]};
  return kv_pool_append<true>(p, k_new, v_new, ks, vs, batch, max_n, qk, qv, st, "lqer_kv_pool_append_ragged");
}

int kv_pool_gather_dispatch(const KvPool& p, int64_t slot, int64_t T, void* cache, int64_t capacity, hipStream_t st) {
  const auto s = kvc::src_of(p);
  const auto d = kvc::src_of((unsigned char*)cache, kvc::layout(p.dtype, 1, p.kv_heads, capacity, p.D));
  kvc::GArgs a = {{s.kc, s.ke, s.vc, s.ve, s.stage}, {d.kc, d.ke, d.vc, d.ve, d.stage}};
  a.row = p.block_table + slot * p.table_stride, a.slot = slot, a.kvh = p.kv_heads, a.D = p.D;
  a.nblk = (T + 15) / 16, a.capb = d.cap16, a.stage16 = p.D * (p.dtype == LQER_F32 ? 4 : 2);  // 16 rows x D x esz / 16
  const int64_t items = p.kv_heads * (a.nblk * 2 * (p.D + p.D / 16) + a.stage16);
  const dim3 grid((unsigned)((items + 255) / 256));  // (the pieces of an item number alike with byte and with nibble codes)
  if (p.k4 && p.v4) kvc::k_kv_pool_gather<true, true><<<grid, 256, 0, st>>>(a);
  else if (p.k4) kvc::k_kv_pool_gather<true, false><<<grid, 256, 0, st>>>(a);
  else if (p.v4) kvc::k_kv_pool_gather<false, true><<<grid, 256, 0, st>>>(a);
  else kvc::k_kv_pool_gather<><<<grid, 256, 0, st>>>(a);
  return check_launch(p.k4 || p.v4 ? "lqer_kv_pool_gather_fmt" : "lqer_kv_pool_gather");
}

// p.seq_slots: the children's slots; the grid comes from n and kv_heads alone
int kv_pool_fork_dispatch(const KvPool& p, const int32_t* src_slots, int64_t n, hipStream_t st) {
  kvc::FArgs a = {kvc::src_of<unsigned char>(p), src_slots, p.D, p.D * (p.dtype == LQER_F32 ? 4 : 2),  // 16 rows x D x esz / 16
                  kvc::code_pitch(p.D, p.k4), kvc::code_pitch(p.D, p.v4)};                             // 16 rows x pitch / 16
  kvc::k_kv_pool_fork<<<dim3((unsigned)(n * p.kv_heads), 2), 256, 0, st>>>(a);
  return check_launch("lqer_kv_pool_fork");
}

// src / dst: pool, dtype, pages, slots, kv_heads, D, k4, v4 (no table, no lengths); the four id arrays are device pointers
int kv_pool_copy_dispatch(const KvPool& src, const KvPool& dst, const int32_t* src_pages, const int32_t* dst_pages, int64_t n_pages,
                          const int32_t* src_slots, const int32_t* dst_slots, int64_t n_slots, hipStream_t st) {
  kvc::CArgs a = {kvc::src_of(src), kvc::src_of<unsigned char>(dst), src_pages, dst_pages, src_slots, dst_slots, n_pages, src.D,
                  src.D * (src.dtype == LQER_F32 ? 4 : 2), kvc::code_pitch(src.D, src.k4), kvc::code_pitch(src.D, src.v4)};
  kvc::k_kv_pool_copy<<<dim3((unsigned)((n_pages + n_slots) * src.kv_heads)), 256, 0, st>>>(a);
  return check_launch("lqer_kv_pool_copy");
}

int kv_cache_unpack_dispatch(const void* cache, int dtype, int64_t batch, int64_t kv_heads, int64_t capacity, int64_t D, int64_t T, const QP& qk,
                             const QP& qv, float* k_f32, float* v_f32, hipStream_t st) {
  kvc::UArgs a;
  a.src = kvc::src_of((const unsigned char*)cache, kvc::layout(dtype, batch, kv_heads, capacity, D));
  a.kf = k_f32, a.vf = v_f32, a.Z = batch * kv_heads, a.T = T, a.D = D, a.qk = qk, a.qv = qv;
  kvc::k_kv_unpack<<<dim3((unsigned)((a.Z * T * D + 255) / 256)), 256, 0, st>>>(a);
  return check_launch("lqer_kv_cache_unpack");
}

// the two images of lqer_attention_q's workspace from the cache's first T keys - or, from the paged pool, from every sequence's first
// lens[b] keys, the images' strides those of T = max_len; the caller (attn_q.hip) checks the launches
void kv_cache_images_dispatch(const AttnCall& c, bf16_t* kimg, int64_t Tp, int64_t Dp, bf16_t* vimg, int64_t Tv) {
  kvc::IArgs a;
  a.src = kvc::src_of(c);
  a.kimg = kimg, a.vimg = vimg, a.D = c.D, a.T = c.T, a.Tp = Tp, a.Dp = Dp, a.Tv = Tv;
  a.qk = make_qp(*c.k_fmt), a.qv = make_qp(*c.v_fmt);
  a.window = c.window, a.S = c.S, a.q_starts = c.paged && c.pool.ragged ? c.pool.starts : nullptr;  // (read by the WIN kernels alone)
  const dim3 kgrid((unsigned)(Tp * (Dp / 16) / 256), (unsigned)(c.batch * c.kv_heads)), vgrid((unsigned)(Tv / 64), (unsigned)(c.batch * c.kv_heads));
  if (c.paged && c.windowed) {  // (each image kernel reads one operand: its own flag of the pool's code storage)
    if (c.pool.k4) kvc::k_kv_kimage<attn::SRC_PAGED, true, true><<<kgrid, 256, 0, c.st>>>(a);
    else kvc::k_kv_kimage<attn::SRC_PAGED, true><<<kgrid, 256, 0, c.st>>>(a);
    if (c.pool.v4) kvc::k_kv_vimage<attn::SRC_PAGED, true, true><<<vgrid, 128, 0, c.st>>>(a);
    else kvc::k_kv_vimage<attn::SRC_PAGED, true><<<vgrid, 128, 0, c.st>>>(a);
  } else if (c.paged) {
    if (c.pool.k4) kvc::k_kv_kimage<attn::SRC_PAGED, false, true><<<kgrid, 256, 0, c.st>>>(a);
    else kvc::k_kv_kimage<attn::SRC_PAGED><<<kgrid, 256, 0, c.st>>>(a);
    if (c.pool.v4) kvc::k_kv_vimage<attn::SRC_PAGED, false, true><<<vgrid, 128, 0, c.st>>>(a);
    else kvc::k_kv_vimage<attn::SRC_PAGED><<<vgrid, 128, 0, c.st>>>(a);
  } else {
    kvc::k_kv_kimage<attn::SRC_PACKED><<<kgrid, 256, 0, c.st>>>(a);
    kvc::k_kv_vimage<attn::SRC_PACKED><<<vgrid, 128, 0, c.st>>>(a);
  }
}

}  // namespace lqer
