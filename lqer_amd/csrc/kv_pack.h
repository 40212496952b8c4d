// The packed KV cache (include/lqer_hip.h "packed KV cache"): what Q_w0(K^T) and Q_w1(V) of the fused attention ARE - a code per
// element and an exponent per block of 16 - so that a decode step converts and scales instead of quantizing the whole K and V again.
// Shared by kv_cache.hip (append, unpack) and attn_decode.hip (the packed operand source): the layout, the quantizer that keeps the
// codes, and the way back to the bf16 bits quant16_bf16 would have written - one spelling of each, so the two sides cannot drift.
//
// A code is SIGN-MAGNITUDE: bit 7 the sign, bits 6..0 the mantissa's magnitude (width <= 8: at most 127).  The quantizer's image
// knows a -0 (a negative value that rounds to zero keeps its sign in the slow path; an fp16 -0 in the fast one): sign-magnitude
// carries it, and the way back is a v_cvt_f32_ubyte, a multiply and an OR of the sign - no sign extension, no special code.
// An exponent byte is e - emin = e + exp_bias (0 .. 2^exp_width - 1); a zero block stores the exponent closest to 0.
//
// NIBBLE codes (the paged pool only, per operand: LQER_Q_MXINT_C4 as k_fmt / v_fmt, width <= 4, so the magnitude is at most 7): two
// codes per byte, a nibble = sign << 3 | magnitude, elements d = 2 j and 2 j + 1 of a key's row the low and the high nibble of byte j.
// A key's row is then D / 2 bytes and the 16 codes of one block of 16 d one aligned 8-byte piece.  The row pitch (code_pitch), the way
// to nibbles (narrow8) and the way back to the byte codes (widen16, in front of codes16_to_bf16) are spelled here once; the kernels
// take the storage as a template parameter N4 and everything else about an item - exponents, staging rows, the item index - is as it was.
#pragma once
#include "qmm_image.h"

namespace lqer {

namespace attn {
constexpr int SRC_RAW = 0, SRC_PACKED = 1, SRC_PAGED = 2;  // where K and V come from (attn_decode.hip; kv_cache.hip's kernels: the last two)
}

namespace kvc {

struct Layout {  // byte offsets of the five sections, each rounded up to 256 bytes
  int64_t cap;   // capacity rounded up to 16 keys
  int64_t kv_heads;
  size_t k_codes, k_exps, v_codes, v_exps, k_stage, total;
};

__host__ inline size_t up256(size_t v) { return (v + 255) / 256 * 256; }

// D a multiple of 16, dtype one of the three: the caller checked
__host__ inline Layout layout(int dtype, int64_t batch, int64_t kv_heads, int64_t capacity, int64_t D) {
  Layout l;
  l.cap = (capacity + 15) / 16 * 16, l.kv_heads = kv_heads;
  const size_t Z = (size_t)(batch * kv_heads), esz = dtype == LQER_F32 ? 4 : 2;
  const size_t codes = up256(Z * l.cap * D), exps = up256(Z * (l.cap / 16) * D);
  l.k_codes = 0;
  l.k_exps = l.k_codes + codes;
  l.v_codes = l.k_exps + exps;
  l.v_exps = l.v_codes + codes;
  l.k_stage = l.v_exps + exps;
  l.total = l.k_stage + up256(Z * 16 * D * esz);
  return l;
}

// The paged pool (include/lqer_hip.h "paged KV pool"): the same five sections, but an ITEM - one (page, kv head), i.e. one block of 16
// keys of one kv head - at index page * kv_heads + g instead of the dense cache's z * (cap / 16) + t / 16; within an item the bytes are
// the dense cache's.  So one spelling of the addresses serves both: block index `blk` -> codes of key t at (blk * 16 + t % 16) * D,
// K exponents at blk * D, V exponents at (blk * (D / 16) + d / 16) * 16 + t % 16.  The staging rows are per sequence SLOT.
struct PoolLayout {
  size_t k_codes, k_exps, v_codes, v_exps, k_stage, total;
};

// bytes of one key's row of codes: a byte per element, or (N4) a nibble
template <bool N4>
__host__ __device__ constexpr int64_t code_pitch(int64_t D) { return N4 ? D / 2 : D; }
__host__ inline int64_t code_pitch(int64_t D, bool n4) { return n4 ? code_pitch<true>(D) : code_pitch<false>(D); }

// D a multiple of 16, dtype one of the three: the caller checked.  k4 / v4: the operand's code section holds nibbles
__host__ inline PoolLayout pool_layout(int dtype, int64_t pages, int64_t slots, int64_t kv_heads, int64_t D, bool k4 = false, bool v4 = false) {
  PoolLayout l;
  const size_t items = (size_t)(pages * kv_heads), esz = dtype == LQER_F32 ? 4 : 2;
  const size_t exps = up256(items * D);
  l.k_codes = 0;
  l.k_exps = l.k_codes + up256(items * 16 * code_pitch(D, k4));
  l.v_codes = l.k_exps + exps;
  l.v_exps = l.v_codes + up256(items * 16 * code_pitch(D, v4));
  l.k_stage = l.v_exps + exps;
  l.total = l.k_stage + up256((size_t)(slots * kv_heads) * 16 * D * esz);
  return l;
}

// Where a kernel finds the codes: the sections of a dense cache or of the pool, and what turns (sequence, kv head, block of 16 keys)
// into a block index.  A host struct and a member of every kernel's argument record; the kernel's template parameter SRC says which
// of the two it describes.
template <class B>  // unsigned char for the writer (append), const unsigned char for the readers
struct KvSrc {
  B *kc, *ke, *vc, *ve;
  int64_t cap16;                      // SRC_PACKED: blocks of 16 keys per (batch, kv head)
  int kvh;                            // kv heads
  const int32_t *tbl, *slots, *lens;  // SRC_PAGED (device): [slots][tstride] pages, [batch] slot and length of the call's b-th sequence
  int64_t tstride;
  B* stage;                           // the staging rows (append and gather only)
};

template <class B>
__host__ inline KvSrc<B> src_of(B* cache, const Layout& l) {
  return {cache + l.k_codes, cache + l.k_exps, cache + l.v_codes, cache + l.v_exps, l.cap / 16, (int)l.kv_heads, nullptr, nullptr, nullptr, 0, cache + l.k_stage};
}
template <class B = const unsigned char>  // (the one place that turns a pool into section pointers)
__host__ inline KvSrc<B> src_of(const KvPool& p) {
  const PoolLayout l = pool_layout(p.dtype, p.pages, p.slots, p.kv_heads, p.D, p.k4, p.v4);
  B* base = (B*)p.pool;
  return {base + l.k_codes, base + l.k_exps, base + l.v_codes, base + l.v_exps, 0, (int)p.kv_heads, p.block_table, p.seq_slots, p.lens, p.table_stride, base + l.k_stage};
}
__host__ inline KvSrc<const unsigned char> src_of(const AttnCall& c) {  // (c.packed)
  return c.paged ? src_of(c.pool) : src_of((const unsigned char*)c.cache, layout(c.dtype, c.batch, c.kv_heads, c.capacity, c.D));
}

// the length of the call's b-th sequence and its row of the page table: lens[b] and the slot's row, or the host's T and no row
template <class B>
__device__ __forceinline__ const int32_t* slot_row(const KvSrc<B>& s, int64_t slot) { return s.tbl + slot * s.tstride; }
template <int SRC, class B>
__device__ __forceinline__ int64_t seq(const KvSrc<B>& s, int64_t b, int64_t T, const int32_t*& row) {
  row = nullptr;
  if constexpr (SRC == attn::SRC_PAGED) {
    row = slot_row(s, (int64_t)s.slots[b]);
    return s.lens[b];
  }
  return T;
}

// the index of the block of keys 16 kb .. 16 kb + 15 of (sequence b, kv head g), z = b kvh + g, in the code and exponent sections:
// the pool's item of (page row[kb], kv head g), or the dense cache's
__device__ __forceinline__ int64_t page_block(const int32_t* row, int64_t kvh, int64_t g, int64_t kb) { return (int64_t)row[kb] * kvh + g; }
template <int SRC, class B>
__device__ __forceinline__ int64_t block(const KvSrc<B>& s, const int32_t* row, int64_t z, int64_t g, int64_t kb) {
  if constexpr (SRC == attn::SRC_PAGED) return page_block(row, s.kvh, g, kb);
  else return z * s.cap16 + kb;
}

// eight nibbles -> their byte codes: (n & 7) | ((n & 8) << 4), nibble i of x in byte i of the pair
__device__ __forceinline__ uint2 widen8(uint32_t x) {
  uint32_t lo = x & 0xffffu, hi = x >> 16;
  lo = (lo | (lo << 8)) & 0x00ff00ffu, hi = (hi | (hi << 8)) & 0x00ff00ffu;
  lo = (lo | (lo << 4)) & 0x0f0f0f0fu, hi = (hi | (hi << 4)) & 0x0f0f0f0fu;
  return make_uint2((lo & 0x07070707u) | ((lo & 0x08080808u) << 4), (hi & 0x07070707u) | ((hi & 0x08080808u) << 4));
}
// the 8-byte piece of 16 nibbles -> the uint4 of 16 byte codes codes16_to_bf16 takes
__device__ __forceinline__ uint4 widen16(const uint2& n) {
  const uint2 a = widen8(n.x), b = widen8(n.y);
  return make_uint4(a.x, a.y, b.x, b.y);
}
// eight byte codes of magnitude <= 7 (lo: elements 0 - 3, hi: 4 - 7) -> eight nibbles, element i in nibble i: widen8's inverse
__device__ __forceinline__ uint32_t narrow8(uint32_t lo, uint32_t hi) {
  lo = (lo & 0x07070707u) | ((lo >> 4) & 0x08080808u), hi = (hi & 0x07070707u) | ((hi >> 4) & 0x08080808u);
  lo = (lo | (lo >> 4)) & 0x00ff00ffu, hi = (hi | (hi >> 4)) & 0x00ff00ffu;
  lo = (lo | (lo >> 8)) & 0xffffu, hi = (hi | (hi >> 8)) & 0xffffu;
  return lo | (hi << 16);
}

// the 16 codes of (row r of block blk, block dg of 16 d) of a code section as byte codes: one 16-byte load, or (N4) one 8-byte load, widened
template <bool N4, class B>
__device__ __forceinline__ uint4 load_codes16(const B* codes, int64_t blk, int64_t r, int64_t D, int dg) {
  if constexpr (N4) return widen16(*(const uint2*)(codes + (blk * 16 + r) * code_pitch<true>(D) + 8 * dg));
  else return *(const uint4*)(codes + (blk * 16 + r) * D + 16 * dg);
}

// 16 d (block db of D / 16) of the V rows of keys t .. t + 3 of block blk, t a multiple of 4: the dword of their four exponents
// (returned) and the four 16-byte code rows; a key at or beyond T is not read and leaves c[r] as it was
template <bool N4 = false, class B>
__device__ __forceinline__ uint32_t load_v4(const KvSrc<B>& s, int64_t blk, int64_t t, int64_t T, int D, int db, uint4 (&c)[4]) {
  const uint32_t e4 = *(const uint32_t*)(s.ve + (blk * (D / 16) + db) * 16 + t % 16);
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if (t + r < T) c[r] = load_codes16<N4>(s.vc, blk, t % 16 + r, D, db);
  return e4;
}

// one block of 16 -> 16 codes (four dwords, element i in byte i) and the exponent byte: quant16_bf16's decisions and arithmetic,
// stopped before the final scaling (the fast path: mxint16_bf16_fast's r; the other: mxint_mantissa)
template <bool FLUSH_TINY>
__device__ __forceinline__ uint32_t quant16_codes(const float (&v)[16], const QP& q, uint32_t (&cw)[4]) {
  typedef __attribute__((ext_vector_type(2))) float f2;
  float amax = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) amax = fmaxf(amax, fabsf(v[i]));
#pragma unroll
  for (int i = 0; i < 4; ++i) cw[i] = 0;
  int e = 0 < q.emin ? q.emin : (0 > q.emax ? q.emax : 0);
  if (amax > 0.f) {
    e = block_exponent(amax, q);
    float r[16];
    if (mxint16_fast_ok(e, q)) {
      const float s = __uint_as_float((uint32_t)(127 + q.mbits - e) << 23);
      const float es = 1e-9f * s, lo = -q.mneg, hi = q.mmax;
      const f2 magic = {12582912.0f, 12582912.0f};
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const f2 x = {v[2 * i], v[2 * i + 1]};
        const f2 c = {copysignf(es, x[0]), copysignf(es, x[1])};
        f2 t = (__builtin_elementwise_fma(x, (f2){s, s}, c) + magic) - magic;
        t[0] = __builtin_amdgcn_fmed3f(t[0], lo, hi);
        t[1] = __builtin_amdgcn_fmed3f(t[1], lo, hi);
        if constexpr (FLUSH_TINY) {
          t[0] = fabsf(x[0]) <= 1e-8f ? 0.f : t[0];
          t[1] = fabsf(x[1]) <= 1e-8f ? 0.f : t[1];
        }
        r[2 * i] = t[0], r[2 * i + 1] = t[1];
      }
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i) r[i] = mxint_mantissa(v[i], e, q);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const uint32_t code = ((__float_as_uint(r[i]) >> 24) & 0x80u) | (uint32_t)fabsf(r[i]);
      cw[i >> 2] |= code << (8 * (i & 3));
    }
  }
  return (uint32_t)(e - q.emin);
}

// value of one code under the exponent byte eb (the unpack hook: the quantizer's output, exact)
__device__ __forceinline__ float code_value(uint32_t code, uint32_t eb, const QP& q) {
  const float m = ldexpf((float)(code & 0x7fu), (int)eb + q.emin - q.mbits);
  return (code & 0x80u) ? -m : m;
}

// 16 codes -> the 16 bf16 values quant16_bf16 writes for them (w[i]: elements 2 i, 2 i + 1), element i under the exponent byte
// (eb[i >> 2] >> 8 (i & 3)) & 0xff.  k = e - mbits within [-126, 126] for all 16 (mxint16_fast_ok): magnitude x 2^k, the power of two
// built from exponent bits; otherwise ldexpf, as the quantizer's slow path (the same values wherever both apply: every product is exact).
__device__ __forceinline__ void codes16_to_bf16(const uint4& c, const uint32_t (&eb)[4], const QP& q, uint32_t (&w)[8]) {
  typedef __attribute__((ext_vector_type(2))) float f2;
  const uint32_t cw[4] = {c.x, c.y, c.z, c.w};
  const int kb = q.emin - q.mbits;
  int k[16];
  bool fast = true;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    k[i] = (int)((eb[i >> 2] >> (8 * (i & 3))) & 0xffu) + kb;
    fast = fast && k[i] >= -126 && k[i] <= 126;
  }
  if (fast) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t m = cw[j] & 0x7f7f7f7fu, s = cw[j] & 0x80808080u;
      const f2 a = (f2){(float)(m & 0xffu), (float)((m >> 8) & 0xffu)} *
                   (f2){__uint_as_float((uint32_t)(127 + k[4 * j]) << 23), __uint_as_float((uint32_t)(127 + k[4 * j + 1]) << 23)};
      const f2 b = (f2){(float)((m >> 16) & 0xffu), (float)(m >> 24)} *
                   (f2){__uint_as_float((uint32_t)(127 + k[4 * j + 2]) << 23), __uint_as_float((uint32_t)(127 + k[4 * j + 3]) << 23)};
      // the two high halves, then the sign bytes into bits 15 and 31
      w[2 * j] = __builtin_amdgcn_perm(__float_as_uint(a[1]), __float_as_uint(a[0]), 0x07060302u) | __builtin_amdgcn_perm(s, s, 0x010c000cu);
      w[2 * j + 1] = __builtin_amdgcn_perm(__float_as_uint(b[1]), __float_as_uint(b[0]), 0x07060302u) | __builtin_amdgcn_perm(s, s, 0x030c020cu);
    }
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const uint32_t c0 = (cw[i >> 1] >> (16 * (i & 1))) & 0xffu, c1 = (cw[i >> 1] >> (16 * (i & 1) + 8)) & 0xffu;
      const uint32_t lo = exact_bf16_bits(ldexpf((float)(c0 & 0x7fu), k[2 * i])) | ((c0 & 0x80u) << 8);
      const uint32_t hi = exact_bf16_bits(ldexpf((float)(c1 & 0x7fu), k[2 * i + 1])) | ((c1 & 0x80u) << 8);
      w[i] = lo | (hi << 16);
    }
  }
}

}  // namespace kvc

namespace attn {

// four consecutive elements; one 8- / 16-byte load when the row is aligned
template <int DT>
__device__ __forceinline__ void load4(const void* base, int64_t off, bool vec, float (&v)[4]) {
  if (vec) {
    if constexpr (DT == LQER_F32) {
      const float4 t = *(const float4*)((const float*)base + off);
      v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
    } else {
      const uint2 t = *(const uint2*)((const bf16_t*)base + off);
      const uint32_t wd[2] = {t.x, t.y};
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        float lo, hi;  // (into locals first: bound to the array elements directly, four k_kv_append kernels come out reordered)
        pair_to_f32<DT>(wd[j], lo, hi);
        v[2 * j] = lo, v[2 * j + 1] = hi;
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = load_elem<DT>(base, off + j);
  }
}

}  // namespace attn

}  // namespace lqer
