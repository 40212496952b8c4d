// Rotary position embedding inside the paged pool's append (lqer_kv_pool_append_rope; include/lqer_hip.h "paged KV pool"): ONE launch
// takes the raw q, k, v of a layer's projections, rotates q and k and appends k and v - per-sequence counts from the device, as
// k_kv_append's RAG instantiation (kv_cache.hip), whose pool bytes it leaves when that kernel is handed the rotated keys.
//
// THE RULE (HF's rotate_half form; the one spelling - the header refers here).  Per head row x[0 .. D), h = D / 2, position p, i < h:
//   out[i]     = rn( rn(x[i]     * cos[p][i]) + rn(-x[i + h] * sin[p][i]) )
//   out[i + h] = rn( rn(x[i + h] * cos[p][i]) + rn( x[i]     * sin[p][i]) )
// rn rounds to the tensors' dtype after each of the three operations: what eager torch computes on dtype tensors.  fp16 / bf16: the fp32
// product of two dtype values is exact, so one conversion gives the correctly rounded product, and the fp32 sum of two dtype values
// followed by one conversion is correctly rounded too (24 >= 2 p + 2 for p = 11 and p = 8).  fp32: the multiply and the add stay two
// instructions - rotate4 is compiled with contraction off, an FMA would skip the product's rounding.  cos / sin are TABLES the caller
// hands over, [rope_rows][h] of the dtype, dense: the first half of what the model's rotary module returns, every scaling rule in them;
// no trigonometry here.  p of new token j of sequence b: lens[b] + j (the length before the call), or positions[starts[b] + j].
//
// One launch, three ranges of workgroups (k_kv_append has two ranges of threads):
//   K  a WAVE per (sequence, kv head, block of 16 keys the new keys touch), four per workgroup, each with an LDS tile [16][D + 16] of
//      dtype bits of its own - no barrier across waves, a wave whose item does not exist leaves before any load.  Phase 1, lane
//      (r = lane / 4, c = lane % 4): row r of the tile in runs of 4 elements c, c + 4, .. of the lower half and the matching runs of
//      the upper - key t = 16 kb + r below len: the slot's staging row r as it is (rotated when it was appended); t in [len, end): k_new's
//      row and the position's cos / sin runs (8- / 16-byte loads; k_new's when al16 allows), rotated; t >= end: zeros.  Phase 2, lane l <
//      D / 4: 4 d of the 16 keys from the tile -> store_kblock4 (kv_pack.h), k_kv_append's store stage.  The rows are padded by 16
//      elements: the 16 rows of phase 1's stores do not start on one bank.
//   V  a thread per 16 d of one new row: store_vrow16, as k_kv_append.  No rotation.
//   Q  a thread per (token, head, run of 4 of the lower half): both halves of its d pairs loaded, then both stored - q_out == q is
//      allowed.  The token's sequence is found in new_starts by bisection; a token outside every sequence is not touched.
//
// THE STAGING ROWS receive the ROTATED keys of the block left open (the next append quantizes that block along t from them), and
// k_kv_append's no-race rule holds lane by lane: the elements (slot, kv head, row r, runs c, c + 4, ..) of the staging rows are read
// and written by ONE thread of the launch - lane (r, c) of the j = 0 item of (sequence, kv head); a slot is named once per call -,
// reads first in program order.  It reads them in phase 1 where 16 kb + r < len.  It writes them (a) in phase 1, from the registers
// the tile gets, where the open block is the item's own (end / 16 == len / 16) and its key is new, or (b) where the open block is a
// later one, after phase 1: it rotates key 16 (end / 16) + r < end - at most 15 keys per (sequence, kv head) - itself.  The bits are
// those the later block's wave puts into its tile, because the rule is deterministic; that is cheaper than ordering two items.
#include "kv_pack.h"
#include "attn_math.h"

namespace lqer {

namespace kvc {

struct RArgs {
  KvSrc<unsigned char> src;
  const void *q, *kn, *vn, *cs, *sn;  // cs / sn: [rope_rows][D / 2]
  void* qo;
  const int32_t *starts, *pos;  // [batch + 1]; [total] or null (device)
  int64_t batch, D, n, nkb, heads, total;  // n, nkb: of the bound max_n, as AArgs'
  int64_t q_ts, q_hs, o_ts, o_hs, k_ts, k_hs, v_ts, v_hs;  // elements over token / head
  QP qk, qv;
  bool qvec, ovec, kvec, vvec;
  unsigned kblocks, vblocks;  // workgroups of the K and of the V range; the Q range follows
};

constexpr int ROPE_PAD = 16;  // elements behind a tile row

// a run of 4 consecutive elements as the bits they are stored in
template <int DT>
using run_t = std::conditional_t<DT == LQER_F32, uint4, uint2>;

template <int DT>
__device__ __forceinline__ run_t<DT> load_run(const void* base, int64_t off, bool vec) {
  if constexpr (DT == LQER_F32) {
    const uint32_t* s = (const uint32_t*)base + off;
    return vec ? *(const uint4*)s : make_uint4(s[0], s[1], s[2], s[3]);
  } else {
    const unsigned short* s = (const unsigned short*)base + off;
    return vec ? *(const uint2*)s : make_uint2((uint32_t)s[0] | ((uint32_t)s[1] << 16), (uint32_t)s[2] | ((uint32_t)s[3] << 16));
  }
}
template <int DT>
__device__ __forceinline__ void store_run(void* base, int64_t off, bool vec, const run_t<DT>& v) {
  if constexpr (DT == LQER_F32) {
    uint32_t* d = (uint32_t*)base + off;
    if (vec) *(uint4*)d = v;
    else d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
  } else {
    unsigned short* d = (unsigned short*)base + off;
    if (vec) *(uint2*)d = v;
    else d[0] = (unsigned short)v.x, d[1] = (unsigned short)(v.x >> 16), d[2] = (unsigned short)v.y, d[3] = (unsigned short)(v.y >> 16);
  }
}
template <int DT>
__device__ __forceinline__ void run_to_f32(const run_t<DT>& b, float (&v)[4]) {
  if constexpr (DT == LQER_F32) {
    v[0] = __uint_as_float(b.x), v[1] = __uint_as_float(b.y), v[2] = __uint_as_float(b.z), v[3] = __uint_as_float(b.w);
  } else {
    float lo, hi;
    pair_to_f32<DT>(b.x, lo, hi);
    v[0] = lo, v[1] = hi;
    pair_to_f32<DT>(b.y, lo, hi);
    v[2] = lo, v[3] = hi;
  }
}
// (v: values of DT already - attn::rnd's -, so the conversion is exact)
template <int DT>
__device__ __forceinline__ run_t<DT> f32_to_run(const float (&v)[4]) {
  if constexpr (DT == LQER_F32) {
    return make_uint4(__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3]));
  } else {
    uint32_t e[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if constexpr (DT == LQER_F16) e[i] = __builtin_bit_cast(unsigned short, (_Float16)v[i]);
      else e[i] = __float_as_uint(v[i]) >> 16;
    }
    return make_uint2(e[0] | (e[1] << 16), e[2] | (e[3] << 16));
  }
}

// the rule on four d pairs; every operation an instruction of its own (no contraction: fp32's product is rounded before the sum)
template <int DT>
__device__ __forceinline__ void rotate4(const float (&xl)[4], const float (&xh)[4], const float (&c)[4], const float (&s)[4], float (&ol)[4],
                                        float (&oh)[4]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float lc = attn::rnd<DT>(xl[i] * c[i]), hs = attn::rnd<DT>(-xh[i] * s[i]);
    const float hc = attn::rnd<DT>(xh[i] * c[i]), ls = attn::rnd<DT>(xl[i] * s[i]);
    ol[i] = attn::rnd<DT>(lc + hs), oh[i] = attn::rnd<DT>(hc + ls);
  }
}

// elements i0 .. i0 + 3 and h + i0 .. of the head row at x + off, rotated to position p: the bits of the two runs
template <int DT>
__device__ __forceinline__ void rope_runs(const RArgs& a, const void* x, int64_t off, bool vec, int64_t p, int i0, int h, run_t<DT>& lo,
                                          run_t<DT>& hi) {
  float xl[4], xh[4], c[4], s[4], ol[4], oh[4];
  run_to_f32<DT>(load_run<DT>(x, off + i0, vec), xl);
  run_to_f32<DT>(load_run<DT>(x, off + h + i0, vec), xh);
  run_to_f32<DT>(load_run<DT>(a.cs, p * h + i0, true), c);  // (16-byte aligned tables, h a multiple of 8, i0 of 4)
  run_to_f32<DT>(load_run<DT>(a.sn, p * h + i0, true), s);
  rotate4<DT>(xl, xh, c, s, ol, oh);
  lo = f32_to_run<DT>(ol), hi = f32_to_run<DT>(oh);
}

template <int DT, bool K4, bool V4>
__global__ __launch_bounds__(256) void k_kv_rope(const RArgs a) {
  constexpr int ESZ = DT == LQER_F32 ? 4 : 2;
  __shared__ __attribute__((aligned(16))) unsigned char tiles[4][16 * (128 + ROPE_PAD) * ESZ];
  const int D = (int)a.D, h = D / 2, hq = D / 8, db_n = D / 16;
  const int64_t kvh = a.src.kvh, Z = a.batch * kvh;
  const int32_t* row;
  if (blockIdx.x < a.kblocks) {  // ---- a wave: one block of 16 keys
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + wave;
    if (w >= Z * a.nkb) return;
    const int64_t z = w / a.nkb, j = w % a.nkb, b = z / kvh, g = z % kvh;
    const int64_t tok0 = a.starts[b], n = a.starts[b + 1] - tok0;
    if (n < 1) return;
    const int64_t len = seq<attn::SRC_PAGED>(a.src, b, 0, row), end = len + n, kb = len / 16 + j;
    if (kb > (end - 1) / 16) return;  // this sequence's new keys touch fewer blocks
    const int64_t zs = (int64_t)a.src.slots[b] * kvh + g, kn0 = tok0 * a.k_ts + g * a.k_hs, open0 = end / 16 * 16;
    unsigned char* tile = tiles[wave];
    const int pitch = D + ROPE_PAD, r = lane >> 2;
    const int64_t srow = (zs * 16 + r) * a.D;  // staging row r of (slot, kv head)
    {
      const int64_t t = 16 * kb + r;
      const bool fresh = t >= len && t < end;
      const int64_t p = !fresh ? 0 : a.pos ? (int64_t)a.pos[tok0 + (t - len)] : t;
      for (int i0 = 4 * (lane & 3); i0 < h; i0 += 16) {
        run_t<DT> lo = {}, hi = {};
        if (t < len) {  // (only j == 0 meets keys below len)
          lo = load_run<DT>(a.src.stage, srow + i0, true), hi = load_run<DT>(a.src.stage, srow + h + i0, true);
        } else if (fresh) {
          rope_runs<DT>(a, a.kn, kn0 + (t - len) * a.k_ts, a.kvec, p, i0, h, lo, hi);
          if (j == 0 && t >= open0) {  // (a): this block stays open
            store_run<DT>(a.src.stage, srow + i0, true, lo), store_run<DT>(a.src.stage, srow + h + i0, true, hi);
          }
        }
        *(run_t<DT>*)(tile + (r * pitch + i0) * ESZ) = lo;
        *(run_t<DT>*)(tile + (r * pitch + h + i0) * ESZ) = hi;
      }
    }
    if (j == 0 && open0 > len && open0 + r < end) {  // (b): a later block stays open - its key of row r
      const int64_t t = open0 + r, p = a.pos ? (int64_t)a.pos[tok0 + (t - len)] : t;
      for (int i0 = 4 * (lane & 3); i0 < h; i0 += 16) {
        run_t<DT> lo, hi;
        rope_runs<DT>(a, a.kn, kn0 + (t - len) * a.k_ts, a.kvec, p, i0, h, lo, hi);
        store_run<DT>(a.src.stage, srow + i0, true, lo), store_run<DT>(a.src.stage, srow + h + i0, true, hi);
      }
    }
    // the wave's own tile, written and read by its lanes alone: LDS serves a wave's requests in order, the fences keep the compiler's
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (lane < D / 4) {
      const int d0 = 4 * lane;
      float x[4][16];
#pragma unroll
      for (int rr = 0; rr < 16; ++rr) {
        float v4[4];
        run_to_f32<DT>(*(const run_t<DT>*)(tile + (rr * pitch + d0) * ESZ), v4);
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) x[jj][rr] = v4[jj];
      }
      const int64_t blk = page_block(row, kvh, g, kb);
      store_kblock4<DT, K4>(x, a.qk, a.src.kc + blk * 16 * code_pitch<K4>(a.D) + (K4 ? d0 / 2 : d0), a.D, a.src.ke + blk * a.D + d0);
    }
    return;
  }
  if (blockIdx.x < a.kblocks + a.vblocks) {  // ---- a thread: 16 d of one new key
    const int64_t i = (int64_t)(blockIdx.x - a.kblocks) * 256 + threadIdx.x;
    if (i >= Z * a.n * db_n) return;
    const int64_t z = i / (a.n * db_n), rem = i % (a.n * db_n);
    const int64_t j = rem / db_n, b = z / kvh, g = z % kvh, tok0 = a.starts[b];
    if (j >= a.starts[b + 1] - tok0) return;  // a key beyond this sequence's count
    const int64_t t = seq<attn::SRC_PAGED>(a.src, b, 0, row) + j;
    const int db = (int)(rem % db_n);
    const int64_t blk = page_block(row, kvh, g, t / 16);
    store_vrow16<DT, V4>(a.vn, g * a.v_hs + (tok0 + j) * a.v_ts + 16 * db, a.vvec, a.qv,
                         a.src.vc + (blk * 16 + t % 16) * code_pitch<V4>(a.D) + (V4 ? 8 : 16) * db, a.src.ve + (blk * db_n + db) * 16 + t % 16);
    return;
  }
  // ---- a thread: a run of 4 d pairs of one query head row
  const int64_t i = (int64_t)(blockIdx.x - a.kblocks - a.vblocks) * 256 + threadIdx.x;
  if (i >= a.total * a.heads * hq) return;
  const int64_t tok = i / (a.heads * hq), rem = i % (a.heads * hq), head = rem / hq;
  const int i0 = 4 * (int)(rem % hq);
  int64_t lo_b = 0, hi_b = a.batch + 1;  // the first entry of starts beyond tok: the token's sequence is the one in front of it
  while (lo_b < hi_b) {
    const int64_t mid = (lo_b + hi_b) / 2;
    if (a.starts[mid] > tok) hi_b = mid;
    else lo_b = mid + 1;
  }
  if (lo_b == 0 || lo_b > a.batch) return;  // a token of no sequence
  const int64_t b = lo_b - 1, p = a.pos ? (int64_t)a.pos[tok] : (int64_t)a.src.lens[b] + (tok - a.starts[b]);
  run_t<DT> lo, hi;
  rope_runs<DT>(a, a.q, tok * a.q_ts + head * a.q_hs, a.qvec, p, i0, h, lo, hi);
  store_run<DT>(a.qo, tok * a.o_ts + head * a.o_hs + i0, a.ovec, lo), store_run<DT>(a.qo, tok * a.o_ts + head * a.o_hs + h + i0, a.ovec, hi);
}

}  // namespace kvc

// p.starts: [batch + 1] token starts (device); the stride pairs: elements over token / head; the K and V grid follows max_n as
// kv_pool_append_ragged_dispatch's, the Q grid follows p.total
int kv_pool_append_rope_dispatch(const KvPool& p, const KvRope& r, const void* k_new, const void* v_new, const int64_t* ks2, const int64_t* vs2,
                                 int64_t batch, int64_t max_n, const QP& qk, const QP& qv, hipStream_t st) {
  kvc::RArgs a;
  a.src = kvc::src_of<unsigned char>(p);
  a.q = r.q, a.qo = r.q_out, a.kn = k_new, a.vn = v_new, a.cs = r.cos, a.sn = r.sin, a.starts = p.starts, a.pos = r.positions;
  a.batch = batch, a.D = p.D, a.n = max_n, a.nkb = (max_n + 14) / 16 + 1, a.heads = r.heads, a.total = p.total;
  a.k_ts = ks2[0], a.k_hs = ks2[1], a.v_ts = vs2[0], a.v_hs = vs2[1];
  a.q_ts = a.q_hs = a.o_ts = a.o_hs = 0;
  a.qk = qk, a.qv = qv;
  const int esz = p.dtype == LQER_F32 ? 4 : 2;
  const auto vec = [&](const void* ptr, const int64_t* s2) {
    const int64_t s3[3] = {0, s2[1], s2[0]};
    return al16(ptr, s3, esz);
  };
  a.kvec = vec(k_new, ks2), a.vvec = vec(v_new, vs2), a.qvec = a.ovec = false;
  if (r.heads > 0) {
    a.q_ts = r.qs[0], a.q_hs = r.qs[1], a.o_ts = r.os[0], a.o_hs = r.os[1];
    a.qvec = vec(r.q, r.qs), a.ovec = vec(r.q_out, r.os);
  }
  const int64_t Z = batch * p.kv_heads;
  a.kblocks = (unsigned)((Z * a.nkb + 3) / 4), a.vblocks = (unsigned)((Z * max_n * (p.D / 16) + 255) / 256);
  const unsigned qblocks = (unsigned)((p.total * r.heads * (p.D / 8) + 255) / 256);
  return with_dtype(p.dtype, [&](auto dt) {
    return with_flags([&](auto k4, auto v4) {
      kvc::k_kv_rope<decltype(dt)::value, decltype(k4)::value, decltype(v4)::value><<<dim3(a.kblocks + a.vblocks + qblocks), 256, 0, st>>>(a);
      return check_launch("lqer_kv_pool_append_rope");
    }, p.k4, p.v4);
  });
}

}  // namespace lqer
