// Records what lqer_linear_gemm_ld LAUNCHES, without a GPU: this program defines the few HIP entry points the GEMM's host code calls
// (a program's own symbols come first when the library it loads is bound), so every kernel launch lands in hipLaunchKernel below and
// is printed - kernel symbol, grid, workgroup, dynamic LDS bytes, and the two sizing arguments of the B_out pre-pass.  The device
// pointers handed in are never dereferenced by host code.  tests/test_launches_cpu.py builds it and holds its output to a record.
//   launch_probe LIBRARY CUS < cases      CUS: what the device query answers; one case per line: K N rank tuning  5 x (kind width block
//                                         exp_width exp_bias)  M dtype b_limbs
//   launch_probe LIBRARY CUS act < cases  the ACTIVATION side (tests/test_act_launches_cpu.py): the descriptor as above, then
//                                         M dtype a_limbs  pointers (0: x aligned, ldx = K; 1: x off by 2 bytes, ldx = K + 1; 2: xq == x)
//                                         scratch (0: ample, 1: exactly lqer_lowrank_xa_scratch_bytes, 2: none).  Per case four calls, " |"
//                                         between them: lqer_quantize_act_xa with xaq, without (the decode-partials form),
//                                         lqer_quantize_act_xa_prep (and its *ready_bytes), lqer_lowrank_xa on the image.  Here the
//                                         sizing arguments of the side kernels that a grid does not pin are printed as well, and the
//                                         two stream calls of this side (hipMemcpy2DAsync, hipMemsetAsync) as pseudo-launches.
//   launch_probe LIBRARY CUS attn < cases the ATTENTION side (tests/test_attn_launches_cpu.py), one call per line, the entry point's name
//                                         (without lqer_) first:
//                                           matmul_q dtype batch S1 K S2 x_block y_block y_layout (0: j contiguous, 1: k contiguous)
//                                                    x_off y_off (pointer off by so many elements) ws (0: what the size function says,
//                                                    1: one byte less)
//                                           attention_q... dtype batch heads kv_heads S T D mask (0: none, 1: tensor with rows of a
//                                                    multiple of four elements, 2: rows of one more, 3: the causal rule) q_off ws nulls
//                                                    (1: no q_strides) block k_kind v_kind window total n_groups
//                                         with S the bound max_s of the entries with per-sequence counts and T the bound max_len of the
//                                         paged ones (window, total, n_groups: read by the entries that have them).  Caches, pools and
//                                         workspaces are sized by the library's own functions; printed behind the launches: ws= the value
//                                         of the entry's *_workspace_bytes function, the return code, the refusal's text.
//   launch_probe LIBRARY CUS fwd < cases  the composed FORWARD (tests/test_fwd_launches_cpu.py), one case per line:
//                                           f K N rank has_bias tuning  5 x format  M dtype a_limbs b_limbs  pointers (0: x aligned,
//                                             ldx = K; 1: x off by 2 bytes, ldx = K + 1; 2: as 0, and the split calls get xq == x)
//                                             ws (0: exactly what the size function says, 1: one byte less, 2: null)
//                                           g n_members M dtype a_limbs  x (0: aligned, 1: off by 2 bytes)  ws (0: exactly
//                                             lqer_group_workspace_bytes, 1: one byte less, 2: off by 8 bytes)  then per member
//                                             K N rank has_bias tuning  5 x format  b_limbs  flaw (0: none, 1: null w_packed, 2: has_bias
//                                             without bias_q, 3: rank = -1)
//                                         An `f` case prints lqer_linear_sizes' five values and then makes four calls, " |" between them:
//                                         lqer_linear_forward; lqer_linear_forward_narrow (behind nws= its workspace size and route= what
//                                         lqer_weight_narrow_route says; ws sizes the workspace of both); lqer_linear_gemm_narrow (ws
//                                         sizes widen_scratch); lqer_linear_gemm_prepared (ready_bytes ample for ws = 0, else 0).  A `g`
//                                         case prints gws= lqer_group_workspace_bytes and calls lqer_linear_forward_group.  Every operand
//                                         has a base of its own, 256 MiB apart, and every pointer a kernel or a stream call receives is
//                                         printed as name+offset - that is the carving; the sizing arguments of mode `act` are printed
//                                         too, the per-call tags (nonce, xch_nonce) are not.
#include <dlfcn.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../include/lqer_hip.h"

struct dim3 {
  uint32_t x, y, z;
};
static int g_cus = 256;
static bool g_act = false, g_fwd = false;
struct XaPlan {  // csrc/xa_common.h
  int row_groups, nchunk, kc;
};
// Mirrors of what the kernels of a forward are handed by value, as far as mode fwd prints them.  The library pins the same offsets with
// static_asserts beside its structs (csrc/common.h, csrc/decode1.hip): a layout that moves fails there first, then here.
struct QP {  // csrc/common.h
  int kind, mbits, block, emin, emax;
  float mmax, mneg, eps, tiny;
  int width;
};
struct QuantOut {  // csrc/common.h
  float* deq;
  int8_t *codes, *exps;
  void* xq;
  int64_t cols_p, nblk;
  int8_t* xq8;
  int64_t cols_p8;
  float* xscale;
};
struct GemmArgs {  // csrc/common.h, up to the last pointer
  const void *xq, *wp, *xaq;
  int xaq_ld;
  const void *bt, *bias;
  void* y;
  int64_t ldy;
  int M, N, Np, Kp, rp, b_limbs, x_f16;
  const float* xa_part;
  int xa_nchunk;
  int64_t xa_cstride;
  QP aout;
  int w_mbits;
  QP bout;
  int tiles_m, tiles_n, w_narrow;
  float* bout_amax;
  int bout_L, bout_nblk, bout_nseg, amax_zeroed;
  const void* w8;
  const float* xscale;
};
static_assert(sizeof(QP) == 40 && offsetof(QuantOut, xq) == 24 && offsetof(QuantOut, xq8) == 48 && offsetof(QuantOut, xscale) == 64, "csrc/common.h");
static_assert(offsetof(GemmArgs, xaq_ld) == 24 && offsetof(GemmArgs, bt) == 32 && offsetof(GemmArgs, ldy) == 56 && offsetof(GemmArgs, M) == 64 &&
                  offsetof(GemmArgs, xa_part) == 96 && offsetof(GemmArgs, bout_amax) == 216 && offsetof(GemmArgs, w8) == 240 &&
                  offsetof(GemmArgs, xscale) == 248, "csrc/common.h");
struct D1Member {  // csrc/decode1.hip, d1::Member
  const void *wp, *bt, *bias;
  void* y;
  int64_t ldy;
  int N, Np, rp, b_limbs, r_off, cb0, nblk;
};
template <int NM>
struct D1Args {  // d1::Args
  D1Member mem[NM];
  int M, Kp;
  QP aout, bout;
  int nmem, rp_all;
  const void* x;
  int64_t ldx;
  int K;
  QP qx;
  int w_exps;
  const void *a_t, *gran;
  uint32_t nonce;
  int np, spin, cpw;
};
static_assert(sizeof(D1Member) == 72 && offsetof(D1Args<1>, M) == 72 && offsetof(D1Args<1>, x) == 168 && offsetof(D1Args<1>, w_exps) == 228 &&
                  offsetof(D1Args<1>, gran) == 240 && offsetof(D1Args<1>, cpw) == 260 && offsetof(D1Args<4>, x) == 384, "csrc/decode1.hip");

// mode fwd: operand i lives at BASE + (i << 28); a pointer prints as the operand's name + its offset
static const uintptr_t BASE = 0x40000000;
enum { P_X, P_W, P_AT, P_BT, P_BIAS, P_Y, P_WIDEN, P_XQ, P_XAQ, P_WS, P_WS2, P_WS3, P_MEM };  // (from P_MEM: four per group member)
static char* at(int i) { return (char*)(BASE + ((uintptr_t)i << 28)); }
static void ptr(const char* tag, const void* p) {
  static const char* const names[] = {"x", "w", "a_t", "b_t", "bias", "y", "widen", "xq", "xaq", "ws", "ws^1", "ws^2"};
  static const char* const mnames[] = {"w", "b_t", "bias", "y"};
  const uintptr_t v = (uintptr_t)p;
  const size_t i = (v - BASE) >> 28, off = (v - BASE) & (((size_t)1 << 28) - 1);
  if (!p) printf(" %s=null", tag);
  else if (v < BASE || i >= P_MEM + 32) printf(" %s=?%zx", tag, (size_t)v);
  else if (i < P_MEM) printf(" %s=%s+%zu", tag, names[i], off);
  else printf(" %s=%s%zu+%zu", tag, mnames[(i - P_MEM) % 4], (i - P_MEM) / 4, off);
}
template <int NM>
static void d1_args(const void* arg) {
  const D1Args<NM>& a = *(const D1Args<NM>*)arg;
  for (int i = 0; i < a.nmem && i < NM; ++i) {
    const D1Member& m = a.mem[i];
    printf(" m%d:", i), ptr("wp", m.wp), ptr("bt", m.bt), ptr("bias", m.bias), ptr("y", m.y);
    printf(" ldy=%lld N=%d Np=%d rp=%d b_limbs=%d r_off=%d cb0=%d nblk=%d", (long long)m.ldy, m.N, m.Np, m.rp, m.b_limbs, m.r_off, m.cb0, m.nblk);
  }
  printf(" M=%d Kp=%d nmem=%d rp_all=%d", a.M, a.Kp, a.nmem, a.rp_all), ptr("x", a.x);
  printf(" ldx=%lld K=%d w_exps=%d", (long long)a.ldx, a.K, a.w_exps), ptr("a_t", a.a_t), ptr("gran", a.gran);
  printf(" np=%d cpw=%d", a.np, a.cpw);
}
// the pointers of one launch, by kernel family (positional arguments: the kernels' signatures in csrc/*.hip)
static void fwd_pointers(const char* name, void** args) {
  const auto has = [&](const char* s) { return strstr(name, s) != nullptr; };
  const auto pos = [&](const char* tag, int i) { ptr(tag, *(void**)args[i]); };
  printf(" {");
  if (has("k_decode1")) {
    if (!has("k_decode1_narrow") && has("Lb1E")) d1_args<4>(args[0]);  // k_decode1<DT, BOUT, GROUP = true>: the table of four members
    else d1_args<1>(args[0]);
  } else if (has("k_lqer_gemm") || has("k_bout_amax")) {
    const GemmArgs& g = *(const GemmArgs*)args[0];
    ptr("xq", g.xq), ptr("wp", g.wp), ptr("xaq", g.xaq), printf(" xaq_ld=%d", g.xaq_ld), ptr("bt", g.bt), ptr("bias", g.bias), ptr("y", g.y);
    printf(" ldy=%lld", (long long)g.ldy), ptr("xa_part", g.xa_part), ptr("bout_amax", g.bout_amax), ptr("w8", g.w8), ptr("xscale", g.xscale);
  } else if (has("k_act16_fused")) pos("x", 0), pos("a_frag", 5), pos("xq", 6), pos("xaq", 7);
  else if (has("k_act8_fused")) pos("x", 0), pos("xq8", 5), pos("xscale", 7), pos("a_frag", 8), pos("xaq", 11), pos("zero_p", 12);
  else if (has("k_quant_xa16")) pos("x", 0), pos("xq", 6), pos("a_t", 8), pos("part", 12);
  else if (has("k_quant_xa128")) pos("x", 0), pos("xq", 5), pos("a_img", 7), pos("part", 12);
  else if (has("k_xa_partial_lds")) pos("xq", 0), pos("a_img", 2), pos("part", 8);
  else if (has("k_xa_partial")) pos("xq", 0), pos("a_t", 4), pos("part", 8);
  else if (has("k_xa_reduce_limbs")) pos("part", 0), pos("xaq", 3), pos("rowscale", 4);
  else if (has("k_xa_reduce")) pos("part", 0), pos("xaq", 4), pos("rowscale", 5);
  else if (has("k_split_act") || has("k_copy_act_f16")) pos("x", 0), pos("xq", 5);
  else if (has("k_quant_row8")) pos("x", 0), pos("xq8", 5), pos("xscale", 7);
  else if (has("k_quant_")) {  // k_quant_seg16 / _row / _blk / _int / _mf: (x, rows, cols, ld, QP, QuantOut ...)
    const QuantOut& o = *(const QuantOut*)args[5];
    pos("x", 0), ptr("xq", o.xq), ptr("xq8", o.xq8), ptr("xscale", o.xscale);
  } else if (has("k_w_widen")) pos("in", 0), pos("out", 5);
  else if (has("k_zero_")) pos("p", 0);
  else printf(" ?");
  printf(" }");
}

extern "C" {
int hipGetDevice(int* dev) { return *dev = 0; }
int hipDeviceGetAttribute(int* v, int, int) { return *v = g_cus, 0; }
int hipFuncSetAttribute(const void*, int, int) { return 0; }
int hipGetLastError(void) { return 0; }
static dim3 c_grid, c_block;  // the one pending <<<...>>> configuration
static size_t c_lds;
int __hipPushCallConfiguration(dim3 grid, dim3 block, size_t lds, void*) { return c_grid = grid, c_block = block, c_lds = lds, 0; }
int __hipPopCallConfiguration(dim3* grid, dim3* block, size_t* lds, void** stream) {
  return *grid = c_grid, *block = c_block, *lds = c_lds, *stream = nullptr, 0;
}
int hipLaunchKernel(const void* f, dim3 grid, dim3 block, void** args, size_t lds, void*) {
  Dl_info info;
  const char* name = (dladdr(f, &info) && info.dli_sname) ? info.dli_sname : "?";
  printf(" %s %u,%u,%u %u %zu", name, grid.x, grid.y, grid.z, block.x, lds);
  if (strstr(name, "k_bout_amax")) printf(" [%d %d]", *(int*)args[1], *(int*)args[2]);
  if (!g_act) return 0;
  auto ints = [&](int first, int n) {  // n consecutive int arguments
    for (int i = 0; i < n; ++i) printf("%s%d", i ? " " : " [", *(int*)args[first + i]);
    printf("]");
  };
  auto plan = [&](int at, int rp_at) {
    const XaPlan& p = *(const XaPlan*)args[at];
    printf(" [plan %d %d %d rp %d]", p.row_groups, p.nchunk, p.kc, *(int*)args[rp_at]);
  };
  if (strstr(name, "k_xa_partial_lds")) ints(4, 4);  // row_groups, nch, spc, steps_total
  else if (strstr(name, "k_quant_xa128")) ints(8, 4);
  else if (strstr(name, "k_xa_partial")) plan(7, 6);
  else if (strstr(name, "k_xa_reduce")) plan(1, 2);
  else if (strstr(name, "k_quant_xa16")) printf(" [vec %d rp %d rg %d]", (int)*(bool*)args[4], *(int*)args[10], *(int*)args[11]);
  else if (strstr(name, "k_act8_fused")) printf(" [zero_n %d]", *(int*)args[13]);
  if (g_fwd) fwd_pointers(name, args);
  return 0;
}
int hipMemcpy2DAsync(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height, int, void*) {
  printf(" hipMemcpy2DAsync %zu %zu %zu %zu", dpitch, spitch, width, height);
  if (g_fwd) printf(" {"), ptr("dst", dst), ptr("src", src), printf(" }");
  return 0;
}
int hipMemsetAsync(void* p, int value, size_t bytes, void*) {
  printf(" hipMemsetAsync %d %zu", value, bytes);
  if (g_fwd) printf(" {"), ptr("p", p), printf(" }");
  return 0;
}
}

// mode attn: the two products and the twelve attention entries
static int attn_cases(void* lib) {
#define SYM(n) const auto n = (decltype(&lqer_##n))dlsym(lib, "lqer_" #n)
  SYM(last_error);
  SYM(matmul_q);
  SYM(matmul_q_workspace_bytes_fmt);
  SYM(kv_cache_bytes);
  SYM(kv_pool_bytes_fmt);
  SYM(attention_q);
  SYM(attention_q_workspace_bytes);
  SYM(attention_q_decode);
  SYM(attention_q_decode_workspace_bytes);
  SYM(attention_q_decode_kv);
  SYM(attention_q_decode_kv_workspace_bytes);
  SYM(attention_q_kv);
  SYM(attention_q_kv_workspace_bytes);
  SYM(attention_q_decode_paged);
  SYM(attention_q_decode_paged_window);
  SYM(attention_q_decode_paged_shared);
  SYM(attention_q_decode_paged_workspace_bytes);
  SYM(attention_q_decode_paged_ragged);
  SYM(attention_q_decode_paged_ragged_workspace_bytes);
  SYM(attention_q_paged);
  SYM(attention_q_paged_window);
  SYM(attention_q_paged_workspace_bytes);
  SYM(attention_q_paged_ragged);
  SYM(attention_q_paged_ragged_window);
  SYM(attention_q_paged_ragged_workspace_bytes);
#undef SYM
  char* const p = (char*)(uintptr_t)0x40000000;  // (aligned, never read; the operands 256 MiB apart)
  const auto at = [&](int i) { return p + ((size_t)i << 28); };
  const auto done = [&](size_t need, int rc) { printf(" ws=%zu -> %d%s%s\n", need, rc, rc ? " " : "", rc ? last_error() : ""); };
  char name[64];
  while (scanf("%63s", name) == 1) {
    const auto is = [&](const char* s) { return !strcmp(name, s); };
    int dtype;
    long long batch;
    if (is("matmul_q")) {
      long long S1, K, S2;
      int xb, yb, lay, xo, yo, wsv;
      if (scanf("%d %lld %lld %lld %lld %d %d %d %d %d %d", &dtype, &batch, &S1, &K, &S2, &xb, &yb, &lay, &xo, &yo, &wsv) != 11) return 2;
      const int esz = dtype == LQER_F32 ? 4 : 2;
      const lqer_qfmt_t fx = {LQER_Q_MXINT, 8, xb, 8, 127}, fy = {LQER_Q_MXINT, 8, yb, 8, 127};
      const size_t need = matmul_q_workspace_bytes_fmt(batch, S1, K, S2, &fx, &fy);
      done(need, matmul_q(at(1) + xo * esz, at(2) + yo * esz, at(3), dtype, batch, S1, K, S2, S1 * K, K, K * S2, lay ? 1 : S2, lay ? K : 1, &fx, &fy,
                          at(4), need - (wsv && need), nullptr));
      continue;
    }
    long long heads, kvh, S, T, D, W, total, groups;
    int mask, qo, wsv, nulls, blk, kk, vk;
    if (scanf("%d %lld %lld %lld %lld %lld %lld %d %d %d %d %d %d %d %lld %lld %lld", &dtype, &batch, &heads, &kvh, &S, &T, &D, &mask, &qo, &wsv, &nulls,
              &blk, &kk, &vk, &W, &total, &groups) != 17)
      return 2;
    const int esz = dtype == LQER_F32 ? 4 : 2, causal = mask == 3;
    const lqer_qfmt_t f = {LQER_Q_MXINT, 8, blk, 8, 127}, fk = {kk, kk == LQER_Q_MXINT_C4 ? 4 : 8, blk, 8, 127},
                      fv = {vk, vk == LQER_Q_MXINT_C4 ? 4 : 8, blk, 8, 127};
    const int64_t mr = (T + 3) / 4 * 4 + (mask == 2);
    const int64_t qs3[3] = {heads * S * D, S * D, D}, kv3[3] = {kvh * T * D, T * D, D}, ms3[3] = {heads * S * mr, S * mr, mr};
    const int64_t qs2[2] = {heads * D, D};  // per-sequence counts: (token, head)
    const int64_t *qs = nulls ? nullptr : qs3, *qsr = nulls ? nullptr : qs2;
    const void *q = at(1) + qo * esz, *k = at(2), *v = at(3), *m = mask == 1 || mask == 2 ? at(4) : nullptr;
    void *out = at(5), *ws = at(6), *kvbuf = at(7);
    float* stats = (float*)at(8);
    const int32_t* dev = (const int32_t*)at(9);  // (every int32 array on the device)
    const auto cut = [&](size_t need) { return need - (wsv && need); };
    // a cache of exactly T keys; a pool of one table row per sequence, max_len keys each
    const int64_t cap = T > 0 ? T : 1, stride = (cap + 15) / 16, slots = batch > 0 ? batch : 1, pages = slots * stride;
    size_t need = 0;
    int rc = 0;
#define DENSE(fn) (need = fn##_workspace_bytes(batch, heads, kvh, S, T, D), \
                   fn(q, k, v, m, out, stats, dtype, batch, heads, kvh, S, T, D, qs, kv3, kv3, ms3, qs3, 0.125f, causal, &f, &fk, &f, &fv, ws, cut(need), nullptr))
#define CACHE(fn) (need = fn##_workspace_bytes(batch, heads, kvh, S, T, D),                                                                \
                   fn(q, kvbuf, kv_cache_bytes(dtype, batch, kvh, cap, D), cap, m, out, stats, dtype, batch, heads, kvh, S, T, D, qs, ms3, qs3, 0.125f, \
                      causal, &f, &fk, &f, &fv, ws, cut(need), nullptr))
#define POOL kvbuf, kv_pool_bytes_fmt(dtype, pages, slots, kvh, D, &fk, &fv), pages, slots, dev, stride, dev, dev, T, out, stats, dtype, batch, heads, kvh
#define TAIL 0.125f, causal, &f, &fk, &f, &fv, ws, cut(need), nullptr
    if (is("attention_q")) rc = DENSE(attention_q);
    else if (is("attention_q_decode")) rc = DENSE(attention_q_decode);
    else if (is("attention_q_decode_kv")) rc = CACHE(attention_q_decode_kv);
    else if (is("attention_q_kv")) rc = CACHE(attention_q_kv);
    else if (!strncmp(name, "attention_q_decode_paged", 24)) {
      need = is("attention_q_decode_paged_ragged") ? attention_q_decode_paged_ragged_workspace_bytes(total, heads, T, D)
                                                   : attention_q_decode_paged_workspace_bytes(batch, heads, kvh, S, T, D);
      if (is("attention_q_decode_paged")) rc = attention_q_decode_paged(q, POOL, S, D, qs, qs3, TAIL);
      else if (is("attention_q_decode_paged_window")) rc = attention_q_decode_paged_window(q, POOL, S, D, qs, qs3, TAIL, W);
      else if (is("attention_q_decode_paged_shared")) rc = attention_q_decode_paged_shared(q, POOL, S, D, qs, qs3, TAIL, dev, dev, dev, dev, groups);
      else if (is("attention_q_decode_paged_ragged")) rc = attention_q_decode_paged_ragged(q, POOL, dev, S, total, D, qsr, qs2, TAIL, W);
      else return 2;
    } else if (is("attention_q_paged") || is("attention_q_paged_window")) {
      need = attention_q_paged_workspace_bytes(batch, heads, kvh, S, T, D);
      rc = is("attention_q_paged") ? attention_q_paged(q, POOL, S, D, qs, qs3, TAIL) : attention_q_paged_window(q, POOL, S, D, qs, qs3, TAIL, W);
    } else if (is("attention_q_paged_ragged") || is("attention_q_paged_ragged_window")) {
      need = attention_q_paged_ragged_workspace_bytes(batch, heads, kvh, S, T, D);
      rc = is("attention_q_paged_ragged") ? attention_q_paged_ragged(q, POOL, dev, S, total, D, qsr, qs2, TAIL)
                                          : attention_q_paged_ragged_window(q, POOL, dev, S, total, D, qsr, qs2, TAIL, W);
    } else {
      return 2;
    }
#undef DENSE
#undef CACHE
#undef POOL
#undef TAIL
    done(need, rc);
  }
  return 0;
}

static bool read_desc(lqer_linear_desc_t* d) {
  memset(d, 0, sizeof(*d));
  lqer_qfmt_t* f[5] = {&d->x_fmt, &d->w_fmt, &d->b_fmt, &d->a_out_fmt, &d->b_out_fmt};
  if (scanf("%d %d %d %d %d", &d->in_features, &d->out_features, &d->rank, &d->has_bias, &d->tuning) != 5) return false;
  for (auto q : f)
    if (scanf("%d %d %d %d %d", &q->kind, &q->width, &q->block, &q->exp_width, &q->exp_bias) != 5) return false;
  return true;
}

// mode fwd: the composed forward, its compact-image and split forms, and the group
static int fwd_cases(void* lib) {
#define SYM(n) const auto n = (decltype(&lqer_##n))dlsym(lib, "lqer_" #n)
  SYM(last_error);
  SYM(padded_r);
  SYM(desc_limbs);
  SYM(linear_sizes);
  SYM(linear_forward);
  SYM(linear_forward_narrow);
  SYM(linear_forward_narrow_workspace_bytes);
  SYM(weight_narrow_route);
  SYM(linear_gemm_narrow);
  SYM(linear_gemm_prepared);
  SYM(linear_forward_group);
  SYM(group_workspace_bytes);
#undef SYM
  g_act = g_fwd = true;
  const auto done = [&](int rc, const char* end) { printf(" -> %d%s%s%s", rc, rc ? " " : "", rc ? last_error() : "", end); };
  const size_t ample = (size_t)1 << 40;
  char kind[8];
  while (scanf("%7s", kind) == 1) {
    if (kind[0] == 'f') {
      lqer_linear_desc_t d;
      long long M;
      int dtype, a_limbs, b_limbs, ptrs, wsv;
      if (!read_desc(&d) || scanf("%lld %d %d %d %d %d", &M, &dtype, &a_limbs, &b_limbs, &ptrs, &wsv) != 6) return 2;
      const void* x = at(P_X) + (ptrs == 1 ? 2 : 0);
      const int64_t ldx = d.in_features + (ptrs == 1), ldy = d.out_features;
      const float* bias = d.has_bias ? (const float*)at(P_BIAS) : nullptr;
      const auto cut = [&](size_t need) { return need - (wsv == 1 && need); };
      const void *a_t = d.rank > 0 ? at(P_AT) : nullptr, *bt = d.rank > 0 ? at(P_BT) : nullptr;  // (no side path: no operands)
      lqer_linear_sizes_t sz;
      memset(&sz, 0, sizeof(sz));
      int rc = linear_sizes(&d, M, &sz);
      printf(" sizes=%zu,%zu,%zu,%zu,%zu rc=%d%s%s |", sz.w_packed, sz.a_t, sz.b_t, sz.bias_q, sz.workspace, rc, rc ? " " : "", rc ? last_error() : "");
      void* const ws = wsv == 2 ? nullptr : at(P_WS);
      done(linear_forward(&d, x, dtype, M, ldx, at(P_W), a_t, bt, a_limbs, b_limbs, bias, at(P_Y), ldy, ws, cut(sz.workspace), nullptr), " |");
      const size_t nws = linear_forward_narrow_workspace_bytes(&d, M);
      rc = weight_narrow_route(&d, M, dtype, ldx, a_limbs, b_limbs);
      printf(" nws=%zu route=%d%s%s", nws, rc, rc < 0 ? " " : "", rc < 0 ? last_error() : "");
      done(linear_forward_narrow(&d, x, dtype, M, ldx, at(P_W), a_t, bt, a_limbs, b_limbs, bias, at(P_Y), ldy, ws, cut(nws), nullptr), " |");
      int xl = 1, al = 1;
      desc_limbs(&d, &xl, &al);
      const void *xq = ptrs == 2 ? x : at(P_XQ), *xaq = d.rank > 0 ? at(P_XAQ) : nullptr;
      const int64_t xaq_ld = padded_r(d.rank) * al;
      done(linear_gemm_narrow(&d, xq, M, at(P_W), xaq, xaq_ld, bt, b_limbs, bias, at(P_Y), dtype, ldy, at(P_WS), ample, wsv == 2 ? nullptr : at(P_WIDEN),
                              cut(sz.w_packed), nullptr), " |");
      done(linear_gemm_prepared(&d, xq, M, at(P_W), xaq, bt, b_limbs, bias, at(P_Y), dtype, ldy, at(P_WS), ample, wsv == 0 ? ample : 0, nullptr), "\n");
    } else if (kind[0] == 'g') {
      enum { MAXN = 8 };
      lqer_linear_desc_t d[MAXN];
      lqer_group_member_t mem[MAXN];
      long long M;
      int n, dtype, a_limbs, xoff, wsv;
      if (scanf("%d %lld %d %d %d %d", &n, &M, &dtype, &a_limbs, &xoff, &wsv) != 6 || n < 1 || n > MAXN) return 2;
      int64_t rp_all = 0;
      for (int i = 0; i < n; ++i) {
        int b_limbs, flaw;
        if (!read_desc(&d[i]) || scanf("%d %d", &b_limbs, &flaw) != 2) return 2;
        rp_all += padded_r(d[i].rank);
        if (flaw == 3) d[i].rank = -1;
        const auto m = [&](int j) { return at(P_MEM + 4 * i + j); };
        mem[i] = lqer_group_member_t{&d[i], flaw == 1 ? nullptr : m(0), m(1), b_limbs, d[i].has_bias && flaw != 2 ? (const float*)m(2) : nullptr, m(3),
                                     d[i].out_features};
      }
      const size_t need = group_workspace_bytes(d[0].in_features, rp_all);
      printf(" gws=%zu", need);
      done(linear_forward_group(mem, n, at(P_X) + (xoff ? 2 : 0), dtype, M, d[0].in_features + (xoff ? 1 : 0), at(P_AT), a_limbs,
                                at(P_WS) + (wsv == 2 ? 8 : 0), need - (wsv == 1 && need), nullptr), "\n");
    } else {
      return 2;
    }
  }
  return 0;
}

int main(int argc, char** argv) {
  void* lib = argc > 1 ? dlopen(argv[1], RTLD_NOW | RTLD_GLOBAL) : nullptr;
  if (argc > 2) sscanf(argv[2], "%d", &g_cus);
  if (!lib) return fprintf(stderr, "launch_probe: %s\n", dlerror()), 2;
  if (argc > 3 && !strcmp(argv[3], "attn")) return attn_cases(lib);
  if (argc > 3 && !strcmp(argv[3], "fwd")) return fwd_cases(lib);
  auto gemm = (decltype(&lqer_linear_gemm_ld))dlsym(lib, "lqer_linear_gemm_ld");
  auto limbs = (decltype(&lqer_desc_limbs))dlsym(lib, "lqer_desc_limbs");
  auto padded_r = (decltype(&lqer_padded_r))dlsym(lib, "lqer_padded_r");
  auto last_error = (decltype(&lqer_last_error))dlsym(lib, "lqer_last_error");
  void* const p = (void*)(uintptr_t)0x40000000;  // (aligned, never read)
  g_act = argc > 3 && !strcmp(argv[3], "act");
  auto act_xa = (decltype(&lqer_quantize_act_xa))dlsym(lib, "lqer_quantize_act_xa");
  auto act_xa_prep = (decltype(&lqer_quantize_act_xa_prep))dlsym(lib, "lqer_quantize_act_xa_prep");
  auto lowrank_xa = (decltype(&lqer_lowrank_xa))dlsym(lib, "lqer_lowrank_xa");
  auto xa_scratch = (decltype(&lqer_lowrank_xa_scratch_bytes))dlsym(lib, "lqer_lowrank_xa_scratch_bytes");
  lqer_linear_desc_t d;
  long long M;
  int dtype, b_limbs;
  for (;;) {
    memset(&d, 0, sizeof(d));
    lqer_qfmt_t* f[5] = {&d.x_fmt, &d.w_fmt, &d.b_fmt, &d.a_out_fmt, &d.b_out_fmt};
    if (scanf("%d %d %d %d", &d.in_features, &d.out_features, &d.rank, &d.tuning) != 4) break;
    for (auto q : f)
      if (scanf("%d %d %d %d %d", &q->kind, &q->width, &q->block, &q->exp_width, &q->exp_bias) != 5) return 2;
    if (scanf("%lld %d %d", &M, &dtype, &b_limbs) != 3) return 2;
    if (g_act) {
      int ptrs, scr;
      if (scanf("%d %d", &ptrs, &scr) != 2) return 2;
      const int a_limbs = b_limbs;
      const void* x = ptrs == 1 ? (char*)p + 2 : p;
      const int64_t ldx = d.in_features + (ptrs == 1);
      void* const xq = ptrs == 2 ? (void*)x : (char*)p + (1 << 28);
      void* const a_t = d.rank > 0 ? p : nullptr;
      const size_t bytes = scr == 0 ? (size_t)1 << 40 : scr == 1 ? xa_scratch(&d, M) : 0;
      void* const scratch = bytes ? p : nullptr;
      auto done = [&](int rc, const char* end) { printf(" -> %d%s%s%s", rc, rc ? " " : "", rc ? last_error() : "", end); };
      done(act_xa(&d, x, dtype, M, ldx, a_t, a_limbs, xq, p, scratch, bytes, nullptr), " |");
      done(act_xa(&d, x, dtype, M, ldx, a_t, a_limbs, xq, nullptr, scratch, bytes, nullptr), " |");
      size_t ready = 0;
      const int rc = act_xa_prep(&d, x, dtype, M, ldx, a_t, a_limbs, xq, p, scratch, bytes, p, &ready, nullptr);
      printf(" ready=%zu", ready);
      done(rc, " |");
      done(lowrank_xa(&d, xq, M, a_t, a_limbs, p, scratch, bytes, nullptr), "\n");
      continue;
    }
    int xl = 1, al = 1;
    limbs(&d, &xl, &al);
    const int rc = gemm(&d, p, M, p, d.rank > 0 ? p : nullptr, padded_r(d.rank) * al, d.rank > 0 ? p : nullptr, b_limbs, nullptr, p, dtype,
                        d.out_features, p, (size_t)1 << 40, nullptr);
    printf(" -> %d%s%s\n", rc, rc ? " " : "", rc ? last_error() : "");
  }
  return 0;
}
