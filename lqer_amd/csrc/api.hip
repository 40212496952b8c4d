// C ABI of liblqer_hip.so (include/lqer_hip.h): argument checking, buffer carving, kernel dispatch.
// No allocation, no synchronisation, no global mutable state besides the thread-local error text.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "gemm_plan.h"
#include "w_narrow.h"

namespace lqer {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: %s", what, hipGetErrorString(e));
    return LQER_E_LAUNCH;
  }
  return LQER_OK;
}

static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
// a refusal as one statement: its text, and the code to return - or a check's "no"
template <class... A>
static int fail(int rc, const char* fmt, A... a) {
  set_error(fmt, a...);
  return rc;
}
template <class... A>
static bool refuse(const char* fmt, A... a) {
  set_error(fmt, a...);
  return false;
}

// What a format may be, by the role it plays in a call: one row per role.  `name` opens every refusal's text.
enum Role {
  ROLE_X, ROLE_W, ROLE_W_GROUP, ROLE_B, ROLE_A_OUT, ROLE_B_OUT, ROLE_QUANTIZE, ROLE_QUANTIZE_TILES, ROLE_MATMUL_X, ROLE_MATMUL_W,
  ROLE_ATTN_Q, ROLE_ATTN_K, ROLE_ATTN_P, ROLE_ATTN_V, ROLE_ATTN_KV
};
struct RoleRow {
  const char* name;
  int max_width;            // the widest block_fp or signed integer format
  bool integer, minifloat;  // LQER_Q_INT / LQER_Q_MINIFLOAT are served
  bool weight;              // a packed weight: signed integers only (two's-complement nibbles), minifloats of 2..4 bits with an e4m3 table
  bool f16, i8;             // LQER_Q_PASSTHROUGH_F16 / LQER_Q_MXINT_I8 are accepted (the x_quantizer kinds)
};
static const RoleRow ROLES[] = {
    {"x_quantizer", 9, true, true, false, true, true},
    {"w_quantizer", 8, true, true, true, false, false},
    {"w_quantizer", 4, true, true, true, false, false},  // a group member's: the one-launch decode kernel reads one image of 4-bit panels
    {"b_quantizer", 24, true, true, false, false, false},
    {"A_out_quantizer", 9, true, true, false, false, false},
    {"B_out_quantizer", 24, true, true, false, false, false},
    {"quantize_mxint", 24, true, true, false, false, false},
    {"quantize_mxint_tiles", 24, false, false, false, false, false},
    {"matmul x_quantizer", 8, false, true, false, false, false},
    {"matmul w_quantizer", 8, false, true, false, false, false},
    {"attention Q quantizer", 8, false, false, false, false, false},
    {"attention K quantizer", 8, false, false, false, false, false},
    {"attention P quantizer", 8, false, false, false, false, false},
    {"attention V quantizer", 8, false, false, false, false, false},
    {"attention K / V quantizer", 8, false, false, false, false, false},
};

// a minifloat format the HIP path serves: width 2..8 (weights: 2..4), exp_width 1..width-1, every non-zero value a normal bf16 number (the
// bf16 images are exact, the MFMAs see no subnormal operand); weights also need the e4m3 table of their 4-bit codes (mf_e4m3_table)
static bool minifloat_fmt_ok(const lqer_qfmt_t& f, const char* name, bool weight) {
  const int max_width = weight ? 4 : 8;
  if (f.width < 2 || f.width > max_width)
    return refuse("%s: minifloat width %d outside [2,%d]%s", name, f.width, max_width,
                  weight ? " (minifloat weights of 5..8 bits need an 8-bit code image: not implemented)" : "");
  if (f.exp_width < 1 || f.exp_width > f.width - 1)
    return refuse("%s: minifloat exponent_width %d outside [1,%d] (width %d: mantissa bits = width - exponent_width - 1 >= 0)", name,
                  f.exp_width, f.width - 1, f.width);
  const int mbits = f.width - f.exp_width - 1;
  const int emax = (1 << f.exp_width) - 1 - f.exp_bias, lowest = 1 - f.exp_bias - mbits;  // exponents of the largest / smallest value
  if (f.exp_bias < -1000 || f.exp_bias > 1000 || emax > 127 || lowest < -126)
    return refuse("%s: minifloat exponent_bias %d: the values span 2^%d .. 2^%d, outside the normal bf16 range 2^-126 .. 2^127", name,
                  f.exp_bias, lowest, emax);
  if (weight) {
    uint32_t lut[2];
    int s;
    if (!mf_e4m3_table(f, lut, &s))
      return refuse("%s: minifloat(%d, %d, %d): its values are not e4m3 numbers times one power of two", name, f.width, f.exp_width,
                    f.exp_bias);
  }
  return true;
}

static bool fmt_ok(const lqer_qfmt_t* f, Role role) {
  const RoleRow& r = ROLES[role];
  const char* const name = r.name;
  const int max_width = r.max_width;
  if (!f) return refuse("%s: null format", name);
  if (f->kind == LQER_Q_PASSTHROUGH) return true;
  if (f->kind == LQER_Q_PASSTHROUGH_F16 && r.f16) return true;
  if (f->kind == LQER_Q_MXINT_I8 && !r.i8) return refuse("%s: LQER_Q_MXINT_I8 is an x_quantizer kind", name);
  if (f->kind == LQER_Q_MXINT_C4)  // (the pool entries replace it by LQER_Q_MXINT before they come here: pool_code_fmt)
    return refuse("%s: LQER_Q_MXINT_C4 names the nibble code storage of the paged KV pool - a k_fmt / v_fmt kind of the lqer_kv_pool_* and "
                  "lqer_attention_q_*paged* entries only", name);
  if (f->kind == LQER_Q_INT) {  // fixed point: exp_bias = frac_width, exp_width = is_signed
    if (!r.integer) return refuse("%s: the integer quantizer is not implemented in this role", name);
    if (r.weight && !f->exp_width)  // codes travel as two's-complement nibbles: signed, 2..4 bits
      return refuse("%s: an unsigned integer weight is not implemented (4-bit codes 0..15 do not fit the two's-complement nibble)", name);
    const int maxw = f->exp_width ? max_width : max_width - 1;  // unsigned: one magnitude bit more per width
    if (f->width < 1 || f->width > maxw || f->exp_bias < -100 || f->exp_bias > 100)
      return refuse("%s: integer width %d outside [1,%d] or frac_width %d outside [-100,100]", name, f->width, maxw, f->exp_bias);
    return true;
  }
  if (f->kind == LQER_Q_MINIFLOAT) {  // width, exp_width, exp_bias = the resolved bias (include/lqer_hip.h)
    if (!r.minifloat) return refuse("%s: the minifloat quantizer is not implemented in this role", name);
    return minifloat_fmt_ok(*f, name, r.weight);
  }
  if (f->kind != LQER_Q_MXINT && f->kind != LQER_Q_MXINT_I8) return refuse("%s: quantizer kind %d is not implemented on the HIP path", name, f->kind);
  if (f->width < 2 || f->width > max_width) return refuse("%s: width %d outside [2,%d]", name, f->width, max_width);
  if (f->exp_width < 1 || f->exp_width > 8) return refuse("%s: exponent_width %d outside [1,8]", name, f->exp_width);
  // every block scale 2^(e - mbits), e in [emin, emax], must be reachable as a normal float from some block: the kernels build it from
  // exponent bits (and flush what is below 1e-8) on the argument that e - mbits < -126 happens only under an upper clamp nobody
  // configures - and an emin beyond 127 would put every block's 2^e past fp32 (include/lqer_hip.h, lqer_qfmt_t)
  const int mbits = f->width - 1, emin = -f->exp_bias, emax = (1 << f->exp_width) - 1 - f->exp_bias;
  if (f->exp_bias > 1000 || f->exp_bias < -1000 || emax - mbits < -126 || emin > 127)
    return refuse("%s: block_fp exponent_bias %d (exponent_width %d, width %d): exponents [%d,%d] - needs emax - (width-1) >= -126 and "
                  "emin <= 127, i.e. a bias in [-127,%d]", name, f->exp_bias, f->exp_width, f->width, emin, emax,
                  (1 << f->exp_width) - 1 - mbits + 126);
  return true;
}

// bf16 limbs of a pass-through tensor: fmt.width = significand bits to carry (8 per limb); block_fp images need one
static int limbs_of(const lqer_qfmt_t& f) {
  if (f.kind != LQER_Q_PASSTHROUGH) return 1;
  return f.width <= 8 ? 1 : (f.width <= 16 ? 2 : 3);
}
static int act_limbs(const lqer_linear_desc_t* d) { return limbs_of(d->x_fmt); }
// 4-bit limbs of the packed weight: block_fp weights of 5..8 bits travel as three signed base-8 digits side by side along k (pack.hip),
// the activation image is repeated to match (include/lqer_hip.h "weights of 5..8 bits")
static int w_panel_limbs(const lqer_linear_desc_t* d) { return (d->w_fmt.kind == LQER_Q_MXINT && d->w_fmt.width > 4) ? 3 : 1; }
// ... and the copies of the activation image that go with them: none on the int8 route (its kernel multiplies the int8 CODES of such
// a weight, one image of its own behind the limb panels)
static int w_limbs(const lqer_linear_desc_t* d) { return d->x_fmt.kind == LQER_Q_MXINT_I8 ? 1 : w_panel_limbs(d); }
static bool x_is_f16(const lqer_linear_desc_t* d) { return d->x_fmt.kind == LQER_Q_PASSTHROUGH_F16; }
static bool x_is_i8(const lqer_linear_desc_t* d) { return d->x_fmt.kind == LQER_Q_MXINT_I8; }
// byte offset of the int8 weight image inside w_packed (behind the sign-magnitude panels)
static size_t i8_image_offset(const lqer_linear_desc_t* d) {
  const size_t Kp = lqer_padded_k(d->in_features), Np = lqer_padded_n(d->out_features);
  return align_up((Np / LQER_PANEL_ROWS) * (Kp / 64) * LQER_PANEL_BYTES * w_panel_limbs(d), 256);
}
// static requirements of the int8 route (include/lqer_hip.h "int8 route")
static bool i8_formats_ok(const lqer_linear_desc_t* d) {
  const lqer_qfmt_t &x = d->x_fmt, &w = d->w_fmt;
  const int64_t K = d->in_features;
  if (x.width < 2 || x.width > 8 || !(x.block <= 0 || x.block >= K))
    return refuse("LQER_Q_MXINT_I8: x_quantizer must be block_fp with width <= 8 and one block per row (got width %d block %d)", x.width, x.block);
  if (w.kind != LQER_Q_MXINT || w.width > 8 || !(w.block <= 0 || w.block >= K || w.block % I8_BK == 0))
    return refuse("LQER_Q_MXINT_I8: w_quantizer blocks must span a multiple of 128 k or the whole row (got block %d)", w.block);
  if (K < I8_BK) return refuse("LQER_Q_MXINT_I8: in_features %lld < 128", (long long)K);
  return true;
}
// LQER_Q_PASSTHROUGH_F16: a dense fp16 tensor whose extents are already the padded ones IS the activation image
// (M a multiple of the row padding: the tile kernels read whole row tiles; M <= 64: the small-M kernel and the side
// GEMM never read past row M - 1 - unless B_out blocks other than 16 send a decode-size call to the tile kernel)
// (route: the plan's for (d, M, LQER_F16) - an integer B_out, or B_out blocks other than 16, send a decode-size call to the tile kernel,
// whose buffer range covers whole row tiles)
static bool f16_image_is_input(const lqer_linear_desc_t* d, const void* x, int64_t M, int64_t ldx, int route) {
  const bool smallm = M <= 64 && route == LQER_ROUTE_SMALLM;
  return x_is_f16(d) && ldx == d->in_features && d->in_features % LQER_K_ALIGN == 0 && (M % LQER_M_ALIGN == 0 || smallm) &&
         ((uintptr_t)x & 15) == 0 && w_limbs(d) == 1;
}
// Decode sizes with the fused-quantizer formats: the small-M GEMM reduces the split-K partial tiles of x A itself
// (lqer_quantize_act_xa / lqer_linear_gemm with xaq == NULL), one launch less on a launch-bound path.
static bool decode_partials_ok(const lqer_linear_desc_t* d, int64_t M) {
  if (!d || d->rank <= 0 || M <= 0 || M > 64) return false;
  if (d->w_fmt.kind != LQER_Q_MXINT) return false;  // (integer weights: two's-complement nibbles - the tile kernel at every M)
  if (w_limbs(d) != 1) return false;  // (5..8-bit weights: the GEMM walks three limb images over a repeated activation image)
  if (d->x_fmt.kind != LQER_Q_MXINT || d->a_out_fmt.kind != LQER_Q_MXINT) return false;
  if (!xa_fused_partials_ok(make_qp(d->x_fmt), make_qp(d->a_out_fmt), d->rank)) return false;
  const lqer_qfmt_t& bo = d->b_out_fmt;  // the small-M kernel: B_out pass-through or blocks of 16
  return bo.kind == LQER_Q_PASSTHROUGH || (bo.kind == LQER_Q_MXINT && bo.block == 16);
}
static bool need_f16(const lqer_linear_desc_t* d, int dtype, const char* what) {
  if (x_is_f16(d) && dtype != LQER_F16) return refuse("%s: x_quantizer LQER_Q_PASSTHROUGH_F16 takes fp16 tensors (dtype %d given)", what, dtype);
  return true;
}
// the side product x A is an fp32 sum: two limbs at least
static int xa_limbs(const lqer_linear_desc_t* d) {
  if (d->a_out_fmt.kind != LQER_Q_PASSTHROUGH) return 1;
  return d->a_out_fmt.width <= 16 ? 2 : 3;
}
// row stride of xaq in elements: the padded rank, once per limb of a pass-through A_out
static int64_t xaq_row_elems(const lqer_linear_desc_t* d) { return lqer_padded_r(d->rank) * xa_limbs(d); }
// bytes of the standard image of d's weight (one copy: what a compact image widens into)
static size_t std_image_bytes(const lqer_linear_desc_t* d) {
  return (size_t)(lqer_padded_n(d->out_features) / LQER_PANEL_ROWS) * (lqer_padded_k(d->in_features) / 64) * LQER_PANEL_BYTES;
}

// Where the pieces of a forward's workspace lie for (d, m_max), as byte offsets from its start, each 256-byte aligned:
//   [activation image | its single copy] [xaq] [shared scratch] ... [widened weight image]
// The ONE carving: lqer_linear_sizes().workspace, lqer_act_image_bytes, the single-copy image of the split calls, lqer_linear_forward
// and lqer_linear_forward_narrow_workspace_bytes read it.
struct Carving {
  // the activation image `xq` of the split calls: [Mp][act limbs x weight limbs x Kp] bf16 from offset 0 and, when the weight has limbs,
  // the single-copy image behind it - the quantizer and the side GEMM work on that one, the GEMM on the wide one (0: one and the same)
  size_t single;
  size_t xaq;         // [Mp][xaq_row_elems] bf16; its offset = the bytes of the activation image buffer
  size_t scratch;     // the side path's scratch, then the GEMM's: the two uses never overlap in time
  size_t side_bytes;  // ... what the side path needs of it (lqer_lowrank_xa_scratch_bytes)
  size_t gemm_bytes;  // ... what the GEMM needs (lqer_linear_gemm_scratch_bytes)
  size_t total;       // lqer_linear_sizes().workspace
  size_t widened;     // lqer_linear_forward_narrow: the standard image (std_image_bytes) a compact one is widened into
};
static Carving carve(const lqer_linear_desc_t* d, int64_t m_max) {
  Carving c;
  const size_t Mp = lqer_padded_m(m_max), one = align_up(Mp * lqer_padded_k(d->in_features) * 2 * act_limbs(d), 256);
  // (an LQER_Q_MXINT_I8 descriptor sizes for the bf16 kernels too: token counts the int8 kernel does not serve run them on the same
  // buffers - lqer_linear_forward switches the kind - while its own quantizer writes one image at the head: only `single` differs)
  const size_t wl = w_panel_limbs(d), wide = wl > 1 ? align_up(one * wl, 256) : 0;
  c.single = w_limbs(d) > 1 ? wide : 0;
  c.xaq = wide + one;
  const bool side = d->rank > 0;
  c.scratch = c.xaq + (side ? align_up(Mp * xaq_row_elems(d) * 2, 256) : 0);
  c.side_bytes = side ? xa_scratch_bytes(m_max, d->in_features, lqer_padded_r(d->rank)) : 0;
  c.gemm_bytes = side && d->b_out_fmt.kind == LQER_Q_MXINT ? gemm_scratch_bytes(m_max, d->out_features, make_qp(d->b_out_fmt)) : 0;
  c.total = c.scratch + align_up(c.side_bytes > c.gemm_bytes ? c.side_bytes : c.gemm_bytes, 256);
  c.widened = align_up(c.total, 256);
  return c;
}
static void* act_single_copy(const lqer_linear_desc_t* d, void* xq, int64_t M) {
  return w_limbs(d) == 1 ? xq : (unsigned char*)xq + carve(d, M).single;
}
// The compact weight image (w_narrow.h) serves block_fp weights of width 2 and 3 whose image exists once: E > 0 = its exponent bytes
// per row, 0 = not served (widths 4..8, integer and minifloat weights)
static int narrow_exps(const lqer_qfmt_t* f, int64_t K) {
  return (f && f->kind == LQER_Q_MXINT) ? wn_exps_per_row(f->width, f->block, K) : 0;
}
static size_t narrow_bytes(int64_t N, int64_t K, const lqer_qfmt_t* f) {
  const int E = narrow_exps(f, K);
  if (!E || N <= 0 || K <= 0) return 0;
  return (size_t)(lqer_padded_n(N) / LQER_PANEL_ROWS) * (lqer_padded_k(K) / 64) * wn_panel_bytes(f->width, E);
}
// a descriptor whose forward can be handed the compact image; fills GemmArgs::w_narrow
static int narrow_args(const lqer_linear_desc_t* d, GemmArgs& g) {
  const int E = narrow_exps(&d->w_fmt, d->in_features);
  if (!E)
    return fail(LQER_E_UNSUPPORTED, "compact weight image: block_fp weights of width 2 or 3 only (w_quantizer kind %d width %d: the standard image)",
                d->w_fmt.kind, d->w_fmt.width);
  if (x_is_i8(d))
    return fail(LQER_E_UNSUPPORTED, "compact weight image: not on the int8 route (LQER_Q_MXINT_I8 reads an int8 image of its own): use LQER_Q_MXINT");
  if (act_limbs(d) != 1)
    return fail(LQER_E_UNSUPPORTED, "compact weight image: pass-through bf16 / fp32 activations read one copy of the image per limb (%d): the standard image",
                act_limbs(d));
  if (d->tuning & LQER_TUNE_W_EXP_TABLE)
    return fail(LQER_E_UNSUPPORTED, "compact weight image: a weight that needs LQER_TUNE_W_EXP_TABLE (an exponent byte above 245) keeps the standard image");
  g.w_narrow = d->w_fmt.width << 8 | E;
  return LQER_OK;
}

static bool passthrough_width_ok(const lqer_qfmt_t& f, const char* name) {
  if (f.kind == LQER_Q_PASSTHROUGH && (f.width < 1 || f.width > 24))
    return refuse("%s: a passthrough format must say how many significand bits to carry in `width` (8 = bf16, 11 = fp16, "
                  "16, 24 = fp32), got %d", name, f.width);
  return true;
}

}  // namespace lqer

using namespace lqer;
#ifdef LQER_HOST_TIMING  // diagnostic build: host nanoseconds between marks of lqer_linear_forward, printed at exit
#include <ctime>
namespace {
struct FwdT {
  double seg[8] = {0}; long n = 0; timespec last;
  void start() { clock_gettime(CLOCK_MONOTONIC, &last); }
  void mark(int i) { timespec t; clock_gettime(CLOCK_MONOTONIC, &t); seg[i] += (t.tv_sec - last.tv_sec) * 1e9 + (t.tv_nsec - last.tv_nsec); last = t; }
  ~FwdT() { if (n) { fprintf(stderr, "[forward host] calls %ld:", n); for (int i = 0; i < 8; ++i) fprintf(stderr, " seg%d %.0f ns", i, seg[i] / n); fprintf(stderr, "\n"); } }
};
FwdT fwd_t;
}
#define HT_START() fwd_t.start()
#define HT_MARK(i) fwd_t.mark(i)
#define HT_DONE() (fwd_t.n++)
#else
#define HT_START()
#define HT_MARK(i)
#define HT_DONE()
#endif

extern "C" {
int lqer_version(void) { return LQER_ABI_VERSION; }
size_t lqer_sizeof_qfmt(void) { return sizeof(lqer_qfmt_t); }
size_t lqer_sizeof_linear_desc(void) { return sizeof(lqer_linear_desc_t); }
size_t lqer_sizeof_linear_sizes(void) { return sizeof(lqer_linear_sizes_t); }
size_t lqer_sizeof_group_member(void) { return sizeof(lqer_group_member_t); }
const char* lqer_last_error(void) { return g_err; }

int64_t lqer_padded_k(int64_t K) { return (K + LQER_K_ALIGN - 1) / LQER_K_ALIGN * LQER_K_ALIGN; }
int64_t lqer_padded_n(int64_t N) { return (N + LQER_N_ALIGN - 1) / LQER_N_ALIGN * LQER_N_ALIGN; }
int64_t lqer_padded_m(int64_t M) { return (M + LQER_M_ALIGN - 1) / LQER_M_ALIGN * LQER_M_ALIGN; }
int64_t lqer_padded_r(int64_t r) { return (r + LQER_R_ALIGN - 1) / LQER_R_ALIGN * LQER_R_ALIGN; }

int lqer_quantize_mxint(const void* x, int dtype, int64_t rows, int64_t cols, int64_t ld, const lqer_qfmt_t* fmt,
                        float* deq_f32, int8_t* codes, int8_t* exps, void* stream) {
  if (!x && rows * cols > 0) {
    set_error("quantize_mxint: null input");
    return LQER_E_INVALID;
  }
  if (rows < 0 || cols < 0 || ld < cols) {
    set_error("quantize_mxint: bad shape rows=%lld cols=%lld ld=%lld", (long long)rows, (long long)cols, (long long)ld);
    return LQER_E_INVALID;
  }
  if (!fmt_ok(fmt, ROLE_QUANTIZE)) return LQER_E_UNSUPPORTED;
  if (fmt->kind != LQER_Q_MXINT && fmt->kind != LQER_Q_INT && fmt->kind != LQER_Q_MINIFLOAT) {
    set_error("quantize_mxint: format is neither block_fp, integer nor minifloat");
    return LQER_E_INVALID;
  }
  if (fmt->kind == LQER_Q_MINIFLOAT && exps) {
    set_error("quantize_mxint: a minifloat format has no block exponents (exps must be NULL)");
    return LQER_E_INVALID;
  }
  if (codes && fmt->width > 8) {
    set_error("quantize_mxint: int8 codes need width <= 8");
    return LQER_E_UNSUPPORTED;
  }
  QP q = make_qp(*fmt);
  QuantOut o{deq_f32, codes, exps, nullptr, 0, 0};
  const int64_t L = (q.block <= 0 || q.block >= cols) ? cols : q.block;
  o.nblk = L > 0 ? (cols + L - 1) / L : 0;
  return quantize_dispatch(x, dtype, rows, cols, ld, q, o, (hipStream_t)stream);
}

int lqer_quantize_mxint_tiles(const void* x, int dtype, int64_t batches, int64_t rows, int64_t cols, const lqer_qfmt_t* fmt,
                              int64_t tile_rows, int64_t tile_cols, float* deq_f32, float* amax_scratch, void* stream) {
  if (batches < 0 || rows < 0 || cols < 0) {
    set_error("quantize_mxint_tiles: bad shape batches=%lld rows=%lld cols=%lld", (long long)batches, (long long)rows, (long long)cols);
    return LQER_E_INVALID;
  }
  if (batches * rows * cols == 0) return LQER_OK;
  if (!x || !deq_f32 || !amax_scratch) {
    set_error("quantize_mxint_tiles: null pointer");
    return LQER_E_INVALID;
  }
  if (!fmt_ok(fmt, ROLE_QUANTIZE_TILES)) return LQER_E_UNSUPPORTED;
  if (fmt->kind != LQER_Q_MXINT) {
    set_error("quantize_mxint_tiles: the format is not block_fp");
    return LQER_E_INVALID;
  }
  const int64_t R = (tile_rows <= 0 || tile_rows > rows) ? rows : tile_rows, L = (tile_cols <= 0 || tile_cols > cols) ? cols : tile_cols;
  return quantize_tiles_dispatch(x, dtype, batches, rows, cols, R, L, make_qp(*fmt), deq_f32, amax_scratch, (hipStream_t)stream);
}

int lqer_quantize_act_mxint(const void* x, int dtype, int64_t M, int64_t K, int64_t ldx, const lqer_qfmt_t* fmt,
                            void* xq_bf16, void* stream) {
  if ((!x || !xq_bf16) && M * K > 0) {
    set_error("quantize_act: null pointer");
    return LQER_E_INVALID;
  }
  if (M < 0 || K < 0 || ldx < K) {
    set_error("quantize_act: bad shape M=%lld K=%lld ldx=%lld", (long long)M, (long long)K, (long long)ldx);
    return LQER_E_INVALID;
  }
  if (!fmt_ok(fmt, ROLE_X)) return LQER_E_UNSUPPORTED;
  if (fmt->kind != LQER_Q_MXINT && fmt->kind != LQER_Q_INT && fmt->kind != LQER_Q_MINIFLOAT) {
    set_error("x_quantizer: only block_fp, integer and minifloat activations have a bf16 image on the HIP path");
    return LQER_E_UNSUPPORTED;
  }
  QP q = make_qp(*fmt);
  QuantOut o{nullptr, nullptr, nullptr, (bf16_t*)xq_bf16, lqer_padded_k(K), 0};
  return quantize_dispatch(x, dtype, M, K, ldx, q, o, (hipStream_t)stream);
}

int lqer_quantize_act_i8(const void* x, int dtype, int64_t M, int64_t K, int64_t ldx, const lqer_qfmt_t* fmt, void* xq_i8,
                         void* stream) {
  if ((!x || !xq_i8) && M * K > 0) {
    set_error("quantize_act_i8: null pointer");
    return LQER_E_INVALID;
  }
  if (M < 0 || K < 0 || ldx < K) {
    set_error("quantize_act_i8: bad shape M=%lld K=%lld ldx=%lld", (long long)M, (long long)K, (long long)ldx);
    return LQER_E_INVALID;
  }
  if (!fmt || (fmt->kind != LQER_Q_MXINT && fmt->kind != LQER_Q_MXINT_I8) || fmt->width < 2 || fmt->width > 8 ||
      !(fmt->block <= 0 || fmt->block >= K)) {
    set_error("quantize_act_i8: needs block_fp with width <= 8 and one block per row");
    return LQER_E_UNSUPPORTED;
  }
  lqer_qfmt_t f = *fmt;
  f.kind = LQER_Q_MXINT;
  f.block = -1;
  QuantOut o{nullptr, nullptr, nullptr, nullptr, 0, 0};
  o.xq8 = (int8_t*)xq_i8;
  o.cols_p8 = padded_k8(K);
  o.xscale = const_cast<float*>(i8_row_scales(xq_i8, M, K));
  return quantize_dispatch(x, dtype, M, K, ldx, make_qp(f), o, (hipStream_t)stream);
}

int lqer_i8_prepare(void* w_packed, int64_t N, int64_t K, const lqer_qfmt_t* w_fmt, int32_t* flags, void* stream) {
  if (!w_packed || !flags || !w_fmt || N <= 0 || K <= 0) {
    set_error("i8_prepare: bad argument");
    return LQER_E_INVALID;
  }
  lqer_linear_desc_t d;
  memset(&d, 0, sizeof(d));
  d.in_features = (int32_t)K, d.out_features = (int32_t)N;
  d.w_fmt = *w_fmt;
  d.x_fmt.kind = LQER_Q_MXINT_I8, d.x_fmt.width = 8, d.x_fmt.block = -1;
  if (!i8_formats_ok(&d)) return LQER_E_UNSUPPORTED;
  return i8_prepare_dispatch(w_packed, N, K, w_fmt->width - 1, (unsigned char*)w_packed + i8_image_offset(&d), flags,
                             (hipStream_t)stream);
}

int lqer_unpack_weight_i8(const void* w_packed, int64_t N, int64_t K, float* w_f32, void* stream) {
  if (!w_packed || !w_f32 || N <= 0 || K <= 0) {
    set_error("unpack_weight_i8: bad argument");
    return LQER_E_INVALID;
  }
  lqer_linear_desc_t d;
  memset(&d, 0, sizeof(d));
  d.in_features = (int32_t)K, d.out_features = (int32_t)N;
  return i8_unpack_dispatch((const unsigned char*)w_packed + i8_image_offset(&d), N, K, w_f32, (hipStream_t)stream);
}

int lqer_unpack_weight_i8_fmt(const void* w_packed, int64_t N, int64_t K, const lqer_qfmt_t* w_fmt, float* w_f32, void* stream) {
  if (!w_packed || !w_f32 || !w_fmt || N <= 0 || K <= 0) {
    set_error("unpack_weight_i8: bad argument");
    return LQER_E_INVALID;
  }
  lqer_linear_desc_t d;
  memset(&d, 0, sizeof(d));
  d.in_features = (int32_t)K, d.out_features = (int32_t)N;
  d.w_fmt = *w_fmt;
  return i8_unpack_dispatch((const unsigned char*)w_packed + i8_image_offset(&d), N, K, w_f32, (hipStream_t)stream, w_panel_limbs(&d) > 1);
}

// lqer_linear_sizes, and the carving its workspace is the total of (the forward goes on with it)
static int linear_sizes_carved(const lqer_linear_desc_t* d, int64_t m_max, lqer_linear_sizes_t* out, Carving* cv) {
  if (!d || !out || d->in_features <= 0 || d->out_features <= 0 || d->rank < 0 || m_max < 0)
    return fail(LQER_E_INVALID, "linear_sizes: bad descriptor");
  const size_t Kp = lqer_padded_k(d->in_features), Np = lqer_padded_n(d->out_features);
  const size_t rp = lqer_padded_r(d->rank), Mp = lqer_padded_m(m_max);
  if (!passthrough_width_ok(d->x_fmt, "x_quantizer") || (d->rank > 0 && !passthrough_width_ok(d->a_out_fmt, "A_out_quantizer")))
    return LQER_E_INVALID;
  const size_t xl = act_limbs(d), al = xa_limbs(d);  // pass-through activations: images repeated per limb
  const size_t wl = w_panel_limbs(d);
  if (!fmt_ok(&d->w_fmt, ROLE_W)) return LQER_E_UNSUPPORTED;
  out->w_packed = (Np / LQER_PANEL_ROWS) * (Kp / 64) * LQER_PANEL_BYTES * xl * wl;
  if (x_is_i8(d)) {
    if (!i8_formats_ok(d)) return LQER_E_UNSUPPORTED;
    out->w_packed = i8_image_offset(d) + (wl > 1 ? i8_weight8_image_bytes(d->out_features, d->in_features)
                                                 : i8_weight_image_bytes(d->out_features, d->in_features));
  }
  out->a_t = 3 * rp * Kp * 2 * xl;
  out->b_t = 3 * Np * rp * 2 * al;
  out->bias_q = Np * 4;
  *cv = carve(d, m_max);
  // (the int8 activation image + row scales of LQER_Q_MXINT_I8 fit the bf16 image's slot: K >= 128)
  if (x_is_i8(d) && i8_act_image_bytes(m_max, d->in_features) + Mp * sizeof(float) > cv->xaq)
    return fail(LQER_E_UNSUPPORTED, "linear_sizes: int8 activation image larger than the bf16 one (K %d)", d->in_features);
  out->workspace = cv->total;
  return LQER_OK;
}

int lqer_linear_sizes(const lqer_linear_desc_t* d, int64_t m_max, lqer_linear_sizes_t* out) {
  Carving cv;
  return linear_sizes_carved(d, m_max, out, &cv);
}

int lqer_pack_weight_mxint(const void* W, int dtype, int64_t N, int64_t K, int64_t ldw, const lqer_qfmt_t* fmt,
                           void* w_packed, void* scratch, void* stream) {
  if (!W || !w_packed || !scratch || N <= 0 || K <= 0 || ldw < K) {
    set_error("pack_weight: bad argument");
    return LQER_E_INVALID;
  }
  if (!fmt_ok(fmt, ROLE_W)) return LQER_E_UNSUPPORTED;
  if (fmt->kind != LQER_Q_MXINT && fmt->kind != LQER_Q_INT && fmt->kind != LQER_Q_MINIFLOAT) {
    set_error("w_quantizer: only block_fp, integer and minifloat weights can be packed");
    return LQER_E_UNSUPPORTED;
  }
  if (fmt->kind == LQER_Q_MINIFLOAT) {  // one scale byte for the whole image: the s of the table the GEMM will expand with
    uint32_t lut[2];
    int s;
    if (!mf_e4m3_table(*fmt, lut, &s)) {
      set_error("w_quantizer: minifloat(%d, %d, %d) has no e4m3 table", fmt->width, fmt->exp_width, fmt->exp_bias);
      return LQER_E_UNSUPPORTED;
    }
    return pack_weight_mf_dispatch(W, dtype, N, K, ldw, make_qp(*fmt), 127 + s, w_packed, (hipStream_t)stream);
  }
  return pack_weight_dispatch(W, dtype, N, K, ldw, make_qp(*fmt), 1, w_packed, scratch, (hipStream_t)stream);
}

int lqer_pack_weight_mxint_2d(const void* W, int dtype, int64_t N, int64_t K, int64_t ldw, const lqer_qfmt_t* fmt, int64_t block_rows,
                              void* w_packed, void* scratch, void* stream) {
  if (!W || !w_packed || !scratch || N <= 0 || K <= 0 || ldw < K) {
    set_error("pack_weight: bad argument");
    return LQER_E_INVALID;
  }
  if (!fmt_ok(fmt, ROLE_W)) return LQER_E_UNSUPPORTED;
  if (fmt->kind != LQER_Q_MXINT) {
    set_error("w_quantizer: only block_fp weights can be packed");
    return LQER_E_UNSUPPORTED;
  }
  return pack_weight_dispatch(W, dtype, N, K, ldw, make_qp(*fmt), block_rows == 0 ? -1 : block_rows, w_packed, scratch, (hipStream_t)stream);
}

int lqer_unpack_weight_mxint(const void* w_packed, int64_t N, int64_t K, const lqer_qfmt_t* fmt, float* w_f32,
                             void* stream) {
  if (!w_packed || !w_f32 || !fmt || N <= 0 || K <= 0) {
    set_error("unpack_weight: bad argument");
    return LQER_E_INVALID;
  }
  if (fmt->kind == LQER_Q_MINIFLOAT) {  // (the image's own e4m3 table and scale bytes, as the GEMM reads them)
    uint32_t lut[2];
    int s;
    if (!fmt_ok(fmt, ROLE_W) || !mf_e4m3_table(*fmt, lut, &s)) return LQER_E_UNSUPPORTED;
    return unpack_weight_mf_dispatch(w_packed, N, K, lut, w_f32, (hipStream_t)stream);
  }
  return unpack_weight_dispatch(w_packed, N, K, fmt->width - 1, fmt->kind == LQER_Q_INT, w_f32, (hipStream_t)stream);
}

int lqer_pack_lowrank(const void* A, const void* B, int dtype, int64_t K, int64_t N, int64_t r, void* a_t, void* b_t,
                      int32_t* limb_flags, void* stream) {
  if (!A || !B || !a_t || !b_t || !limb_flags || K <= 0 || N <= 0 || r <= 0) {
    set_error("pack_lowrank: bad argument");
    return LQER_E_INVALID;
  }
  return pack_lowrank_dispatch(A, B, dtype, K, N, r, a_t, b_t, limb_flags, (hipStream_t)stream);
}

int lqer_pack_bias(const void* bias, int dtype, int64_t N, const lqer_qfmt_t* fmt, float* bias_q, void* stream) {
  if (!bias || !bias_q || N <= 0) {
    set_error("pack_bias: bad argument");
    return LQER_E_INVALID;
  }
  if (!fmt_ok(fmt, ROLE_B)) return LQER_E_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  if (fmt->kind == LQER_Q_PASSTHROUGH) return bias_passthrough_dispatch(bias, dtype, N, bias_q, st);
  (void)hipMemsetAsync(bias_q, 0, lqer_padded_n(N) * sizeof(float), st);
  QP q = make_qp(*fmt);
  QuantOut o{bias_q, nullptr, nullptr, nullptr, 0, 0};
  return quantize_dispatch(bias, dtype, 1, N, N, q, o, st);
}

size_t lqer_lowrank_xa_scratch_bytes(const lqer_linear_desc_t* d, int64_t m_max) {
  return (d && d->rank > 0) ? xa_scratch_bytes(m_max, d->in_features, lqer_padded_r(d->rank)) : 0;
}

int lqer_lowrank_xa(const lqer_linear_desc_t* d, const void* xq, int64_t M, const void* a_t, int a_limbs, void* xaq,
                    void* scratch, size_t scratch_bytes, void* stream) {
  if (!d || !xq || !a_t || !xaq || M < 0 || d->rank <= 0) {
    set_error("lowrank_xa: bad argument");
    return LQER_E_INVALID;
  }
  if (!fmt_ok(&d->a_out_fmt, ROLE_A_OUT)) return LQER_E_UNSUPPORTED;
  if (!passthrough_width_ok(d->x_fmt, "x_quantizer") || !passthrough_width_ok(d->a_out_fmt, "A_out_quantizer")) return LQER_E_INVALID;
  if ((a_limbs < 0 || a_limbs > 3) && !(a_limbs == -1 && x_is_i8(d))) {
    set_error("lowrank_xa: a_limbs %d outside [0,3] (-1 = one fp16 image of A^T: the int8 route only)", a_limbs);
    return LQER_E_INVALID;
  }
  return lowrank_xa_dispatch((const bf16_t*)xq, M, d->in_features, x_is_f16(d) ? 0 : (x_is_i8(d) ? -1 : act_limbs(d)), (const bf16_t*)a_t, a_limbs, d->rank,
                             make_qp(d->a_out_fmt), d->a_out_fmt.kind == LQER_Q_PASSTHROUGH ? xa_limbs(d) : 0,
                             (bf16_t*)xaq, (float*)scratch, scratch_bytes, (hipStream_t)stream);
}

// lqer_linear_forward only: the GEMM call behind this one wants `bytes` at the head of the shared scratch zeroed (GemmPlan::prep_zero_bytes);
// `done` says whether a kernel of this call wrote the zeros (the one-launch int8 activation kernel does, the other routes do not)
struct AmaxZeroReq {
  void* p;       // head of the scratch the GEMM call will be handed
  size_t bytes;
  bool done;
};
// What a GEMM call of (d, M, dtype) launches: the kernel arguments that depend on the descriptor and the token count alone, and their
// plan.  Evaluated once per descriptor a call launches with and handed down (lqer_linear_forward -> linear_gemm_impl).
struct Planned {
  int rc;  // of gemm_shape_args (its text kept in p.msg: calls in between may leave their own)
  GemmArgs g;
  GemmPlan p;
};
static Planned plan_for(const lqer_linear_desc_t* d, int64_t M, int dtype, int b_limbs, bool for_launch = true, bool narrow = false);
static int plan_route(const Planned& pl);
// a call in front of the GEMM call can zero the pre-pass cells on its behalf (GemmPlan::prep_zero_bytes at the head of gemm_scratch): the
// int8 route's one-launch activation kernel
static bool can_prep_amax(const lqer_linear_desc_t* d, int64_t M, int a_limbs, const void* gemm_scratch) {
  return d && gemm_scratch && d->rank > 0 && x_is_i8(d) && a_limbs == -1 && M > 0;
}
static int quantize_act_xa_single(const lqer_linear_desc_t* d, const void* x, int dtype, int64_t M, int64_t ldx, const void* a_t,
                                  int a_limbs, void* xq, void* xaq, void* scratch, size_t scratch_bytes, void* stream, AmaxZeroReq* zr);
static int quantize_act_xa_impl(const lqer_linear_desc_t* d, const void* x, int dtype, int64_t M, int64_t ldx, const void* a_t,
                                int a_limbs, void* xq, void* xaq, void* scratch, size_t scratch_bytes, void* stream, AmaxZeroReq* zr);

int lqer_quantize_act_xa(const lqer_linear_desc_t* d, const void* x, int dtype, int64_t M, int64_t ldx, const void* a_t,
                         int a_limbs, void* xq, void* xaq, void* scratch, size_t scratch_bytes, void* stream) {
  return quantize_act_xa_impl(d, x, dtype, M, ldx, a_t, a_limbs, xq, xaq, scratch, scratch_bytes, stream, nullptr);
}

int lqer_quantize_act_xa_prep(const lqer_linear_desc_t* d, const void* x, int dtype, int64_t M, int64_t ldx, const void* a_t,
                              int a_limbs, void* xq, void* xaq, void* scratch, size_t scratch_bytes, void* gemm_scratch,
                              size_t* ready_bytes, void* stream) {
  if (ready_bytes) *ready_bytes = 0;
  AmaxZeroReq zr{ready_bytes ? gemm_scratch : nullptr, 0, false};
  if (can_prep_amax(d, M, a_limbs, zr.p)) {  // (a split-API call: the plan of the GEMM call that will follow)
    const Planned pl = plan_for(d, M, dtype, 0);
    if (pl.rc == LQER_OK) zr.bytes = pl.p.prep_zero_bytes;
  }
  const int rc = quantize_act_xa_impl(d, x, dtype, M, ldx, a_t, a_limbs, xq, xaq, scratch, scratch_bytes, stream, &zr);
  if (rc == LQER_OK && ready_bytes && zr.done) *ready_bytes = zr.bytes;
  return rc;
}

static int quantize_act_xa_impl(const lqer_linear_desc_t* d, const void* x, int dtype, int64_t M, int64_t ldx, const void* a_t,
                                int a_limbs, void* xq, void* xaq, void* scratch, size_t scratch_bytes, void* stream, AmaxZeroReq* zr) {
  if (!d || (!x && M > 0) || !xq || M < 0 || ldx < d->in_features) {
    set_error("quantize_act_xa: bad argument");
    return LQER_E_INVALID;
  }
  if (!fmt_ok(&d->w_fmt, ROLE_W)) return LQER_E_UNSUPPORTED;
  const int wl = w_limbs(d);
  if (wl == 1) return quantize_act_xa_single(d, x, dtype, M, ldx, a_t, a_limbs, xq, xaq, scratch, scratch_bytes, stream, zr);
  // a weight of three 4-bit limbs: the quantizer and the side GEMM work on the single-copy image behind the wide one, which is
  // then written as three copies side by side along k (one per weight limb) for the GEMM
  if (!passthrough_width_ok(d->x_fmt, "x_quantizer")) return LQER_E_INVALID;
  void* const one = act_single_copy(d, xq, M);
  const int rc = quantize_act_xa_single(d, x, dtype, M, ldx, a_t, a_limbs, one, xaq, scratch, scratch_bytes, stream, zr);
  if (rc || M == 0) return rc;
  return lqer_replicate_rows(one, xq, M, lqer_padded_k(d->in_features) * 2 * act_limbs(d), wl, stream);
}

static int quantize_act_xa_single(const lqer_linear_desc_t* d, const void* x, int dtype, int64_t M, int64_t ldx, const void* a_t,
                                  int a_limbs, void* xq, void* xaq, void* scratch, size_t scratch_bytes, void* stream, AmaxZeroReq* zr) {
  if (a_limbs == -2) {
    // the bf16 image of A^T with its fragment-major copy (lqer_a_b16_prepare): block-16 MXINT activations run quantizer + x A + A_out as
    // ONE launch where act16_fused.hip applies; everything else reads the image's first part as the one-limb image it is
    if (d->rank > 0 && a_t && xaq && xq && d->x_fmt.kind == LQER_Q_MXINT && fmt_ok(&d->x_fmt, ROLE_X) &&
        fmt_ok(&d->a_out_fmt, ROLE_A_OUT)) {
      const int rc = act16_fused_dispatch(x, dtype, M, d->in_features, ldx, make_qp(d->x_fmt), (bf16_t*)xq, a_t, d->rank, make_qp(d->a_out_fmt),
                                          (bf16_t*)xaq, d->tuning, (hipStream_t)stream);
      if (rc != LQER_E_UNSUPPORTED) return rc;
    }
    a_limbs = 1;
  }
  if (d->rank > 0 && a_t && !xaq) {  // partial tiles only: the GEMM reduces them (decode sizes)
    if (!decode_partials_ok(d, M)) {
      set_error("quantize_act_xa: xaq == NULL needs M <= 64, x / A_out block_fp in blocks of 16 (width <= 9), padded rank <= 64 "
                "and B_out pass-through or in blocks of 16");
      return LQER_E_INVALID;
    }
    const int rc = quant_xa_fused_dispatch(x, dtype, M, d->in_features, ldx, make_qp(d->x_fmt), (bf16_t*)xq, (const bf16_t*)a_t,
                                           a_limbs, d->rank, make_qp(d->a_out_fmt), nullptr, (float*)scratch, scratch_bytes,
                                           (hipStream_t)stream);
    if (rc == LQER_E_UNSUPPORTED) set_error("quantize_act_xa: scratch too small for the partial tiles");
    return rc == LQER_E_UNSUPPORTED ? LQER_E_WORKSPACE : rc;
  }
  if (d->rank > 0 && a_t && xaq) {
    if (!fmt_ok(&d->x_fmt, ROLE_X) || !fmt_ok(&d->a_out_fmt, ROLE_A_OUT)) return LQER_E_UNSUPPORTED;
    const int rc = quant_xa_fused_dispatch(x, dtype, M, d->in_features, ldx, make_qp(d->x_fmt), (bf16_t*)xq,
                                           (const bf16_t*)a_t, a_limbs, d->rank, make_qp(d->a_out_fmt), (bf16_t*)xaq,
                                           (float*)scratch, scratch_bytes, (hipStream_t)stream);
    if (rc != LQER_E_UNSUPPORTED) return rc;
  }
  int rc;
  if (x_is_f16(d)) {
    if (!need_f16(d, dtype, "quantize_act_xa")) return LQER_E_INVALID;
    if (xq == x) {  // the tensor itself is the image: nothing to write
      if (!f16_image_is_input(d, x, M, ldx, M <= 64 ? lqer_gemm_route(d, M, LQER_F16) : LQER_ROUTE_TILE128)) {
        set_error("quantize_act_xa: xq == x needs a dense fp16 tensor with K %% %d == 0, M %% %d == 0 or M <= 64, 16-byte aligned",
                  LQER_K_ALIGN, LQER_M_ALIGN);
        return LQER_E_INVALID;
      }
      rc = LQER_OK;
    } else {
      rc = copy_act_f16_dispatch(x, M, d->in_features, ldx, (bf16_t*)xq, (hipStream_t)stream);
    }
  } else if (d->x_fmt.kind == LQER_Q_PASSTHROUGH) {
    if (!passthrough_width_ok(d->x_fmt, "x_quantizer")) return LQER_E_INVALID;
    rc = split_act_dispatch(x, dtype, M, d->in_features, ldx, act_limbs(d), (bf16_t*)xq, (hipStream_t)stream);
  } else if (x_is_i8(d)) {
    // one launch for quantizer + x A + A_out where the fused kernel applies (act8_fused.hip: 16-bit tensor, fp16 image of A^T with
    // its fragment-major copy, small token counts); else quantizer, split-K side GEMM and reduce as three launches
    if (d->rank > 0 && a_t && xaq && a_limbs == -1) {
      lqer_qfmt_t fx = d->x_fmt;
      fx.kind = LQER_Q_MXINT, fx.block = -1;
      const bool zreq = zr && zr->bytes > 0 && zr->p;
      bool zeroed = false;
      rc = act8_fused_dispatch(x, dtype, M, d->in_features, ldx, make_qp(fx), xq, a_t, d->rank, make_qp(d->a_out_fmt), (bf16_t*)xaq,
                               d->tuning, (hipStream_t)stream, zreq ? (float*)zr->p : nullptr, zreq ? zr->bytes : 0, &zeroed);
      if (rc == LQER_OK && zr) zr->done = zeroed;
      if (rc != LQER_E_UNSUPPORTED) return rc;
    }
    rc = lqer_quantize_act_i8(x, dtype, M, d->in_features, ldx, &d->x_fmt, xq, stream);
  } else {
    rc = lqer_quantize_act_mxint(x, dtype, M, d->in_features, ldx, &d->x_fmt, xq, stream);
  }
  if (rc || d->rank <= 0) return rc;
  return lqer_lowrank_xa(d, xq, M, a_t, a_limbs, xaq, scratch, scratch_bytes, stream);
}

size_t lqer_act_image_bytes(const lqer_linear_desc_t* d, int64_t m_max) {
  return (d && m_max >= 0 && d->in_features > 0) ? carve(d, m_max).xaq : 0;
}

size_t lqer_linear_gemm_scratch_bytes(const lqer_linear_desc_t* d, int64_t m_max) {
  if (!d || d->rank <= 0 || d->b_out_fmt.kind != LQER_Q_MXINT) return 0;
  return gemm_scratch_bytes(m_max, d->out_features, make_qp(d->b_out_fmt));
}

int lqer_linear_gemm(const lqer_linear_desc_t* d, const void* xq, int64_t M, const void* w_packed, const void* xaq,
                     const void* b_t, int b_limbs, const float* bias_q, void* y, int dtype, int64_t ldy, void* scratch,
                     size_t scratch_bytes, void* stream) {
  return lqer_linear_gemm_ld(d, xq, M, w_packed, xaq, d ? xaq_row_elems(d) : 0, b_t, b_limbs, bias_q, y,
                             dtype, ldy, scratch, scratch_bytes, stream);
}

// fills the kernel arguments that depend on the descriptor and the token count alone (shapes, formats, limb counts)
static int gemm_shape_args(const lqer_linear_desc_t* d, int64_t M, int dtype, GemmArgs& g) {
  const bool lowrank = d->rank > 0;
  if (!fmt_ok(&d->w_fmt, ROLE_W)) return LQER_E_UNSUPPORTED;
  if (lowrank && !fmt_ok(&d->b_out_fmt, ROLE_B_OUT)) return LQER_E_UNSUPPORTED;
  if (!passthrough_width_ok(d->x_fmt, "x_quantizer") || (lowrank && !passthrough_width_ok(d->a_out_fmt, "A_out_quantizer")))
    return LQER_E_INVALID;
  if (!need_f16(d, dtype, "linear_gemm")) return LQER_E_INVALID;
  const int xl = act_limbs(d), al = lowrank ? xa_limbs(d) : 1;
  g.M = (int)M;
  g.N = d->out_features;
  g.Np = (int)lqer_padded_n(d->out_features);
  g.x_f16 = x_is_f16(d) ? 1 : 0;
  // activation limbs side by side along k with the weight image repeated to match - and the other way round for the three
  // 4-bit limbs of a 5..8-bit weight
  g.Kp = (int)lqer_padded_k(d->in_features) * xl * w_limbs(d);
  g.rp = (int)lqer_padded_r(d->rank) * al;
  g.w_mbits = w_limbs(d) > 1 ? 3 : d->w_fmt.width - 1;
  g.tuning = d->tuning;
  g.w_twos = d->w_fmt.kind == LQER_Q_INT ? 1 : 0;
  if (d->w_fmt.kind == LQER_Q_MINIFLOAT) {  // minifloat weights: the nibble's magnitude code through the format's e4m3 table
    int s;
    if (x_is_f16(d) || x_is_i8(d))
      return fail(LQER_E_UNSUPPORTED, "linear_gemm: minifloat weights run the bf16 128-row tile kernel only (x_quantizer %s)",
                  x_is_f16(d) ? "LQER_Q_PASSTHROUGH_F16: use LQER_Q_PASSTHROUGH" : "LQER_Q_MXINT_I8: use LQER_Q_MXINT");
    if (!mf_e4m3_table(d->w_fmt, g.w_lut, &s)) return LQER_E_UNSUPPORTED;
    g.w_mf = 1;
  }
  // sign-magnitude nibbles whose image holds an exponent byte the table-free expand cannot carry (expand_frag_lin): the table
  // instantiations, with the integers 0..7 as the table (expand_frag's own).  The fp16 and int8 main loops expand otherwise.
  if ((d->tuning & LQER_TUNE_W_EXP_TABLE) && d->w_fmt.kind == LQER_Q_MXINT && !x_is_f16(d) && !x_is_i8(d)) {
    g.w_lut[0] = 0x44403800u, g.w_lut[1] = 0x4E4C4A48u;
    g.w_mf = 1;
  }
  if (lowrank && d->b_out_fmt.kind == LQER_Q_MINIFLOAT && (x_is_i8(d) || x_is_f16(d)))
    return fail(LQER_E_UNSUPPORTED, "linear_gemm: a minifloat B_out runs on the bf16 128-row tile kernel only (x_quantizer %s)",
                x_is_f16(d) ? "LQER_Q_PASSTHROUGH_F16: use LQER_Q_PASSTHROUGH with width 11" : "LQER_Q_MXINT_I8: use LQER_Q_MXINT");
  if (lowrank) g.bout = make_qp(d->b_out_fmt);
  if (x_is_i8(d)) {
    if (!i8_formats_ok(d)) return LQER_E_UNSUPPORTED;
    g.Kp = (int)padded_k8(d->in_features);  // row stride of the int8 activation image
    g.i8_shift = !(d->w_fmt.block <= 0 || d->w_fmt.block >= d->in_features);  // one weight block per row: no shifts at all
    g.w_i8codes = w_panel_limbs(d) > 1 ? 1 : 0;  // weights of 5..8 bits: the image holds the codes, one exponent per row (lqer_i8_prepare checked)
    if (g.w_i8codes) g.i8_shift = 0;
  }
  return LQER_OK;
}

// for_launch = false (the route queries): no HIP call - the CU count, which only the travel of the row maxima depends on, is not asked
// narrow: w_packed is the compact image of a 2- / 3-bit weight (the _narrow entry points)
static Planned plan_for(const lqer_linear_desc_t* d, int64_t M, int dtype, int b_limbs, bool for_launch, bool narrow) {
  Planned pl;
  memset(&pl.g, 0, sizeof(pl.g));
  pl.rc = gemm_shape_args(d, M, dtype, pl.g);
  pl.g.b_limbs = b_limbs;
  if (pl.rc == LQER_OK && narrow) pl.rc = narrow_args(d, pl.g);
  if (pl.rc == LQER_OK) {
    // (the device's CUs decide one thing: whether the int8 kernel exchanges the row maxima of a wide-block B_out itself)
    const bool asks_cus = for_launch && x_is_i8(d) && d->rank > 0 && d->b_out_fmt.kind == LQER_Q_MXINT && d->b_out_fmt.block != 16;
    pl.p = plan_gemm(pl.g, d->rank > 0, x_is_i8(d), dtype, asks_cus ? device_cus() : 0);
  } else {
    pl.p = GemmPlan{};
    snprintf(pl.p.msg, sizeof(pl.p.msg), "%s", g_err);
  }
  return pl;
}

// LQER_ROUTE_* of the plan, or the refusal the route queries report (with its text)
static int plan_route(const Planned& pl) {
  const int rc = pl.rc ? pl.rc : pl.p.err;
  if (rc) set_error("%s", pl.p.msg);
  return rc ? rc : pl.p.route;
}

int lqer_gemm_route(const lqer_linear_desc_t* d, int64_t M, int dtype) {
  if (!d || M < 0) return fail(LQER_E_INVALID, "gemm_route: bad argument");
  return plan_route(plan_for(d, M, dtype, 0, false));
}

int lqer_gemm_tile_rows(const lqer_linear_desc_t* d, int64_t M, int dtype) {
  if (!d || M < 0) return fail(LQER_E_INVALID, "gemm_tile_rows: bad argument");
  const Planned pl = plan_for(d, M, dtype, 0, false);
  const int route = plan_route(pl);
  return route < 0 ? route : pl.p.tile_rows;
}

// The operands of ONE Linear in a launch, written once: as the one-launch decode kernel's table entry, and from it as the per-call part
// of GemmArgs (linear_gemm_impl; the one-launch branch of the forward and the group hand the entries to decode1_dispatch)
static DecodeMember member_of(const lqer_linear_desc_t* d, const void* w_packed, const void* b_t, int b_limbs, const float* bias_q, void* y,
                              int64_t ldy) {
  return DecodeMember{(const uint8_t*)w_packed, (const bf16_t*)b_t, d->has_bias ? bias_q : nullptr, y, ldy, d->out_features,
                      (int)lqer_padded_n(d->out_features), (int)xaq_row_elems(d), b_limbs};
}
static void fill_call(GemmArgs& g, const DecodeMember& m) {
  g.wp = m.wp, g.bt = m.bt, g.bias = m.bias, g.y = m.y, g.ldy = m.ldy, g.b_limbs = m.b_limbs;
}

static int linear_gemm_impl(const lqer_linear_desc_t* d, const void* xq, int64_t M, const void* w_packed, const void* xaq,
                            int64_t xaq_ld, const void* b_t, int b_limbs, const float* bias_q, void* y, int dtype, int64_t ldy,
                            void* scratch, size_t scratch_bytes, void* stream, bool amax_zeroed, const Planned* pl, bool narrow = false) {
  if (!d || !xq || !w_packed || !y || M < 0 || ldy < d->out_features) return fail(LQER_E_INVALID, "linear_gemm: bad argument");
  const bool lowrank = d->rank > 0;
  const bool from_partials = lowrank && !xaq && b_t && scratch && decode_partials_ok(d, M);
  if (lowrank && ((!xaq && !from_partials) || !b_t))
    return fail(LQER_E_INVALID, "linear_gemm: rank %d but no side-path operands (xaq == NULL: only the decode route, see lqer_decode_partials)", d->rank);
  if (b_limbs < 0 || b_limbs > 3) return fail(LQER_E_INVALID, "linear_gemm: b_limbs %d outside [0,3]", b_limbs);
  Planned own;
  if (!pl) own = plan_for(d, M, dtype, b_limbs, true, narrow), pl = &own;
  if (pl->rc) return fail(pl->rc, "%s", pl->p.msg);
  if (lowrank && !from_partials && (xaq_ld < xaq_row_elems(d) || xaq_ld % 8 != 0 || ((uintptr_t)xaq & 15) != 0))
    return fail(LQER_E_INVALID, "linear_gemm: xaq row stride %lld (elements) must be a multiple of 8 and at least the padded rank %lld, "
                "xaq 16-byte aligned", (long long)xaq_ld, (long long)lqer_padded_r(d->rank));
  GemmArgs g = pl->g;
  fill_call(g, member_of(d, w_packed, b_t, b_limbs, bias_q, y, ldy));
  g.xq = (const bf16_t*)xq;
  g.xaq = (const bf16_t*)xaq;
  g.xaq_ld = (int)xaq_ld;
  if (x_is_i8(d)) {
    g.w8 = (const uint8_t*)w_packed + i8_image_offset(d);
    g.xscale = i8_row_scales(xq, M, d->in_features);
  }
  if (from_partials) {
    xa_fused_plan(M, d->in_features, d->rank, &g.xa_nchunk, &g.xa_cstride);
    if (scratch_bytes < (size_t)g.xa_nchunk * g.xa_cstride * sizeof(float))
      return fail(LQER_E_WORKSPACE, "linear_gemm: scratch %zu B does not hold the partial tiles of x A", scratch_bytes);
    g.xa_part = (const float*)scratch;
    g.aout = make_qp(d->a_out_fmt);
  }
  return gemm_launch(pl->p, g, dtype, scratch, scratch_bytes, amax_zeroed, (hipStream_t)stream);
}

int lqer_linear_gemm_ld(const lqer_linear_desc_t* d, const void* xq, int64_t M, const void* w_packed, const void* xaq,
                        int64_t xaq_ld, const void* b_t, int b_limbs, const float* bias_q, void* y, int dtype, int64_t ldy,
                        void* scratch, size_t scratch_bytes, void* stream) {
  return linear_gemm_impl(d, xq, M, w_packed, xaq, xaq_ld, b_t, b_limbs, bias_q, y, dtype, ldy, scratch, scratch_bytes, stream, false, nullptr);
}

int lqer_linear_gemm_prepared(const lqer_linear_desc_t* d, const void* xq, int64_t M, const void* w_packed, const void* xaq,
                              const void* b_t, int b_limbs, const float* bias_q, void* y, int dtype, int64_t ldy, void* scratch,
                              size_t scratch_bytes, size_t ready_bytes, void* stream) {
  bool zeroed = false;
  Planned pl;
  const bool planned = ready_bytes > 0 && can_prep_amax(d, M, -1, scratch);  // (a_limbs = -1: met by whoever prepared the cells)
  if (planned) {  // covers this launch's cells?
    pl = plan_for(d, M, dtype, b_limbs);
    zeroed = pl.rc == LQER_OK && pl.p.prep_zero_bytes > 0 && ready_bytes >= pl.p.prep_zero_bytes;
  }
  return linear_gemm_impl(d, xq, M, w_packed, xaq, d ? xaq_row_elems(d) : 0, b_t, b_limbs, bias_q, y, dtype, ldy,
                          scratch, scratch_bytes, stream, zeroed, planned ? &pl : nullptr);
}

// "The one-launch decode kernel (decode1.hip) takes this call" - asked by lqer_linear_forward, by lqer_weight_narrow_route and, per
// member, by lqer_linear_forward_group.  The limits are the kernel's own (d1:: in common.h).  What only its dispatch can say - K a
// multiple of d1::K_STEP, a token image that fits the LDS, the scratch - it answers with LQER_E_UNSUPPORTED, and every caller goes its
// own way from there.  First the form for a query, which has no pointer; then the call's.
static bool decode1_takes(const lqer_linear_desc_t* d, int64_t M, int dtype, int64_t ldx, int a_limbs, int b_limbs) {
  const int esz = dtype == LQER_F32 ? 4 : 2;
  return M <= d1::MAXM && a_limbs == 1 && !x_is_f16(d) && (ldx * esz) % 16 == 0 && b_limbs >= 1 && b_limbs <= 3 && decode_partials_ok(d, M);
}
static bool decode1_takes(const lqer_linear_desc_t* d, int64_t M, int dtype, const void* x, int64_t ldx, int a_limbs, int b_limbs) {
  return ((uintptr_t)x & 15) == 0 && decode1_takes(d, M, dtype, ldx, a_limbs, b_limbs);
}
// ... and its launch for the Linears `mem`, which are handed the same tokens: `shared` = the arguments of (d, M) that do not depend on
// the Linear (gemm_shape_args), A_out and the B_out form are d's
static int decode1_call(const GemmArgs& shared, const lqer_linear_desc_t* d, int dtype, const void* x, int64_t ldx, const void* a_t,
                        const DecodeMember* mem, int nmem, void* scratch, size_t scratch_bytes, void* stream) {
  GemmArgs g = shared;
  g.aout = make_qp(d->a_out_fmt);
  const int bout = d->b_out_fmt.kind == LQER_Q_PASSTHROUGH ? 0 : 1;  // (decode_partials_ok: pass-through or blocks of 16)
  return decode1_dispatch(g, dtype, x, ldx, d->in_features, make_qp(d->x_fmt), (const bf16_t*)a_t, bout, mem, nmem, scratch, scratch_bytes,
                          (hipStream_t)stream);
}

// what lqer_linear_forward / lqer_linear_forward_narrow are handed besides the descriptor and the weight image
struct FwdArgs {
  const void* x; int dtype; int64_t M, ldx;
  const void *a_t, *b_t; int a_limbs, b_limbs;
  const float* bias_q; void* y; int64_t ldy;
  void* workspace; size_t workspace_bytes; void* stream;
};

// The forward of descriptor d on the weight image w_packed (narrow: the compact one, read by the plan's kernel directly) under its
// plan pl, on the carving cv
static int forward_body(const lqer_linear_desc_t* d, const void* w_packed, bool narrow, const Planned& pl, const Carving& cv, const FwdArgs& a) {
  if (a.workspace_bytes < cv.total || (!a.workspace && cv.total))
    return fail(LQER_E_WORKSPACE, "linear_forward: workspace %zu B < %zu B needed for M=%lld", a.workspace_bytes, cv.total, (long long)a.M);
  if (a.M == 0) return LQER_OK;
  unsigned char* const ws = (unsigned char*)a.workspace;
  HT_MARK(1);
  const bool x_is_image = a.dtype == LQER_F16 && f16_image_is_input(d, a.x, a.M, a.ldx, plan_route(pl));  // no copy (never written)
  void* const xq = x_is_image ? const_cast<void*>(a.x) : ws;
  HT_MARK(2);
  void *const xaq = ws + cv.xaq, *const scratch = ws + cv.scratch;
  const bool sides = a.a_t && a.b_t;
  const bool one_launch = sides && decode1_takes(d, a.M, a.dtype, a.x, a.ldx, a.a_limbs, a.b_limbs);
  if (one_launch || (sides && decode_partials_ok(d, a.M))) {
    HT_MARK(3);
    const size_t nscr = cv.side_bytes;
    HT_MARK(4);
    // up to 8 tokens: ONE launch (decode1.hip) - producer workgroups publish the partial tiles of x A, the weight-streaming
    // workgroups quantize x themselves and pick the tiles up at their very end
    // (capturable: the kernel mixes its dispatch id into the granule tag, so a replayed graph node never accepts the
    // previous replay's tiles although its arguments - the host's per-call counter among them - are frozen)
    if (one_launch) {
      if (pl.rc) return fail(pl.rc, "%s", pl.p.msg);
      HT_MARK(5);
      const DecodeMember one = member_of(d, w_packed, a.b_t, a.b_limbs, a.bias_q, a.y, a.ldy);
      const int rc = decode1_call(pl.g, d, a.dtype, a.x, a.ldx, a.a_t, &one, 1, scratch, nscr, a.stream);
      HT_MARK(6);
      HT_DONE();
      if (rc != LQER_E_UNSUPPORTED) return rc;
    }
    // two launches: the GEMM sums the partial tiles of x A itself
    const int rc = lqer_quantize_act_xa(d, a.x, a.dtype, a.M, a.ldx, a.a_t, a.a_limbs, xq, nullptr, scratch, nscr, a.stream);
    if (rc) return rc;
    return linear_gemm_impl(d, xq, a.M, w_packed, nullptr, xaq_row_elems(d), a.b_t, a.b_limbs, a.bias_q, a.y, a.dtype, a.ldy, scratch, nscr,
                            a.stream, false, &pl, narrow);
  }
  // (a pre-pass on atomicMax cells behind the one-launch int8 activation kernel: that kernel zeroes the cells - the two calls share the
  // scratch, whose size is the larger of their needs - instead of a memset launch between them)
  AmaxZeroReq zr{a.b_t ? scratch : nullptr, 0, false};
  if (can_prep_amax(d, a.M, a.a_limbs, zr.p) && pl.rc == LQER_OK) zr.bytes = pl.p.prep_zero_bytes;
  const int rc = quantize_act_xa_impl(d, a.x, a.dtype, a.M, a.ldx, a.a_t, a.a_limbs, xq, xaq, scratch, cv.side_bytes, a.stream, &zr);
  if (rc) return rc;
  return linear_gemm_impl(d, xq, a.M, w_packed, d->rank > 0 ? xaq : nullptr, xaq_row_elems(d), a.b_t, a.b_limbs, a.bias_q, a.y, a.dtype, a.ldy,
                          scratch, cv.gemm_bytes, a.stream, zr.done, &pl, narrow);
}

// Step in front of the body: token counts the int8 tile kernel does not serve run the bf16 kernels on the sign-magnitude image (same
// buffers, same carving but for the single-copy image, which only the split calls place) - a second descriptor, a second plan
static int forward_planned(const lqer_linear_desc_t* d, const void* w_packed, bool narrow, const Planned& pl, const Carving& cv, const FwdArgs& a) {
  if (!x_is_i8(d) || plan_route(pl) == LQER_ROUTE_I8) return forward_body(d, w_packed, narrow, pl, cv, a);
  lqer_linear_desc_t plain = *d;
  plain.x_fmt.kind = LQER_Q_MXINT;
  return forward_body(&plain, w_packed, narrow, plan_for(&plain, a.M, a.dtype, a.b_limbs), cv, a);
}

// the standard image of the compact image w_narrow, whose plan is pl, written to `wide` (std_image_bytes)
static int widen_for(const lqer_linear_desc_t* d, const Planned& pl, const void* w_narrow, void* wide, void* stream) {
  return weight_widen_dispatch(w_narrow, d->out_features, d->in_features, d->w_fmt.width, pl.g.w_narrow & 0xff, wide, (hipStream_t)stream);
}

// Step in front of the body: a compact image on a route whose kernel reads standard panels is widened into the workspace behind the
// standard carving, and the call goes on as the standard image's
static int forward_widened(const lqer_linear_desc_t* d, const void* w_narrow, const Planned& pl, const Carving& cv, const FwdArgs& a) {
  if (!a.workspace || a.workspace_bytes < cv.widened + std_image_bytes(d))
    return fail(LQER_E_WORKSPACE, "linear_forward_narrow: workspace %zu B < %zu B needed for M=%lld (the widened weight image included)", a.workspace_bytes,
                cv.widened + std_image_bytes(d), (long long)a.M);
  if (a.M == 0) return LQER_OK;
  void* const wide = (unsigned char*)a.workspace + cv.widened;
  const int rc = widen_for(d, pl, w_narrow, wide, a.stream);
  if (rc) return rc;
  return forward_planned(d, wide, false, plan_for(d, a.M, a.dtype, a.b_limbs), cv, a);
}

// narrow: w_packed is the compact image (lqer_linear_forward_narrow).  Routes whose kernel reads it directly go on with the plan's
// w_img; every other route widens it first.
static int linear_forward_impl(const lqer_linear_desc_t* d, const void* w_packed, bool narrow, const FwdArgs& a) {
  if (!d) return fail(LQER_E_INVALID, "linear_forward: null descriptor");
  HT_START();
  lqer_linear_sizes_t sz;
  Carving cv;
  const int rc = linear_sizes_carved(d, a.M, &sz, &cv);
  if (rc) return rc;
  HT_MARK(0);
  // the one plan of this forward (its refusals are reported where the GEMM call reports them)
  const Planned pl = plan_for(d, a.M, a.dtype, a.b_limbs, true, narrow);
  if (narrow) {
    if (plan_route(pl) < 0) return pl.rc ? pl.rc : pl.p.err;
    if (pl.p.w_img < 0) return forward_widened(d, w_packed, pl, cv, a);
  }
  return forward_planned(d, w_packed, narrow, pl, cv, a);
}

int lqer_linear_forward(const lqer_linear_desc_t* d, const void* x, int dtype, int64_t M, int64_t ldx,
                        const void* w_packed, const void* a_t, const void* b_t, int a_limbs, int b_limbs,
                        const float* bias_q, void* y, int64_t ldy, void* workspace, size_t workspace_bytes,
                        void* stream) {
  return linear_forward_impl(d, w_packed, false, FwdArgs{x, dtype, M, ldx, a_t, b_t, a_limbs, b_limbs, bias_q, y, ldy, workspace, workspace_bytes, stream});
}

// ---- the compact image of 2- / 3-bit block_fp weights (include/lqer_hip.h "compact weight image") -----------------------------------
size_t lqer_weight_narrow_bytes(int64_t N, int64_t K, const lqer_qfmt_t* w_fmt) { return narrow_bytes(N, K, w_fmt); }

static int narrow_conv_check(const char* who, const void* a, const void* b, int64_t N, int64_t K, const lqer_qfmt_t* f) {
  if (!a || !b || !f || N <= 0 || K <= 0 || ((uintptr_t)a & 15) || ((uintptr_t)b & 15))
    return fail(LQER_E_INVALID, "%s: bad argument (null pointer, non-positive size, or an image that is not 16-byte aligned)", who);
  if (!narrow_exps(f, K))
    return fail(LQER_E_UNSUPPORTED, "%s: the compact image holds block_fp weights of width 2 or 3 (kind %d width %d)", who, f->kind, f->width);
  return LQER_OK;
}

int lqer_weight_narrow(const void* w_packed, int64_t N, int64_t K, const lqer_qfmt_t* w_fmt, void* w_narrow, void* stream) {
  const int rc = narrow_conv_check("weight_narrow", w_packed, w_narrow, N, K, w_fmt);
  return rc ? rc : weight_narrow_dispatch(w_packed, N, K, w_fmt->width, narrow_exps(w_fmt, K), w_narrow, (hipStream_t)stream);
}

int lqer_weight_widen(const void* w_narrow, int64_t N, int64_t K, const lqer_qfmt_t* w_fmt, void* w_packed, void* stream) {
  const int rc = narrow_conv_check("weight_widen", w_narrow, w_packed, N, K, w_fmt);
  return rc ? rc : weight_widen_dispatch(w_narrow, N, K, w_fmt->width, narrow_exps(w_fmt, K), w_packed, (hipStream_t)stream);
}

int lqer_weight_narrow_host(const void* w_packed, int64_t N, int64_t K, const lqer_qfmt_t* w_fmt, void* w_narrow) {
  const int rc = narrow_conv_check("weight_narrow_host", w_packed, w_narrow, N, K, w_fmt);
  if (rc) return rc;
  if (!weight_narrow_host((const uint8_t*)w_packed, N, K, w_fmt->width, narrow_exps(w_fmt, K), (uint8_t*)w_narrow))
    return fail(LQER_E_INVALID, "weight_narrow_host: not the standard image of a width-%d weight in blocks of %d (a magnitude bit above bit %d, or "
                "exponent bytes of one block that differ): widening would not give it back", w_fmt->width, w_fmt->block, w_fmt->width - 2);
  return LQER_OK;
}

int lqer_weight_widen_host(const void* w_narrow, int64_t N, int64_t K, const lqer_qfmt_t* w_fmt, void* w_packed) {
  const int rc = narrow_conv_check("weight_widen_host", w_narrow, w_packed, N, K, w_fmt);
  if (rc) return rc;
  weight_widen_host((const uint8_t*)w_narrow, N, K, w_fmt->width, narrow_exps(w_fmt, K), (uint8_t*)w_packed);
  return LQER_OK;
}

int lqer_weight_narrow_route(const lqer_linear_desc_t* d, int64_t M, int dtype, int64_t ldx, int a_limbs, int b_limbs) {
  if (!d || M < 0) return fail(LQER_E_INVALID, "weight_narrow_route: bad argument");
  const Planned pl = plan_for(d, M, dtype, b_limbs, false, true);
  const int route = plan_route(pl);
  if (route < 0) return route;
  if (pl.p.w_img < 0) return LQER_NARROW_WIDEN;
  // (a query answers for the kernel's dispatch as well, which the forward simply asks: K in whole steps)
  const bool one = decode1_takes(d, M, dtype, ldx, a_limbs, b_limbs) && d->in_features % d1::K_STEP == 0;
  return one ? LQER_NARROW_DIRECT_ONE_LAUNCH : LQER_NARROW_DIRECT;
}

// does a token count up to m_max reach a route that widens?  Decode sizes share one answer (the small-M route does not depend on M
// below 65), every larger count takes a tile kernel.
static bool narrow_may_widen(const lqer_linear_desc_t* d, int64_t m_max) {
  if (m_max > SM_MAX_M) return true;
  const Planned pl = plan_for(d, m_max > 0 ? m_max : 1, LQER_F16, 0, false, true);
  return pl.rc == LQER_OK && !pl.p.err && pl.p.w_img < 0;
}

size_t lqer_linear_forward_narrow_workspace_bytes(const lqer_linear_desc_t* d, int64_t m_max) {
  lqer_linear_sizes_t sz;
  Carving cv;
  if (!d || linear_sizes_carved(d, m_max, &sz, &cv)) return 0;
  GemmArgs g;
  memset(&g, 0, sizeof(g));
  if (narrow_args(d, g)) return 0;
  return narrow_may_widen(d, m_max) ? cv.widened + std_image_bytes(d) : cv.total;
}

int lqer_linear_forward_narrow(const lqer_linear_desc_t* d, const void* x, int dtype, int64_t M, int64_t ldx, const void* w_narrow,
                               const void* a_t, const void* b_t, int a_limbs, int b_limbs, const float* bias_q, void* y, int64_t ldy,
                               void* workspace, size_t workspace_bytes, void* stream) {
  return linear_forward_impl(d, w_narrow, true, FwdArgs{x, dtype, M, ldx, a_t, b_t, a_limbs, b_limbs, bias_q, y, ldy, workspace, workspace_bytes, stream});
}

int lqer_linear_gemm_narrow(const lqer_linear_desc_t* d, const void* xq, int64_t M, const void* w_narrow, const void* xaq, int64_t xaq_ld,
                            const void* b_t, int b_limbs, const float* bias_q, void* y, int dtype, int64_t ldy, void* scratch,
                            size_t scratch_bytes, void* widen_scratch, size_t widen_bytes, void* stream) {
  if (!d || !w_narrow || M < 0) return fail(LQER_E_INVALID, "linear_gemm_narrow: bad argument");
  const Planned pl = plan_for(d, M, dtype, b_limbs, true, true);
  if (plan_route(pl) < 0) return pl.rc ? pl.rc : pl.p.err;
  if (pl.p.w_img >= 0)
    return linear_gemm_impl(d, xq, M, w_narrow, xaq, xaq_ld, b_t, b_limbs, bias_q, y, dtype, ldy, scratch, scratch_bytes, stream, false, &pl, true);
  if (!widen_scratch || widen_bytes < std_image_bytes(d) || ((uintptr_t)widen_scratch & 15))
    return fail(LQER_E_WORKSPACE, "linear_gemm_narrow: M=%lld takes a kernel that reads standard panels: widen_scratch %zu B < %zu B (16-byte aligned)",
                (long long)M, widen_bytes, std_image_bytes(d));
  if (M == 0) return LQER_OK;
  const int rc = widen_for(d, pl, w_narrow, widen_scratch, stream);
  if (rc) return rc;
  return linear_gemm_impl(d, xq, M, widen_scratch, xaq, xaq_ld, b_t, b_limbs, bias_q, y, dtype, ldy, scratch, scratch_bytes, stream, false,
                          nullptr);
}

size_t lqer_group_workspace_bytes(int64_t K, int64_t rank_padded_sum) {
  return (K > 0 && rank_padded_sum > 0) ? (decode1_scratch_bytes(lqer_padded_k(K), (int)rank_padded_sum) + 255) / 256 * 256 : 0;
}

int lqer_linear_forward_group(const lqer_group_member_t* members, int n_members, const void* x, int dtype, int64_t M, int64_t ldx,
                              const void* a_t_cat, int a_limbs, void* workspace, size_t workspace_bytes, void* stream) {
  if (!members || n_members < 1 || !x || !a_t_cat || !workspace || M < 0) return fail(LQER_E_INVALID, "linear_forward_group: bad argument");
  if (M == 0) return LQER_OK;
  const lqer_linear_desc_t* d0 = members[0].desc;
  auto same = [](const lqer_qfmt_t& a, const lqer_qfmt_t& b) {
    return a.kind == b.kind && a.width == b.width && a.block == b.block && a.exp_width == b.exp_width && a.exp_bias == b.exp_bias;
  };
  // the one-launch route's conditions (lqer_linear_forward's: decode1_takes), for every member; anything else: the caller's
  // member-by-member loop
  bool ok = n_members >= 2 && n_members <= d1::MAXMEM && ((uintptr_t)workspace & 15) == 0;
  DecodeMember mem[d1::MAXMEM];
  int64_t rp_all = 0;
  // malformed members are errors, not "outside the route" (what lqer_linear_forward gets from lqer_linear_sizes / gemm_shape_args)
  for (int i = 0; i < n_members && i < d1::MAXMEM; ++i) {
    const lqer_linear_desc_t* d = members[i].desc;
    if (!d || d->in_features <= 0 || d->out_features <= 0 || d->rank < 0)
      return fail(LQER_E_INVALID, "linear_forward_group: member %d: bad descriptor", i);
    if (!fmt_ok(&d->w_fmt, ROLE_W_GROUP) || !fmt_ok(&d->x_fmt, ROLE_X) || !fmt_ok(&d->a_out_fmt, ROLE_A_OUT) ||
        !fmt_ok(&d->b_out_fmt, ROLE_B_OUT))
      return LQER_E_UNSUPPORTED;
    if (d->has_bias && !members[i].bias_q) return fail(LQER_E_INVALID, "linear_forward_group: member %d: has_bias = 1 but bias_q == NULL", i);
  }
  for (int i = 0; ok && i < n_members; ++i) {
    const lqer_group_member_t& m = members[i];
    const lqer_linear_desc_t* d = m.desc;
    ok = m.w_packed && m.b_t && m.y && decode1_takes(d, M, dtype, x, ldx, a_limbs, m.b_limbs) && d->in_features == d0->in_features &&
         same(d->x_fmt, d0->x_fmt) && same(d->a_out_fmt, d0->a_out_fmt) && same(d->b_out_fmt, d0->b_out_fmt) && m.ldy >= d->out_features &&
         ldx >= d->in_features;
    if (!ok) break;
    mem[i] = member_of(d, m.w_packed, m.b_t, m.b_limbs, m.bias_q, m.y, m.ldy);
    rp_all += mem[i].rp;
  }
  if (!ok || rp_all > d1::MAX_RP_ALL)
    return fail(LQER_E_UNSUPPORTED, "linear_forward_group: outside the one-launch decode route (2..4 members with equal K and x / A_out / B_out formats, "
                "lqer_decode_partials, M <= 8, one limb of A, aligned x): run the members one by one");
  if (workspace_bytes < lqer_group_workspace_bytes(d0->in_features, rp_all))
    return fail(LQER_E_WORKSPACE, "linear_forward_group: workspace %zu B < %zu B", workspace_bytes, lqer_group_workspace_bytes(d0->in_features, rp_all));
  GemmArgs g;
  memset(&g, 0, sizeof(g));
  int rc = gemm_shape_args(d0, M, dtype, g);  // the shared part: M, Kp, formats
  if (rc) return rc;
  rc = decode1_call(g, d0, dtype, x, ldx, a_t_cat, mem, n_members, workspace, workspace_bytes, stream);
  if (rc == LQER_E_UNSUPPORTED) set_error("linear_forward_group: shape outside the one-launch decode kernel (K too long for its LDS image)");
  return rc;
}

int lqer_desc_limbs(const lqer_linear_desc_t* d, int* act, int* xa) {
  if (!d || !passthrough_width_ok(d->x_fmt, "x_quantizer") || (d->rank > 0 && !passthrough_width_ok(d->a_out_fmt, "A_out_quantizer"))) {
    if (!d) set_error("desc_limbs: null descriptor");
    return LQER_E_INVALID;
  }
  if (act) *act = act_limbs(d);
  if (xa) *xa = d->rank > 0 ? xa_limbs(d) : 1;
  return LQER_OK;
}

int lqer_decode_partials(const lqer_linear_desc_t* d, int64_t M) { return decode_partials_ok(d, M) ? 1 : 0; }

int lqer_tile_partials(const lqer_linear_desc_t*, int64_t, int) { return 0; }  // (the route it reported is retired)

int lqer_f16_prepare(const void* w_packed, int64_t N, int64_t K, const void* a_t_limbs, int a_limbs, int64_t r, void* a_t_f16,
                     int32_t* flags, void* stream) {
  if (!w_packed || !flags || N <= 0 || K <= 0 || r < 0 || (r > 0 && (!a_t_limbs || !a_t_f16 || a_limbs < 0 || a_limbs > 3))) {
    set_error("f16_prepare: bad argument");
    return LQER_E_INVALID;
  }
  const int rc = f16_prepare_dispatch(w_packed, N, K, a_t_limbs, a_limbs, r, a_t_f16, flags, (hipStream_t)stream);
  if (rc || r <= 0) return rc;
  return a_frag_dispatch(a_t_f16, K, r, (hipStream_t)stream);  // the fragment-major copy behind [rp][Kp] (lqer_a_f16_image_bytes)
}

size_t lqer_a_b16_image_bytes(int64_t K, int64_t r) { return (K > 0 && r > 0) ? a_b16_image_bytes(K, r) : 0; }

int lqer_a_b16_prepare(const void* a_t_limbs, int64_t K, int64_t r, void* out, void* stream) {
  if (!a_t_limbs || !out || K <= 0 || r <= 0) {
    set_error("a_b16_prepare: bad argument");
    return LQER_E_INVALID;
  }
  return a_b16_prepare_dispatch(a_t_limbs, K, r, out, (hipStream_t)stream);
}

size_t lqer_a_f16_image_bytes(int64_t K, int64_t r) {
  return (K > 0 && r > 0) ? a_f16_image_bytes(K, r) : 0;
}

size_t lqer_matmul_q_workspace_bytes(int64_t batch, int64_t K, int64_t S2) {
  return (batch > 0 && K > 0 && S2 > 0) ? qmatmul_workspace_bytes(batch, K, S2) : 0;
}

size_t lqer_matmul_q_workspace_bytes_fmt(int64_t batch, int64_t S1, int64_t K, int64_t S2, const lqer_qfmt_t* x_fmt, const lqer_qfmt_t* y_fmt) {
  if (batch <= 0 || K <= 0 || S2 <= 0 || S1 < 0 || !x_fmt || !y_fmt) return 0;
  return qmatmul_workspace_bytes_ex(batch, S1, K, S2, x_fmt->block != 16, y_fmt->block != 16);
}

int lqer_matmul_q(const void* x, const void* y, void* out, int dtype, int64_t batch, int64_t S1, int64_t K, int64_t S2, int64_t x_bs,
                  int64_t x_rs, int64_t y_bs, int64_t y_ks, int64_t y_js, const lqer_qfmt_t* x_fmt, const lqer_qfmt_t* y_fmt,
                  void* workspace, size_t workspace_bytes, void* stream) {
  if (batch < 0 || S1 < 0 || K <= 0 || S2 < 0) {
    set_error("matmul_q: bad shape batch=%lld S1=%lld K=%lld S2=%lld", (long long)batch, (long long)S1, (long long)K, (long long)S2);
    return LQER_E_INVALID;
  }
  if (batch == 0 || S1 == 0 || S2 == 0) return LQER_OK;
  if (!x || !y || !out || !workspace) {
    set_error("matmul_q: null pointer");
    return LQER_E_INVALID;
  }
  if (!fmt_ok(x_fmt, ROLE_MATMUL_X) || !fmt_ok(y_fmt, ROLE_MATMUL_W)) return LQER_E_UNSUPPORTED;
  auto blk_ok = [](const lqer_qfmt_t* f, int64_t cols) { return f->block <= 0 || f->block >= cols || f->block % 16 == 0; };
  // (minifloat operands: elementwise - block -1, the standalone quantizer's bf16 image)
  auto kind_ok = [](const lqer_qfmt_t* f) { return f->kind == LQER_Q_MXINT || f->kind == LQER_Q_MINIFLOAT; };
  if (!kind_ok(x_fmt) || !kind_ok(y_fmt) || !blk_ok(x_fmt, K) || !blk_ok(y_fmt, S2)) {
    set_error("matmul_q: both quantizers must be block_fp with blocks of 16 n elements, or whole rows, along the last dim, or minifloat (got kinds %d / %d, "
              "blocks %d / %d)", x_fmt->kind, y_fmt->kind, x_fmt->block, y_fmt->block);
    return LQER_E_UNSUPPORTED;
  }
  if (x_rs < K || (y_ks != 1 && y_js != 1)) {
    set_error("matmul_q: x rows must be dense along k (row stride %lld < K) and y dense along k or along j (strides %lld, %lld)",
              (long long)x_rs, (long long)y_ks, (long long)y_js);
    return LQER_E_INVALID;
  }
  // blocks other than 16: the standalone quantizer writes the operand's bf16 image first - rows evenly spaced over the batch,
  // y dense along j (its blocks' dim)
  const bool x_pre = x_fmt->block != 16, y_pre = y_fmt->block != 16;
  if ((x_pre && batch > 1 && x_bs != S1 * x_rs) || (y_pre && (y_js != 1 || (batch > 1 && y_bs != K * y_ks)))) {
    set_error("matmul_q: operands with blocks other than 16 must have evenly spaced rows over the batch (x_bs == S1 x_rs; y dense along j with "
              "y_bs == K y_ks)");
    return LQER_E_INVALID;
  }
  if (workspace_bytes < qmatmul_workspace_bytes_ex(batch, S1, K, S2, x_pre, y_pre)) {
    set_error("matmul_q: workspace %zu B < %zu B (lqer_matmul_q_workspace_bytes_fmt)", workspace_bytes,
              qmatmul_workspace_bytes_ex(batch, S1, K, S2, x_pre, y_pre));
    return LQER_E_WORKSPACE;
  }
  return qmatmul_dispatch(x, y, out, dtype, batch, S1, K, S2, x_bs, x_rs, y_bs, y_ks, y_js, make_qp(*x_fmt), make_qp(*y_fmt), workspace,
                          (hipStream_t)stream);
}

size_t lqer_attention_q_workspace_bytes(int64_t batch, int64_t heads, int64_t kv_heads, int64_t S, int64_t T, int64_t D) {
  if (batch <= 0 || heads <= 0 || kv_heads <= 0 || S < 0 || T <= 0 || D <= 0) return 0;
  return attention_q_workspace_bytes(batch, kv_heads, T, D);
}

size_t lqer_attention_q_decode_workspace_bytes(int64_t batch, int64_t heads, int64_t kv_heads, int64_t S, int64_t T, int64_t D) {
  if (batch <= 0 || heads <= 0 || kv_heads <= 0 || S <= 0 || T <= 0 || D <= 0) return 0;
  return attention_q_decode_workspace_bytes(batch, heads, S, T, D);
}

// What the one check asks on behalf of the kernel that will run: everything in which the prefill kernel (attn_q.hip) and the split over
// the keys (attn_decode.hip) differ.
struct AttnKernel {
  int max_s;          // query rows taken; 0 = any
  const char* takes;  // the head-dim message's words for what runs
  int (*grid_limits)(const char* who, const AttnCall& c);  // S, T, batch and heads against the launch grids: LQER_OK or the refusal
  bool ws_al16_raw;   // the workspace must be 16-byte aligned with raw K and V too (with a cache it always must)
  size_t (*workspace_bytes)(const AttnCall& c);
  int (*dispatch)(const AttnCall& c);  // its launches
};

static int prefill_grid_limits(const char* who, const AttnCall& c) {
  if (c.T > (int64_t)65535 * 64 || c.S > (int64_t)1 << 30) {  // (the image kernels put T / 64 on a grid dim of 65535; tile indices are 32-bit)
    set_error("%s: S = %lld / T = %lld beyond the launch grid (T <= 4194240, S <= 2^30)", who, (long long)c.S, (long long)c.T);
    return LQER_E_UNSUPPORTED;
  }
  if (c.batch > 65535 || c.heads > 65535 || c.batch * c.kv_heads > 65535) {
    set_error("%s: batch %lld x heads %lld beyond the launch grid (65535 heads, batch x kv_heads): call in chunks", who, (long long)c.batch,
              (long long)c.heads);
    return LQER_E_UNSUPPORTED;
  }
  return LQER_OK;
}

static int decode_grid_limits(const char* who, const AttnCall& c) {
  if (c.T > (int64_t)1 << 30) {  // (chunk indices and the fold over them are 32-bit)
    set_error("%s: T = %lld beyond 2^30 keys", who, (long long)c.T);
    return LQER_E_UNSUPPORTED;
  }
  if (c.batch > 65535 || c.kv_heads > 65535) {
    set_error("%s: batch %lld / kv_heads %lld beyond the launch grid (65535 each): call in chunks", who, (long long)c.batch,
              (long long)c.kv_heads);
    return LQER_E_UNSUPPORTED;
  }
  return LQER_OK;
}

static size_t prefill_workspace_bytes(const AttnCall& c) { return attention_q_workspace_bytes(c.batch, c.kv_heads, c.T, c.D); }
// (on the paged pool c.T is the bound max_len, which sizes the workspace and the grid)
static size_t decode_workspace_bytes(const AttnCall& c) {
  // (per-sequence counts: rows by packed token; a negative total is the pool check's to refuse, right after this one)
  if (c.paged && c.pool.ragged) return c.pool.total < 0 ? 0 : attention_q_decode_paged_ragged_workspace_bytes(c.pool.total, c.heads, c.T, c.D);
  return c.paged ? attention_q_decode_paged_workspace_bytes(c.batch, c.heads, c.S, c.T, c.D)
                 : attention_q_decode_workspace_bytes(c.batch, c.heads, c.S, c.T, c.D);
}

// (only the cache's image kernels store the prefill workspace in 16-byte pieces; the decode kernels store and load theirs so from any source)
static const AttnKernel ATTN_PREFILL = {0, "kernel takes", prefill_grid_limits, false, prefill_workspace_bytes,
                                        attention_q_dispatch};
static const AttnKernel ATTN_DECODE = {attention_q_decode_max_s(), "kernels take", decode_grid_limits, true, decode_workspace_bytes,
                                       attention_q_decode_dispatch};

// the check of every attention call, for the kernel `kn` that will run: LQER_OK = go on, 1 = nothing to do, else the refusal
static int attn_check(const char* who, const AttnKernel& kn, const AttnCall& c) {
  if (c.batch < 0 || c.heads <= 0 || c.kv_heads <= 0 || c.S < 0 || c.T < 0 || c.D <= 0) {
    set_error("%s: bad shape batch=%lld heads=%lld kv_heads=%lld S=%lld T=%lld D=%lld", who, (long long)c.batch, (long long)c.heads,
              (long long)c.kv_heads, (long long)c.S, (long long)c.T, (long long)c.D);
    return LQER_E_INVALID;
  }
  if (c.heads % c.kv_heads != 0) {
    set_error("%s: heads %lld is not a multiple of kv_heads %lld", who, (long long)c.heads, (long long)c.kv_heads);
    return LQER_E_INVALID;
  }
  if (c.dtype != LQER_F32 && c.dtype != LQER_F16 && c.dtype != LQER_BF16) {
    set_error("%s: unknown dtype %d", who, c.dtype);
    return LQER_E_INVALID;
  }
  if (!c.qs || (!c.packed && (!c.ks || !c.vs)) || !c.os || (c.mask && !c.ms)) {
    set_error("%s: null stride array", who);
    return LQER_E_INVALID;
  }
  if (c.mask && c.causal) {
    set_error("%s: a mask tensor and causal = 1 are two forms of one mask - pass one", who);
    return LQER_E_INVALID;
  }
  if (c.windowed && (c.window < 1 || !c.causal)) {
    set_error("%s: window = %lld, causal = %d - a sliding window is W >= 1 keys on top of the causal rule (causal = 1)", who, (long long)c.window,
              c.causal);
    return LQER_E_INVALID;
  }
  if (c.treed) {  // (what the host can see of a tree; the words themselves fall under the caller's contract, as the table and the lengths do)
    const int most = kn.max_s ? kn.max_s : 64;  // (a row's word has 64 bits; the split over the keys takes 8 rows)
    if (!c.tree) {
      set_error("%s: null tree (one uint64 per packed query token, on the device)", who);
      return LQER_E_INVALID;
    }
    if (!c.causal) {
      set_error("%s: causal = 0 - a tree is a rule on top of the causal one (causal = 1)", who);
      return LQER_E_INVALID;
    }
    if (c.S > most) {
      set_error("%s: max_s = %lld nodes - a tree of this call has up to %d, and max_s bounds every sequence's count%s", who, (long long)c.S,
                most, kn.max_s ? " (lqer_attention_q_paged_tree takes up to 64)" : "");
      return LQER_E_INVALID;
    }
  }
  if (!c.q_fmt || !c.k_fmt || !c.p_fmt || !c.v_fmt) {
    set_error("%s: null quantizer format", who);
    return LQER_E_INVALID;
  }
  const bool ragged = c.paged && c.pool.ragged;  // (S: the bound max_s on the per-sequence counts, which sizes the grid)
  if (ragged && kn.max_s && c.S > kn.max_s) {  // (a bound the caller chose, not a shape: invalid, as max_s < 1 below)
    set_error("%s: max_s = %lld query rows - the split over the keys takes counts up to %d, and max_s bounds every sequence's count "
              "(lqer_attention_q_paged_ragged takes any)", who, (long long)c.S, kn.max_s);
    return LQER_E_INVALID;
  }
  if (kn.max_s && c.S > kn.max_s) {
    set_error("%s: S = %lld query rows - the split over the keys takes up to %d (lqer_attention_q takes any)", who, (long long)c.S,
              kn.max_s);
    return LQER_E_UNSUPPORTED;
  }
  if (c.D % 16 != 0 || c.D > 128) {
    set_error("%s: head dim %lld - the fused %s multiples of 16 up to 128 (the two products of lqer_matmul_q take any)", who, (long long)c.D,
              kn.takes);
    return LQER_E_UNSUPPORTED;
  }
  if (!fmt_ok(c.q_fmt, ROLE_ATTN_Q) || !fmt_ok(c.k_fmt, ROLE_ATTN_K) ||
      !fmt_ok(c.p_fmt, ROLE_ATTN_P) || !fmt_ok(c.v_fmt, ROLE_ATTN_V))
    return LQER_E_UNSUPPORTED;
  for (const lqer_qfmt_t* f : {c.q_fmt, c.k_fmt, c.p_fmt, c.v_fmt})
    if (f->kind != LQER_Q_MXINT || f->block != 16) {
      set_error("%s: the four quantizers must be block_fp with blocks of 16 along the last dim (got kind %d, block %d); other "
                "formats run as the two products of lqer_matmul_q", who, f->kind, f->block);
      return LQER_E_UNSUPPORTED;
    }
  if (ragged && c.S < 1) {
    set_error("%s: max_s = %lld query rows (max_s >= 1 bounds every sequence's count)", who, (long long)c.S);
    return LQER_E_INVALID;
  }
  if (c.grouped && (!c.grp_of || !c.grp_starts || !c.grp_members || !c.grp_keys || c.n_groups < 1 || c.n_groups > c.batch)) {
    set_error("%s: group arrays %p / %p / %p / %p, n_groups = %lld for batch %lld (grp_of, grp_starts, grp_members, grp_keys: int32 on the "
              "device, 1 <= n_groups <= batch)", who, (const void*)c.grp_of, (const void*)c.grp_starts, (const void*)c.grp_members,
              (const void*)c.grp_keys, (long long)c.n_groups, (long long)c.batch);
    return LQER_E_INVALID;
  }
  if (const int rc = kn.grid_limits(who, c)) return rc;
  if (c.batch == 0 || c.S == 0 || (ragged && c.pool.total == 0)) return 1;
  if (c.T == 0) {
    set_error("%s: T = 0 (a softmax over no keys)", who);
    return LQER_E_INVALID;
  }
  if (!c.q || (!c.packed && (!c.k || !c.v)) || !c.out || !c.workspace) {
    set_error("%s: null pointer", who);
    return LQER_E_INVALID;
  }
  if ((c.packed || kn.ws_al16_raw) && (uintptr_t)c.workspace % 16 != 0) {
    set_error("%s: workspace %p is not 16-byte aligned", who, c.workspace);
    return LQER_E_INVALID;
  }
  const size_t need = kn.workspace_bytes(c);
  if (c.workspace_bytes < need) {
    // (a windowed call has the unwindowed one's workspace; the ragged decode call takes its window as an argument of its own)
    const char* sized_by = c.grouped   ? "attention_q_decode_paged"  // (the grouped call has the plain call's workspace too)
                           : c.treed   ? (kn.max_s ? "attention_q_decode_paged_ragged" : "attention_q_paged_ragged")  // (a tree call its sibling's)
                           : !c.windowed ? who
                           : kn.max_s  ?(ragged ? who : "attention_q_decode_paged")
                                       : (ragged ? "attention_q_paged_ragged" : "attention_q_paged");
    set_error("%s: workspace %zu B < %zu B (lqer_%s_workspace_bytes)", who, c.workspace_bytes, need, sized_by);
    return LQER_E_INVALID;
  }
  return LQER_OK;
}

// ---- the packed KV cache (kv_pack.h, kv_cache.hip) ----
static bool kv_dtype_ok(int dtype) { return dtype == LQER_F32 || dtype == LQER_F16 || dtype == LQER_BF16; }

size_t lqer_kv_cache_bytes(int dtype, int64_t batch, int64_t kv_heads, int64_t capacity, int64_t D) {
  if (!kv_dtype_ok(dtype) || batch <= 0 || kv_heads <= 0 || capacity <= 0 || D <= 0 || D % 16 != 0 || D > 128) return 0;
  return kv_cache_bytes(dtype, batch, kv_heads, capacity, D);
}

// what the codes of a cache or a pool ask of the head dim and the two quantizers: LQER_OK or the refusal
static int kv_codes_check(const char* who, int64_t D, const lqer_qfmt_t* k_fmt, const lqer_qfmt_t* v_fmt) {
  if (!k_fmt || !v_fmt) {
    set_error("%s: null quantizer format of the KV cache", who);
    return LQER_E_INVALID;
  }
  if (D % 16 != 0 || D > 128) {
    set_error("%s: head dim %lld - the packed KV cache takes multiples of 16 up to 128", who, (long long)D);
    return LQER_E_UNSUPPORTED;
  }
  if (!fmt_ok(k_fmt, ROLE_ATTN_K) || !fmt_ok(v_fmt, ROLE_ATTN_V)) return LQER_E_UNSUPPORTED;
  for (const lqer_qfmt_t* f : {k_fmt, v_fmt})
    if (f->kind != LQER_Q_MXINT || f->block != 16) {
      set_error("%s: the packed KV cache holds block_fp codes of width <= 8 with blocks of 16 (got kind %d, block %d)", who, f->kind, f->block);
      return LQER_E_UNSUPPORTED;
    }
  return LQER_OK;
}

// what append, attention and unpack ask of a cache: LQER_OK or the refusal
static int kv_cache_check(const char* who, const void* cache, size_t cache_bytes, int dtype, int64_t batch, int64_t kv_heads, int64_t capacity,
                          int64_t D, int64_t T, const lqer_qfmt_t* k_fmt, const lqer_qfmt_t* v_fmt) {
  if (batch < 0 || kv_heads <= 0 || capacity <= 0 || D <= 0 || T < 0) {
    set_error("%s: bad KV cache shape batch=%lld kv_heads=%lld capacity=%lld D=%lld length=%lld", who, (long long)batch, (long long)kv_heads,
              (long long)capacity, (long long)D, (long long)T);
    return LQER_E_INVALID;
  }
  if (!kv_dtype_ok(dtype)) {
    set_error("%s: unknown dtype %d of the KV cache", who, dtype);
    return LQER_E_INVALID;
  }
  if (const int rc = kv_codes_check(who, D, k_fmt, v_fmt)) return rc;
  if (T > capacity) {
    set_error("%s: %lld keys beyond the KV cache's capacity %lld", who, (long long)T, (long long)capacity);
    return LQER_E_INVALID;
  }
  if (batch == 0) return LQER_OK;
  if (!cache) {
    set_error("%s: null KV cache", who);
    return LQER_E_INVALID;
  }
  if ((uintptr_t)cache % 16 != 0) {  // (codes and exponents travel in 16-byte pieces)
    set_error("%s: KV cache %p is not 16-byte aligned", who, cache);
    return LQER_E_INVALID;
  }
  const size_t need = kv_cache_bytes(dtype, batch, kv_heads, capacity, D);
  if (cache_bytes < need) {
    set_error("%s: KV cache of %zu B < %zu B (lqer_kv_cache_bytes)", who, cache_bytes, need);
    return LQER_E_INVALID;
  }
  return LQER_OK;
}

int lqer_kv_cache_append(void* cache, size_t cache_bytes, const void* k_new, const void* v_new, const int64_t* k_strides, const int64_t* v_strides,
                         int dtype, int64_t batch, int64_t kv_heads, int64_t capacity, int64_t D, int64_t len, int64_t n, const lqer_qfmt_t* k_fmt,
                         const lqer_qfmt_t* v_fmt, void* stream) {
  if (len < 0 || n < 1) {
    set_error("kv_cache_append: length %lld / %lld new keys of the KV cache (length >= 0, at least one new key)", (long long)len, (long long)n);
    return LQER_E_INVALID;
  }
  if (capacity > 0 && n > capacity) {  // (before len + n can overflow)
    set_error("kv_cache_append: %lld new keys beyond the KV cache's capacity %lld", (long long)n, (long long)capacity);
    return LQER_E_INVALID;
  }
  const int rc = kv_cache_check("kv_cache_append", cache, cache_bytes, dtype, batch, kv_heads, capacity, D, len + n, k_fmt, v_fmt);
  if (rc != LQER_OK) return rc;
  if (batch == 0) return LQER_OK;
  if (!k_new || !v_new || !k_strides || !v_strides) {
    set_error("kv_cache_append: null pointer (new keys / values of the KV cache or their strides)");
    return LQER_E_INVALID;
  }
  if (batch * kv_heads * ((n + 15) / 16 + 1 + n) > ((int64_t)1 << 31)) {  // (work items over grid.x, 256 a workgroup: D / 4 <= 32 per row)
    set_error("kv_cache_append: %lld new keys for %lld KV cache streams beyond one launch grid: append in pieces", (long long)n,
              (long long)(batch * kv_heads));
    return LQER_E_UNSUPPORTED;
  }
  return kv_cache_append_dispatch(cache, k_new, v_new, k_strides, v_strides, dtype, batch, kv_heads, capacity, D, len, n, make_qp(*k_fmt),
                                  make_qp(*v_fmt), (hipStream_t)stream);
}

int lqer_kv_cache_unpack(const void* cache, size_t cache_bytes, int dtype, int64_t batch, int64_t kv_heads, int64_t capacity, int64_t D, int64_t T,
                         const lqer_qfmt_t* k_fmt, const lqer_qfmt_t* v_fmt, float* k_f32, float* v_f32, void* stream) {
  const int rc = kv_cache_check("kv_cache_unpack", cache, cache_bytes, dtype, batch, kv_heads, capacity, D, T, k_fmt, v_fmt);
  if (rc != LQER_OK) return rc;
  if (batch == 0 || T == 0) return LQER_OK;
  if (!k_f32 && !v_f32) {
    set_error("kv_cache_unpack: null outputs for the KV cache's K and V");
    return LQER_E_INVALID;
  }
  if (batch * kv_heads * T * D > ((int64_t)1 << 39)) {
    set_error("kv_cache_unpack: %lld elements of the KV cache beyond one launch grid", (long long)(batch * kv_heads * T * D));
    return LQER_E_UNSUPPORTED;
  }
  return kv_cache_unpack_dispatch(cache, dtype, batch, kv_heads, capacity, D, T, make_qp(*k_fmt), make_qp(*v_fmt), k_f32, v_f32,
                                  (hipStream_t)stream);
}

size_t lqer_attention_q_decode_kv_workspace_bytes(int64_t batch, int64_t heads, int64_t kv_heads, int64_t S, int64_t T, int64_t D) {
  return lqer_attention_q_decode_workspace_bytes(batch, heads, kv_heads, S, T, D);
}

size_t lqer_attention_q_kv_workspace_bytes(int64_t batch, int64_t heads, int64_t kv_heads, int64_t S, int64_t T, int64_t D) {
  return lqer_attention_q_workspace_bytes(batch, heads, kv_heads, S, T, D);
}

// ---- the paged KV pool (kv_pack.h: PoolLayout; kv_cache.hip, attn_decode.hip) ----
size_t lqer_kv_pool_bytes(int dtype, int64_t pages, int64_t slots, int64_t kv_heads, int64_t D) {
  if (!kv_dtype_ok(dtype) || pages <= 0 || slots <= 0 || kv_heads <= 0 || D <= 0 || D % 16 != 0 || D > 128) return 0;
  return kv_pool_bytes(dtype, pages, slots, kv_heads, D);
}

// LQER_Q_MXINT_C4 as the k_fmt / v_fmt of a pool entry: the operand's codes are stored as nibbles (kv_pack.h) and quantized exactly as
// LQER_Q_MXINT of the same fields.  The format the checks and the kernels go by - `own`, the caller's with the kind replaced, or the
// caller's itself (null included: the checks' to refuse) - and whether the storage is nibbles.
static const lqer_qfmt_t* pool_code_fmt(const lqer_qfmt_t* f, lqer_qfmt_t& own, bool& n4) {
  n4 = f && f->kind == LQER_Q_MXINT_C4;
  if (!n4) return f;
  own = *f, own.kind = LQER_Q_MXINT;
  return &own;
}
// what nibble storage asks of the operand's format (a magnitude of at most 7, the 8-byte piece of one block of 16 d): LQER_OK or the refusal
static int pool_nibble_check(const char* who, const KvPool& p, const lqer_qfmt_t* k_fmt, const lqer_qfmt_t* v_fmt) {
  const struct { bool n4; const lqer_qfmt_t* f; const char* name; } ops[2] = {{p.k4, k_fmt, "k_fmt"}, {p.v4, v_fmt, "v_fmt"}};
  for (const auto& o : ops)
    if (o.n4 && (o.f->width < 2 || o.f->width > 4 || o.f->block != 16)) {
      set_error("%s: %s of kind LQER_Q_MXINT_C4 with width %d, block %d - nibble codes of the KV pool hold block_fp of width 2..4 with blocks of 16",
                who, o.name, o.f->width, o.f->block);
      return LQER_E_UNSUPPORTED;
    }
  return LQER_OK;
}
// the two formats of a pool entry resolved in place: k_fmt / v_fmt then point at what the checks and the kernels go by, p knows the storage
struct PoolFmts {
  lqer_qfmt_t k, v;
  void resolve(KvPool& p, const lqer_qfmt_t*& k_fmt, const lqer_qfmt_t*& v_fmt) {
    k_fmt = pool_code_fmt(k_fmt, k, p.k4), v_fmt = pool_code_fmt(v_fmt, v, p.v4);
  }
};

size_t lqer_kv_pool_bytes_fmt(int dtype, int64_t pages, int64_t slots, int64_t kv_heads, int64_t D, const lqer_qfmt_t* k_fmt,
                              const lqer_qfmt_t* v_fmt) {
  if (!lqer_kv_pool_bytes(dtype, pages, slots, kv_heads, D) || !k_fmt || !v_fmt) return 0;
  KvPool p = {};
  PoolFmts own;
  own.resolve(p, k_fmt, v_fmt);
  if (pool_nibble_check("kv_pool_bytes_fmt", p, k_fmt, v_fmt) != LQER_OK) return 0;
  for (const lqer_qfmt_t* f : {k_fmt, v_fmt})
    if (f->kind != LQER_Q_MXINT || f->block != 16 || !fmt_ok(f, ROLE_ATTN_KV)) return 0;
  return kv_pool_bytes(dtype, pages, slots, kv_heads, D, p.k4, p.v4);
}

// what append, attention and gather ask of a pool and its page table (host arguments only: the table's and the lengths' CONTENTS are
// the caller's contract).  A call that addresses sequences through seq_slots / lens (append, attention) needs the two arrays; gather
// names its slot on the host; a call with per-sequence counts (p.ragged) also needs their starts.  The quantizers are the caller's to
// check (kv_codes_check, attn_check).  LQER_OK or the refusal
enum PoolUse { POOL_BATCH, POOL_ONE_SLOT };
static int kv_pool_check(const char* who, const KvPool& p, PoolUse use) {
  if (p.pages < 1 || p.slots < 1 || p.kv_heads < 1 || p.table_stride < 1 || p.D <= 0) {
    set_error("%s: bad KV pool shape pages=%lld slots=%lld kv_heads=%lld table_stride=%lld D=%lld", who, (long long)p.pages, (long long)p.slots,
              (long long)p.kv_heads, (long long)p.table_stride, (long long)p.D);
    return LQER_E_INVALID;
  }
  if (!kv_dtype_ok(p.dtype)) {
    set_error("%s: unknown dtype %d of the KV pool", who, p.dtype);
    return LQER_E_INVALID;
  }
  if (p.D % 16 != 0 || p.D > 128) {
    set_error("%s: head dim %lld - the KV pool takes multiples of 16 up to 128", who, (long long)p.D);
    return LQER_E_UNSUPPORTED;
  }
  if (p.pages > ((int64_t)1 << 31) - 1 || p.slots > ((int64_t)1 << 31) - 1) {
    set_error("%s: %lld pages / %lld slots of the KV pool beyond the 32-bit page table", who, (long long)p.pages, (long long)p.slots);
    return LQER_E_UNSUPPORTED;
  }
  if (p.max_len > ((int64_t)1 << 30)) {  // (as the decode kernels' T: chunk indices are 32-bit)
    set_error("%s: max_len %lld of the KV pool beyond 2^30 keys", who, (long long)p.max_len);
    return LQER_E_UNSUPPORTED;
  }
  if (p.max_len < 1 || (p.max_len + 15) / 16 > p.table_stride) {
    set_error("%s: max_len %lld of the KV pool outside 1 .. 16 table_stride = 16 x %lld keys", who, (long long)p.max_len,
              (long long)p.table_stride);
    return LQER_E_INVALID;
  }
  if (!p.block_table || (use == POOL_BATCH && (!p.seq_slots || !p.lens))) {
    set_error("%s: null block_table / seq_slots / lens of the KV pool", who);
    return LQER_E_INVALID;
  }
  if (p.ragged && (!p.starts || p.total < 0)) {
    set_error("%s: starts %p / total = %lld of a call with per-sequence counts on the KV pool (new_starts / q_starts: int32 [batch + 1] on the "
              "device, total >= 0 tokens)", who, (const void*)p.starts, (long long)p.total);
    return LQER_E_INVALID;
  }
  if (!p.pool) {
    set_error("%s: null KV pool", who);
    return LQER_E_INVALID;
  }
  if ((uintptr_t)p.pool % 16 != 0) {
    set_error("%s: KV pool %p is not 16-byte aligned", who, p.pool);
    return LQER_E_INVALID;
  }
  const size_t need = kv_pool_bytes(p.dtype, p.pages, p.slots, p.kv_heads, p.D, p.k4, p.v4);
  if (p.pool_bytes < need) {
    set_error("%s: KV pool of %zu B < %zu B (lqer_kv_pool_bytes%s)", who, p.pool_bytes, need, p.k4 || p.v4 ? "_fmt" : "");
    return LQER_E_INVALID;
  }
  return LQER_OK;
}

// the pool record from the arguments every pool call has, in the order the ABI lists them (no per-sequence counts: the caller's to add)
static KvPool kv_pool(const void* pool, size_t pool_bytes, int64_t pages, int64_t slots, const int32_t* block_table, int64_t table_stride,
                      const int32_t* seq_slots, const int32_t* lens, int64_t max_len, int dtype, int64_t kv_heads, int64_t D) {
  return {pool, pool_bytes, dtype, pages, slots, kv_heads, D, block_table, seq_slots, lens, table_stride, max_len};
}

int lqer_kv_pool_append(void* pool, size_t pool_bytes, int64_t pages, int64_t slots, const int32_t* block_table, int64_t table_stride,
                        const int32_t* seq_slots, const int32_t* lens, int64_t max_len, const void* k_new, const void* v_new,
                        const int64_t* k_strides, const int64_t* v_strides, int dtype, int64_t batch, int64_t kv_heads, int64_t D, int64_t n,
                        const lqer_qfmt_t* k_fmt, const lqer_qfmt_t* v_fmt, void* stream) {
  if (batch < 0 || n < 1) {
    set_error("kv_pool_append: batch %lld / %lld new keys for the KV pool (batch >= 0, at least one new key)", (long long)batch, (long long)n);
    return LQER_E_INVALID;
  }
  KvPool p = kv_pool(pool, pool_bytes, pages, slots, block_table, table_stride, seq_slots, lens, max_len, dtype, kv_heads, D);
  PoolFmts own;
  own.resolve(p, k_fmt, v_fmt);
  int rc = pool_nibble_check("kv_pool_append", p, k_fmt, v_fmt);
  if (rc == LQER_OK) rc = kv_codes_check("kv_pool_append", D, k_fmt, v_fmt);
  if (rc == LQER_OK) rc = kv_pool_check("kv_pool_append", p, POOL_BATCH);
  if (rc != LQER_OK) return rc;
  if (n > max_len) {
    set_error("kv_pool_append: %lld new keys beyond max_len %lld of the KV pool (a bound on lens[b] + n)", (long long)n, (long long)max_len);
    return LQER_E_INVALID;
  }
  if (batch == 0) return LQER_OK;
  if (!k_new || !v_new || !k_strides || !v_strides) {
    set_error("kv_pool_append: null pointer (new keys / values for the KV pool or their strides)");
    return LQER_E_INVALID;
  }
  if (batch * kv_heads * ((n + 14) / 16 + 1 + n) > ((int64_t)1 << 31)) {  // (work items over grid.x, 256 a workgroup: D / 4 <= 32 per row)
    set_error("kv_pool_append: %lld new keys for %lld KV pool streams beyond one launch grid: append in pieces", (long long)n,
              (long long)(batch * kv_heads));
    return LQER_E_UNSUPPORTED;
  }
  return kv_pool_append_dispatch(p, k_new, v_new, k_strides, v_strides, batch, n, make_qp(*k_fmt), make_qp(*v_fmt), (hipStream_t)stream);
}

int lqer_kv_pool_append_ragged(void* pool, size_t pool_bytes, int64_t pages, int64_t slots, const int32_t* block_table, int64_t table_stride,
                               const int32_t* seq_slots, const int32_t* lens, int64_t max_len, const int32_t* new_starts, int64_t max_n,
                               const void* k_new, const void* v_new, const int64_t* k_strides, const int64_t* v_strides, int dtype, int64_t batch,
                               int64_t kv_heads, int64_t D, int64_t total, const lqer_qfmt_t* k_fmt, const lqer_qfmt_t* v_fmt, void* stream) {
  if (batch < 0 || max_n < 1) {
    set_error("kv_pool_append_ragged: batch %lld / max_n %lld new keys for the KV pool (batch >= 0, max_n >= 1 bounds every sequence's count)",
              (long long)batch, (long long)max_n);
    return LQER_E_INVALID;
  }
  KvPool p = kv_pool(pool, pool_bytes, pages, slots, block_table, table_stride, seq_slots, lens, max_len, dtype, kv_heads, D);
  p.ragged = true, p.starts = new_starts, p.total = total;
  PoolFmts own;
  own.resolve(p, k_fmt, v_fmt);
  int rc = pool_nibble_check("kv_pool_append_ragged", p, k_fmt, v_fmt);
  if (rc == LQER_OK) rc = kv_codes_check("kv_pool_append_ragged", D, k_fmt, v_fmt);
  if (rc == LQER_OK) rc = kv_pool_check("kv_pool_append_ragged", p, POOL_BATCH);
  if (rc != LQER_OK) return rc;
  if (max_n > max_len) {
    set_error("kv_pool_append_ragged: max_n %lld new keys beyond max_len %lld of the KV pool (a bound on lens[b] + n_b)", (long long)max_n,
              (long long)max_len);
    return LQER_E_INVALID;
  }
  if (batch == 0 || total == 0) return LQER_OK;
  if (!k_new || !v_new || !k_strides || !v_strides) {
    set_error("kv_pool_append_ragged: null pointer (new keys / values for the KV pool or their strides)");
    return LQER_E_INVALID;
  }
  if (batch * kv_heads * ((max_n + 14) / 16 + 1 + max_n) > ((int64_t)1 << 31)) {  // (work items over grid.x, as lqer_kv_pool_append's at n = max_n)
    set_error("kv_pool_append_ragged: max_n %lld new keys for %lld KV pool streams beyond one launch grid: append in pieces", (long long)max_n,
              (long long)(batch * kv_heads));
    return LQER_E_UNSUPPORTED;
  }
  return kv_pool_append_ragged_dispatch(p, k_new, v_new, k_strides, v_strides, batch, max_n, make_qp(*k_fmt), make_qp(*v_fmt), (hipStream_t)stream);
}

// gather with and without formats: k_fmt / v_fmt null (both) - lqer_kv_pool_gather, a pool of byte codes
static int kv_pool_gather(const char* who, const void* pool, size_t pool_bytes, int dtype, int64_t pages, int64_t slots, int64_t kv_heads, int64_t D,
                          const int32_t* block_table, int64_t table_stride, int64_t slot, int64_t T, void* cache, size_t cache_bytes,
                          int64_t capacity, const lqer_qfmt_t* k_fmt, const lqer_qfmt_t* v_fmt, bool with_fmts, void* stream) {
  if (slot < 0 || slot >= slots || T < 0 || capacity < 1 || T > capacity) {
    set_error("%s: slot %lld of %lld / %lld keys of the KV pool into a cache of capacity %lld", who, (long long)slot, (long long)slots,
              (long long)T, (long long)capacity);
    return LQER_E_INVALID;
  }
  KvPool p = kv_pool(pool, pool_bytes, pages, slots, block_table, table_stride, nullptr, nullptr, T > 0 ? T : 1, dtype, kv_heads, D);
  PoolFmts own;
  int rc = LQER_OK;
  if (with_fmts) {
    own.resolve(p, k_fmt, v_fmt);
    rc = pool_nibble_check(who, p, k_fmt, v_fmt);
  }
  if (rc == LQER_OK) rc = kv_pool_check(who, p, POOL_ONE_SLOT);
  if (rc == LQER_OK && with_fmts) rc = kv_codes_check(who, D, k_fmt, v_fmt);
  if (rc != LQER_OK) return rc;
  if (!cache || (uintptr_t)cache % 16 != 0 || cache_bytes < kv_cache_bytes(dtype, 1, kv_heads, capacity, D)) {
    set_error("%s: KV cache %p of %zu B - null, not 16-byte aligned or shorter than lqer_kv_cache_bytes(batch 1) = %zu B", who, cache,
              cache_bytes, kv_cache_bytes(dtype, 1, kv_heads, capacity, D));
    return LQER_E_INVALID;
  }
  return kv_pool_gather_dispatch(p, slot, T, cache, capacity, (hipStream_t)stream);
}

int lqer_kv_pool_gather(const void* pool, size_t pool_bytes, int dtype, int64_t pages, int64_t slots, int64_t kv_heads, int64_t D,
                        const int32_t* block_table, int64_t table_stride, int64_t slot, int64_t T, void* cache, size_t cache_bytes,
                        int64_t capacity, void* stream) {
  return kv_pool_gather("kv_pool_gather", pool, pool_bytes, dtype, pages, slots, kv_heads, D, block_table, table_stride, slot, T, cache, cache_bytes,
                        capacity, nullptr, nullptr, false, stream);
}

int lqer_kv_pool_gather_fmt(const void* pool, size_t pool_bytes, int dtype, int64_t pages, int64_t slots, int64_t kv_heads, int64_t D,
                            const int32_t* block_table, int64_t table_stride, int64_t slot, int64_t T, void* cache, size_t cache_bytes,
                            int64_t capacity, const lqer_qfmt_t* k_fmt, const lqer_qfmt_t* v_fmt, void* stream) {
  return kv_pool_gather("kv_pool_gather_fmt", pool, pool_bytes, dtype, pages, slots, kv_heads, D, block_table, table_stride, slot, T, cache,
                        cache_bytes, capacity, k_fmt, v_fmt, true, stream);
}

// fork with and without formats: without (lqer_kv_pool_fork) a pool of byte codes
static int kv_pool_fork(const char* who, void* pool, size_t pool_bytes, int dtype, int64_t pages, int64_t slots, int64_t kv_heads, int64_t D,
                        const int32_t* block_table, int64_t table_stride, const int32_t* src_slots, const int32_t* dst_slots, const int32_t* lens,
                        int64_t n, const lqer_qfmt_t* k_fmt, const lqer_qfmt_t* v_fmt, bool with_fmts, void* stream) {
  if (n < 1) {
    set_error("%s: %lld pairs for the KV pool (at least one)", who, (long long)n);
    return LQER_E_INVALID;
  }
  if (!src_slots) {
    set_error("%s: null src_slots for the KV pool", who);
    return LQER_E_INVALID;
  }
  if (!kv_dtype_ok(dtype)) {  // (what lqer_kv_pool_bytes rejects, one code for dtype and head dim)
    set_error("%s: dtype %d - the KV pool takes fp32, fp16 and bf16", who, dtype);
    return LQER_E_UNSUPPORTED;
  }
  // the bound on the lengths is the room of a table row, or the library's 2^30 where the row has more
  const int64_t room = table_stride < ((int64_t)1 << 26) ? 16 * table_stride : (int64_t)1 << 30;
  KvPool p = kv_pool(pool, pool_bytes, pages, slots, block_table, table_stride, dst_slots, lens, room, dtype, kv_heads, D);
  PoolFmts own;
  int rc = LQER_OK;
  if (with_fmts) {
    own.resolve(p, k_fmt, v_fmt);
    rc = pool_nibble_check(who, p, k_fmt, v_fmt);
  }
  if (rc == LQER_OK) rc = kv_pool_check(who, p, POOL_BATCH);
  if (rc == LQER_OK && with_fmts) rc = kv_codes_check(who, D, k_fmt, v_fmt);
  if (rc != LQER_OK) return rc;
  if (n > (((int64_t)1 << 31) - 1) / kv_heads) {  // (a workgroup pair per (pair, kv head) over grid.x)
    set_error("%s: %lld pairs x %lld kv heads of the KV pool beyond one launch grid: fork in pieces", who, (long long)n, (long long)kv_heads);
    return LQER_E_UNSUPPORTED;
  }
  return kv_pool_fork_dispatch(p, src_slots, n, (hipStream_t)stream);
}

int lqer_kv_pool_fork(void* pool, size_t pool_bytes, int dtype, int64_t pages, int64_t slots, int64_t kv_heads, int64_t D,
                      const int32_t* block_table, int64_t table_stride, const int32_t* src_slots, const int32_t* dst_slots, const int32_t* lens,
                      int64_t n, void* stream) {
  return kv_pool_fork("kv_pool_fork", pool, pool_bytes, dtype, pages, slots, kv_heads, D, block_table, table_stride, src_slots, dst_slots, lens, n,
                      nullptr, nullptr, false, stream);
}

int lqer_kv_pool_fork_fmt(void* pool, size_t pool_bytes, int dtype, int64_t pages, int64_t slots, int64_t kv_heads, int64_t D,
                          const int32_t* block_table, int64_t table_stride, const int32_t* src_slots, const int32_t* dst_slots, const int32_t* lens,
                          int64_t n, const lqer_qfmt_t* k_fmt, const lqer_qfmt_t* v_fmt, void* stream) {
  return kv_pool_fork("kv_pool_fork_fmt", pool, pool_bytes, dtype, pages, slots, kv_heads, D, block_table, table_stride, src_slots, dst_slots, lens,
                      n, k_fmt, v_fmt, true, stream);
}

// one side of lqer_kv_pool_copy - a pool by its own page and slot counts, no table and no lengths: p.k4 / p.v4 and `need`, the bytes
// lqer_kv_pool_bytes(_fmt) gives its geometry, or the refusal
static int kv_pool_copy_side(const char* side, KvPool& p, const lqer_qfmt_t* k_fmt, const lqer_qfmt_t* v_fmt, size_t& need) {
  if (!p.pool) {
    set_error("kv_pool_copy: null %s KV pool", side);
    return LQER_E_INVALID;
  }
  if (p.pages < 1 || p.slots < 1 || p.kv_heads < 1 || p.D < 1) {
    set_error("kv_pool_copy: bad shape of the %s KV pool pages=%lld slots=%lld kv_heads=%lld D=%lld", side, (long long)p.pages, (long long)p.slots,
              (long long)p.kv_heads, (long long)p.D);
    return LQER_E_INVALID;
  }
  need = k_fmt ? lqer_kv_pool_bytes_fmt(p.dtype, p.pages, p.slots, p.kv_heads, p.D, k_fmt, v_fmt)
               : lqer_kv_pool_bytes(p.dtype, p.pages, p.slots, p.kv_heads, p.D);
  if (!need) {
    set_error("kv_pool_copy: lqer_kv_pool_bytes%s sizes no %s KV pool of dtype %d, head dim %lld%s (fp32 / fp16 / bf16, multiples of 16 up to "
              "128, block_fp of width <= 8 - nibble codes: 2..4 - with blocks of 16)", k_fmt ? "_fmt" : "", side, p.dtype, (long long)p.D,
              k_fmt ? " and these K / V formats" : "");
    return LQER_E_UNSUPPORTED;
  }
  PoolFmts own;
  own.resolve(p, k_fmt, v_fmt);  // (the storage alone: nothing here quantizes)
  if ((uintptr_t)p.pool % 16 != 0) {
    set_error("kv_pool_copy: %s KV pool %p is not 16-byte aligned", side, p.pool);
    return LQER_E_INVALID;
  }
  if (p.pool_bytes < need) {
    set_error("kv_pool_copy: %s KV pool of %zu B < %zu B (lqer_kv_pool_bytes%s)", side, p.pool_bytes, need, k_fmt ? "_fmt" : "");
    return LQER_E_INVALID;
  }
  return LQER_OK;
}

int lqer_kv_pool_copy(const void* src_pool, size_t src_bytes, int64_t src_pages, int64_t src_slots, void* dst_pool, size_t dst_bytes,
                      int64_t dst_pages, int64_t dst_slots, int dtype, int64_t kv_heads, int64_t D, const int32_t* src_page_ids,
                      const int32_t* dst_page_ids, int64_t n_pages, const int32_t* src_slot_ids, const int32_t* dst_slot_ids, int64_t n_slots,
                      const lqer_qfmt_t* k_fmt, const lqer_qfmt_t* v_fmt, void* stream) {
  if (!k_fmt != !v_fmt) {
    set_error("kv_pool_copy: k_fmt %p / v_fmt %p of the KV pools - both null (byte codes) or the two formats whose kinds name the storage",
              (const void*)k_fmt, (const void*)v_fmt);
    return LQER_E_INVALID;
  }
  if (n_pages < 0 || n_slots < 0) {
    set_error("kv_pool_copy: %lld page pairs / %lld slot pairs of the KV pools (each >= 0)", (long long)n_pages, (long long)n_slots);
    return LQER_E_INVALID;
  }
  KvPool s = kv_pool(src_pool, src_bytes, src_pages, src_slots, nullptr, 0, nullptr, nullptr, 0, dtype, kv_heads, D);
  KvPool d = kv_pool(dst_pool, dst_bytes, dst_pages, dst_slots, nullptr, 0, nullptr, nullptr, 0, dtype, kv_heads, D);
  size_t s_need = 0, d_need = 0;
  if (const int rc = kv_pool_copy_side("source", s, k_fmt, v_fmt, s_need)) return rc;
  if (const int rc = kv_pool_copy_side("destination", d, k_fmt, v_fmt, d_need)) return rc;
  if ((n_pages > 0 && (!src_page_ids || !dst_page_ids)) || (n_slots > 0 && (!src_slot_ids || !dst_slot_ids))) {
    set_error("kv_pool_copy: null id array of the KV pools (src / dst page ids for %lld pairs, src / dst slot ids for %lld: int32 on the device)",
              (long long)n_pages, (long long)n_slots);
    return LQER_E_INVALID;
  }
  // the kernel reaches s_need / d_need bytes of each: two ranges that meet must be ONE pool (the caller then keeps sources and destinations apart)
  const uintptr_t s0 = (uintptr_t)src_pool, d0 = (uintptr_t)dst_pool;
  if (s0 < d0 + d_need && d0 < s0 + s_need && !(s0 == d0 && src_pages == dst_pages && src_slots == dst_slots)) {
    set_error("kv_pool_copy: source KV pool %p (%zu B, %lld pages, %lld slots) and destination %p (%zu B, %lld pages, %lld slots) overlap "
              "without being the same pool", src_pool, s_need, (long long)src_pages, (long long)src_slots, (const void*)dst_pool, d_need,
              (long long)dst_pages, (long long)dst_slots);
    return LQER_E_INVALID;
  }
  const int64_t room = (((int64_t)1 << 31) - 1) / kv_heads;  // (a workgroup per (pair, kv head) over grid.x)
  if (n_pages > room || n_slots > room || n_pages + n_slots > room) {
    set_error("kv_pool_copy: (%lld page pairs + %lld slot pairs) x %lld kv heads of the KV pools beyond one launch grid: copy in pieces",
              (long long)n_pages, (long long)n_slots, (long long)kv_heads);
    return LQER_E_UNSUPPORTED;
  }
  if (n_pages + n_slots == 0) return LQER_OK;
  return kv_pool_copy_dispatch(s, d, src_page_ids, dst_page_ids, n_pages, src_slot_ids, dst_slot_ids, n_slots, (hipStream_t)stream);
}

size_t lqer_attention_q_decode_paged_workspace_bytes(int64_t batch, int64_t heads, int64_t kv_heads, int64_t S, int64_t max_len, int64_t D) {
  if (batch <= 0 || heads <= 0 || kv_heads <= 0 || S <= 0 || max_len <= 0 || D <= 0) return 0;
  return attention_q_decode_paged_workspace_bytes(batch, heads, S, max_len, D);
}

// the check for the kernel that will run, the cache's or the pool's check where K and V come from one, the launches
static int attn_run(const char* who, const AttnKernel& kn, const AttnCall& c) {
  if (c.paged && (c.pool.k4 || c.pool.v4)) {  // a pool with nibble codes (PagedAttn resolved k_fmt / v_fmt: non-null where the flag is set)
    if (const int rc4 = pool_nibble_check(who, c.pool, c.k_fmt, c.v_fmt)) return rc4;
    if (c.grouped) {
      set_error("%s: k_fmt / v_fmt of kind LQER_Q_MXINT_C4 - the grouped kernels are not instantiated for nibble codes; "
                "lqer_attention_q_decode_paged gives the same bits", who);
      return LQER_E_UNSUPPORTED;
    }
  }
  int rc = attn_check(who, kn, c);
  if (rc != LQER_OK) return rc > 0 ? LQER_OK : rc;
  if (c.paged) {
    rc = kv_pool_check(who, c.pool, POOL_BATCH);  // (attn_check has seen D and the four quantizers)
    if (rc != LQER_OK) return rc;
  } else if (c.packed) {
    rc = kv_cache_check(who, c.cache, c.cache_bytes, c.dtype, c.batch, c.kv_heads, c.capacity, c.D, c.T, c.k_fmt, c.v_fmt);
    if (rc != LQER_OK) return rc;
  }
  return kn.dispatch(c);
}

// what every attention entry point fills alike; each then says where K and V come from
static AttnCall attn_call(const void* q, const void* mask, void* out, float* row_stats, int dtype, int64_t batch, int64_t heads, int64_t kv_heads,
                          int64_t S, int64_t T, int64_t D, const int64_t* q_strides, const int64_t* mask_strides, const int64_t* out_strides,
                          float scaling, int causal, const lqer_qfmt_t* q_fmt, const lqer_qfmt_t* k_fmt, const lqer_qfmt_t* p_fmt,
                          const lqer_qfmt_t* v_fmt, void* workspace, size_t workspace_bytes, void* stream) {
  AttnCall c = {};
  c.q = q, c.mask = mask, c.out = out, c.row_stats = row_stats, c.dtype = dtype;
  c.batch = batch, c.heads = heads, c.kv_heads = kv_heads, c.S = S, c.T = T, c.D = D;
  c.qs = q_strides, c.ms = mask_strides, c.os = out_strides, c.scaling = scaling, c.causal = causal;
  c.q_fmt = q_fmt, c.k_fmt = k_fmt, c.p_fmt = p_fmt, c.v_fmt = v_fmt;
  c.workspace = workspace, c.workspace_bytes = workspace_bytes, c.st = (hipStream_t)stream;
  return c;
}

int lqer_attention_q(const void* q, const void* k, const void* v, const void* mask, void* out, float* row_stats, int dtype, int64_t batch,
                     int64_t heads, int64_t kv_heads, int64_t S, int64_t T, int64_t D, const int64_t* q_strides, const int64_t* k_strides,
                     const int64_t* v_strides, const int64_t* mask_strides, const int64_t* out_strides, float scaling, int causal,
                     const lqer_qfmt_t* q_fmt, const lqer_qfmt_t* k_fmt, const lqer_qfmt_t* p_fmt, const lqer_qfmt_t* v_fmt, void* workspace,
                     size_t workspace_bytes, void* stream) {
  AttnCall c = attn_call(q, mask, out, row_stats, dtype, batch, heads, kv_heads, S, T, D, q_strides, mask_strides, out_strides, scaling, causal, q_fmt,
                         k_fmt, p_fmt, v_fmt, workspace, workspace_bytes, stream);
  c.k = k, c.v = v, c.ks = k_strides, c.vs = v_strides;
  return attn_run("attention_q", ATTN_PREFILL, c);
}

int lqer_attention_q_decode(const void* q, const void* k, const void* v, const void* mask, void* out, float* row_stats, int dtype, int64_t batch,
                            int64_t heads, int64_t kv_heads, int64_t S, int64_t T, int64_t D, const int64_t* q_strides, const int64_t* k_strides,
                            const int64_t* v_strides, const int64_t* mask_strides, const int64_t* out_strides, float scaling, int causal,
                            const lqer_qfmt_t* q_fmt, const lqer_qfmt_t* k_fmt, const lqer_qfmt_t* p_fmt, const lqer_qfmt_t* v_fmt, void* workspace,
                            size_t workspace_bytes, void* stream) {
  AttnCall c = attn_call(q, mask, out, row_stats, dtype, batch, heads, kv_heads, S, T, D, q_strides, mask_strides, out_strides, scaling, causal, q_fmt,
                         k_fmt, p_fmt, v_fmt, workspace, workspace_bytes, stream);
  c.k = k, c.v = v, c.ks = k_strides, c.vs = v_strides;
  return attn_run("attention_q_decode", ATTN_DECODE, c);
}

int lqer_attention_q_decode_kv(const void* q, const void* cache, size_t cache_bytes, int64_t capacity, const void* mask, void* out, float* row_stats,
                               int dtype, int64_t batch, int64_t heads, int64_t kv_heads, int64_t S, int64_t T, int64_t D, const int64_t* q_strides,
                               const int64_t* mask_strides, const int64_t* out_strides, float scaling, int causal, const lqer_qfmt_t* q_fmt,
                               const lqer_qfmt_t* k_fmt, const lqer_qfmt_t* p_fmt, const lqer_qfmt_t* v_fmt, void* workspace, size_t workspace_bytes,
                               void* stream) {
  AttnCall c = attn_call(q, mask, out, row_stats, dtype, batch, heads, kv_heads, S, T, D, q_strides, mask_strides, out_strides, scaling, causal, q_fmt,
                         k_fmt, p_fmt, v_fmt, workspace, workspace_bytes, stream);
  c.packed = true, c.cache = cache, c.cache_bytes = cache_bytes, c.capacity = capacity;
  return attn_run("attention_q_decode_kv", ATTN_DECODE, c);
}

int lqer_attention_q_kv(const void* q, const void* cache, size_t cache_bytes, int64_t capacity, const void* mask, void* out, float* row_stats,
                        int dtype, int64_t batch, int64_t heads, int64_t kv_heads, int64_t S, int64_t T, int64_t D, const int64_t* q_strides,
                        const int64_t* mask_strides, const int64_t* out_strides, float scaling, int causal, const lqer_qfmt_t* q_fmt,
                        const lqer_qfmt_t* k_fmt, const lqer_qfmt_t* p_fmt, const lqer_qfmt_t* v_fmt, void* workspace, size_t workspace_bytes,
                        void* stream) {
  AttnCall c = attn_call(q, mask, out, row_stats, dtype, batch, heads, kv_heads, S, T, D, q_strides, mask_strides, out_strides, scaling, causal, q_fmt,
                         k_fmt, p_fmt, v_fmt, workspace, workspace_bytes, stream);
  c.packed = true, c.cache = cache, c.cache_bytes = cache_bytes, c.capacity = capacity;
  return attn_run("attention_q_kv", ATTN_PREFILL, c);
}

// The record of an attention call over the pool from the arguments all ten entries have, in the ABI's order (no mask; T: the bound max_len -
// the check's, the workspace's).  Built in place, never copied: with per-sequence counts it points into the stride triples it holds.
struct PagedAttn {
  AttnCall c;
  int64_t qs[3], os[3];
  PoolFmts own;  // k_fmt / v_fmt of kind LQER_Q_MXINT_C4 as the formats the kernels go by (pool_code_fmt); c.pool knows the storage
  PagedAttn(const void* q, const void* pool, size_t pool_bytes, int64_t pages, int64_t slots, const int32_t* block_table, int64_t table_stride,
            const int32_t* seq_slots, const int32_t* lens, int64_t max_len, void* out, float* row_stats, int dtype, int64_t batch, int64_t heads,
            int64_t kv_heads, int64_t S, int64_t D, const int64_t* q_strides, const int64_t* out_strides, float scaling, int causal,
            const lqer_qfmt_t* q_fmt, const lqer_qfmt_t* k_fmt, const lqer_qfmt_t* p_fmt, const lqer_qfmt_t* v_fmt, void* workspace,
            size_t workspace_bytes, void* stream)
      : c(attn_call(q, nullptr, out, row_stats, dtype, batch, heads, kv_heads, S, max_len, D, q_strides, nullptr, out_strides, scaling, causal, q_fmt,
                    k_fmt, p_fmt, v_fmt, workspace, workspace_bytes, stream)) {
    c.packed = c.paged = true;
    c.pool = kv_pool(pool, pool_bytes, pages, slots, block_table, table_stride, seq_slots, lens, max_len, dtype, kv_heads, D);
    own.resolve(c.pool, c.k_fmt, c.v_fmt);
  }
  PagedAttn(const PagedAttn&) = delete;
  // per-sequence counts: a stride pair (token, head) becomes the triple (batch, head, row) the record holds, with no batch stride - a
  // sequence's rows start at its token starts[b]; null strides stay null, for the check to refuse
  void ragged(const int32_t* starts, int64_t total) {
    c.pool.ragged = true, c.pool.starts = starts, c.pool.total = total;
    c.qs = triple(qs, c.qs), c.os = triple(os, c.os);
  }
  static const int64_t* triple(int64_t (&t)[3], const int64_t* pair) { return pair ? (t[0] = 0, t[1] = pair[1], t[2] = pair[0], t) : nullptr; }
};

int lqer_attention_q_decode_paged(const void* q, const void* pool, size_t pool_bytes, int64_t pages, int64_t slots, const int32_t* block_table,
                                  int64_t table_stride, const int32_t* seq_slots, const int32_t* lens, int64_t max_len, void* out, float* row_stats,
                                  int dtype, int64_t batch, int64_t heads, int64_t kv_heads, int64_t S, int64_t D, const int64_t* q_strides,
                                  const int64_t* out_strides, float scaling, int causal, const lqer_qfmt_t* q_fmt, const lqer_qfmt_t* k_fmt,
                                  const lqer_qfmt_t* p_fmt, const lqer_qfmt_t* v_fmt, void* workspace, size_t workspace_bytes, void* stream) {
  const PagedAttn a(q, pool, pool_bytes, pages, slots, block_table, table_stride, seq_slots, lens, max_len, out, row_stats, dtype, batch, heads,
                    kv_heads, S, D, q_strides, out_strides, scaling, causal, q_fmt, k_fmt, p_fmt, v_fmt, workspace, workspace_bytes, stream);
  return attn_run("attention_q_decode_paged", ATTN_DECODE, a.c);
}

int lqer_attention_q_decode_paged_window(const void* q, const void* pool, size_t pool_bytes, int64_t pages, int64_t slots, const int32_t* block_table,
                                         int64_t table_stride, const int32_t* seq_slots, const int32_t* lens, int64_t max_len, void* out,
                                         float* row_stats, int dtype, int64_t batch, int64_t heads, int64_t kv_heads, int64_t S, int64_t D,
                                         const int64_t* q_strides, const int64_t* out_strides, float scaling, int causal, const lqer_qfmt_t* q_fmt,
                                         const lqer_qfmt_t* k_fmt, const lqer_qfmt_t* p_fmt, const lqer_qfmt_t* v_fmt, void* workspace,
                                         size_t workspace_bytes, void* stream, int64_t window) {
  PagedAttn a(q, pool, pool_bytes, pages, slots, block_table, table_stride, seq_slots, lens, max_len, out, row_stats, dtype, batch, heads, kv_heads, S,
              D, q_strides, out_strides, scaling, causal, q_fmt, k_fmt, p_fmt, v_fmt, workspace, workspace_bytes, stream);
  a.c.windowed = true, a.c.window = window;  // (the call above with the window rule; grid and workspace still follow max_len)
  return attn_run("attention_q_decode_paged_window", ATTN_DECODE, a.c);
}

int lqer_attention_q_decode_chunk(int64_t T, int64_t D) { return attention_q_decode_chunk(T, D); }

int lqer_attention_q_decode_paged_shared(const void* q, const void* pool, size_t pool_bytes, int64_t pages, int64_t slots, const int32_t* block_table,
                                         int64_t table_stride, const int32_t* seq_slots, const int32_t* lens, int64_t max_len, void* out,
                                         float* row_stats, int dtype, int64_t batch, int64_t heads, int64_t kv_heads, int64_t S, int64_t D,
                                         const int64_t* q_strides, const int64_t* out_strides, float scaling, int causal, const lqer_qfmt_t* q_fmt,
                                         const lqer_qfmt_t* k_fmt, const lqer_qfmt_t* p_fmt, const lqer_qfmt_t* v_fmt, void* workspace,
                                         size_t workspace_bytes, void* stream, const int32_t* grp_of, const int32_t* grp_starts,
                                         const int32_t* grp_members, const int32_t* grp_keys, int64_t n_groups) {
  PagedAttn a(q, pool, pool_bytes, pages, slots, block_table, table_stride, seq_slots, lens, max_len, out, row_stats, dtype, batch, heads, kv_heads, S,
              D, q_strides, out_strides, scaling, causal, q_fmt, k_fmt, p_fmt, v_fmt, workspace, workspace_bytes, stream);
  // (lqer_attention_q_decode_paged with a shared chunk read once per group; grid and workspace are that call's)
  a.c.grouped = true, a.c.grp_of = grp_of, a.c.grp_starts = grp_starts, a.c.grp_members = grp_members, a.c.grp_keys = grp_keys;
  a.c.n_groups = n_groups;
  return attn_run("attention_q_decode_paged_shared", ATTN_DECODE, a.c);
}

size_t lqer_attention_q_paged_workspace_bytes(int64_t batch, int64_t heads, int64_t kv_heads, int64_t S, int64_t max_len, int64_t D) {
  return lqer_attention_q_kv_workspace_bytes(batch, heads, kv_heads, S, max_len, D);
}

int lqer_attention_q_paged(const void* q, const void* pool, size_t pool_bytes, int64_t pages, int64_t slots, const int32_t* block_table,
                           int64_t table_stride, const int32_t* seq_slots, const int32_t* lens, int64_t max_len, void* out, float* row_stats,
                           int dtype, int64_t batch, int64_t heads, int64_t kv_heads, int64_t S, int64_t D, const int64_t* q_strides,
                           const int64_t* out_strides, float scaling, int causal, const lqer_qfmt_t* q_fmt, const lqer_qfmt_t* k_fmt,
                           const lqer_qfmt_t* p_fmt, const lqer_qfmt_t* v_fmt, void* workspace, size_t workspace_bytes, void* stream) {
  const PagedAttn a(q, pool, pool_bytes, pages, slots, block_table, table_stride, seq_slots, lens, max_len, out, row_stats, dtype, batch, heads,
                    kv_heads, S, D, q_strides, out_strides, scaling, causal, q_fmt, k_fmt, p_fmt, v_fmt, workspace, workspace_bytes, stream);
  return attn_run("attention_q_paged", ATTN_PREFILL, a.c);  // (the prefill kernel's limits and workspace at T = max_len)
}

int lqer_attention_q_paged_window(const void* q, const void* pool, size_t pool_bytes, int64_t pages, int64_t slots, const int32_t* block_table,
                                  int64_t table_stride, const int32_t* seq_slots, const int32_t* lens, int64_t max_len, void* out, float* row_stats,
                                  int dtype, int64_t batch, int64_t heads, int64_t kv_heads, int64_t S, int64_t D, const int64_t* q_strides,
                                  const int64_t* out_strides, float scaling, int causal, const lqer_qfmt_t* q_fmt, const lqer_qfmt_t* k_fmt,
                                  const lqer_qfmt_t* p_fmt, const lqer_qfmt_t* v_fmt, void* workspace, size_t workspace_bytes, void* stream,
                                  int64_t window) {
  PagedAttn a(q, pool, pool_bytes, pages, slots, block_table, table_stride, seq_slots, lens, max_len, out, row_stats, dtype, batch, heads, kv_heads, S,
              D, q_strides, out_strides, scaling, causal, q_fmt, k_fmt, p_fmt, v_fmt, workspace, workspace_bytes, stream);
  a.c.windowed = true, a.c.window = window;  // (the call above with the window rule; grid and workspace still follow max_len)
  return attn_run("attention_q_paged_window", ATTN_PREFILL, a.c);
}

size_t lqer_attention_q_paged_ragged_workspace_bytes(int64_t batch, int64_t heads, int64_t kv_heads, int64_t max_s, int64_t max_len, int64_t D) {
  return lqer_attention_q_paged_workspace_bytes(batch, heads, kv_heads, max_s, max_len, D);  // (the images only: nothing follows the counts)
}

int lqer_attention_q_paged_ragged(const void* q, const void* pool, size_t pool_bytes, int64_t pages, int64_t slots, const int32_t* block_table,
                                  int64_t table_stride, const int32_t* seq_slots, const int32_t* lens, int64_t max_len, void* out, float* row_stats,
                                  int dtype, int64_t batch, int64_t heads, int64_t kv_heads, const int32_t* q_starts, int64_t max_s, int64_t total,
                                  int64_t D, const int64_t* q_strides, const int64_t* out_strides, float scaling, int causal,
                                  const lqer_qfmt_t* q_fmt, const lqer_qfmt_t* k_fmt, const lqer_qfmt_t* p_fmt, const lqer_qfmt_t* v_fmt,
                                  void* workspace, size_t workspace_bytes, void* stream) {
  // (S: the bound max_s - the check's, the grid's)
  PagedAttn a(q, pool, pool_bytes, pages, slots, block_table, table_stride, seq_slots, lens, max_len, out, row_stats, dtype, batch, heads, kv_heads,
              max_s, D, q_strides, out_strides, scaling, causal, q_fmt, k_fmt, p_fmt, v_fmt, workspace, workspace_bytes, stream);
  a.ragged(q_starts, total);
  return attn_run("attention_q_paged_ragged", ATTN_PREFILL, a.c);  // (the prefill kernel's limits and workspace at T = max_len)
}

int lqer_attention_q_paged_ragged_window(const void* q, const void* pool, size_t pool_bytes, int64_t pages, int64_t slots,
                                         const int32_t* block_table, int64_t table_stride, const int32_t* seq_slots, const int32_t* lens,
                                         int64_t max_len, void* out, float* row_stats, int dtype, int64_t batch, int64_t heads,
                                         int64_t kv_heads, const int32_t* q_starts, int64_t max_s, int64_t total, int64_t D,
                                         const int64_t* q_strides, const int64_t* out_strides, float scaling, int causal,
                                         const lqer_qfmt_t* q_fmt, const lqer_qfmt_t* k_fmt, const lqer_qfmt_t* p_fmt, const lqer_qfmt_t* v_fmt,
                                         void* workspace, size_t workspace_bytes, void* stream, int64_t window) {
  PagedAttn a(q, pool, pool_bytes, pages, slots, block_table, table_stride, seq_slots, lens, max_len, out, row_stats, dtype, batch, heads, kv_heads,
              max_s, D, q_strides, out_strides, scaling, causal, q_fmt, k_fmt, p_fmt, v_fmt, workspace, workspace_bytes, stream);
  a.ragged(q_starts, total);
  a.c.windowed = true, a.c.window = window;  // (the call above with the window rule, every sequence by its own count)
  return attn_run("attention_q_paged_ragged_window", ATTN_PREFILL, a.c);
}

size_t lqer_attention_q_decode_paged_ragged_workspace_bytes(int64_t total, int64_t heads, int64_t max_len, int64_t D) {
  if (total <= 0 || heads <= 0 || max_len <= 0 || D <= 0) return 0;
  return attention_q_decode_paged_ragged_workspace_bytes(total, heads, max_len, D);
}

int lqer_attention_q_decode_paged_ragged(const void* q, const void* pool, size_t pool_bytes, int64_t pages, int64_t slots,
                                         const int32_t* block_table, int64_t table_stride, const int32_t* seq_slots, const int32_t* lens,
                                         int64_t max_len, void* out, float* row_stats, int dtype, int64_t batch, int64_t heads,
                                         int64_t kv_heads, const int32_t* q_starts, int64_t max_s, int64_t total, int64_t D,
                                         const int64_t* q_strides, const int64_t* out_strides, float scaling, int causal,
                                         const lqer_qfmt_t* q_fmt, const lqer_qfmt_t* k_fmt, const lqer_qfmt_t* p_fmt, const lqer_qfmt_t* v_fmt,
                                         void* workspace, size_t workspace_bytes, void* stream, int64_t window) {
  // the call above on the decode kernels: S the bound max_s (here <= 8), and the window rule when window != 0 (a negative one is the
  // check's to refuse)
  PagedAttn a(q, pool, pool_bytes, pages, slots, block_table, table_stride, seq_slots, lens, max_len, out, row_stats, dtype, batch, heads, kv_heads,
              max_s, D, q_strides, out_strides, scaling, causal, q_fmt, k_fmt, p_fmt, v_fmt, workspace, workspace_bytes, stream);
  a.ragged(q_starts, total);
  a.c.windowed = window != 0, a.c.window = window;
  return attn_run("attention_q_decode_paged_ragged", ATTN_DECODE, a.c);
}

int lqer_attention_q_decode_paged_tree(const void* q, const void* pool, size_t pool_bytes, int64_t pages, int64_t slots,
                                       const int32_t* block_table, int64_t table_stride, const int32_t* seq_slots, const int32_t* lens,
                                       int64_t max_len, void* out, float* row_stats, int dtype, int64_t batch, int64_t heads, int64_t kv_heads,
                                       const int32_t* q_starts, int64_t max_s, int64_t total, int64_t D, const int64_t* q_strides,
                                       const int64_t* out_strides, float scaling, int causal, const lqer_qfmt_t* q_fmt,
                                       const lqer_qfmt_t* k_fmt, const lqer_qfmt_t* p_fmt, const lqer_qfmt_t* v_fmt, void* workspace,
                                       size_t workspace_bytes, void* stream, const uint64_t* tree) {
  // lqer_attention_q_decode_paged_ragged without a window, every row with the word of its node of the sequence's draft tree
  PagedAttn a(q, pool, pool_bytes, pages, slots, block_table, table_stride, seq_slots, lens, max_len, out, row_stats, dtype, batch, heads, kv_heads,
              max_s, D, q_strides, out_strides, scaling, causal, q_fmt, k_fmt, p_fmt, v_fmt, workspace, workspace_bytes, stream);
  a.ragged(q_starts, total);
  a.c.treed = true, a.c.tree = tree;
  return attn_run("attention_q_decode_paged_tree", ATTN_DECODE, a.c);
}

int lqer_attention_q_paged_tree(const void* q, const void* pool, size_t pool_bytes, int64_t pages, int64_t slots, const int32_t* block_table,
                                int64_t table_stride, const int32_t* seq_slots, const int32_t* lens, int64_t max_len, void* out, float* row_stats,
                                int dtype, int64_t batch, int64_t heads, int64_t kv_heads, const int32_t* q_starts, int64_t max_s, int64_t total,
                                int64_t D, const int64_t* q_strides, const int64_t* out_strides, float scaling, int causal,
                                const lqer_qfmt_t* q_fmt, const lqer_qfmt_t* k_fmt, const lqer_qfmt_t* p_fmt, const lqer_qfmt_t* v_fmt,
                                void* workspace, size_t workspace_bytes, void* stream, const uint64_t* tree) {
  // lqer_attention_q_paged_ragged for trees of up to 64 nodes: the image kernels as they are, the attention kernel's TREE instantiation
  PagedAttn a(q, pool, pool_bytes, pages, slots, block_table, table_stride, seq_slots, lens, max_len, out, row_stats, dtype, batch, heads, kv_heads,
              max_s, D, q_strides, out_strides, scaling, causal, q_fmt, k_fmt, p_fmt, v_fmt, workspace, workspace_bytes, stream);
  a.ragged(q_starts, total);
  a.c.treed = true, a.c.tree = tree;
  return attn_run("attention_q_paged_tree", ATTN_PREFILL, a.c);
}

int lqer_replicate_rows(const void* src, void* dst, int64_t rows, int64_t row_bytes, int copies, void* stream) {
  if (!src || !dst || rows < 0 || row_bytes < 0 || copies < 1) {
    set_error("replicate_rows: bad argument");
    return LQER_E_INVALID;
  }
  if (rows == 0 || row_bytes == 0) return LQER_OK;
  for (int c = 0; c < copies; ++c) {
    const hipError_t e = hipMemcpy2DAsync((char*)dst + (size_t)c * row_bytes, (size_t)copies * row_bytes, src, (size_t)row_bytes,
                                          (size_t)row_bytes, (size_t)rows, hipMemcpyDeviceToDevice, (hipStream_t)stream);
    if (e != hipSuccess) {
      set_error("replicate_rows: %s", hipGetErrorString(e));
      return LQER_E_LAUNCH;
    }
  }
  return LQER_OK;
}

}  // extern "C"
