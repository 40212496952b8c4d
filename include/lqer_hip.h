/*
 * lqer_hip.h - C ABI of liblqer_hip.so: the MI355X (gfx950) implementation of the LQER quantized
 * Linear forward      y = Q_x(x) W_q^T + b_q + Q_Bout( Q_Aout( Q_x(x) A ) B )
 *
 * The reference (ChengZhang-98/lqer) is pure Python and has no FFI: its boundary for this path is
 * the nn.Module `LinearFlexibleLqer` (src/lqer/quantize/quantized_layers/linear.py:112-166).  Each
 * entry point below replaces one step of that module's forward; the reference line it stands in
 * for is cited on the declaration.  The Python mirror of the module (lqer_amd/linear.py) binds
 * these with ctypes; INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *  - plain pointers and sizes only; every pointer is a DEVICE pointer unless named host_*;
 *  - kernels are launched on the calling thread's CURRENT HIP device: the caller makes the device that owns the buffers
 *    current (hipSetDevice) before the call - the Python mirror does (lqer_amd/linear.py, ops.py);
 *  - the caller owns every buffer (incl. workspace); the library never allocates, frees or
 *    retains pointers, and is re-entrant (its only process-wide state are std::once_flag-guarded, idempotent kernel
 *    attribute settings, one atomic call counter - the tag of the one-launch decode route, see lqer_linear_forward - and
 *    the thread-local error text; kernel-selection knobs for tests travel in the descriptor: lqer_linear_desc_t.tuning);
 *  - every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = default
 *    stream) and performs no host synchronisation, so calls may be captured in a hipGraph;
 *  - return value 0 = success, <0 = error (LQER_E_*); lqer_last_error() gives the text of the
 *    last error raised on the calling thread.
 *  - extents (held by tests/test_gpu_footprint.py between guard zones, at exactly these sizes): a strided tensor x / y / W of
 *    [rows, cols] with row stride ld is (rows - 1) * ld + cols elements - no call writes a column >= cols of any row (the gaps
 *    between the rows of y keep their bytes) or anything behind the last element of the last row, whatever ld and the
 *    pointer's alignment are (rows that are not 16-byte aligned take element stores: same bits); every other output is written
 *    inside the size its declaration names and, for the one-time images (lqer_pack_*, lqer_*_prepare), written WHOLE - padding
 *    included - so an image never carries bytes of whatever the buffer held before.  The per-call buffers are the exception by
 *    design: xq has lqer_padded_m(M) rows of which only rows < M are written (the tile kernels read the others; no output bit
 *    of a row < M depends on them), xaq likewise ([lqer_padded_m(M)][padded rank x limbs] bf16, 16-byte aligned), and
 *    workspace / scratch contents are never assumed: every call gives the same bits over any previous contents, NaN patterns
 *    included.  Inputs are never written.  workspace, xq, xaq, scratch: 256-byte aligned in the tests; the group workspace and
 *    the small flag / count outputs: 16-byte aligned there.
 *  - "MXINT(w, L)" = the reference's block_fp format (quantizers/block_fp.py:7-82): blocks of L
 *    consecutive elements along the last dim share an exponent e = ceil(log2(max|block|)); each
 *    element is a sign and a (w-1)-bit magnitude m; value = +-m * 2^(e-(w-1)).
 */
#ifndef LQER_HIP_H
#define LQER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LQER_ABI_VERSION 14

/* error codes */
#define LQER_OK 0
#define LQER_E_INVALID (-1)     /* bad argument (null pointer, negative size, misalignment) */
#define LQER_E_UNSUPPORTED (-2) /* format / shape outside what the kernels implement       */
#define LQER_E_LAUNCH (-3)      /* HIP reported an error at launch                          */
#define LQER_E_WORKSPACE (-4)   /* workspace too small                                     */

/* element types of caller tensors */
#define LQER_F32 0
#define LQER_F16 1
#define LQER_BF16 2

/* quantizer kinds (reference quantizers/__init__.py:7-18) */
#define LQER_Q_PASSTHROUGH 0
#define LQER_Q_MXINT 1 /* "block_fp" */
#define LQER_Q_PASSTHROUGH_F16 2 /* x_fmt only: pass-through fp16 activations multiplied natively (v_mfma_*_f16) - needs
                                    lqer_f16_prepare to report both operands exact, see "pass-through activations" */

#define LQER_Q_MXINT_I8 3 /* x_fmt only: block_fp activations with ONE block per row (width <= 8) carried as int8 mantissas and
                            multiplied on the int8 MFMA - needs lqer_i8_prepare to report the weight eligible, see "int8 route" */

#define LQER_Q_INT 4 /* "integer" (reference quantizers/integer.py:10-43): fixed point, clamp(rne(x 2^frac), lo, hi) / 2^frac with
                        lo, hi = -2^(width-1), 2^(width-1)-1 (signed) or 0, 2^width-1.  Fields: width; exp_bias = frac_width;
                        exp_width = is_signed (1 / 0); block is ignored.  Implemented for the x, b and A_out quantizers (width
                        <= 9 signed / 8 unsigned, so that every value is a bf16 number), for B_out (any width <= 24: applied to
                        the fp32 side product inside the tile kernels' prologues - the reference's fall-back when x_quantizer is
                        integer, linear.py:115-119; decode sizes then take the tile kernel) and in lqer_quantize_mxint; as
                        w_quantizer: signed, width 2..4 - the codes -8..7 travel as two's-complement nibbles in the same panels
                        (lqer_pack_weight_mxint; the 128-row tile kernel at every token count); unsigned or wider integer
                        weights: LQER_E_UNSUPPORTED */

#define LQER_Q_MINIFLOAT 5 /* "minifloat" (reference quantizers/minifloat.py:120-182, minifloat_ieee): per element, in fp32,
                        e = clamp(floor(log2(|x| + 1e-9)), -exp_bias, 2^exp_width-1-exp_bias) with torch's correctly rounded log2;
                        m = width-exp_width-1 mantissa bits; normal (e != -exp_bias): S = clamp(rne(|x| 2^(m-e) - 2^m), 0, 2^m-1),
                        v = 2^e (1 + S 2^-m); subnormal (e == -exp_bias): S = clamp(rne(|x| 2^(m-1-e)), 0, 2^m-1),
                        v = 2^(e+1) S 2^-m; result sign(x) v (no rounding into the next binade, no inf / NaN: the largest value is
                        (2 - 2^-m) 2^(2^exp_width-1-exp_bias)); |x| <= 1e-8 is kept as is (packed and bf16 images: 0).  Fields:
                        width 2..8; exp_width 1..width-1; exp_bias = the resolved bias (reference default 2^(exp_width-1)-1),
                        such that every non-zero value is a normal bf16 number; block is ignored.  Implemented for the x, b,
                        A_out and B_out quantizers (elementwise: no maxima, no pre-pass - B_out in the 128-row tile kernel's
                        prologue at every token count), in lqer_quantize_mxint (deq, and as codes the minifloat bit pattern
                        sign | exponent | mantissa; exps must be NULL) and as w_quantizer of width 2..4: the nibble holds
                        sign << 3 | exponent << m | mantissa, expanded through a per-format 8-entry e4m3 table times one
                        constant power-of-two scale (lqer_pack_weight_mxint; the 128-row tile kernel at every token count).
                        Minifloat weights of 5..8 bits, minifloat on the int8 route (LQER_Q_MXINT_I8) and 2-D weight tiles:
                        LQER_E_UNSUPPORTED */

#define LQER_Q_MXINT_C4 6 /* k_fmt / v_fmt of the paged KV pool's entries only: block_fp quantized exactly as LQER_Q_MXINT of the same
                            width, exp_width and exp_bias (width 2..4, block 16), the operand's codes STORED AS NIBBLES - two per byte,
                            see "paged KV pool", nibble codes.  Names a storage, as the two kinds above name a route, not another
                            quantizer.  Anywhere else - q / p formats, the dense lqer_kv_cache_* entries, a Linear's formats,
                            lqer_attention_q_decode_paged_shared - LQER_E_UNSUPPORTED */

/* Geometry of the packed operands (fixed by the kernels; exported so callers can size buffers). */
#define LQER_K_ALIGN 64     /* K is zero-padded to a multiple of this                        */
#define LQER_M_ALIGN 256    /* activation workspaces are row-padded to a multiple of this    */
#define LQER_N_ALIGN 256    /* packed weights are row-padded to a multiple of this           */
#define LQER_R_ALIGN 16     /* rank is zero-padded to a multiple of this                     */
#define LQER_PANEL_ROWS 16  /* packed W: panels of 16 rows x 64 k                            */
#define LQER_PANEL_BYTES 576 /* 16*32 B of 4-bit codes + 16*4 B of block exponents           */

/* One MXINT quantizer: `width` bits per element incl. sign; `block` elements share an exponent
 * (block <= 0: one block per row); exponent clamped to [-exp_bias, 2^exp_width-1-exp_bias]
 * (block_fp.py:46-51; exp_width=8, exp_bias=127 in every template config): e = clamp(ceil(log2(max |x|)), emin, emax) with
 * emin = -exp_bias, emax = 2^exp_width - 1 - exp_bias, for exp_width 1..8.  The bias is bounded like the minifloat one: a format with
 * emax - (width - 1) < -126 or emin > 127 is LQER_E_UNSUPPORTED (the message states the range).  Every kernel builds the block scale
 * 2^(e - (width-1)) from exponent bits where that is a normal float and argues that it is not one only for blocks wholly below the
 * 1e-8 flush; that holds for the lower end of any accepted format (e - mbits < -126 then needs max |x| < 2^-119) but not when the
 * UPPER clamp itself lies below mbits - 126, where blocks of any size would take it.  With emin > 127 every block's 2^e is beyond fp32.
 * Accepted biases: [-127, 2^exp_width - 1 - (width-1) + 126]. */
typedef struct lqer_qfmt {
  int32_t kind;      /* LQER_Q_* */
  int32_t width;     /* passthrough (x / A_out): significand bits to carry - 8 bf16, 11 fp16, 24 fp32 - see
                        "pass-through activations" below; ignored for passthrough b / B_out               */
  int32_t block;
  int32_t exp_width;
  int32_t exp_bias;
} lqer_qfmt_t;

/* Static description of one Linear.  M (tokens) is a per-call argument. */
typedef struct lqer_linear_desc {
  int32_t in_features;   /* K */
  int32_t out_features;  /* N */
  int32_t rank;          /* r; 0 = no side path (LinearFlexible, linear.py:88-109) */
  int32_t has_bias;
  lqer_qfmt_t x_fmt;     /* linear.py:148   x_quantizer                        */
  lqer_qfmt_t w_fmt;     /* linear.py:150   w_quantizer (block_fp width <= 8: 5..8 bits see "weights of 5..8 bits"; integer <= 4) */
  lqer_qfmt_t b_fmt;     /* linear.py:152   b_quantizer                        */
  lqer_qfmt_t a_out_fmt; /* linear.py:154   A_out_quantizer                    */
  lqer_qfmt_t b_out_fmt; /* linear.py:155   B_out_quantizer                    */
  int32_t tuning;        /* 0 = the library decides everything (what every caller wants).  LQER_TUNE_* bits: per-CALL kernel
                            selection knobs for tests and measurements - they change which kernel variant runs, never a result
                            bit.  Carried by the descriptor, not by process-wide state: two threads never see each other's. */
} lqer_linear_desc_t;

/* lqer_linear_desc_t.tuning (all variants give the same bits) */
#define LQER_TUNE_TILE_ROWS_128 0x1   /* 128-row kernel family (LQER_ROUTE_TILE128): always 128-row tiles                     */
#define LQER_TUNE_TILE_ROWS_64 0x2    /* ... always 64-row tiles (two workgroups per CU); default: 64 rows when the 128-row grid
                                         covers at most half of the CUs                                                        */
/* 0x3f0: retired (once XCD-local tile blocks in the 128-row and int8 kernels); ignored - do not reuse */
#define LQER_TUNE_I8_ROWS_128 0x4      /* int8 kernel (LQER_ROUTE_I8): always 128-row tiles                                      */
#define LQER_TUNE_I8_ROWS_256 0x8      /* ... always 256-row tiles; default: whichever takes fewer weighted rounds of one tile per
                                         CU (lqer_gemm_tile_rows says which)                                                    */
#define LQER_TUNE_AMAX_ATOMIC 0x40000  /* int8 route, B_out with one block per row: the pre-pass of row maxima with one atomicMax cell per
                                         row behind a zero-fill launch (the round-4 form) instead of per-segment partial maxima in plain
                                         stores that the GEMM folds (no zero-fill launch); max is order-independent: same bits         */
#define LQER_TUNE_AMAX_PARTS 0x80000   /* ... the segment partials at every N (default: up to N = 4096, where they are faster)     */
#define LQER_TUNE_AMAX_XCH_MISS 0x100000 /* int8 route, ONE round of 128-row tiles (at most one tile per CU) and one B_out block per row:
                                         by default there is NO pre-pass launch - every workgroup publishes the row maxima of its own
                                         tile's side product as tagged granules and gathers its row band's at the epilogue (either
                                         AMAX pin above restores the pre-pass).  This bit makes every workgroup treat the others'
                                         granules as missing, i.e. take the fall-back that computes the whole band's maxima itself (a
                                         workgroup that times out on a neighbour does the same): same bits                          */
/* 0x20000: retired (once the partial tiles of x A summed inside the 128-row GEMM); ignored - do not reuse */
#define LQER_TUNE_ACT8_SPLIT 0x200000 /* int8 route (LQER_Q_MXINT_I8), lqer_quantize_act_xa / lqer_linear_forward: quantizer, split-K side GEMM
                                         and reduce as three launches even where the one-launch kernel applies (16-bit tensors, a_limbs =
                                         -1, padded rank 16 / 32 / 64, M <= 4096): bit-identical int8 image and row scales, x A summed in
                                         another order (A_out of it inside the summation-order envelope)                            */
#define LQER_TUNE_ACT8_FUSED 0x400000 /* ... the one-launch kernel at every token count (default: M <= 4096 - every workgroup of 8 token
                                         rows streams the whole A^T image)                                                          */
#define LQER_TUNE_ACT16_SPLIT 0x800000 /* block-16 MXINT activations with a_limbs = -2: the quantizer + split-K kernel and the reduce as two
                                         launches even where the one-launch kernel applies (act16_fused.hip; same image, x A in another
                                         summation order)                                                                            */
#define LQER_TUNE_ACT16_FUSED 0x1000000 /* ... the one-launch kernel at every token count (default: 1024 <= M <= 4096; the same window
                                         applies to LQER_TUNE_ACT8_FUSED's kernel)                                                    */
#define LQER_TUNE_AMAX_NO_MRX 0x4000000 /* int8 route, SEVERAL rounds of 128-row tiles on a resident grid (up to 2048 tokens), one B_out block per
                                           row, 4-bit weights: keep the k_bout_amax pre-pass launch (rounds 3-5) instead of the default - the
                                           GEMM's workgroups compute the pre-pass themselves, one item each at their start, and exchange
                                           tagged granules (csrc/gemm_w4a8_i8.hip, MRX)                                                   */
#define LQER_TUNE_BOUT_IN_PROLOGUE 0x2000000 /* 128-row tile kernel, B_out in blocks of 16: re-quantize the side product in front of the main
                                              loop (rounds 1-5) instead of under its first 16 k-steps with the product added behind the
                                              last one (default from K = 1024; csrc/gemm_w4a8.hip, DEFER)                               */
#define LQER_TUNE_W_EXP_TABLE 0x8000000 /* 128-row kernel family, sign-magnitude 4-bit weights on the bf16 main loop: expand the nibbles
                                           through the e4m3 table (the minifloat weights' instantiations with the integers' table:
                                           128-row tiles, staged side path) instead of reading them as e4m3 subnormals with the
                                           block scale carrying 2^9.  Same bits - and REQUIRED for a weight image that holds an
                                           exponent byte above 245 (a block maximum of 2^121 or more; lqer_f16_prepare reports
                                           it as flags[0] & 2), where byte + 9 leaves the fp32 exponent field                  */
#define LQER_TUNE_NO_KSPLIT 0x10000000 /* 128-row tile kernel, B_out in blocks of 16 under the main loop, side product of at most two
                                          16-deep slices: every wave takes all four k slices of its own 32 columns (each reads the
                                          whole activation slot from LDS) instead of the default - the two waves of a SIMD share 64
                                          columns and take two slices each, and exchange partial sums behind the main loop
                                          (csrc/gemm_w4a8.hip, KSPLIT)                                                          */
#define LQER_TUNE_DECODE_NO_POLL 0x10000 /* one-launch decode route: no wait for the producers' tiles - every weight-streaming
                                         workgroup computes the partial tiles of x A itself (the bounded wait's fall-back)     */

/* Sizes (bytes) of the derived, caller-allocated device buffers of one Linear. */
typedef struct lqer_linear_sizes {
  size_t w_packed;   /* 4-bit codes + block exponents, panel layout            */
  size_t a_t;        /* A^T as bf16 limbs [3][rp][Kp]                          */
  size_t b_t;        /* B^T as bf16 limbs [3][Np][rp]                          */
  size_t bias_q;     /* quantized bias, fp32 [Np]                              */
  size_t workspace;  /* per-call scratch for `m_max` tokens                    */
} lqer_linear_sizes_t;

int lqer_version(void);
const char* lqer_last_error(void);
/* sizeof of the structs above as THIS library was compiled: a binding in another language asserts its own layouts against
 * these once (the library reads sizeof(lqer_linear_desc_t) bytes behind a descriptor pointer - a shorter struct is undefined
 * behaviour).  INTEGRATION.md section B's ctypes stub does; tests/test_abi_cpu.py executes that stub against the library. */
size_t lqer_sizeof_qfmt(void);
size_t lqer_sizeof_linear_desc(void);
size_t lqer_sizeof_linear_sizes(void);
size_t lqer_sizeof_group_member(void);

/* Padded extents used by the packed buffers. */
int64_t lqer_padded_k(int64_t K);
int64_t lqer_padded_n(int64_t N);
int64_t lqer_padded_m(int64_t M);
int64_t lqer_padded_r(int64_t r);

/* ---- quantizers -------------------------------------------------------------------------- */

/* MXINT quantizer over the rows of a [rows, cols] matrix (row stride `ld` elements), blocks along
 * the last dim.  Replaces x_quantizer / A_out_quantizer / B_out_quantizer / b_quantizer calls of
 * linear.py:148,152,154,155 -> block_fp.py:111.  Any of the outputs may be NULL:
 *   deq_f32 [rows, cols]   dequantized values (|x| <= 1e-8 kept as is, block_fp.py:79-80)
 *   codes   [rows, cols]   signed mantissas, int8 (needs width <= 8); |x| <= 1e-8 -> 0
 *   exps    [rows, ceil(cols/L)]  shared exponents, int8 (0 for an all-zero block)          */
int lqer_quantize_mxint(const void* x, int dtype, int64_t rows, int64_t cols, int64_t ld,
                        const lqer_qfmt_t* fmt, float* deq_f32, int8_t* codes, int8_t* exps,
                        void* stream);

/* The same quantizer over 2-D TILES of an activation - blocks that span token rows: x [batches][rows][cols] dense, tiles of
 * tile_rows x tile_cols (<= 0 or larger than the extent: the whole extent) anchored at (0, 0) of every batch element, ragged
 * edges clipped (the reference pads them with zeros, which cannot raise a block maximum).  Replaces block_fp.py:111 ->
 * quantizers/utils.py:211-237 (`_block_3d_activation`: x / A_out / B_out of a [batch, tokens, features] tensor with
 * block_size [R, L], skip_first_dim = true) and utils.py:161-183 as utils.py:261-270 applies it to a 2-D activation with
 * skip_first_dim = false (batches = 1).  deq_f32 [batches][rows][cols]; amax_scratch: one float per tile
 * (batches * ceil(rows / R) * ceil(cols / L)).  A cold path - no template configuration has such blocks; the fused kernels
 * keep per-row blocks. */
int lqer_quantize_mxint_tiles(const void* x, int dtype, int64_t batches, int64_t rows, int64_t cols, const lqer_qfmt_t* fmt,
                              int64_t tile_rows, int64_t tile_cols, float* deq_f32, float* amax_scratch, void* stream);

/* Activation quantizer of the fast path (linear.py:148): x [M,K] -> exact bf16 image
 * xq [lqer_padded_m(M), lqer_padded_k(K)] (K padding zeroed; |x| <= 1e-8 flushed to 0).
 * Needs fmt->width <= 9 so that every value m*2^(e-w+1) is exactly representable in bf16.   */
int lqer_quantize_act_mxint(const void* x, int dtype, int64_t M, int64_t K, int64_t ldx,
                            const lqer_qfmt_t* fmt, void* xq_bf16, void* stream);

/* ---- one-time packing (replaces the in-place first-forward quantization, linear.py:149-153) */

int lqer_linear_sizes(const lqer_linear_desc_t* desc, int64_t m_max, lqer_linear_sizes_t* out);

/* W [N,K] (row stride ldw) -> packed panels: w_quantizer(W) as 4-bit sign-magnitude mantissas
 * (bit 3 = sign) + block exponents.  Panel (n/16, k/64) = 16 rows x 32 B codes followed by
 * 16 x 4 exponent bytes (one per 16 k; a coarser block repeats its exponent), stored biased:
 * byte = clamp(e - (width-1) + 127, 1, 254).  Within each 32-bit word of codes (8 consecutive k)
 * nibble p holds k = p/2 (p even) or 4 + p/2 (p odd); a row's 8 words are stored in the order
 * {0,2,4,6,1,3,5,7}.  |w| <= 1e-8 is flushed to code 0.  `scratch` needs N*ceil(K/16) bytes.   */
int lqer_pack_weight_mxint(const void* W, int dtype, int64_t N, int64_t K, int64_t ldw,
                           const lqer_qfmt_t* fmt, void* w_packed, void* scratch, void* stream);
/* The same for 2-D tiles (w_quantizer block_size [R, L] with skip_first_dim = false, reference quantizers/utils.py:161-183):
 * one exponent per tile of `block_rows` weight rows x fmt->block k (block_rows <= 0 or >= N: all rows; 1 = the call above).  The
 * image layout does not change - a tile's exponent is repeated for each of its rows - so every GEMM route reads it as it is. */
int lqer_pack_weight_mxint_2d(const void* W, int dtype, int64_t N, int64_t K, int64_t ldw,
                              const lqer_qfmt_t* fmt, int64_t block_rows, void* w_packed, void* scratch,
                              void* stream);

/* Test hook: packed panels -> dequantized fp32 [N,K]. */
int lqer_unpack_weight_mxint(const void* w_packed, int64_t N, int64_t K, const lqer_qfmt_t* fmt,
                             float* w_f32, void* stream);

/* A [K,r] and B [r,N] (linear.py:142-143; values as stored in the state dict) -> transposed bf16
 * limb images a_t [3][rp][Kp], b_t [3][Np][rp]; v = limb0 + limb1 + limb2 exactly (an 8-bit
 * MXINT value needs one limb, fp16 two, fp32 three).  limb_flags[0..1] (device int32[2]) receive
 * the number of non-zero limbs of A and of B.                                                */
int lqer_pack_lowrank(const void* A, const void* B, int dtype, int64_t K, int64_t N, int64_t r,
                      void* a_t, void* b_t, int32_t* limb_flags, void* stream);

/* bias [N] -> b_quantizer(bias) as fp32 [Np] (linear.py:151-152). fmt->kind may be passthrough. */
int lqer_pack_bias(const void* bias, int dtype, int64_t N, const lqer_qfmt_t* fmt, float* bias_q,
                   void* stream);

/* ---- the forward (linear.py:145-157, PTQ branch) ------------------------------------------- */

/* y[M,N] (row stride ldy, same dtype as x) from x[M,K] (row stride ldx).  a_limbs / b_limbs =
 * the limb counts reported by lqer_pack_lowrank.  workspace >= lqer_linear_sizes(...).workspace
 * for m_max >= M.  Two to four stream-ordered launches, no host synchronisation: the activation quantizer (fused
 * with the split-K partials of the rank-r side GEMM when x blocks are 16 and the padded rank <= 64; nothing at all for
 * a dense fp16 tensor on the LQER_Q_PASSTHROUGH_F16 route), a fixed-order reduce of the partials with the A_out
 * re-quantization (taken over by the GEMM at decode sizes, lqer_decode_partials), a pre-pass for B_out blocks other
 * than 16 columns, and the fused W4 GEMM with the B side GEMM, B_out re-quantization, bias and add in its prologue.
 * a_limbs = -1 (LQER_Q_MXINT_I8 descriptors at token counts of LQER_ROUTE_I8 only; also lqer_quantize_act_xa and
 * lqer_lowrank_xa): a_t is ONE fp16 image of A^T [padded rank][padded K] as lqer_f16_prepare writes it (its flag for A
 * clear: every element exact in fp16) - the side GEMM then multiplies the int8 mantissas with it on the fp16 MFMA, half
 * the A^T bytes and MFMAs of the two-limb image. */
int lqer_linear_forward(const lqer_linear_desc_t* desc, const void* x, int dtype, int64_t M,
                        int64_t ldx, const void* w_packed, const void* a_t, const void* b_t,
                        int a_limbs, int b_limbs, const float* bias_q, void* y, int64_t ldy,
                        void* workspace, size_t workspace_bytes, void* stream);

/* Up to 8 tokens (block_fp activations in blocks of 16, A_out in blocks of 16, padded rank <= 64, one limb of A, B_out
 * pass-through or in blocks of 16 - lqer_decode_partials -, in_features a multiple of 16 and 16-byte aligned rows of x; anything
 * else at decode sizes: the two-launch route, same bits) lqer_linear_forward issues ONE
 * launch (csrc/decode1.hip): producer workgroups publish the split-K partial tiles of x A as {value, tag} granules in the
 * workspace, the weight-streaming workgroups quantize x themselves and read the tiles at their very end.  The tag is a
 * per-LAUNCH value: a process-wide atomic call counter (the library's only mutable state besides the thread-local error
 * text) mixed, inside the kernel, with the launch's AQL dispatch id and queue address - so the route is taken under stream
 * capture as well: a replayed graph node carries the captured counter but gets a fresh dispatch id, and never accepts the
 * previous replay's tiles.  The wait for the tiles is bounded; a workgroup that does not see them computes them itself
 * (same bits). */

/* The same, split for callers that share one quantized activation between several Linears
 * (q/k/v, gate/up) and for per-stage timing.  xq = output of lqer_quantize_act_mxint.         */
/* x_quantizer + side path in one call: xq and (rank > 0) xaq.  Uses a fused kernel (the activation
 * image is quantized and multiplied by A from LDS, never re-read from HBM) when x blocks are 16 and the
 * padded rank <= 64 - or <= 128 from 512 tokens on, with 16-byte aligned 16-bit rows -, the two separate
 * steps otherwise (same bits).  scratch as for lqer_lowrank_xa.                                      */
int lqer_quantize_act_xa(const lqer_linear_desc_t* desc, const void* x, int dtype, int64_t M,
                         int64_t ldx, const void* a_t, int a_limbs, void* xq_bf16, void* xaq_bf16,
                         void* scratch, size_t scratch_bytes, void* stream);
size_t lqer_lowrank_xa_scratch_bytes(const lqer_linear_desc_t* desc, int64_t m_max);
/* Bytes of the activation image buffer `xq_bf16` of the split calls for up to m_max tokens (what lqer_linear_sizes counts inside
 * `workspace`): [padded M][padded K x activation limbs x weight limbs] bf16, plus - for weights of 5..8 bits - the single-copy
 * image behind it.  xaq and the scratch follow at 256-byte aligned offsets in lqer_linear_forward's own carving. */
size_t lqer_act_image_bytes(const lqer_linear_desc_t* desc, int64_t m_max);
int lqer_lowrank_xa(const lqer_linear_desc_t* desc, const void* xq_bf16, int64_t M,
                    const void* a_t, int a_limbs, void* xaq_bf16, void* scratch,
                    size_t scratch_bytes, void* stream);
/* scratch of lqer_linear_gemm: 0 unless B_out blocks differ from 16 columns (then the kernel needs
 * the per-row-block maxima of xAq @ B: a pre-pass it launches itself - or, on the int8 route with one block per row and one round
 * of 128-row tiles, tagged granules that the GEMM's own workgroups exchange through this scratch, LQER_TUNE_AMAX_XCH_MISS above).
 * The contents of the scratch need no initialisation and may be anything left by earlier calls. */
size_t lqer_linear_gemm_scratch_bytes(const lqer_linear_desc_t* desc, int64_t m_max);
int lqer_linear_gemm(const lqer_linear_desc_t* desc, const void* xq_bf16, int64_t M,
                     const void* w_packed, const void* xaq_bf16, const void* b_t, int b_limbs,
                     const float* bias_q, void* y, int dtype, int64_t ldy, void* scratch,
                     size_t scratch_bytes, void* stream);
/* The zero fill of lqer_linear_gemm's pre-pass, handed to the activation call in front of it (ABI 13).  Launches whose B_out blocks
 * differ from 16 columns and whose grid is more than one round of tiles start with a pre-pass that folds the row-block maxima of
 * xAq @ B with atomicMax into cells at the head of `scratch`, which lqer_linear_gemm zero-fills first - a memset launch between two
 * kernels (4.8 us of a 116-us forward at 2048 x 4096 -> 11008, rank 32).  lqer_quantize_act_xa_prep is lqer_quantize_act_xa which,
 * where its work runs as the one-launch int8 kernel (csrc/act8_fused.hip: LQER_Q_MXINT_I8, a_limbs = -1, 1024..4096 tokens), lets that
 * kernel write those zeros to `gemm_scratch` (one store per thread) and reports in *ready_bytes how many bytes at its head are ready -
 * 0 when nothing was prepared (another route, or a GEMM that needs none).  lqer_linear_gemm_prepared is lqer_linear_gemm which skips
 * its own zero fill when ready_bytes covers its cells.  The caller's side of the contract: the same gemm_scratch / scratch pointer,
 * the same stream, and nothing else writing that scratch between the two calls (it may alias the first call's own `scratch`: the
 * one-launch kernel does not use it).  lqer_linear_forward does this hand-over on its own; same results either way. */
int lqer_quantize_act_xa_prep(const lqer_linear_desc_t* desc, const void* x, int dtype, int64_t M,
                              int64_t ldx, const void* a_t, int a_limbs, void* xq_bf16, void* xaq_bf16,
                              void* scratch, size_t scratch_bytes, void* gemm_scratch, size_t* ready_bytes, void* stream);
int lqer_linear_gemm_prepared(const lqer_linear_desc_t* desc, const void* xq_bf16, int64_t M,
                              const void* w_packed, const void* xaq_bf16, const void* b_t, int b_limbs,
                              const float* bias_q, void* y, int dtype, int64_t ldy, void* scratch,
                              size_t scratch_bytes, size_t ready_bytes, void* stream);

/* Which GEMM kernel lqer_linear_gemm launches for `M` tokens of this descriptor and element type (the choice depends on
 * nothing else): LQER_ROUTE_SMALLM (M <= 64: one workgroup per 16 output columns streams its packed weight rows),
 * LQER_ROUTE_TILE128 (128 x 256 tiles; 64 x 256 tiles of the same kernel when the 128-row grid would cover at most half of
 * the CUs and the side product is at most two 16-deep slices - M = 65..1024 at N = 4096), LQER_ROUTE_TILE256 (256 x 256 tiles, M >= 512 when that needs fewer rounds of one
 * tile per CU).  < 0: the error lqer_linear_gemm would return.  For benchmarks and tests that must know which kernel
 * they are looking at. */
#define LQER_ROUTE_SMALLM 0
#define LQER_ROUTE_TILE128 1
#define LQER_ROUTE_TILE256 2
#define LQER_ROUTE_I8 3 /* int8 MFMA main loop (x_fmt.kind = LQER_Q_MXINT_I8 only): 256 x 256 tiles, or 128 x 256 tiles where those
                           take fewer weighted rounds of one tile per CU (Llama-7B projections at M = 2048) - lqer_gemm_tile_rows */
int lqer_gemm_route(const lqer_linear_desc_t* desc, int64_t M, int dtype);
/* Token rows of a tile of the kernel lqer_gemm_route names: 64 / 128 (LQER_ROUTE_TILE128 family), 256 (LQER_ROUTE_TILE256),
 * 128 / 256 (LQER_ROUTE_I8); 0 for LQER_ROUTE_SMALLM; < 0: the error.  For tests and benchmarks that assert the variant. */
int lqer_gemm_tile_rows(const lqer_linear_desc_t* desc, int64_t M, int dtype);

/* Decode sizes (launch-bound: each kernel runs ~3 us).  Returns 1 when, for this descriptor and token count, the
 * re-quantized side product never has to be materialised: M <= 64, x and A_out block_fp in blocks of 16 (width <= 9),
 * padded rank <= 64, B_out pass-through or in blocks of 16.  Then lqer_quantize_act_xa may be called with
 * xaq_bf16 == NULL - it leaves the split-K partial tiles of x A in `scratch` and skips the reduce launch - and
 * lqer_linear_gemm with xaq_bf16 == NULL and the SAME scratch buffer (scratch_bytes = lqer_lowrank_xa_scratch_bytes):
 * the GEMM sums the tiles in the same fixed order and applies A_out itself.  lqer_linear_forward does this on its own. */
int lqer_decode_partials(const lqer_linear_desc_t* desc, int64_t M);
/* The partial-tile hand-over at the 128-row tile kernel's token counts is retired: 0 for every descriptor, token count and
 * dtype.  Kept for ABI compatibility; lqer_decode_partials names the only route that takes xaq_bf16 == NULL. */
int lqer_tile_partials(const lqer_linear_desc_t* desc, int64_t M, int dtype);

/* lqer_linear_gemm with an explicit row stride of xaq (elements; a multiple of 8, >= the padded rank): Linears that
 * share one input (q/k/v, gate/up; llama_decoder.py:246-248, :176) can run ONE lqer_quantize_act_xa over the
 * concatenation of their A matrices (descriptor rank = sum of the padded ranks, a_t = the concatenated limb image)
 * and hand each GEMM its columns of the result: xaq = xaq_cat + column offset, xaq_ld = total padded rank. */
int lqer_linear_gemm_ld(const lqer_linear_desc_t* desc, const void* xq_bf16, int64_t M, const void* w_packed,
                        const void* xaq_bf16, int64_t xaq_ld, const void* b_t, int b_limbs, const float* bias_q,
                        void* y, int dtype, int64_t ldy, void* scratch, size_t scratch_bytes, void* stream);

/* ---- decode: Linears that are handed the SAME tokens in ONE launch ---------------------------------------------------
 * q/k/v and gate/up receive one tensor (reference models/llama_decoder.py:222-224, :104; opt_decoder.py q/k/v).  At decode
 * sizes a forward is a chain of latencies around a 9 MB weight stream; a group's members run as ONE launch of the one-launch
 * decode route (see lqer_linear_forward above): the producers multiply x with the concatenation of the members' A, every
 * member's weight-streaming workgroups pick their rank columns out of the shared tiles.  Per member the arithmetic is that of
 * its own lqer_linear_forward: the same bits.
 *   members[i]: the member's descriptor, packed operands (as for lqer_linear_forward) and output y_i [M, N_i] (row stride ldy);
 *   a_t_cat:    A^T of the members concatenated along the rank: bf16 [sum of padded ranks][padded K] - lqer_pack_lowrank of
 *               [A_0 | A_1 | ...] (each A_i zero-padded to its padded rank); a_limbs must be 1 (8-bit MXINT values);
 *   workspace:  >= lqer_group_workspace_bytes(K, sum of padded ranks), 16-byte aligned.
 * Served: 2..4 members with equal in_features (a multiple of 16) and equal x / A_out / B_out formats, each with
 * lqer_decode_partials(desc, M) == 1, M <= 8, 16-byte aligned rows of x, sum of padded ranks <= 128.  Anything else returns LQER_E_UNSUPPORTED WITHOUT launching:
 * the caller then runs the members one by one. */
typedef struct lqer_group_member {
  const lqer_linear_desc_t* desc;
  const void* w_packed;
  const void* b_t;
  int32_t b_limbs;
  const float* bias_q;
  void* y;
  int64_t ldy;
} lqer_group_member_t;
size_t lqer_group_workspace_bytes(int64_t K, int64_t rank_padded_sum);
int lqer_linear_forward_group(const lqer_group_member_t* members, int n_members, const void* x, int dtype, int64_t M,
                              int64_t ldx, const void* a_t_cat, int a_limbs, void* workspace, size_t workspace_bytes,
                              void* stream);

/* ---- compact weight image: block_fp weights of 2 and 3 bits at their own width -----------------------------------------------
 * The standard image spends 4.5 bits per weight whatever w_fmt.width is.  For w_fmt.kind = LQER_Q_MXINT with width 2 or 3 there is a
 * second, opt-in image on the same panel grid (panel (n/16, k/64), padded to LQER_N_ALIGN / LQER_K_ALIGN, the panels of a 16-row band
 * contiguous along k).  A compact panel takes 128 * width + 16 * E bytes:
 *   [16 rows][4 q]  code dwords                                            offset 0
 *   [16 rows][2]    sign dwords - width 3 only                             offset 256
 *   [16 rows][E]    exponent bytes, biased as in the standard image        offset 128 * width
 * E = 64 / block for blocks of 16 or 32 k; 1 for one block per row (block <= 0 or >= K) and for blocks that are a multiple of 64 k; 4
 * (one byte per 16 k, the standard image's repetition) for any other block.  2-D tiles keep their per-row repetition.
 * Code dword (row, q) holds what one lane of the decode-size kernels multiplies per panel: the row's 8 k of chunk q (k 8q .. 8q+7 of
 * the panel) and of chunk q + 4.  Its byte j carries four 2-bit fields t = 0..3: k = j and k = 4 + j of chunk q, then of chunk q + 4.
 *   width 2: field = sign << 1 | magnitude;
 *   width 3: field = the 2-bit magnitude; the signs lie in sign dword (row, q >> 1): bit 4 (q & 1) + t of byte j.
 * The sign bit is kept as the nibble has it, also beside a zero magnitude.  W2 in blocks of 16: 320 B per panel (0.56 of 576), W2 /
 * 32: 288, W3 / 32: 416, W3 / 16: 448, W3 / 128: 400.
 * lqer_weight_narrow converts the standard image of such a weight (as lqer_pack_weight_mxint[_2d] wrote it; the quantizer is not
 * restated), lqer_weight_widen converts back: over the whole padded image widen(narrow(img)) == img byte for byte.  (A 16-k segment
 * that starts at or past K carries the packer's padding byte 127 - (width - 1), whatever block it lies in; the compact image does not
 * store it where its byte spans live k as well - widen writes it back from K.)  The _host functions do the same on host buffers with
 * no HIP call; lqer_weight_narrow_host returns LQER_E_INVALID for bytes that are not such an image.  Images are 16-byte aligned.
 * lqer_weight_narrow_bytes: bytes of the compact image; 0 for a format that is not served (widths 4..8, integer, minifloat).
 *
 * lqer_linear_forward_narrow is lqer_linear_forward with w_packed replaced by the compact image, lqer_linear_gemm_narrow is
 * lqer_linear_gemm_ld likewise.  Where the weight-streaming kernels run - LQER_ROUTE_SMALLM, and the one-launch decode route of up to
 * 8 tokens - they read the compact image directly: the same panels on the same waves in the same order, so the same bits as with the
 * standard image.  Every other route (M > 64, B_out formats that send decode sizes to the tile kernel) first widens the image into
 * caller memory - the workspace behind lqer_linear_sizes(...).workspace rounded up to 256 (lqer_linear_forward_narrow_workspace_bytes
 * counts it where m_max can reach such a route), or widen_scratch (>= lqer_linear_sizes(...).w_packed bytes, 16-byte aligned; unused
 * and may be NULL on the direct routes) - and runs the existing kernel on that copy.  LQER_E_UNSUPPORTED, with the reason in
 * lqer_last_error(): LQER_Q_MXINT_I8 descriptors, pass-through bf16 / fp32 activations (one image copy per limb), weights that are
 * not block_fp of width 2 or 3, descriptors with LQER_TUNE_W_EXP_TABLE.  lqer_linear_forward_group takes standard images only.
 * lqer_weight_narrow_route says what a call does (host only, no HIP call): LQER_NARROW_DIRECT, LQER_NARROW_DIRECT_ONE_LAUNCH (the
 * one-launch decode route, given a 16-byte aligned x and a shape its kernel serves) or LQER_NARROW_WIDEN; < 0: the refusal. */
#define LQER_NARROW_DIRECT 1
#define LQER_NARROW_DIRECT_ONE_LAUNCH 2
#define LQER_NARROW_WIDEN 3
size_t lqer_weight_narrow_bytes(int64_t N, int64_t K, const lqer_qfmt_t* w_fmt);
int lqer_weight_narrow(const void* w_packed, int64_t N, int64_t K, const lqer_qfmt_t* w_fmt, void* w_narrow, void* stream);
int lqer_weight_widen(const void* w_narrow, int64_t N, int64_t K, const lqer_qfmt_t* w_fmt, void* w_packed, void* stream);
int lqer_weight_narrow_host(const void* w_packed, int64_t N, int64_t K, const lqer_qfmt_t* w_fmt, void* w_narrow);
int lqer_weight_widen_host(const void* w_narrow, int64_t N, int64_t K, const lqer_qfmt_t* w_fmt, void* w_packed);
int lqer_weight_narrow_route(const lqer_linear_desc_t* desc, int64_t M, int dtype, int64_t ldx, int a_limbs, int b_limbs);
size_t lqer_linear_forward_narrow_workspace_bytes(const lqer_linear_desc_t* desc, int64_t m_max);
int lqer_linear_forward_narrow(const lqer_linear_desc_t* desc, const void* x, int dtype, int64_t M, int64_t ldx,
                               const void* w_narrow, const void* a_t, const void* b_t, int a_limbs, int b_limbs,
                               const float* bias_q, void* y, int64_t ldy, void* workspace, size_t workspace_bytes, void* stream);
int lqer_linear_gemm_narrow(const lqer_linear_desc_t* desc, const void* xq_bf16, int64_t M, const void* w_narrow,
                            const void* xaq_bf16, int64_t xaq_ld, const void* b_t, int b_limbs, const float* bias_q, void* y,
                            int dtype, int64_t ldy, void* scratch, size_t scratch_bytes, void* widen_scratch, size_t widen_bytes,
                            void* stream);

/* ---- pass-through activations ("A16": x_quantizer = passthrough, reference quantizers/passthrough.py:1, every
 * experiments/configs/template/ *-int.toml) ------------------------------------------------------------------
 * The kernels multiply exact bf16 operands.  A pass-through activation is therefore carried as the sum of
 * L = ceil(x_fmt.width / 8) bf16 limbs (1 for a bf16 tensor, 2 for fp16, 3 for fp32) laid side by side along k:
 * xq is [Mp][L*Kp], and w_packed / a_t must hold L copies of the packed image along k.  Likewise a pass-through
 * A_out hands x A on as LA limbs (2 when a_out_fmt.width <= 16, else 3): xaq is [Mp][LA*rp] and b_t holds LA
 * copies along r.  lqer_linear_sizes reports the enlarged sizes; pack into a buffer of the single-copy size (the
 * sizes of a descriptor whose x / A_out formats are block_fp) and expand with lqer_replicate_rows:
 *   w_packed: rows = Np/16,  row_bytes = (Kp/64)*LQER_PANEL_BYTES, copies = L
 *   a_t:      rows = 3*rp,   row_bytes = Kp*2,                      copies = L
 *   b_t:      rows = 3*Np,   row_bytes = rp*2,                      copies = LA
 * Every product stays exact and accumulation is fp32, as in the reference's F.linear on 16-bit tensors. */
int lqer_desc_limbs(const lqer_linear_desc_t* desc, int* act_limbs, int* xa_limbs);
/* fp16 tensors have a faster exact route: x_fmt.kind = LQER_Q_PASSTHROUGH_F16.  The activation image is then the
 * fp16 tensor itself ([Mp][Kp], one copy of w_packed), the main loops expand the weights to fp16 and run the fp16 MFMA
 * (products exact, fp32 accumulation - the reference's F.linear on fp16 tensors), and the side GEMM reads A as ONE
 * fp16 image a_t = [rp][Kp] fp16 written by this call from the limb image of lqer_pack_lowrank - followed (ABI 12) by its
 * FRAGMENT-MAJOR copy for the int8 route's one-launch activation kernel (per 32-k step and 16-rank tile 64 lanes x 8 halves, the B
 * operand of v_mfma_f32_16x16x32_f16, over ceil(K / 128) * 128 columns): a_t_f16 must hold lqer_a_f16_image_bytes(K, r) bytes.
 * Allowed only when
 * this call leaves flags[0] (a weight block scale outside the fp16 range 2^-24 .. 2^13) and flags[1] (an element of
 * A that is not an fp16 number) at zero (device int32[2]); otherwise use LQER_Q_PASSTHROUGH with width 11.
 * flags[0] & 2 (r = 0 and null A images ask for the weight flags alone): an exponent byte above 245 - such an image needs
 * LQER_TUNE_W_EXP_TABLE in the descriptor of every lqer_linear_gemm* / lqer_linear_forward* call on the bf16 route.
 * A_out / xaq / b_t are as for LQER_Q_PASSTHROUGH.  Calls take dtype = LQER_F16.  A dense tensor (ldx == K) with
 * K % LQER_K_ALIGN == 0, M % LQER_M_ALIGN == 0 (or M <= 64) and 16-byte alignment already is its image: lqer_linear_forward
 * then skips the copy, and the split API accepts xq == x in lqer_quantize_act_xa / lqer_linear_gemm. */
int lqer_f16_prepare(const void* w_packed, int64_t N, int64_t K, const void* a_t_limbs, int a_limbs, int64_t r,
                     void* a_t_f16, int32_t* flags, void* stream);
/* bytes of the fp16 image of A^T that lqer_f16_prepare writes (the [rp][Kp] image every a_limbs = -1 consumer reads + its
 * fragment-major copy); the reference has nothing to replace here - A is an fp16 nn.Parameter (quantized_layers/linear.py:142) */
size_t lqer_a_f16_image_bytes(int64_t K, int64_t r);
/* The same for block-16 MXINT activations (x_fmt block_fp [1, 16], the llama-7b.toml / opt-6.7b.toml templates) and an A of ONE bf16 limb
 * (8-bit block_fp A, llama-7b.toml:60-73): lqer_a_b16_prepare copies limb 0 of lqer_pack_lowrank's a_t ([rp][Kp] bf16) into `out` and
 * writes its fragment-major copy (the B operand of v_mfma_f32_16x16x32_bf16) behind it; out holds lqer_a_b16_image_bytes(K, r) bytes.
 * Passed as a_t with a_limbs = -2 to lqer_quantize_act_xa / lqer_linear_forward, it lets quantizer + x A + A_out run as ONE launch
 * (csrc/act16_fused.hip) for 16-bit, 16-byte aligned tensors with K % 16 == 0, padded rank 16 / 32 / 64 and 1024 <= M <= 4096; every
 * other call reads the image's first part exactly like a_limbs = 1.  Reference: linear.py:154-156 (x_quantizer, matmul, A_out_quantizer). */
size_t lqer_a_b16_image_bytes(int64_t K, int64_t r);
int lqer_a_b16_prepare(const void* a_t_limbs, int64_t K, int64_t r, void* out, void* stream);

/* ---- weights of 5..8 bits (the reference's no-LQER baseline: W8A8 block_fp with one block per row and per token,
 * experiments/pipeline/sweep_baseline_no_lqer.sh:73-76, through LinearFlexible, quantized_layers/linear.py:50-64) ---------------
 * The packed image holds 4-bit codes, so a mantissa m of up to 8 bits (|m| <= 127) travels as three signed base-8 digits,
 * m = 64 a + 8 b + c (a in [-2, 2]; b, c in [-4, 3]): three 4-bit sign-magnitude LIMB images with block exponents e - mbits + 6,
 * + 3, + 0, side by side along k - w_packed is [Np / 16][3][Kp / 64] panels (lqer_linear_sizes: three times the 4-bit size) - and
 * the activation image is repeated three times along k to match (the dual of the pass-through activation limbs below).  Every
 * kernel of the 4-bit path then multiplies the 8-bit weight EXACTLY (digits x powers of two; fp32 accumulation of exact products)
 * at three times the MFMA work and 13.5 bits per weight: the universal route, at every token count and for every x format.
 * lqer_pack_weight_mxint writes the three limbs for w_fmt.width in 5..8; lqer_quantize_act_xa writes the single-copy image behind
 * the wide one (lqer_act_image_bytes) and repeats it; the side path (x A, A_out) works on the single copy.  The one-launch decode
 * route and the shared-input groups do not take such weights (lqer_decode_partials = 0): decode sizes run the two-launch route.
 * The FAST route for the reference's own W8A8 configuration - per-token 8-bit activations, one weight block per row - is the
 * int8 MFMA kernel on an int8 image of the codes themselves (no expand at all): see "int8 route". */

/* ---- int8 route (the "W4A8 INT" configurations: x_quantizer block_fp with block_size [1,-1], i.e. one exponent per token,
 * reference experiments/pipeline/sweep_lqer_act_int.sh:83; w_quantizer blocks of 128 k or one block per row,
 * llama-7b-int.toml:87) ---------------------------------------------------------------------------------------------
 * With one activation exponent per token and one weight exponent per 128 k (or more) the products of a 128-k group share
 * one scale per output element, so their integer mantissas can be summed exactly on v_mfma_i32_32x32x32_i8 at twice the
 * bf16 rate.  x_fmt.kind = LQER_Q_MXINT_I8 selects this:
 *  - lqer_linear_sizes reports w_packed = the 4-bit sign-magnitude image of lqer_pack_weight_mxint followed (256-byte
 *    aligned) by a second image for the int8 main loop: two's-complement nibbles + one left shift per (row, 128-k group)
 *    + one scale per row (4.06 bit per weight).  Pack the first image as usual, then call lqer_i8_prepare on the same
 *    buffer.  flags[0] != 0 (device int32[2]): some row's integer sums could leave the i32 range, or the image holds two
 *    exponents inside one 128-k group - do not use LQER_Q_MXINT_I8 for this weight (plain LQER_Q_MXINT is always exact).
 *  - the activation image xq is then int8: [Mp][K padded to 128] mantissas followed (256-byte aligned) by Mp fp32 row
 *    scales; never larger than the bf16 image (K >= 128 required), so the workspace carving does not change.
 *  - the split calls lqer_quantize_act_xa / lqer_lowrank_xa / lqer_linear_gemm[_ld] with this kind ALWAYS produce /
 *    consume the int8 images; lqer_gemm_route says whether that is possible for M tokens (LQER_ROUTE_I8: M >= 128,
 *    B_out pass-through or one block per row, padded rank x limbs of x A <= 128);
 *    otherwise call them with kind LQER_Q_MXINT on the same buffers.  lqer_linear_forward chooses by itself.
 * Requires x_fmt.width <= 8, x_fmt.block <= 0 or >= K, w_fmt.block <= 0, >= K or a multiple of 128.
 *  - weights of 5..8 bits (the reference's W8A8 baseline, sweep_baseline_no_lqer.sh:73-76): the second image holds the int8 CODES
 *    themselves - per (256-row tile, 64-k half-step) 256 rows x 64 B, then one scale per row - and the main loop is LDS-DMA, one
 *    16-byte LDS read per weight fragment and the MFMA: no expand.  It needs ONE exponent per weight row (block_size [1,-1], or
 *    coarser blocks whose exponents happen to agree): lqer_i8_prepare sets flags[0] otherwise, and such a weight keeps the limb
 *    route (exact, three times the work).  128- or 256-row tiles (lqer_gemm_tile_rows says which): on 128-row tiles a wave's codes go
 *    straight from this image into registers (four coalesced 16-byte loads per lane and step, no LDS), on 256-row tiles through a
 *    half-step LDS ring. */
/* lqer_i8_prepare reads the first image and writes the second one whole, the 256-byte padding of its per-tile mode table included;
 * the first image and the alignment gap between the two are not touched. */
int lqer_i8_prepare(void* w_packed, int64_t N, int64_t K, const lqer_qfmt_t* w_fmt, int32_t* flags, void* stream);
/* Test hooks: the int8 weight image (inside w_packed) -> dequantized fp32 [N,K]; x [M,K] -> the int8 activation image. */
int lqer_unpack_weight_i8(const void* w_packed, int64_t N, int64_t K, float* w_f32, void* stream);
int lqer_unpack_weight_i8_fmt(const void* w_packed, int64_t N, int64_t K, const lqer_qfmt_t* w_fmt, float* w_f32, void* stream); /* ... of
   a weight of any width (5..8 bits: the image of codes behind the three limb images) */
int lqer_quantize_act_i8(const void* x, int dtype, int64_t M, int64_t K, int64_t ldx, const lqer_qfmt_t* fmt, void* xq_i8,
                         void* stream);
/* dst[row] = src[row] repeated `copies` times (device to device, stream-ordered; dst != src). */
int lqer_replicate_rows(const void* src, void* dst, int64_t rows, int64_t row_bytes, int copies, void* stream);

/* ---- quantized attention products (reference quantized_functions/matmul.py:12-37: matmul_flexible / bmm_flexible; call
 * sites models/llama_decoder.py:263,294, opt_decoder.py:125,190) -------------------------------------------------------
 *     out[b] = x_quantizer(x[b]) @ w_quantizer(y[b]),   b < batch;  x[b]: [S1, K], y[b]: [K, S2], out[b]: [S1, S2] (dense)
 * Both quantizers block_fp with blocks along the LAST dim of their operand (width <= 8; blocks of 16 - the templates' - run fused,
 * other lengths see lqer_matmul_q_workspace_bytes_fmt) - for y that is the output dim j, not the contraction dim (llama-7b.toml:110-126).  x is quantized in the GEMM's load path (read from HBM
 * once, no quantized copy); y goes through a bf16 image [batch][S2 padded to 128][K padded to 64] in `workspace`
 * (lqer_matmul_q_workspace_bytes).  Element strides: x[b][i][k] at b x_bs + i x_rs + k (k contiguous);
 * y[b][k][j] at b y_bs + k y_ks + j y_js with y_ks == 1 or y_js == 1 (Q K^T hands over the transposed VIEW of K: y_ks == 1).
 * fp32 accumulation of exact products (every 8-bit MXINT value is a bf16 number); out has the element type `dtype` of x, y. */
size_t lqer_matmul_q_workspace_bytes(int64_t batch, int64_t K, int64_t S2);
/* Blocks other than 16 (16 n elements, or whole rows: quantized_functions/matmul.py:12-29 takes any block_size): the library's
 * standalone quantizer writes that operand's bf16 image into the workspace first and the image / product kernels take it as
 * it is - same bits, one more pass over the operand.  Such an operand needs evenly spaced rows over the batch (x_bs == S1
 * x_rs; y dense along j with y_bs == K y_ks); the workspace then also holds those images: */
size_t lqer_matmul_q_workspace_bytes_fmt(int64_t batch, int64_t S1, int64_t K, int64_t S2, const lqer_qfmt_t* x_fmt,
                                         const lqer_qfmt_t* y_fmt);
int lqer_matmul_q(const void* x, const void* y, void* out, int dtype, int64_t batch, int64_t S1, int64_t K, int64_t S2,
                  int64_t x_bs, int64_t x_rs, int64_t y_bs, int64_t y_ks, int64_t y_js, const lqer_qfmt_t* x_fmt,
                  const lqer_qfmt_t* y_fmt, void* workspace, size_t workspace_bytes, void* stream);

/* ---- fused quantized attention (reference models/llama_decoder.py:259-297, opt_decoder.py:125,190: both products through
 * matmul_flexible / bmm_flexible, the softmax in fp32 between them) ------------------------------------------------------------
 * Per batch element b and head h, with g = h / (heads / kv_heads) (grouped-query K / V are read through the head mapping, never
 * repeated in memory) and DT the element type `dtype` of q, k, v, mask and out; ->DT is a rounding to DT:
 *     S  = q_fmt(Q[b,h]) k_fmt(K[b,g]^T) ->DT        [S, T]  blocks of 16 along d resp. along t; fp32 accumulation of exact products
 *     S1 = S scaling ->DT;   S2 = S1 + mask[b,h] ->DT  (with a mask tensor);   P = softmax_fp32(S2 over t) ->DT
 *     out[b,h] = p_fmt(P) v_fmt(V[b,g]) ->DT          [S, D]  blocks of 16 along t resp. along d
 * - bit for bit the two lqer_matmul_q products with torch's scale, add and fp32 softmax between them, each materialised in DT
 * (lqer_amd/attention.py), but for the order of the fp32 sums and the last bits of exp: the [S, T] scores never reach memory.
 * The four formats must be LQER_Q_MXINT, width <= 8, block 16; D a multiple of 16, D <= 128; S, T >= 1 arbitrary (ragged last
 * blocks are zero-padded on the right, as in lqer_matmul_q).  Anything else: LQER_E_UNSUPPORTED, nothing launched.
 * Strides are in ELEMENTS over (batch, head, row) - q_strides[3], k_strides[3] (head = kv head), v_strides[3], out_strides[3] - with
 * the last dim (d) contiguous; out_strides let the call write [b, s, h, d] directly.  Mask, one of:
 *   mask != NULL   additive tensor of DT, mask_strides[3] over (batch, head, query row) with 0 = broadcast, t contiguous; added and
 *                  rounded literally, so fully masked rows behave as in the unfused route;
 *   causal = 1     key j is visible to query i iff j <= i + (T - S); invisible keys contribute exactly 0 and key tiles without a
 *                  visible key are skipped (for S <= T the same bits as the tensor form of that mask).  Not both.
 * row_stats (may be NULL): float [batch][heads][S][2] = {row maximum of S2, row sum of exp(S2 - maximum)} over the visible keys.
 * workspace: lqer_attention_q_workspace_bytes(...) bytes, 256-byte aligned, contents irrelevant, layout
 *   [bf16 image of k_fmt(K^T): batch kv_heads x (T rounded up to 128) x (D rounded up to 64)]
 *   [bf16 image of v_fmt(V):   batch kv_heads x 128 x (T rounded up to 64)]          each part rounded up to 256 bytes
 * - independent of heads and S.  A workspace shorter than that is LQER_E_INVALID.  Three launches on `stream` (two image kernels,
 * the attention kernel), no allocation, no host synchronisation: capturable in a hipGraph. */
size_t lqer_attention_q_workspace_bytes(int64_t batch, int64_t heads, int64_t kv_heads, int64_t S, int64_t T, int64_t D);
int lqer_attention_q(const void* q, const void* k, const void* v, const void* mask, void* out, float* row_stats, int dtype,
                     int64_t batch, int64_t heads, int64_t kv_heads, int64_t S, int64_t T, int64_t D, const int64_t* q_strides,
                     const int64_t* k_strides, const int64_t* v_strides, const int64_t* mask_strides, const int64_t* out_strides,
                     float scaling, int causal, const lqer_qfmt_t* q_fmt, const lqer_qfmt_t* k_fmt, const lqer_qfmt_t* p_fmt,
                     const lqer_qfmt_t* v_fmt, void* workspace, size_t workspace_bytes, void* stream);

/* ---- the same attention for decode steps, split over the keys (reference models/llama_decoder.py:259-297, opt_decoder.py:125,190
 * with 1 <= S <= 8 query rows - a step of generate() with a KV cache, or up to 8 speculated tokens) ------------------------------
 * The arithmetic, the strides, the two mask forms (causal: key j visible to query i iff j <= i + (T - S)), row_stats and the
 * argument list are lqer_attention_q's; the results agree with it within the order of the fp32 sums.  lqer_attention_q gives every
 * query a lane and every 128 queries a workgroup - one live lane in 32 at S = 1 - and writes two bf16 images of K and V first; this
 * call gives every CHUNK of keys a workgroup that serves all (heads / kv_heads) S query rows of a kv head and reads K and V once, in
 * DT, from the caller's tensors (rows of q, k, v that are not 16-byte aligned take element loads: same bits).  P is normalised by
 * the whole row's sum before it is quantized, so there is no online softmax: the scores of all chunks come first.
 * Chunks: C = 16 min(max(ceil(T / 256), 1), 8) keys, nch = ceil(T / C) of them - a function of T alone; every sum over chunks runs in
 * chunk order and nothing is accumulated with atomics: the same bits run to run, for a batch slice, and for a slice of the heads of
 * one kv group.
 * workspace: lqer_attention_q_decode_workspace_bytes(...) bytes, 256-byte aligned, contents irrelevant on entry (nothing survives
 * between calls, no counters), layout with rows = batch heads S
 *   [S2, fp32: rows x (nch C)][chunk statistics {max, sum exp(S2 - max)}, fp32: rows x nch x 2][partial outputs, fp32: rows x nch x D]
 * each part rounded up to 256 bytes; 0 for batch = 0, S = 0 or T = 0.  Three launches on `stream` (scores and chunk statistics;
 * P and the chunk's P V; the sum over chunks, which stores through out_strides), no allocation, no host synchronisation, no wait:
 * capturable in a hipGraph.
 * Refused with a message, nothing launched or touched:
 *   LQER_E_UNSUPPORTED  S > 8; a format that is not LQER_Q_MXINT, width <= 8, block 16; D not a multiple of 16 or > 128; T > 2^30;
 *                       batch or kv_heads > 65535;
 *   LQER_E_INVALID      a null pointer (q, k, v, out, workspace, a stride array, a format); heads not a multiple of kv_heads; negative
 *                       sizes; T = 0 with work to do; an unknown dtype; a workspace shorter than the query function's or not
 *                       16-byte aligned (the kernels access it in 16-byte pieces); mask together with causal = 1. */
size_t lqer_attention_q_decode_workspace_bytes(int64_t batch, int64_t heads, int64_t kv_heads, int64_t S, int64_t T, int64_t D);
int lqer_attention_q_decode(const void* q, const void* k, const void* v, const void* mask, void* out, float* row_stats, int dtype,
                            int64_t batch, int64_t heads, int64_t kv_heads, int64_t S, int64_t T, int64_t D, const int64_t* q_strides,
                            const int64_t* k_strides, const int64_t* v_strides, const int64_t* mask_strides, const int64_t* out_strides,
                            float scaling, int causal, const lqer_qfmt_t* q_fmt, const lqer_qfmt_t* k_fmt, const lqer_qfmt_t* p_fmt,
                            const lqer_qfmt_t* v_fmt, void* workspace, size_t workspace_bytes, void* stream);

/* ---- packed KV cache: what lqer_attention_q_decode multiplies, kept between the steps ---------------------------------------------
 * A decode step quantizes the whole K (k_fmt, blocks of 16 along t) and V (v_fmt, blocks of 16 along d) again, with the results of
 * the step before: a block of 16 keys never changes once it is full, a V row never changes at all.  The cache holds the quantizer's
 * OUTPUT - a one-byte code per element and a one-byte exponent per block - and lqer_attention_q_decode_kv reads that: the same codes,
 * exponents, chunks and order of sums as lqer_attention_q_decode on the raw tensors, so the SAME BITS (K or V holding a NaN excepted:
 * a code cannot carry one), from 2 D (1 + 1/16) bytes per cached token and kv head instead of 2 D sizeof(DT).
 * One caller-allocated buffer per cache, 16-byte aligned, lqer_kv_cache_bytes(...) bytes (0 for a dtype, head dim or size the cache
 * does not take); the library keeps no pointer.  With cap = capacity rounded up to 16, Z = batch kv_heads, sections in this order,
 * each rounded up to 256 bytes:
 *   K codes      [Z][cap][D]            uint8  sign-magnitude: bit 7 the sign, bits 6..0 |mantissa| (value = +-m 2^(e - (width - 1)));
 *                                              sign-magnitude keeps the quantizer's -0, which a two's-complement code cannot
 *   K exponents  [Z][cap / 16][D]       uint8  e + exp_bias of the block of keys 16 i .. 16 i + 15 at this d
 *   V codes      [Z][cap][D]            uint8  as K codes
 *   V exponents  [Z][cap / 16][D / 16][16] uint8  e + exp_bias of (key 16 i + r, block j of 16 d) at [i][j][r] - the bytes of
 *                                              [cap][D / 16] regrouped so that the exponents of four consecutive keys are one dword
 *   K staging    [Z][16][D]             DT     the raw keys of the open (last, partial) block of keys, rows 0 .. len % 16 - 1
 * A block whose values are all zero stores codes 0 and the exponent nearest to 0.
 * lqer_kv_cache_append: k_new / v_new [batch][kv_heads][n][D] of DT through k_strides[3] / v_strides[3] (elements, over batch, kv
 * head, row; d contiguous; rows that are not 16-byte aligned take element loads: same bits) become keys len .. len + n - 1 of a cache
 * that holds len.  V rows are quantized and stored at once.  Every block of 16 keys the new keys touch is quantized from the staging
 * rows plus the new keys - the open block at the end included, zero-padded on the right as the quantizer pads a ragged block - and
 * its codes (all 16 rows) and exponents are rewritten; the raw keys of the block left open go to the staging rows.  So the reader
 * sees one format and has no tail path.  n >= 1 is arbitrary (a prefill goes in with one call); nothing depends on cache contents
 * beyond row len or on staging rows beyond len % 16, so a fresh cache needs no initialisation (len = 0).  One launch on `stream`, two
 * when the new keys leave a non-empty open block; k_new and v_new are only read.  Appends are issued once, in order: one that leaves a
 * non-empty open block overwrites the staging rows it read, so repeating it at the same len does not give the same cache (a captured
 * graph that is replayed restarts from a length whose open block it rebuilds itself, e.g. 0, or appends inside one open block).
 * lqer_attention_q_decode_kv: lqer_attention_q_decode with (k, v, k_strides, v_strides) replaced by (cache, cache_bytes, capacity); T
 * is the cache's length; k_fmt and v_fmt are those of the appends.  Arithmetic, masks, row_stats, workspace (size and layout), chunks,
 * launches and refusals are lqer_attention_q_decode's; the cache is only read.  Rows at and beyond T are never read.
 * lqer_attention_q_kv: lqer_attention_q with (k, v, k_strides, v_strides) replaced by (cache, cache_bytes, capacity) - the argument list
 * of lqer_attention_q_decode_kv - for ANY S >= 1: a second prompt, a long prompt fed in chunks, a speculated block of more than 8
 * tokens on a cache that no longer has the raw K and V.  T is the cache's length; k_fmt and v_fmt are those of the appends.  The two
 * bf16 images of lqer_attention_q's workspace (same size, same layout: lqer_attention_q_kv_workspace_bytes) are written from the
 * codes and exponents - a conversion and a scaling, the padding as zeros - instead of quantizing K and V, and the same attention
 * kernel runs on them: the SAME BITS as lqer_attention_q on the raw K and V that were appended - out and row_stats, both mask forms,
 * grouped-query heads (K or V holding a NaN excepted, as above).  The cache is only read; rows at and beyond T are never read.  Three
 * launches on `stream` (K image, V image, the attention kernel), no allocation, no host synchronisation, no atomics: capturable in a
 * hipGraph.  Refusals: lqer_attention_q's (formats, D, null pointers, heads not a multiple of kv_heads, mask together with causal, a
 * short workspace, S or T beyond the launch grid) and the cache's below; also LQER_E_INVALID for a workspace that is not 16-byte aligned.
 * lqer_kv_cache_unpack (test hook): the dequantized K and V [batch][kv_heads][T][D] as dense fp32 (either may be NULL).
 * Refused with a message, nothing launched or touched:
 *   LQER_E_UNSUPPORTED  k_fmt / v_fmt not LQER_Q_MXINT, width <= 8, block 16; D not a multiple of 16 or > 128;
 *   LQER_E_INVALID      null pointers; negative sizes; n < 1; len + n (append) or T (attention, unpack) > capacity; an unknown dtype;
 *                       a cache shorter than lqer_kv_cache_bytes or not 16-byte aligned. */
size_t lqer_kv_cache_bytes(int dtype, int64_t batch, int64_t kv_heads, int64_t capacity, int64_t D);
int lqer_kv_cache_append(void* cache, size_t cache_bytes, const void* k_new, const void* v_new, const int64_t* k_strides,
                         const int64_t* v_strides, int dtype, int64_t batch, int64_t kv_heads, int64_t capacity, int64_t D, int64_t len,
                         int64_t n, const lqer_qfmt_t* k_fmt, const lqer_qfmt_t* v_fmt, void* stream);
int lqer_kv_cache_unpack(const void* cache, size_t cache_bytes, int dtype, int64_t batch, int64_t kv_heads, int64_t capacity, int64_t D,
                         int64_t T, const lqer_qfmt_t* k_fmt, const lqer_qfmt_t* v_fmt, float* k_f32, float* v_f32, void* stream);
size_t lqer_attention_q_decode_kv_workspace_bytes(int64_t batch, int64_t heads, int64_t kv_heads, int64_t S, int64_t T, int64_t D);
int lqer_attention_q_decode_kv(const void* q, const void* cache, size_t cache_bytes, int64_t capacity, const void* mask, void* out,
                               float* row_stats, int dtype, int64_t batch, int64_t heads, int64_t kv_heads, int64_t S, int64_t T, int64_t D,
                               const int64_t* q_strides, const int64_t* mask_strides, const int64_t* out_strides, float scaling, int causal,
                               const lqer_qfmt_t* q_fmt, const lqer_qfmt_t* k_fmt, const lqer_qfmt_t* p_fmt, const lqer_qfmt_t* v_fmt,
                               void* workspace, size_t workspace_bytes, void* stream);
size_t lqer_attention_q_kv_workspace_bytes(int64_t batch, int64_t heads, int64_t kv_heads, int64_t S, int64_t T, int64_t D);
int lqer_attention_q_kv(const void* q, const void* cache, size_t cache_bytes, int64_t capacity, const void* mask, void* out, float* row_stats,
                        int dtype, int64_t batch, int64_t heads, int64_t kv_heads, int64_t S, int64_t T, int64_t D, const int64_t* q_strides,
                        const int64_t* mask_strides, const int64_t* out_strides, float scaling, int causal, const lqer_qfmt_t* q_fmt,
                        const lqer_qfmt_t* k_fmt, const lqer_qfmt_t* p_fmt, const lqer_qfmt_t* v_fmt, void* workspace,
                        size_t workspace_bytes, void* stream);

/* ---- paged KV pool: the packed KV cache in pages of 16 keys, per-sequence lengths in a decode batch ------------------------------
 * The packed cache above has one length for the whole batch and one dense slab: a ragged batch is padded to its longest sequence, a
 * finished sequence cannot hand its memory to a new one, and growing copies everything.  The pool stores the SAME codes and exponents
 * in PAGES: a page holds LQER_KV_PAGE_KEYS = 16 keys of ALL kv heads of one sequence - one block of the K quantizer, one group of V
 * exponents, so a page is a whole number of everything the cache stores, and a decode chunk (a multiple of 16 keys) a whole number
 * of pages.  One caller-allocated buffer, 16-byte aligned, lqer_kv_pool_bytes(...) bytes (0 for a dtype, head dim or size the pool does
 * not take); the library keeps no pointer.  Page p and kv head g address ITEM p kv_heads + g of each section; sections in this order,
 * each rounded up to 256 bytes:
 *   K codes      [pages][kv_heads][16][D]        uint8   the dense cache's codes (sign-magnitude)
 *   K exponents  [pages][kv_heads][D]            uint8
 *   V codes      [pages][kv_heads][16][D]        uint8
 *   V exponents  [pages][kv_heads][D / 16][16]   uint8   the dense cache's regrouping: four consecutive keys' exponents in one dword
 *   K staging    [slots][kv_heads][16][D]        DT      raw keys of a sequence's open block - one set per sequence SLOT, not per page
 * Within an item the bytes are exactly the dense cache's bytes for that block of 16 keys.
 * NIBBLE CODES (opt-in, per operand: k_fmt / v_fmt of kind LQER_Q_MXINT_C4, width 2..4, so |mantissa| <= 7).  The operand's code section
 * is then, in place of the byte section above,
 *   K / V codes  [pages][kv_heads][16][D / 2]    uint8   elements d = 2 j and 2 j + 1 of a key's row are the low and the high nibble of
 *                                                        byte j; a nibble is sign << 3 | |mantissa| - sign-magnitude, so the quantizer's
 *                                                        -0 is kept as the byte code keeps it; the byte code is (n & 7) | ((n & 8) << 4)
 * and everything else - the exponent sections, the staging rows, the item index p kv_heads + g, the 256-byte rounding of each section -
 * is unchanged: 2 D (1/2 + 1/16) bytes per token and kv head with both operands in nibbles, 144 B instead of 272 B at D = 128.  A key's
 * row is D / 2 bytes, a multiple of 8, and the 16 codes of one block of 16 d are one aligned 8-byte piece.  K and V choose
 * independently (K of width 8 beside V in nibbles is a valid pool).  The pool is sized by lqer_kv_pool_bytes_fmt(dtype, pages, slots,
 * kv_heads, D, k_fmt, v_fmt) - lqer_kv_pool_bytes when both kinds are LQER_Q_MXINT, 0 for anything the pool does not take - and EVERY
 * call on it passes the same two kinds: the appends and the attention entries in their k_fmt / v_fmt, gather and fork through
 * lqer_kv_pool_gather_fmt / lqer_kv_pool_fork_fmt (the entries without formats address a pool of byte codes).  The values, and with
 * them every result, are those of a byte pool of LQER_Q_MXINT formats with the same fields: the storage changes no rounding.  An
 * append writes every byte of a nibble section whole, from one thread - the open block is still rewritten over all 16 rows -, so
 * pages are reused dirty as ever.  lqer_kv_pool_gather_fmt writes the dense BYTE cache lqer_kv_pool_gather writes from a byte pool
 * (nibbles widened, exponents and staging rows copied); lqer_kv_pool_fork_fmt copies an item at the size the formats give it.
 * Refused, LQER_E_UNSUPPORTED: the kind with width > 4 or block != 16; the kind on lqer_attention_q_decode_paged_shared (the grouped
 * kernels are not instantiated for it - lqer_attention_q_decode_paged gives the same bits).
 * Metadata, all on the DEVICE and written by the caller:
 *   block_table  int32 [slots][table_stride]: entry [s][i] is the page of keys 16 i .. 16 i + 15 of the sequence in slot s;
 *   seq_slots    int32 [batch]: the slot of the b-th sequence of THIS call - any subset of the slots, in any order;
 *   lens         int32 [batch]: for append the sequence's length BEFORE the call, for attention its number of keys T_b;
 *   max_len      host: an upper bound on every lens[b] (for append: on lens[b] + n), 1 <= max_len <= min(16 table_stride, 2^30).  It
 *                sizes grids and the workspace only - no result depends on it, and no host decision depends on a length.
 * The library cannot see device contents from the host, so VALID TABLES AND LENGTHS ARE THE CALLER'S CONTRACT, as valid pointers are:
 * every page index a call reaches (entries 0 .. ceil(len / 16) - 1 of an addressed slot's row) lies in [0, pages); a page may belong to
 * several live sequences only if all of its 16 keys lie below the length of every owner (a full page is never written again, so it
 * can be shared: lqer_kv_pool_fork) - the page at len / 16 of a sequence with len % 16 != 0 belongs to it alone; no slot is named
 * twice in one call; every seq_slots[b] lies in [0, slots); 0 <= lens[b] and lens[b] (+ n)
 * <= max_len.  A call that breaks this reads or writes outside the pool.  Nothing depends on the contents of a page beyond its
 * sequence's length or on staging rows beyond len % 16: pages and slots are reused dirty, a fresh pool needs no initialisation.
 * lqer_kv_pool_append: k_new / v_new [batch][kv_heads][n][D] of DT through k_strides[3] / v_strides[3], n >= 1 uniform over the call
 * (a decode step: n = 1 for every live sequence; a prompt: a call with batch = 1; counts of their own: lqer_kv_pool_append_ragged).  Per sequence lqer_kv_cache_append's semantics, word
 * for word: V rows quantized and stored at once, every block of 16 keys the new keys touch re-quantized from the staging rows plus the
 * new keys, zero-padded on the right, and rewritten whole, the raw keys of the block left open to the slot's staging rows.  ONE launch
 * on `stream` whatever the lengths are (the thread that reads a staging column also writes it); like the dense append it is issued
 * once per step, in order.
 * lqer_attention_q_decode_paged: lqer_attention_q_decode_kv with (cache, cache_bytes, capacity, T) replaced by (pool, pool_bytes, pages,
 * slots, block_table, table_stride, seq_slots, lens, max_len) and without a mask tensor: the mask forms are none and causal = 1, with
 * sequence b's own offset T_b - S (S <= T_b is the caller's to keep); per-sequence lengths replace the padding mask.  (A draft tree's
 * mask is one word per query row: the two _tree entries below.)  S <= 8, uniform over the call.  A workgroup takes T = lens[b] and from it the chunk length C, the chunk count nch and the causal offset of ITS
 * sequence; the grid's x is the largest nch that any T <= max_len has (nch is not monotonic in T), and workgroups beyond their
 * sequence's nch leave at once.  For every b, out[b] and row_stats[b] are the SAME BITS as lqer_attention_q_decode with batch = 1 on
 * the raw K and V of that sequence - whatever else is in the batch, whatever pages it lives on, whatever max_len is.  A sequence
 * with lens[b] = 0 gets out[b] = 0 and its row_stats untouched.  The pool is only read.
 * workspace: lqer_attention_q_decode_paged_workspace_bytes(batch, heads, kv_heads, S, max_len, D) bytes, 16-byte aligned, contents
 * irrelevant, strides fixed by max_len: with rows = batch heads S, Tp = max_len rounded up to 128 and nchs = the largest nch of any
 * T <= max_len (ceil(max_len / 16) up to 256 keys, 16 up to 2048, ceil(max_len / 128) beyond)
 *   [S2, fp32: rows x Tp][chunk statistics, fp32: rows x nchs x 2][partial outputs, fp32: rows x nchs x D]    each rounded up to 256 bytes.
 * Three launches on `stream`, no allocation, no host synchronisation, no atomics: capturable in a hipGraph.
 * lqer_attention_q_decode_paged_window: lqer_attention_q_decode_paged's argument list plus `window` = W >= 1, a SLIDING WINDOW on top of
 * the causal rule (causal = 1 is required): query row i of sequence b sits at position p = i + (lens[b] - S) and sees the keys j with
 * p - W < j <= p - W keys including its own, as Mistral's sliding_window; W >= lens[b] is plain causal.  For every b, out[b] and
 * row_stats[b] are the SAME BITS as lqer_attention_q_decode with batch = 1 on the FULL raw K and V of that sequence and the additive
 * window mask - 0 inside the window, the dtype's most negative finite value outside - WHATEVER THE PAGES BELOW THE WINDOW NOW HOLD:
 * no table entry and no page wholly below key lens[b] - S - window + 1 is read (K or V, codes or exponents), so the caller may hand
 * those pages to other sequences and leave the stale entries in the row - they must only still be the row's first entries by
 * position: the table stays indexed by absolute key / 16.  Chunks wholly below that key cost nothing but an early exit.  Workspace,
 * grid and strides are lqer_attention_q_decode_paged's (lqer_attention_q_decode_paged_workspace_bytes, sized by max_len), three
 * launches, capturable alike.  Refused as the call above, and LQER_E_INVALID for window < 1 or causal = 0.
 * lqer_attention_q_decode_paged_shared: lqer_attention_q_decode_paged's argument list plus (grp_of, grp_starts, grp_members, grp_keys,
 * n_groups): sequences that hold their first keys on the SAME PAGES (lqer_kv_pool_fork: beams, samples of one prompt, requests behind
 * one system prompt) are named as a group, and a chunk of keys that every member of a group holds on shared pages is loaded ONCE, by
 * the workgroup of the group's first member (its leader), which computes that chunk for the query rows of all members; the other
 * members' workgroups of that chunk leave at once.  Four int32 arrays on the DEVICE, written by the caller:
 *   grp_of       [batch]         the group of the call's b-th sequence, in [0, n_groups)
 *   grp_starts   [n_groups + 1]  group i owns entries grp_starts[i] .. grp_starts[i + 1] - 1 of grp_members (CSR: grp_starts[0] = 0,
 *                                non-decreasing, grp_starts[n_groups] = batch); no group is empty
 *   grp_members  [batch]         call indices, group by group; the first member of a group is its leader
 *   grp_keys     [n_groups]      P: the leading keys the group's members hold on the same pages; a multiple of 16, 0 for a group of one
 * They fall under the caller's contract, as the table and the lengths do: the arrays are a partition of 0 .. batch - 1 (every call
 * index in exactly one group, grp_of[grp_members[e]] = i for the entries e of group i); for every group with P > 0 all members have
 * the same chunk length lqer_attention_q_decode_chunk(lens[b], D); the first P / 16 entries of all members' table rows are the same
 * pages; P <= 16 (lens[b] / 16) for every member b.  A call that breaks this reads or writes outside its buffers or gives a sequence
 * another's keys.  Chunk c (keys c C .. c C + C - 1, C the chunk length) of a group of two or more is shared when (c + 1) C <= P;
 * every other chunk, and every chunk of a group of one, is computed as lqer_attention_q_decode_paged computes it.  P is a licence, not
 * a fact the kernels rely on beyond it: a smaller P than the members really share (0 included) is valid and gives the same bits.
 * For every b, out[b] and row_stats[b] are the SAME BITS as lqer_attention_q_decode_paged gives - those of lqer_attention_q_decode with
 * batch = 1 on the raw K and V of that sequence - whatever the groups are: a row's arithmetic is that row's alone.  Workspace
 * (lqer_attention_q_decode_paged_workspace_bytes - there is no size function of its own), grid and strides are
 * lqer_attention_q_decode_paged's; every workspace cell is written by exactly one workgroup; three launches on `stream`, no allocation,
 * no host synchronisation, no atomics: capturable in a hipGraph.  The pool is only read.  Refused as lqer_attention_q_decode_paged,
 * and LQER_E_INVALID for a null group array, n_groups < 1 or n_groups > batch (so also batch = 0).
 * lqer_attention_q_decode_chunk(T, D): the chunk length C of a sequence of T keys in the split-over-keys kernels - 16 ceil(T / 256)
 * clamped to [16, 128]; D is accepted for the rule's sake and does not enter it today.
 * lqer_attention_q_paged: lqer_attention_q_decode_paged's argument list, word for word, and its metadata contract, for ANY S >= 1
 * (uniform over the call) - a prompt, a second turn, a chunk of a long prompt or a speculated block of more than 8 tokens on paged
 * sequences, the whole ragged batch in one call.  It is to lqer_attention_q_kv what the call above is to lqer_attention_q_decode_kv:
 * the two bf16 images of the prefill kernel are written from the pool's codes and exponents, found through the block table - no
 * gather, no dense copy -, and the attention kernel takes T = lens[b], and with it the causal offset T_b - S, per sequence.  For every
 * b, out[b] and row_stats[b] are the SAME BITS as lqer_attention_q with batch = 1 on the raw K and V of that sequence - whatever else
 * is in the batch, whatever pages it lives on, whatever max_len is and whatever the workspace held (K or V holding a NaN excepted, as
 * with the packed cache).  A sequence with lens[b] = 0 gets out[b] = 0 and its row_stats untouched.  The pool is only read.
 * workspace: lqer_attention_q_paged_workspace_bytes(batch, heads, kv_heads, S, max_len, D) = lqer_attention_q_kv_workspace_bytes at
 * T = max_len bytes, 16-byte aligned, contents irrelevant: K image [batch kv_heads][Tp][Dp], V image [batch kv_heads][128][Tv], the
 * strides fixed by max_len.  Of sequence b's images the call writes the keys up to the end of the last 64-key tile that holds a key
 * below lens[b] - converted codes below lens[b], zeros from there on - which is all the attention kernel reads of them; image
 * workgroups beyond that leave at once, so a ragged batch pays for its keys and not for max_len.  Three launches on `stream` (K image,
 * V image, the attention kernel), no allocation, no host synchronisation, no atomics: capturable in a hipGraph.
 * lqer_attention_q_paged_window: lqer_attention_q_paged's argument list plus `window` = W >= 1, the SLIDING WINDOW of
 * lqer_attention_q_decode_paged_window for any S >= 1 (causal = 1 is required): query row i of sequence b sits at position
 * p = i + (lens[b] - S) and sees the keys p - W < j <= p.  The rule is a compile-time instantiation of the prefill kernel: a workgroup
 * starts both sweeps at the first 64-key tile one of its 128 queries sees, a wave skips the 32-key subtiles wholly below its own first
 * key, a lane selects by its own - work per call follows W + S, not lens[b].  For every b, out[b] and row_stats[b] are the SAME BITS as
 * lqer_attention_q with batch = 1 on the FULL raw K and V of that sequence and the additive window mask - 0 inside the window, the
 * dtype's most negative finite value outside - WHATEVER THE PAGES BELOW THE WINDOW NOW HOLD AND WHATEVER THE WORKSPACE HELD: with
 * lo_b = max(0, lens[b] - S - W + 1), the first key the call's first row sees, the caller guarantees that the keys from
 * 16 (lo_b / 16) on are in the pool; no table entry and no page below that key is read (K or V, codes or exponents).  Of sequence b's
 * images the call writes from key 64 (lo_b / 64) on: zeros up to 16 (lo_b / 16) (a zero probability times a stale image row must be 0,
 * not NaN), the converted codes from there; image workgroups below that tile leave at once and the attention kernel loads no tile
 * below it.  The images stay indexed by absolute key: workspace, grid and strides are lqer_attention_q_paged's
 * (lqer_attention_q_paged_workspace_bytes, sized by max_len), three launches, capturable alike.  Refused as lqer_attention_q_paged,
 * and LQER_E_INVALID for window < 1 or causal = 0.
 * PER-SEQUENCE TOKEN COUNTS - a scheduler step in which most sequences decode one token while a few take a prompt chunk - go through
 * the two _ragged calls.  The metadata contract is the one above, with:
 *   new_starts / q_starts  int32 [batch + 1], on the DEVICE, written by the caller: non-decreasing, starts[0] >= 0, starts[batch] <=
 *                total.  Sequence b of the call owns tokens starts[b] .. starts[b + 1] - 1 of a packed [total][heads][D] tensor,
 *                addressed through TWO strides - elements over token, then over head; D dense.  A count of 0 is allowed.
 *   max_n / max_s  host: an upper bound on every count, 1 <= bound.  It sizes grids only - no result depends on it, and no host
 *                decision depends on a device value.
 * lqer_kv_pool_append_ragged: lqer_kv_pool_append's pool and metadata, then new_starts and max_n, k_new / v_new [total][kv_heads][D] of
 * DT through k_strides[2] / v_strides[2].  Sequence b is appended n_b = new_starts[b + 1] - new_starts[b] keys: afterwards the pool's
 * bytes for it - codes, exponents, the staging rows below len % 16 - are those lqer_kv_pool_append leaves with batch = 1, n = n_b on the
 * same keys; with n_b = 0 no byte of its pages or staging rows is written.  lens[b] + n_b <= max_len is the caller's to keep.  ONE
 * launch on `stream` whatever the counts are, its grid sized by max_n; threads beyond a sequence's n_b leave at once, and per sequence
 * the thread that reads a staging column is still the one that writes it.  Refused as lqer_kv_pool_append, and LQER_E_INVALID for a
 * null new_starts, max_n < 1 or > max_len, total < 0, null strides.
 * lqer_attention_q_paged_ragged: lqer_attention_q_paged with S replaced by (q_starts, max_s, total): q and out are [total][heads][D]
 * through q_strides[2] / out_strides[2], row_stats a dense [total][heads][2] fp32 or NULL.  For every b, the rows of sequence b in out
 * and row_stats are the SAME BITS as lqer_attention_q with batch = 1, S = S_b = q_starts[b + 1] - q_starts[b] on the raw K and V of that
 * sequence - whatever else is in the batch, whatever max_s, max_len and total are and whatever the workspace held.  Causal uses the
 * sequence's own offset T_b - S_b (S_b <= T_b is the caller's to keep).  With S_b = 0 nothing is written for the sequence; with
 * lens[b] = 0 its rows get zeros and no statistics, as above.  The attention grid's x is ceil(max_s / 128): a workgroup whose tile lies
 * beyond its sequence's S_b leaves at once, and the causal "long tiles first" order follows the sequence's own tile count.
 * workspace: lqer_attention_q_paged_ragged_workspace_bytes(batch, heads, kv_heads, max_s, max_len, D) =
 * lqer_attention_q_paged_workspace_bytes at the same arguments - the two images, nothing that follows the counts.  Three launches on
 * `stream` (K image, V image, the attention kernel), no allocation, no host synchronisation, no atomics: capturable in a hipGraph.
 * Refused as lqer_attention_q_paged, and LQER_E_INVALID for a null q_starts, max_s < 1, total < 0.
 * lqer_attention_q_paged_ragged_window: lqer_attention_q_paged_ragged's argument list plus `window` = W >= 1 - the rule and the
 * guarantees of lqer_attention_q_paged_window, every sequence by its own count: lo_b = max(0, lens[b] - S_b - W + 1), the keys from
 * 16 (lo_b / 16) on are in the pool (the caller's to keep), nothing below is read, and the rows of sequence b are the SAME BITS as
 * lqer_attention_q with batch = 1, S = S_b on its FULL raw K and V and the additive window mask.  Workspace
 * (lqer_attention_q_paged_ragged_workspace_bytes), grid and launches are lqer_attention_q_paged_ragged's.  Refused as that call, and
 * LQER_E_INVALID for window < 1 or causal = 0.
 * lqer_attention_q_decode_paged_ragged: lqer_attention_q_paged_ragged's argument list plus `window`, on the split-over-keys kernels of
 * lqer_attention_q_decode_paged - for counts of up to 8 rows: the verify step of a speculative decoder (1 .. 8 draft tokens per
 * sequence), a scheduler step of one-token decoders beside sequences that take a few.  1 <= max_s <= 8; counts above max_s are the
 * caller's breach.  window = 0: no window rule; window = W >= 1: the rule of lqer_attention_q_decode_paged_window (causal = 1 is
 * required), every sequence by its own count - row i of sequence b at position p = i + (lens[b] - S_b) sees keys p - W < j <= p.
 * A workgroup takes S_b = q_starts[b + 1] - q_starts[b] from the device as it takes T_b = lens[b]: the causal offset T_b - S_b, the
 * window's first key, its first live chunk and the token q_starts[b] at which the sequence's rows of q, out and row_stats begin.  For
 * every b, the rows of sequence b in out and row_stats are the SAME BITS as lqer_attention_q_decode with batch = 1 and S = S_b on the
 * raw K and V of that sequence - with a window: on its FULL raw K and V and the additive window mask, and no table entry and no page
 * wholly below key lens[b] - S_b - window + 1 is read - whatever else is in the batch, whatever max_s, max_len and total are and
 * whatever the workspace held.  With S_b = 0 nothing is written for the sequence; with lens[b] = 0 its rows get zeros and no
 * statistics, as above.  The grid is (largest nch of any T <= max_len, kv_heads, batch); no result depends on max_s, which sizes
 * the last launch alone.
 * workspace: lqer_attention_q_decode_paged_ragged_workspace_bytes(total, heads, max_len, D) bytes, 16-byte aligned, contents
 * irrelevant - the three parts of lqer_attention_q_decode_paged's with rows = total heads (its size at batch 1, S = total): the rows
 * are indexed by packed token, sequence b owning rows q_starts[b] heads .. q_starts[b + 1] heads - 1, so the size follows the tokens
 * of the step and not batch x max_s.  Three launches on `stream`, no allocation, no host synchronisation, no atomics: capturable in
 * a hipGraph.  Refused as lqer_attention_q_decode_paged, and LQER_E_INVALID for a null q_starts, max_s < 1 or > 8, total < 0,
 * window < 0, window > 0 with causal = 0, a short or misaligned workspace.  batch = 0 or total = 0: LQER_OK, nothing launched.
 * A DRAFT TREE - the verify step of a speculative decoder that drafts a tree (Medusa, EAGLE, SpecInfer) - goes through the two _tree
 * calls, one rule for both.  The draft nodes of sequence b are its last S_b = q_starts[b + 1] - q_starts[b] keys, in the order they were
 * appended (lqer_kv_pool_append_ragged), parents before children; query row i is node i.  Per packed query token there is one word
 *   tree     uint64 [total], on the DEVICE, written by the caller: bit j (0 <= j < S_b) of tree[q_starts[b] + i] is set iff draft node
 *            j of sequence b is node i itself or one of its ancestors.
 * With T_b = lens[b] and base = T_b - S_b, row i of sequence b sees key t iff t < base (the committed context, all of it) or
 * t = base + j with j <= i and bit j of its word set; bits j > i are ignored.  It is the causal rule with holes in the draft region - a
 * chain, word i = (2 << i) - 1, IS the causal rule - applied as a select in the kernels' TREE instantiation wherever the causal limit is
 * tested; a key a row does not see contributes exactly 0 and is left out of the row's maximum and sum.  Caller's contract, on device
 * data like the table and the lengths: bit i of row i is set (a token sees itself), and S_b <= T_b.
 * lqer_attention_q_decode_paged_tree: lqer_attention_q_decode_paged_ragged's argument list with the trailing `window` replaced by `tree`;
 * 1 <= max_s <= 8, only bits 0 .. 7 are read.  lqer_attention_q_paged_tree: lqer_attention_q_paged_ragged's argument list plus `tree`;
 * 1 <= max_s <= 64.  causal = 1 is required by both.  THE GUARANTEE: for every b, the rows of sequence b in out and row_stats are the
 * SAME BITS as a call of batch 1 with S = S_b - lqer_attention_q_decode for the first entry, lqer_attention_q for the second - on the
 * raw K and V of that sequence (the context plus ALL its draft nodes) with the tree as an additive mask tensor, 0 where visible and
 * the dtype's most negative finite value elsewhere - whatever else is in the batch, whatever pages it lives on, whatever max_s,
 * max_len and total are and whatever the workspace held: a masked score's exponential is exactly 0 in every dtype, as under the
 * window rule.  Mind what that comparison says: sibling draft nodes share blocks of the K quantizer (blocks of 16 keys along t), so a
 * node's bits are those of the masked call on the WHOLE draft, not those of a chain verify of its root-to-node path alone.
 * With S_b = 0 nothing is written for the sequence; with lens[b] = 0 its rows get zeros and no statistics.  The pool is only read.
 * Workspace, grid and launch count are the sibling's - lqer_attention_q_decode_paged_ragged_workspace_bytes(total, heads, max_len, D)
 * and lqer_attention_q_paged_ragged_workspace_bytes(batch, heads, kv_heads, max_s, max_len, D); there is no size function of their
 * own -, three launches on `stream` (the second entry's two image kernels run unchanged, nibble pools included), no allocation, no
 * host synchronisation, no atomics: capturable in a hipGraph.  Refused as the sibling, in its words, and LQER_E_INVALID for a null
 * tree, causal = 0, max_s > 8 (the first entry) or > 64 (the second).  batch = 0 or total = 0: LQER_OK, nothing launched.
 * lqer_kv_pool_gather: one sequence - row `slot` of block_table, T keys (host) - out of the pool into a dense lqer_kv_cache buffer of
 * batch 1 and the given capacity (>= T): codes, exponents and the slot's staging rows, a pure byte copy in one launch.  The result is
 * the cache lqer_kv_cache_append would have built: the test hook (lqer_kv_cache_unpack) and an export path (more than 8 query rows
 * on paged sequences need no copy: lqer_attention_q_paged).
 * lqer_kv_pool_fork: n pairs (src_slots[i], dst_slots[i], lens[i]), three DEVICE arrays: the sequence in slot dst becomes a copy of the
 * first L = lens[i] keys of the one in slot src - a second sample of one prompt, a beam, a snapshot to come back to when speculated
 * tokens are rejected.  The caller writes src's entries 0 .. L / 16 - 1 into dst's table row: full pages are shared by reference and
 * nothing of them is copied.  With L % 16 != 0 the item (block_table[src][L / 16], g) is copied to (block_table[dst][L / 16], g) - a
 * page of dst's own - for every kv head g in all four code and exponent sections, bytes as they are; always, the 16 staging rows of
 * slot src are copied to slot dst for every kv head (with L % 16 == 0 only they move, and nothing depends on them).  From there on
 * dst appends and attends like any sequence, with the bits of a sequence that was appended the same keys itself.  ONE launch on
 * `stream` for all pairs, in 16-byte pieces; the grid comes from n and kv_heads alone - a workgroup whose pair has no open block leaves
 * at once -, no allocation, no host synchronisation, no atomics.  Caller's contract: a slot may be src of several pairs; every dst is
 * named once and is not a src of the same call; the table rows of dst are valid up to ceil(L / 16) entries before the launch; L is
 * at most src's length.  Refused: LQER_E_INVALID - any null pointer, n < 1, pages, slots, kv_heads, table_stride or D < 1, a short or
 * misaligned pool; LQER_E_UNSUPPORTED - a dtype or D lqer_kv_pool_bytes rejects, n x kv_heads beyond the launch grid (2^31 - 1).
 * lqer_kv_pool_copy: pages and slots' staging rows from one pool to another, bytes as they are - swap sequences out to a small pool
 * (which may then go to the host or a file) and back in, hand cached keys from a prefill pool to a decode pool, move pages within one
 * pool.  The two pools have the same dtype, kv_heads, D and code storage and their OWN page and slot counts: (src_pool, src_bytes,
 * src_pages, src_slots) and (dst_pool, dst_bytes, dst_pages, dst_slots), each sized by lqer_kv_pool_bytes - or, with k_fmt / v_fmt,
 * lqer_kv_pool_bytes_fmt - for its own counts.  k_fmt and v_fmt are both NULL for pools of byte codes, otherwise the two formats whose
 * kinds name the storage (as lqer_kv_pool_fork_fmt's; nothing is quantized).  Four int32 arrays on the DEVICE, written by the caller:
 * pair i < n_pages copies page src_page_ids[i] to page dst_page_ids[i] - for every kv head g the item of the K codes, the K exponents,
 * the V codes and the V exponents -, pair j < n_slots the staging rows [kv_heads][16][D] of DT of slot src_slot_ids[j] to slot
 * dst_slot_ids[j].  No table and no length enters: which pages make a sequence is the caller's books' to say, on both sides.  ONE
 * launch on `stream`, a workgroup of 256 per (page pair, kv head) and per (slot pair, kv head), in 16-byte pieces; no allocation, no
 * host synchronisation, no atomics: capturable in a hipGraph.  Either count may be 0; with both 0 the call validates, launches nothing
 * and returns LQER_OK.  The source is only read.  Caller's contract: every id lies in range (pages: [0, src_pages) / [0, dst_pages),
 * slots: [0, src_slots) / [0, dst_slots)); dst_page_ids are distinct, and so are dst_slot_ids; the two pools are either disjoint
 * buffers or the same buffer with the same geometry; if they are the same buffer, no destination page or slot is also a source of
 * this call.  A call that breaks this reads or writes outside the pools or leaves a destination undefined.  Refused with a message,
 * nothing launched: LQER_E_INVALID - a null pool, a pool not 16-byte aligned or shorter than lqer_kv_pool_bytes(_fmt) for its own
 * counts, pages, slots, kv_heads or D < 1, a negative count, a null id array with a positive count, exactly one of k_fmt / v_fmt
 * NULL, two buffers that overlap without being the same pool (same pointer, same counts); LQER_E_UNSUPPORTED - whatever
 * lqer_kv_pool_bytes(_fmt) answers 0 for (dtype, D, kind, width, block), (n_pages + n_slots) x kv_heads beyond the launch grid (2^31 - 1).
 * Refused with a message, nothing launched or touched (decided from host arguments only):
 *   LQER_E_UNSUPPORTED  what lqer_attention_q_decode_kv / lqer_kv_cache_append refuse so (S > 8, formats, D, batch or kv_heads > 65535);
 *                       max_len > 2^30 (every call); lqer_attention_q_paged: what lqer_attention_q_kv refuses so instead (formats, D, S
 *                       or max_len beyond the launch grid, batch, heads or batch x kv_heads > 65535) - S > 8 is not among them;
 *   LQER_E_INVALID      null block_table / seq_slots / lens or any other null pointer; pages, slots or table_stride < 1; max_len < 1
 *                       or > 16 table_stride; n < 1 or n > max_len; a pool shorter than lqer_kv_pool_bytes (with nibble codes:
 *                       lqer_kv_pool_bytes_fmt) or not 16-byte aligned;
 *                       a short or misaligned workspace; gather: slot outside [0, slots), T > capacity, a short or misaligned cache. */
#define LQER_KV_PAGE_KEYS 16
size_t lqer_kv_pool_bytes(int dtype, int64_t pages, int64_t slots, int64_t kv_heads, int64_t D);
size_t lqer_kv_pool_bytes_fmt(int dtype, int64_t pages, int64_t slots, int64_t kv_heads, int64_t D, const lqer_qfmt_t* k_fmt,
                              const lqer_qfmt_t* v_fmt);
int lqer_kv_pool_append(void* pool, size_t pool_bytes, int64_t pages, int64_t slots, const int32_t* block_table, int64_t table_stride,
                        const int32_t* seq_slots, const int32_t* lens, int64_t max_len, const void* k_new, const void* v_new,
                        const int64_t* k_strides, const int64_t* v_strides, int dtype, int64_t batch, int64_t kv_heads, int64_t D, int64_t n,
                        const lqer_qfmt_t* k_fmt, const lqer_qfmt_t* v_fmt, void* stream);
int lqer_kv_pool_append_ragged(void* pool, size_t pool_bytes, int64_t pages, int64_t slots, const int32_t* block_table, int64_t table_stride,
                               const int32_t* seq_slots, const int32_t* lens, int64_t max_len, const int32_t* new_starts, int64_t max_n,
                               const void* k_new, const void* v_new, const int64_t* k_strides, const int64_t* v_strides, int dtype,
                               int64_t batch, int64_t kv_heads, int64_t D, int64_t total, const lqer_qfmt_t* k_fmt, const lqer_qfmt_t* v_fmt,
                               void* stream);
int lqer_kv_pool_gather(const void* pool, size_t pool_bytes, int dtype, int64_t pages, int64_t slots, int64_t kv_heads, int64_t D,
                        const int32_t* block_table, int64_t table_stride, int64_t slot, int64_t T, void* cache, size_t cache_bytes,
                        int64_t capacity, void* stream);
int lqer_kv_pool_fork(void* pool, size_t pool_bytes, int dtype, int64_t pages, int64_t slots, int64_t kv_heads, int64_t D,
                      const int32_t* block_table, int64_t table_stride, const int32_t* src_slots, const int32_t* dst_slots, const int32_t* lens,
                      int64_t n, void* stream);
int lqer_kv_pool_gather_fmt(const void* pool, size_t pool_bytes, int dtype, int64_t pages, int64_t slots, int64_t kv_heads, int64_t D,
                            const int32_t* block_table, int64_t table_stride, int64_t slot, int64_t T, void* cache, size_t cache_bytes,
                            int64_t capacity, const lqer_qfmt_t* k_fmt, const lqer_qfmt_t* v_fmt, void* stream);
int lqer_kv_pool_fork_fmt(void* pool, size_t pool_bytes, int dtype, int64_t pages, int64_t slots, int64_t kv_heads, int64_t D,
                          const int32_t* block_table, int64_t table_stride, const int32_t* src_slots, const int32_t* dst_slots,
                          const int32_t* lens, int64_t n, const lqer_qfmt_t* k_fmt, const lqer_qfmt_t* v_fmt, void* stream);
int lqer_kv_pool_copy(const void* src_pool, size_t src_bytes, int64_t src_pages, int64_t src_slots, void* dst_pool, size_t dst_bytes,
                      int64_t dst_pages, int64_t dst_slots, int dtype, int64_t kv_heads, int64_t D, const int32_t* src_page_ids,
                      const int32_t* dst_page_ids, int64_t n_pages, const int32_t* src_slot_ids, const int32_t* dst_slot_ids, int64_t n_slots,
                      const lqer_qfmt_t* k_fmt, const lqer_qfmt_t* v_fmt, void* stream);
size_t lqer_attention_q_decode_paged_workspace_bytes(int64_t batch, int64_t heads, int64_t kv_heads, int64_t S, int64_t max_len, int64_t D);
int lqer_attention_q_decode_paged(const void* q, const void* pool, size_t pool_bytes, int64_t pages, int64_t slots, const int32_t* block_table,
                                  int64_t table_stride, const int32_t* seq_slots, const int32_t* lens, int64_t max_len, void* out,
                                  float* row_stats, int dtype, int64_t batch, int64_t heads, int64_t kv_heads, int64_t S, int64_t D,
                                  const int64_t* q_strides, const int64_t* out_strides, float scaling, int causal, const lqer_qfmt_t* q_fmt,
                                  const lqer_qfmt_t* k_fmt, const lqer_qfmt_t* p_fmt, const lqer_qfmt_t* v_fmt, void* workspace,
                                  size_t workspace_bytes, void* stream);
int lqer_attention_q_decode_paged_window(const void* q, const void* pool, size_t pool_bytes, int64_t pages, int64_t slots,
                                         const int32_t* block_table, int64_t table_stride, const int32_t* seq_slots, const int32_t* lens,
                                         int64_t max_len, void* out, float* row_stats, int dtype, int64_t batch, int64_t heads,
                                         int64_t kv_heads, int64_t S, int64_t D, const int64_t* q_strides, const int64_t* out_strides,
                                         float scaling, int causal, const lqer_qfmt_t* q_fmt, const lqer_qfmt_t* k_fmt,
                                         const lqer_qfmt_t* p_fmt, const lqer_qfmt_t* v_fmt, void* workspace, size_t workspace_bytes,
                                         void* stream, int64_t window);
int lqer_attention_q_decode_paged_shared(const void* q, const void* pool, size_t pool_bytes, int64_t pages, int64_t slots,
                                         const int32_t* block_table, int64_t table_stride, const int32_t* seq_slots, const int32_t* lens,
                                         int64_t max_len, void* out, float* row_stats, int dtype, int64_t batch, int64_t heads,
                                         int64_t kv_heads, int64_t S, int64_t D, const int64_t* q_strides, const int64_t* out_strides,
                                         float scaling, int causal, const lqer_qfmt_t* q_fmt, const lqer_qfmt_t* k_fmt,
                                         const lqer_qfmt_t* p_fmt, const lqer_qfmt_t* v_fmt, void* workspace, size_t workspace_bytes,
                                         void* stream, const int32_t* grp_of, const int32_t* grp_starts, const int32_t* grp_members,
                                         const int32_t* grp_keys, int64_t n_groups);
int lqer_attention_q_decode_chunk(int64_t T, int64_t D);
size_t lqer_attention_q_paged_workspace_bytes(int64_t batch, int64_t heads, int64_t kv_heads, int64_t S, int64_t max_len, int64_t D);
int lqer_attention_q_paged(const void* q, const void* pool, size_t pool_bytes, int64_t pages, int64_t slots, const int32_t* block_table,
                           int64_t table_stride, const int32_t* seq_slots, const int32_t* lens, int64_t max_len, void* out, float* row_stats,
                           int dtype, int64_t batch, int64_t heads, int64_t kv_heads, int64_t S, int64_t D, const int64_t* q_strides,
                           const int64_t* out_strides, float scaling, int causal, const lqer_qfmt_t* q_fmt, const lqer_qfmt_t* k_fmt,
                           const lqer_qfmt_t* p_fmt, const lqer_qfmt_t* v_fmt, void* workspace, size_t workspace_bytes, void* stream);
int lqer_attention_q_paged_window(const void* q, const void* pool, size_t pool_bytes, int64_t pages, int64_t slots, const int32_t* block_table,
                           int64_t table_stride, const int32_t* seq_slots, const int32_t* lens, int64_t max_len, void* out, float* row_stats,
                           int dtype, int64_t batch, int64_t heads, int64_t kv_heads, int64_t S, int64_t D, const int64_t* q_strides,
                           const int64_t* out_strides, float scaling, int causal, const lqer_qfmt_t* q_fmt, const lqer_qfmt_t* k_fmt,
                           const lqer_qfmt_t* p_fmt, const lqer_qfmt_t* v_fmt, void* workspace, size_t workspace_bytes, void* stream,
                           int64_t window);
size_t lqer_attention_q_paged_ragged_workspace_bytes(int64_t batch, int64_t heads, int64_t kv_heads, int64_t max_s, int64_t max_len, int64_t D);
int lqer_attention_q_paged_ragged(const void* q, const void* pool, size_t pool_bytes, int64_t pages, int64_t slots, const int32_t* block_table,
                                  int64_t table_stride, const int32_t* seq_slots, const int32_t* lens, int64_t max_len, void* out,
                                  float* row_stats, int dtype, int64_t batch, int64_t heads, int64_t kv_heads, const int32_t* q_starts,
                                  int64_t max_s, int64_t total, int64_t D, const int64_t* q_strides, const int64_t* out_strides, float scaling,
                                  int causal, const lqer_qfmt_t* q_fmt, const lqer_qfmt_t* k_fmt, const lqer_qfmt_t* p_fmt,
                                  const lqer_qfmt_t* v_fmt, void* workspace, size_t workspace_bytes, void* stream);
int lqer_attention_q_paged_ragged_window(const void* q, const void* pool, size_t pool_bytes, int64_t pages, int64_t slots,
                                  const int32_t* block_table, int64_t table_stride, const int32_t* seq_slots, const int32_t* lens,
                                  int64_t max_len, void* out, float* row_stats, int dtype, int64_t batch, int64_t heads, int64_t kv_heads,
                                  const int32_t* q_starts, int64_t max_s, int64_t total, int64_t D, const int64_t* q_strides,
                                  const int64_t* out_strides, float scaling, int causal, const lqer_qfmt_t* q_fmt, const lqer_qfmt_t* k_fmt,
                                  const lqer_qfmt_t* p_fmt, const lqer_qfmt_t* v_fmt, void* workspace, size_t workspace_bytes, void* stream,
                                  int64_t window);
size_t lqer_attention_q_decode_paged_ragged_workspace_bytes(int64_t total, int64_t heads, int64_t max_len, int64_t D);
int lqer_attention_q_decode_paged_ragged(const void* q, const void* pool, size_t pool_bytes, int64_t pages, int64_t slots,
                                         const int32_t* block_table, int64_t table_stride, const int32_t* seq_slots, const int32_t* lens,
                                         int64_t max_len, void* out, float* row_stats, int dtype, int64_t batch, int64_t heads,
                                         int64_t kv_heads, const int32_t* q_starts, int64_t max_s, int64_t total, int64_t D,
                                         const int64_t* q_strides, const int64_t* out_strides, float scaling, int causal,
                                         const lqer_qfmt_t* q_fmt, const lqer_qfmt_t* k_fmt, const lqer_qfmt_t* p_fmt,
                                         const lqer_qfmt_t* v_fmt, void* workspace, size_t workspace_bytes, void* stream, int64_t window);
int lqer_attention_q_decode_paged_tree(const void* q, const void* pool, size_t pool_bytes, int64_t pages, int64_t slots,
                                       const int32_t* block_table, int64_t table_stride, const int32_t* seq_slots, const int32_t* lens,
                                       int64_t max_len, void* out, float* row_stats, int dtype, int64_t batch, int64_t heads,
                                       int64_t kv_heads, const int32_t* q_starts, int64_t max_s, int64_t total, int64_t D,
                                       const int64_t* q_strides, const int64_t* out_strides, float scaling, int causal,
                                       const lqer_qfmt_t* q_fmt, const lqer_qfmt_t* k_fmt, const lqer_qfmt_t* p_fmt,
                                       const lqer_qfmt_t* v_fmt, void* workspace, size_t workspace_bytes, void* stream, const uint64_t* tree);
int lqer_attention_q_paged_tree(const void* q, const void* pool, size_t pool_bytes, int64_t pages, int64_t slots, const int32_t* block_table,
                                int64_t table_stride, const int32_t* seq_slots, const int32_t* lens, int64_t max_len, void* out,
                                float* row_stats, int dtype, int64_t batch, int64_t heads, int64_t kv_heads, const int32_t* q_starts,
                                int64_t max_s, int64_t total, int64_t D, const int64_t* q_strides, const int64_t* out_strides, float scaling,
                                int causal, const lqer_qfmt_t* q_fmt, const lqer_qfmt_t* k_fmt, const lqer_qfmt_t* p_fmt,
                                const lqer_qfmt_t* v_fmt, void* workspace, size_t workspace_bytes, void* stream, const uint64_t* tree);

/* ---- calibration statistics (the producer of L2QER's scale_dict; reference src/lqer/statistic_profiler/) ----------------------
 * One pass over an activation x [M, K] (row stride ldx elements; fp32 / fp16 / bf16, values upcast to fp32 as the hook's
 * x.float() does) for the per-input-channel sum|x| and max|x|; any of the three outputs may be NULL, not all of them:
 *   run_absmean_max [K] fp32, in/out: max(run, sum|x[:, k]| / M) - the scale hook's body, scale.py:32-38
 *                       (x.float().abs().view(-1, K).mean(0), torch.maximum into the running scale); a NaN on either side stays;
 *   col_absmax      [K] fp32, out: max|x[:, k]| of this call, exact (NaN for a column that holds one, as torch's amax);
 *   n_cols_ge       [1] int32, out: #{k : some |x[m, k]| >= threshold} of this call - the threshold hook's count,
 *                       threshold.py:39-40 (x.abs().ge(t).view(-1, K).any(dim=0).sum(); a NaN compares false).
 * The sums are added in an order fixed by (M, K, dtype) - no floating-point atomics - so two calls on the same input give the
 * same bits; any K, any ldx >= K, any alignment of x (16-byte aligned rows take 16-byte loads, others element loads: same bits).
 * workspace: lqer_col_abs_stats_workspace_bytes(M, K) bytes, 4-byte aligned, contents irrelevant.  Two launches on `stream`. */
size_t lqer_col_abs_stats_workspace_bytes(int64_t M, int64_t K);
int lqer_col_abs_stats(const void* x, int dtype, int64_t M, int64_t K, int64_t ldx, float* run_absmean_max, float* col_absmax,
                       float threshold, int32_t* n_cols_ge, void* workspace, size_t workspace_bytes, void* stream);

/* ---- measurement aid ---------------------------------------------------------------------------------------------------
 * The shader clock the chip holds while other work runs: `nblocks` (1..64) one-wave workgroups on `stream` (a stream of its
 * own, beside the kernels under study) each write {shader cycles, 100 MHz ticks} elapsed over the last three quarters of about `duration_us` of real time to
 * out_pairs[2 b], out_pairs[2 b + 1] (device uint64).  MHz = cycles / ticks x 100.  bench.py: roofline.sustained_mhz. */
int lqer_clock_probe(unsigned long long* out_pairs, int nblocks, int64_t duration_us, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LQER_HIP_H */
