// plan_gemm: the one place that decides which fused-GEMM kernel runs, on what grid, in which variant, and how the row maxima of a
// B_out in wide blocks travel.  Host only, pure: a function of its arguments (the tests of tests/test_routes_cpu.py hold its answers
// to a record).  The CU count of the rounds arithmetic is the full part's 256 (PLAN_CUS: persistent grids, tile heights); the device's
// own count only decides whether a grid is resident at once (the exchange of the row maxima).
#include <stdarg.h>
#include <stdio.h>

#include "gemm_plan.h"

namespace lqer {

namespace {

constexpr int64_t PLAN_CUS = 256;

int refuse(GemmPlan& p, bool at_launch, int code, const char* fmt, ...) {
  if (p.err || p.launch_err) return code;  // (the first refusal is the one a call reports)
  (at_launch ? p.launch_err : p.err) = code;
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(p.msg, sizeof(p.msg), fmt, ap);
  va_end(ap);
  return code;
}

int64_t rounds(int64_t tiles) { return (tiles + PLAN_CUS - 1) / PLAN_CUS; }

// Rows of a tile of the int8 kernel: rounds of one tile per CU (the grid is persistent: a CU walks ceil(tiles / 256) tiles), a
// 128-row tile priced at 0.56 of a 256-row one (half the main loop and epilogue, the same ring fill and launch ramp; the weight
// expand per MFMA doubles).  Llama-7B projections at M = 2048: 4096 x 4096 fills 128 CUs with 256-row tiles and all 256 with
// 128-row ones; N = 11008: 2 rounds of 256 rows against 3 x 0.56.  LQER_TUNE_I8_ROWS_* pins the choice (tests: same bits).
// (8-bit weight codes: the same rule - the 128-row kernel, codes straight into registers, takes 35.8 us per round of 4096-k tiles
// against 63.5 us of the 256-row kernel's half-step LDS ring: 0.56 again.  M = 2048 x 4096 x 4096: 128 rows, all 256 CUs,
// 35.8 us against 63 us on half of them; M = 8192: 256 rows, 127 us against 137 us)
int i8_tile_rows(const GemmArgs& g) {
  if (g.tuning & LQER_TUNE_I8_ROWS_128) return 128;
  if (g.tuning & LQER_TUNE_I8_ROWS_256) return 256;
  const int64_t tn = g.Np / BN;
  const int64_t r256 = rounds(((g.M + 255) / 256) * tn), r128 = rounds(((g.M + 127) / 128) * tn);
  return r128 * LQER_I8_ROWS128_COST < r256 * 100 ? 128 : 256;
}

// Rows of a tile of the 128-row kernel family.  Token counts whose 128-row grid covers at most half of the CUs: 64-row tiles
// (twice the workgroups, half the MFMA work per expanded weight fragment - the k-step is then paced by the weight expand,
// NOTEBOOK.md §4.1) as long as they still fit one round.  Integer / minifloat nibbles and a minifloat B_out: 128-row instantiations only.
int tile128_rows(const GemmArgs& g) {
  const int64_t tn = g.Np / BN;
  const int64_t t128 = (int64_t)((g.M + BM - 1) / BM) * tn, t64 = (int64_t)((g.M + 63) / 64) * tn;
  const int pin = (g.tuning & LQER_TUNE_TILE_ROWS_128) ? 128 : ((g.tuning & LQER_TUNE_TILE_ROWS_64) ? 64 : 0);  // (tests)
  const bool mf = g.w_mf || g.bout.kind == LQER_Q_MINIFLOAT;
  if (!g.w_twos && !mf && ((pin != 128 && 2 * t128 <= PLAN_CUS && t64 > t128 && g.M > 64) || (pin == 64 && g.M > 64))) return 64;
  return BM;
}

// A 256 x 256 tile costs about 1.9 tiles of 128 x 256 (one weight expand per 8 MFMAs instead of 4, half the per-tile
// fixed work), but both kernels run in whole rounds of one tile per CU: take the large tiles only when they still need
// less time after rounding up - e.g. 16384 x 5120: 5 rounds against 10, 4096 x 4096: 1 against 2, but 2048 x 11008:
// 2 (344 tiles) against 3 (688) keeps the small tiles (measured: 157 vs 178 us).
bool m256_eligible(const GemmArgs& g) {
  const int64_t tn = g.Np / BN;
  const int64_t r256 = rounds((int64_t)((g.M + 255) / 256) * tn), r128 = rounds((int64_t)((g.M + 127) / 128) * tn);
  return g.M >= LQER_M256_MIN_M && r256 * LQER_M256_COST < r128 * 10;
}

// The int8 kernel computes the B_out row maxima inside its own launch (no pre-pass) when its 128-row tiles are resident at once,
// the side product is at most 2 limbs x 4 slices (its operands wait in registers under the ring fill), and
//   AMAX_XCH - there is ONE round, at most one tile per CU, and a row band has at most LQER_AMAX_NSEG column tiles (one granule each
//              per row);
//   AMAX_MRX - or several rounds of 4-bit weights on the persistent grid of min(tiles, 256) workgroups, where every (row band,
//              sixteenth of the columns) item of the pre-pass has a workgroup of its own.
// (cus: the CUs this device really has - a partitioned part shows 32 of them: a grid that runs in rounds there would send every
// workgroup through its polls and its fall-back)
AmaxTravel i8_in_launch_amax(const GemmArgs& g, int tile_rows, int b_limbs, int cus) {
  if (tile_rows != 128) return AMAX_NONE;
  const int nsl = g.rp / 16;
  if (!((b_limbs == 1 || b_limbs == 2) && (nsl == 1 || nsl == 2 || nsl == 4))) return AMAX_NONE;
  const int64_t tn = g.Np / BN, tm = (g.M + 127) / 128;
  const int64_t resident = cus < PLAN_CUS ? cus : PLAN_CUS;
  const bool no_pin = !(g.tuning & (LQER_TUNE_AMAX_ATOMIC | LQER_TUNE_AMAX_PARTS));
  if (no_pin && tn <= LQER_AMAX_NSEG && tm * tn <= resident) return AMAX_XCH;
  if (!no_pin || (g.tuning & LQER_TUNE_AMAX_NO_MRX) || g.w_i8codes || g.rp > 64) return AMAX_NONE;
  const int64_t grid = tm * tn < PLAN_CUS ? tm * tn : PLAN_CUS;
  if (tm * tn <= resident && tn <= LQER_AMAX_NSEG) return AMAX_NONE;  // (one round: the exchange instantiation)
  return (grid > cus || tm * LQER_AMAX_NSEG > grid) ? AMAX_NONE : AMAX_MRX;
}

// How a launch with B_out blocks other than 16 (block_fp; p.bout_nblk set) gets its row-block maxima - AmaxTravel.  Segment partials
// are taken while the segments stay narrow (up to 8 column tiles: beyond N = 4096 wider segments mean half the waves, each twice as
// long - 2048 x 11008, rank 32: 111.9 us with partials against 104.4 with cells; tools/ab_i8.py --rows --amax), or where the
// pre-pass would not use more than LQER_AMAX_NSEG segments anyway (token counts from ~16k: C4 - the same pre-pass grid, minus the
// zero fill: 4.7 us of a 62-us step at M = 2048).
AmaxTravel amax_travel(const GemmPlan& p, const GemmArgs& g, bool i8_image, bool i8_ok, int b_limbs, int cus) {
  const int tiles_n32 = g.Np / 32;
  const bool one = i8_image && p.bout_nblk == 1;
  if (!one) return AMAX_CELLS;
  if (i8_ok) {
    const AmaxTravel in_launch = i8_in_launch_amax(g, p.tile_rows, b_limbs, cus);
    if (in_launch != AMAX_NONE) return in_launch;
  }
  // segments the pre-pass would use with no cap (its LDS variant at rank 64, else the register variant at its default row groups)
  int64_t uncapped;
  if (g.rp == 64) {
    const int64_t wgroups4 = ((((g.M + 31) / 32 + 3) / 4) + 3) / 4;
    uncapped = (LQER_AMAX_WAVES / 4) / wgroups4;
  } else {
    const int RG = g.rp <= 64 ? 4 : (g.rp <= 128 ? 2 : 1);
    uncapped = LQER_AMAX_WAVES / (((g.M + 31) / 32 + RG - 1) / RG);
  }
  const bool parts = !(g.tuning & LQER_TUNE_AMAX_ATOMIC) &&
                     (tiles_n32 <= 8 * LQER_AMAX_NSEG || uncapped <= LQER_AMAX_NSEG || (g.tuning & LQER_TUNE_AMAX_PARTS));
  return parts ? AMAX_PARTS : AMAX_CELLS;
}

size_t amax_need(const GemmPlan& p, const GemmArgs& g, AmaxTravel t) {
  const int per_row = (t == AMAX_XCH || t == AMAX_MRX) ? 2 * LQER_AMAX_NSEG : (t == AMAX_PARTS ? LQER_AMAX_NSEG_WIDE : p.bout_nblk);
  return (size_t)lqer_padded_m(g.M) * per_row * sizeof(float);
}

// The pre-pass launch (k_bout_amax / k_bout_amax_lds): one wave = 32 rg token rows x a run of seg_tiles 32-column tiles.
void plan_prepass(GemmPlan& p, const GemmArgs& g) {
  const bool parts = p.amax == AMAX_PARTS;
  const int tiles_n32 = g.Np / 32;
  // padded rank (x limbs of x A) -> 16-deep slices (a template parameter: exact, no per-slice branch) and row groups per wave
  const int nks = g.rp / 16;
  int RG = g.rp <= 64 ? 4 : (g.rp <= 128 ? 2 : 1);
  const int nseg_cap = parts ? (tiles_n32 <= 8 * LQER_AMAX_NSEG ? LQER_AMAX_NSEG : LQER_AMAX_NSEG_WIDE) : tiles_n32;
  // (segment partials cap the column split: fewer row groups per wave keep the grid at about a thousand waves)
  if (parts && nks <= 4)
    while (RG > 1 && (((g.M + 31) / 32 + RG - 1) / RG) * nseg_cap < 1024) RG >>= 1;
  const int64_t wgroups4 = ((((g.M + 31) / 32 + 3) / 4) + 3) / 4;  // workgroups of the LDS variant along the rows (4 waves x 4 row groups)
  // rank 64: the B^T run through LDS, four row groups per workgroup
  p.pre.lds = nks == 4 && g.rp == 64 && (!parts || wgroups4 * LQER_AMAX_NSEG >= 256);
  // one round of two waves per SIMD (the register variant holds 184-256 registers); the LDS variant counts workgroups
  const int64_t groups = p.pre.lds ? wgroups4 : ((g.M + 31) / 32 + RG - 1) / RG;
  int nseg = (int)((p.pre.lds ? LQER_AMAX_WAVES / 4 : LQER_AMAX_WAVES) / groups);
  nseg = nseg < 1 ? 1 : (nseg > tiles_n32 ? tiles_n32 : nseg);
  nseg = nseg > nseg_cap ? nseg_cap : nseg;
  const int seg_tiles = (tiles_n32 + nseg - 1) / nseg;
  const int nseg_used = (tiles_n32 + seg_tiles - 1) / seg_tiles;
  p.pre.rg = RG, p.pre.nks = nks;
  p.pre.tiles_n32 = tiles_n32, p.pre.seg_tiles = seg_tiles;
  p.pre.nseg = parts ? nseg_used : 0;
  p.pre.grid = (unsigned)(p.pre.lds ? groups * nseg_used : (groups * nseg_used + 3) / 4);
  if (!p.pre.lds && (nks < 1 || nks > 16)) refuse(p, true, LQER_E_UNSUPPORTED, "B_out pre-pass: padded rank %d x limbs > 256", g.rp);
}

}  // namespace

GemmPlan plan_gemm(const GemmArgs& g, bool lowrank, bool i8_image, int dtype, int cus) {
  GemmPlan p = {};
  p.empty = g.M == 0 || g.N == 0;
  p.lowrank = lowrank;
  p.f16x = dtype == LQER_F16 && g.x_f16;

  // ---- B_out handling -----------------------------------------------------------------------------------------------------------
  const bool bout_blocks = lowrank && g.bout.kind == LQER_Q_MXINT && g.bout.block != 16;
  if (lowrank && g.bout.kind == LQER_Q_MXINT && g.bout.block == 16) {
    p.bout = 1;
  } else if (bout_blocks) {
    const int L = (g.bout.block <= 0 || g.bout.block >= g.N) ? g.Np : g.bout.block;
    if (L % 16 != 0) {
      refuse(p, false, LQER_E_UNSUPPORTED, "B_out_quantizer block %d: must be a multiple of 16 or cover the row", g.bout.block);
      return p;
    }
    p.bout = 2, p.bout_L = L, p.bout_nblk = (g.Np + L - 1) / L;
  } else if (lowrank && g.bout.kind == LQER_Q_INT) {  // fixed point: elementwise, no block maxima - the "any block" code without its pre-pass
    p.bout = 2, p.bout_L = 16, p.bout_nblk = 0;
  } else if (lowrank && g.bout.kind == LQER_Q_MINIFLOAT) {  // elementwise with an exponent per element: the 128-row tile kernel's BOUT 3
    p.bout = 3;
  } else if (lowrank && g.bout.kind != LQER_Q_PASSTHROUGH) {
    refuse(p, false, LQER_E_UNSUPPORTED, "B_out_quantizer kind %d not implemented", g.bout.kind);
    return p;
  }

  // ---- route and tile ------------------------------------------------------------------------------------------------------------
  // The int8 main loop needs: the int8 images, a token count of the tile kernels (M >= 128; below, the sign-magnitude image serves the
  // weight-streaming and 64-row kernels), B_out pass-through or one block per row, at most two 64-column panels of xAq.  An int8 tile
  // costs 0.58 (256 rows) / 0.65 (128 rows) of the bf16 kernel's tiles over the same rows, so there is no token count from which the
  // bf16 tile kernel would be the better choice.
  const bool i8_ok = i8_image && g.M >= 128 && (p.bout == 0 || (p.bout == 2 && p.bout_nblk == 1)) && g.rp <= 128;
  const bool nibbles128 = g.w_twos || g.w_mf || p.bout == 3;  // integer / minifloat nibbles, minifloat B_out: the 128-row tile kernel at every M
  if (i8_ok) {
    p.route = LQER_ROUTE_I8, p.tile_rows = i8_tile_rows(g);
  } else if (!nibbles128 && g.M <= SM_MAX_M && p.bout <= 1) {  // decode sizes: the HBM-bound variant
    p.route = LQER_ROUTE_SMALLM, p.tile_rows = 0;
  } else if (!nibbles128 && m256_eligible(g)) {
    p.route = LQER_ROUTE_TILE256, p.tile_rows = 256;
  } else {
    p.route = LQER_ROUTE_TILE128, p.tile_rows = tile128_rows(g);
  }
  // ---- the compact image of a 2- / 3-bit weight: read directly by the weight-streaming kernel, widened first for every other
  if (g.w_narrow) {
    if (i8_image)
      refuse(p, false, LQER_E_UNSUPPORTED, "compact weight image: not on the int8 route (LQER_Q_MXINT_I8 reads an int8 image of its own)");
    else if (g.w_twos || g.w_mf)
      refuse(p, false, LQER_E_UNSUPPORTED,
             "compact weight image: block_fp weights on the table-free expand only (integer / minifloat nibbles, LQER_TUNE_W_EXP_TABLE)");
    else
      p.w_img = p.route == LQER_ROUTE_SMALLM ? (g.w_narrow >> 8) : -1;
    if (p.err) return p;
  }
  if (p.empty) return p;

  // ---- the row maxima of B_out blocks other than 16 ---------------------------------------------------------------------------------
  if (bout_blocks) {
    p.amax = amax_travel(p, g, i8_image, i8_ok, g.b_limbs, cus);
    p.need = amax_need(p, g, p.amax);
    p.zero_bytes = p.amax == AMAX_CELLS ? p.need : 0;
    const AmaxTravel one_limb = g.b_limbs == 1 ? p.amax : amax_travel(p, g, i8_image, i8_ok, 1, cus);
    p.prep_zero_bytes = one_limb == AMAX_CELLS ? amax_need(p, g, one_limb) : 0;
    if (p.amax == AMAX_CELLS || p.amax == AMAX_PARTS) plan_prepass(p, g);
  }

  // ---- grid and kernel variant ---------------------------------------------------------------------------------------------------
  if (i8_image && !i8_ok)  // xq is the int8 image - only the int8 kernel can read it
    refuse(p, true, LQER_E_UNSUPPORTED,
           "linear_gemm: LQER_Q_MXINT_I8 is not served for M=%d here (lqer_gemm_route != LQER_ROUTE_I8): call with LQER_Q_MXINT", g.M);
  switch (p.route) {
    case LQER_ROUTE_I8:
      // persistent: at most one workgroup per CU (the LDS ring leaves room for one), each walks tiles b, b + grid, ...
      p.tiles_m = (g.M + p.tile_rows - 1) / p.tile_rows, p.tiles_n = g.Np / BN;
      p.grid = (unsigned)(p.tiles_m * p.tiles_n < PLAN_CUS ? p.tiles_m * p.tiles_n : PLAN_CUS);
      p.i8_codes = g.w_i8codes, p.i8_shift = g.i8_shift;
      break;
    case LQER_ROUTE_SMALLM:
      p.grid = (unsigned)(g.Np / 16);
      p.mt = g.M > 48 ? 4 : (g.M + 15) / 16;
      break;
    case LQER_ROUTE_TILE256:
      p.tiles_m = (g.M + 255) / 256, p.tiles_n = g.Np / BN;
      p.grid = (unsigned)(p.tiles_m * p.tiles_n);
      break;
    default:
      p.tiles_m = (g.M + p.tile_rows - 1) / p.tile_rows, p.tiles_n = g.Np / BN;
      p.grid = (unsigned)(p.tiles_m * p.tiles_n);
      p.w_twos = g.w_twos, p.w_mf = g.w_mf;
      if (p.f16x && (p.w_mf || p.bout == 3))
        refuse(p, true, LQER_E_UNSUPPORTED,
               "linear_gemm: minifloat weights and B_out have no fp16 main loop (pass-through fp16 activations take the limb route)");
      else if (p.f16x && p.w_twos)
        refuse(p, true, LQER_E_UNSUPPORTED,
               "linear_gemm: integer weights have no fp16 main loop (pass-through fp16 activations take the limb route)");
      // the side product's operands through LDS: more than two 16-deep slices of it - and always beside integer / minifloat nibbles
      p.staged = lowrank && (p.w_twos || p.w_mf || g.rp * g.b_limbs > LQER_STAGE_MIN);
      // B_out in blocks of 16 re-quantized under the first 16 k-steps instead of in front of the main loop: 128-row tiles of plain
      // nibbles, K >= 1024, clamps within the magic-number rounding, and the 1e-8 pass-through that makes the clamped scale exponent exact
      p.defer = p.bout == 1 && !nibbles128 && p.tile_rows == 128 && !(g.tuning & LQER_TUNE_BOUT_IN_PROLOGUE) && g.Kp / BK >= 16 &&
                g.bout.kind == LQER_Q_MXINT && g.bout.mmax <= 4194304.0f && g.bout.mneg <= 4194304.0f && g.bout.tiny >= 1e-8f;
      // the wave pairs of a SIMD split the k-step (half the LDS activation reads): the deferred kernel with the direct side path on
      // the bf16 main loop (gemm_w4a8.hip: that instantiation itself; the pin runs k_lqer_gemm_nks)
      p.ksplit = p.defer && !p.staged && !p.f16x && !(g.tuning & LQER_TUNE_NO_KSPLIT);
      break;
  }
  return p;
}

}  // namespace lqer
