// The launch plan of the fused GEMM: what runs for a (descriptor, token count, element type) - computed once, by one pure function
// (gemm_plan.hip), read by the launches (gemm_launch.hip, bout_amax.hip, gemm_w4a8*.hip, gemm_smallm.hip) and by the public queries (api.hip).
#pragma once
#include "common.h"

namespace lqer {

// how the row-block maxima of a B_out with blocks other than 16 (block_fp) reach the GEMM
enum AmaxTravel {
  AMAX_NONE = 0,  // no maxima: B_out pass-through, blocks of 16 (in registers), fixed point, minifloat
  AMAX_CELLS,     // pre-pass launch, one atomicMax cell per (row, block), zeroed first: `need` bytes at the head of the scratch
  AMAX_PARTS,     // pre-pass launch, one block per row on the int8 route: every wave leaves the maximum of ITS column segment in its own
                  // cell [segment][row] (plain stores, nothing zeroed); the GEMM folds them when it reads a row's constants
  AMAX_XCH,       // no pre-pass: one round of the int8 kernel's 128-row tiles exchanges {maximum, tag} granules inside the GEMM launch
  AMAX_MRX,       // no pre-pass: several rounds on a resident grid, the GEMM's workgroups each compute one item of the pre-pass first
};

struct GemmPlan {
  // refusals.  err: what the route queries report too (B_out formats).  launch_err: what only a launch reports, after it has checked
  // the caller's scratch and run the zero fill and the pre-pass (pre-pass rank - instead of the pre-pass -, an int8 image at a token
  // count its kernel does not serve, fp16 main loops that do not exist).
  int err, launch_err;
  char msg[256];
  bool empty;  // M == 0 or N == 0: a launch does nothing and reports nothing

  int bout;  // B_out handling: 0 pass-through, 1 blocks of 16 (maxima in registers), 2 other blocks / fixed point, 3 minifloat
  int bout_L, bout_nblk;
  int route;      // LQER_ROUTE_*; an int8 descriptor outside its kernel's token counts: the route of the same call with LQER_Q_MXINT
  int tile_rows;  // 0 (small-M kernel), 64, 128 or 256
  int tiles_m, tiles_n;
  unsigned grid;

  // the kernel variant, i.e. the template arguments of the route's kernel
  bool lowrank;
  bool f16x;                  // fp16 activations multiplied natively (LQER_F16X in place of LQER_F16)
  bool staged, defer;         // 128-row family: side-product operands through LDS; blocks of 16 re-quantized under the main loop
  bool ksplit;                // ... the deferred, direct kernel with a SIMD's two waves splitting the k-step (gemm_w4a8.hip, KSPLIT)
  bool w_twos, w_mf;          // 128-row family: integer / minifloat nibbles
  bool i8_shift, i8_codes;    // int8 route: weight groups with shifts; 8-bit weight codes
  int mt;                     // small-M kernel: 16-row token tiles, 1..4
  // the weight image the route's kernel reads when the caller holds the compact image of a 2- / 3-bit weight (GemmArgs::w_narrow):
  // 2 or 3 - the small-M kernel's instantiation that reads it directly; -1 - the route's kernel reads standard panels only, the
  // caller widens the image into its workspace first; 0 - the caller holds the standard image
  int w_img;

  AmaxTravel amax;
  size_t need;        // bytes of the caller's scratch the maxima take
  size_t zero_bytes;  // ... of which a pre-pass on atomicMax cells wants zeroed (0: parts, exchange, none)
  // what a call that prepares the scratch ahead of the GEMM call is told: zero_bytes of the same shape with ONE limb of B, whatever
  // the launch's limb count (NOTEBOOK.md "host plan: preserved quirks")
  size_t prep_zero_bytes;
  struct {
    bool lds;  // k_bout_amax_lds (rank 64), else k_bout_amax<rg, nks>
    int rg, nks;
    unsigned grid;
    int tiles_n32, seg_tiles;
    int nseg;  // GemmArgs::bout_nseg: segments used (AMAX_PARTS), else 0
  } pre;
};

// Pure: no HIP call, no static.  `shape`: the shape and format members of GemmArgs (api.hip::gemm_shape_args) plus b_limbs and tuning;
// i8_image: the descriptor is LQER_Q_MXINT_I8 (xq / w8 are the int8 images); cus: device_cus() - or 0 from a caller that reads nothing
// but err, route and tile_rows (the public route queries: no HIP call), since only `amax` and what follows it depend on the count.
GemmPlan plan_gemm(const GemmArgs& shape, bool lowrank, bool i8_image, int dtype, int cus);

int device_cus();  // CUs of the current device (gemm_w4a8_i8.hip: the one HIP query of the plan's inputs)

// fills the plan's share of the kernel arguments (tiles, B_out blocks, segments), checks the scratch, runs the pre-pass or draws the
// exchange tag, and launches the route's kernel
int gemm_launch(const GemmPlan& p, GemmArgs g, int dtype, void* scratch, size_t scratch_bytes, bool amax_zeroed, hipStream_t st);  // gemm_launch.hip
int launch_amax(const GemmPlan& p, const GemmArgs& g, bool amax_zeroed, hipStream_t st);  // bout_amax.hip: zero fill (unless done) + pre-pass
int tile128_launch(const GemmPlan& p, const GemmArgs& g, int dtype, hipStream_t st);  // gemm_w4a8.hip
int m256_launch(const GemmPlan& p, const GemmArgs& g, int dtype, hipStream_t st);     // gemm_w4a8_m256.hip
int i8_launch(const GemmPlan& p, const GemmArgs& g, int dtype, hipStream_t st);       // gemm_w4a8_i8.hip
int smallm_launch(const GemmPlan& p, const GemmArgs& g, int dtype, hipStream_t st);   // gemm_smallm.hip

}  // namespace lqer
