// The one dispatcher of the fused GEMM: executes a launch plan (gemm_plan.hip) - the plan's share of the kernel arguments, the
// scratch check, the B_out pre-pass (bout_amax.hip) or the exchange tag, then the route's kernel.
#include <atomic>

#include "gemm_plan.h"

namespace lqer {

int gemm_launch(const GemmPlan& p, GemmArgs g, int dtype, void* scratch, size_t scratch_bytes, bool amax_zeroed, hipStream_t st) {
  if (p.empty) return LQER_OK;
  if (p.err) {
    set_error("%s", p.msg);
    return p.err;
  }
  if (p.w_img < 0) {  // (api.hip widens into the caller's workspace and launches the standard image's plan: never reached from there)
    set_error("linear_gemm: this route's kernel reads standard panels - the compact weight image must be widened first");
    return LQER_E_INVALID;
  }
  g.tiles_m = p.tiles_m, g.tiles_n = p.tiles_n;
  if (p.bout == 2) g.bout_L = p.bout_L, g.bout_nblk = p.bout_nblk, g.bout_amax = nullptr, g.bout_nseg = p.pre.nseg;
  if (p.amax != AMAX_NONE) {
    if (!scratch || scratch_bytes < p.need) {
      set_error("linear_gemm: scratch %zu B < %zu B for the B_out row-block maxima", scratch_bytes, p.need);
      return LQER_E_WORKSPACE;
    }
    g.bout_amax = (float*)scratch;
  }
  if (p.amax == AMAX_XCH || p.amax == AMAX_MRX) {
    // the call's tag: a counter spread over all 32 bits (odd multiplier: a bijection); the kernel mixes in its dispatch id and queue
    static std::atomic<uint32_t> xch_calls{1};
    g.xch_nonce = xch_calls.fetch_add(1, std::memory_order_relaxed) * 0x9E3779B1u;
  } else if (p.amax != AMAX_NONE) {
    const int rc = launch_amax(p, g, amax_zeroed, st);
    if (rc) return rc;
  }
  if (p.launch_err) {  // (behind the pre-pass, where these refusals have always been reported)
    set_error("%s", p.msg);
    return p.launch_err;
  }
  switch (p.route) {
    case LQER_ROUTE_I8: return i8_launch(p, g, dtype, st);
    case LQER_ROUTE_SMALLM: return smallm_launch(p, g, dtype, st);  // decode sizes: HBM-bound variant
    case LQER_ROUTE_TILE256: return m256_launch(p, g, dtype, st);   // large M: 256 x 256 tiles
    default: return tile128_launch(p, g, dtype, st);
  }
}

}  // namespace lqer
