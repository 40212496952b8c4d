// The GATE instantiations of the one-launch decode kernel (decode1_kernel.h: k_decode1_gated - x = h = act(gate) * up formed from the gate
// and up projections' outputs) in a translation unit of their own, for decode1_normed.hip's reason: decode1.hip's module - and with it the
// code of the standard kernels - stays what it was before they existed.  decode1_dispatch (decode1.hip) checks the call, fills the
// argument block and sizes the launch.
#include "decode1_kernel.h"

namespace lqer {

int decode1_gated_launch(int dtype, int bout, int act, unsigned grid, int lds, hipStream_t st, const d1::ArgsG& one) {
  constexpr int LIMIT = 150 * 1024;
  const unsigned block = 64 * d1::NW;
  auto run = [&](auto dt, auto bo, auto gk) {
    constexpr int DT = decltype(dt)::value, BO = decltype(bo)::value, GATE = decltype(gk)::value;
    return launch_k<d1::k_decode1_gated<DT, BO, GATE>, LIMIT>("lqer_decode1 (gate)", grid, block, lds, st, one);
  };
  auto by_gate = [&](auto dt, auto bo) {  // d1::GateKind: 1 silu * up, 2 silu, 3 relu * up, 4 relu
    const int gate = (act == LQER_ACT_RELU ? 3 : 1) + (one.gz.up ? 0 : 1);
    switch (gate) {
      case 1: return run(dt, bo, std::integral_constant<int, 1>{});
      case 2: return run(dt, bo, std::integral_constant<int, 2>{});
      case 3: return run(dt, bo, std::integral_constant<int, 3>{});
      default: return run(dt, bo, std::integral_constant<int, 4>{});
    }
  };
  auto by_bout = [&](auto dt) { return bout == 1 ? by_gate(dt, std::integral_constant<int, 1>{}) : by_gate(dt, std::integral_constant<int, 0>{}); };
  return dtype == LQER_F16 ? by_bout(std::integral_constant<int, LQER_F16>{}) : by_bout(std::integral_constant<int, LQER_BF16>{});
}

}  // namespace lqer
