// The NORM instantiations of the one-launch decode kernel (decode1_kernel.h: k_decode1_normed - x formed from the raw hidden state, RMSNorm
// or LayerNorm) in a translation unit of their own, so that decode1.hip's module - and with it the code of the standard kernels - is what
// it was before they existed.  decode1_dispatch (decode1.hip) checks the call, fills the argument blocks and sizes the launch.
#include "decode1_kernel.h"

namespace lqer {

int decode1_normed_launch(int dtype, int bout, int norm, unsigned grid, int lds, hipStream_t st, const d1::ArgsN<d1::MAXMEM>& group,
                          const d1::ArgsN<1>& one, bool is_group) {
  constexpr int LIMIT = 150 * 1024;
  const unsigned block = 64 * d1::NW;
  auto run = [&](auto dt, auto bo, auto nm) {
    constexpr int DT = decltype(dt)::value, BO = decltype(bo)::value, NM = decltype(nm)::value;
    return is_group ? launch_k<d1::k_decode1_normed<DT, BO, true, NM>, LIMIT>("lqer_decode1 (norm)", grid, block, lds, st, group)
                    : launch_k<d1::k_decode1_normed<DT, BO, false, NM>, LIMIT>("lqer_decode1 (norm)", grid, block, lds, st, one);
  };
  auto by_norm = [&](auto dt, auto bo) {
    return norm == NORM_LAYER ? run(dt, bo, std::integral_constant<int, 2>{}) : run(dt, bo, std::integral_constant<int, 1>{});
  };
  auto by_bout = [&](auto dt) { return bout == 1 ? by_norm(dt, std::integral_constant<int, 1>{}) : by_norm(dt, std::integral_constant<int, 0>{}); };
  return dtype == LQER_F16 ? by_bout(std::integral_constant<int, LQER_F16>{}) : by_bout(std::integral_constant<int, LQER_BF16>{});
}

}  // namespace lqer
