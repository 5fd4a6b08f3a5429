// welsh_split.hip — the role-split Welsh kernel of mid-size banks (welsh_split.h: ctl | osc | tangent + quotients | back), with its
// own class-specialised role bodies.
#define GROOVE_WELSH_CLASS_TU 1
#define GROOVE_WELSH_SPLIT_TU 1
#include "kernels.h"
#include "welsh_split.h"
namespace groove {
void launch_welsh_split4(const UniformArgs& a, const uint8_t* wg_base, hipStream_t st, bool fused, hipEvent_t done) {
  if (fused) launch_bound(welsh_render_split4_kernel<true>, dim3(a.n_wgs), dim3(4 * kSplitLanes), st, done, a, wg_base);
  else launch_bound(welsh_render_split4_kernel<false>, dim3(a.n_wgs), dim3(4 * kSplitLanes), st, done, a, wg_base);
}
} // namespace groove
#ifdef GROOVE_SPLIT_PROBE
extern "C" int groove_debug_split_probe_read(unsigned long long out[12], int reset) { // measurement build only
  if (hipDeviceSynchronize() != hipSuccess) return 2;
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(groove::g_split_probe), sizeof(groove::g_split_probe)) != hipSuccess) return 3;
  if (reset) { unsigned long long z[12] = {}; if (hipMemcpyToSymbol(HIP_SYMBOL(groove::g_split_probe), z, sizeof(z)) != hipSuccess) return 4; }
  return 0;
}
#endif
