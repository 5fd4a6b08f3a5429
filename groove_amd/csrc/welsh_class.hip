// welsh_class.hip — one wave-uniform Welsh kernel and its launcher per translation unit, so that the block bodies build in
// parallel: -DGROOVE_BASE_KIND=0..5 the kernel of ONE base kind (0 - 3: its block-writing form only), 9 the all-kinds kernel of small
// banks (8: its block-writing form), 10 / 11 the mix kernel of big banks.  See kernels.h, "Workgroup KINDS".
#define GROOVE_WELSH_CLASS_TU 1
#if defined(GROOVE_BASE_KIND) && (GROOVE_BASE_KIND == 9 || GROOVE_BASE_KIND == 8)
#define GROOVE_WELSH_ANY_TU 1
#endif
#if defined(GROOVE_BASE_KIND) && (GROOVE_BASE_KIND == 10 || GROOVE_BASE_KIND == 11)
#define GROOVE_WELSH_MIX_TU 1
#endif
#include "kernels.h"
#include <cstdio>
#include <cstdlib>
#ifndef GROOVE_BASE_KIND
#error "compile with -DGROOVE_BASE_KIND=<0..5, 8, 9, 10, 11>"
#endif
namespace groove {
#if GROOVE_BASE_KIND >= 0 && GROOVE_BASE_KIND < 6
template <int BASE_KIND>
void launch_welsh_uniform_specialised(const UniformArgs& a, hipStream_t st, bool fused, hipEvent_t done) {
  constexpr int LFO_MODE = BASE_KIND < 2 ? LFO_F32 : BASE_KIND < 4 ? LFO_F64_SMOOTH : LFO_F64;
  constexpr bool RETUNE = BASE_KIND % 2 == 1;
  static_assert(wg_base_kind_of(LFO_MODE, RETUNE) == BASE_KIND, "base kind numbering");
  if constexpr (LFO_MODE == LFO_F64) {
    if (fused) { launch_bound(welsh_render_uniform_kernel<true, LFO_MODE, RETUNE, true>, dim3(a.n_wgs), dim3(kThreads), st, done, a); return; }
  } else if (fused) {
    // kinds 0 - 3 have no fused kernel of their own (groove_hip.hip launch_render refuses the call): a fused caller's `out` is
    // its partial rows, which the block-writing kernel below would overrun
    fprintf(stderr, "groove: no fused per-kind kernel for base kind %d\n", BASE_KIND);
    abort();
  }
  launch_bound(welsh_render_uniform_kernel<false, LFO_MODE, RETUNE, true>, dim3(a.n_wgs), dim3(kThreads), st, done, a);
}
template void launch_welsh_uniform_specialised<GROOVE_BASE_KIND>(const UniformArgs&, hipStream_t, bool, hipEvent_t);
#elif GROOVE_BASE_KIND == 9
void launch_welsh_uniform_any(const UniformArgs& a, const uint8_t* wg_base, hipStream_t st, hipEvent_t done) {
  launch_bound(welsh_render_uniform_any_kernel<true>, dim3(a.n_wgs), dim3(kThreads), st, done, a, wg_base);
}
#elif GROOVE_BASE_KIND == 8
void launch_welsh_uniform_any_unfused(const UniformArgs& a, const uint8_t* wg_base, hipStream_t st, hipEvent_t done) {
  launch_bound(welsh_render_uniform_any_kernel<false>, dim3(a.n_wgs), dim3(kThreads), st, done, a, wg_base);
}
#elif GROOVE_BASE_KIND == 10
void launch_welsh_uniform_mix(const UniformArgs& a, const uint8_t* wg_base, hipStream_t st, hipEvent_t done) {
  launch_bound(welsh_render_uniform_mix_kernel<true>, dim3(a.n_wgs), dim3(kThreads), st, done, a, wg_base);
}
#elif GROOVE_BASE_KIND == 11
void launch_welsh_uniform_mix_unfused(const UniformArgs& a, const uint8_t* wg_base, hipStream_t st, hipEvent_t done) {
  launch_bound(welsh_render_uniform_mix_kernel<false>, dim3(a.n_wgs), dim3(kThreads), st, done, a, wg_base);
}
#else
#error "GROOVE_BASE_KIND out of range"
#endif
static_assert(wg_base_kind_of(LFO_F32, false) == 0 && wg_base_kind_of(LFO_F32, true) == 1 &&
              wg_base_kind_of(LFO_F64_SMOOTH, false) == 2 && wg_base_kind_of(LFO_F64_SMOOTH, true) == 3, "base kind numbering");
} // namespace groove
