// ctl_link.h — the two kernels of a device-resident CONTROL LINK (include/groove_hip.h, groove_ctl_link_*).
//
// A controller's value reaches its target effect without the host: the capture kernel keeps the last frame of the block a
// signal passthrough has passed on, the apply kernel computes the control value (ctl_core.h) and writes it into the
// target's per-lane parameter array — the same d_fa / d_ua words the effect kernels read — both on the ctx stream, where
// stream order is the order of the calls.  One thread per lane, kThreads per workgroup like the other per-lane kernels
// (kernels.h); a launch of either is a few wavefronts and all latency.
#pragma once
#include "kernels.h"
#include "ctl_core.h"

namespace groove {

// The per-source-lane description of a link, SoA on the device: delta64[n_src], duty64[n_src], waveform[n_src], law[n_src].
struct CtlLanes {
  const uint64_t* __restrict__ delta64;
  const uint64_t* __restrict__ duty64;
  const uint32_t* __restrict__ waveform;
  const uint32_t* __restrict__ law;
};

// value[e] = the mono sample of frame `frame` of block[ch][frame][lane] (channel stride chs = capacity * n, NOT frames * n).
__global__ __launch_bounds__(kThreads) void ctl_capture_kernel(const float* __restrict__ block, size_t chs, uint32_t n, uint32_t frame,
                                                               float* __restrict__ value, uint32_t* __restrict__ captured) {
  const uint32_t e = blockIdx.x * kThreads + threadIdx.x;
  if (e >= n) return;
  const size_t at = (size_t)frame * n + e;
  value[e] = ctl_signal_mono(block[at], block[chs + at]);
  if (e == 0) *captured = 1u;
}

// dst[e] = target law(control value of source lane e, or of the one source lane there is).  Exactly one of dst_f / dst_u is set.
// A signal link that has captured nothing yet leaves the target as it is.
__global__ __launch_bounds__(kThreads) void ctl_apply_kernel(uint32_t source, CtlLanes src, uint32_t n_src, uint64_t at_frame,
                                                             const float* __restrict__ value, const uint32_t* __restrict__ captured,
                                                             float* __restrict__ dst_f, uint32_t* __restrict__ dst_u, uint32_t n) {
  const uint32_t e = blockIdx.x * kThreads + threadIdx.x;
  if (e >= n) return;
  const uint32_t s = n_src == 1u ? 0u : e;
  float v;
  if (source == GROOVE_CTL_SRC_LFO) {
    v = ctl_lfo_value01(src.waveform[s], src.delta64[s], src.duty64[s], at_frame);
  } else {
    if (*captured == 0u) return;
    v = ctl_signal_value01(src.law[s], value[s]);
  }
  if (dst_u) dst_u[e] = ctl_target_bits(v);
  else dst_f[e] = ctl_target_float(v);
}

} // namespace groove
