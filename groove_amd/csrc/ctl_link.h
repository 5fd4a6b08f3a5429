// ctl_link.h — the kernels of a device-resident CONTROL LINK (include/groove_hip.h, groove_ctl_link_*).
//
// A controller's value reaches its target effect without the host: the capture kernel keeps the last frame of the block a
// signal passthrough has passed on, the apply kernel computes the control value (ctl_core.h) and writes it into the
// target's per-lane parameter array — the same d_fa / d_ua words the effect kernels read — both on the ctx stream, where
// stream order is the order of the calls.  One thread per lane, kThreads per workgroup like the other per-lane kernels
// (kernels.h); a launch of either is a few wavefronts and all latency.  A link onto a Welsh BANK (dca-gain, dca-pan, filter-cutoff) writes
// the voices' parameter words instead: the last section below.
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

// What a filter link's apply does with the parameter `mine` of lane e: into the lane's word of the parameter shadow, then the lane's
// coefficients from the five shadow words in f64 (fx_coef.h: the host's own text), stored where the IIR kernels read them, coef[k * n + lane].
__device__ __forceinline__ void ctl_filter_store(uint32_t kind, uint32_t control_index, float mine, double sr, float* __restrict__ shadow,
                                                 double* __restrict__ coef, uint32_t n, uint32_t e) {
  const uint32_t word = ctl_shadow_word(control_index);
  shadow[(size_t)word * n + e] = mine;
  float p[CTL_SHADOW_WORDS];
#pragma unroll
  for (uint32_t k = 0; k < CTL_SHADOW_WORDS; ++k) p[k] = k == word ? mine : shadow[(size_t)k * n + e];
  double c[6];
  uint32_t nc = 5;
  if (kind == GROOVE_FX_BIQUAD_LP24) {
    fx_lp24_coeffs((double)p[CTL_SHADOW_CUTOFF], (double)p[CTL_SHADOW_RIPPLE], sr, c);
    nc = 6;
  } else if (!fx_rbj_for_kind(kind, (double)p[CTL_SHADOW_CUTOFF], (double)p[CTL_SHADOW_Q], (double)p[CTL_SHADOW_BANDWIDTH],
                              (double)p[CTL_SHADOW_DB_GAIN], sr, c)) {
    return; // (not an IIR kind: groove_ctl_filter_link_create refuses it)
  }
#pragma unroll
  for (uint32_t k = 0; k < 6; ++k)
    if (k < nc) coef[(size_t)k * n + e] = c[k];
}

// A link onto a filter's cutoff, q or passband-ripple (ctl_target_derived): the control value becomes the parameter by
// groove_fx_set_param's law, lands in the lane's word of the parameter shadow, and the lane's coefficients are derived from the five
// shadow words in f64 (fx_coef.h: the host's own text) and stored where the IIR kernels read them, coef[k * n + lane].  A second link
// onto the same effect runs behind this one on the ctx stream and loads what this one stored.
__global__ __launch_bounds__(kThreads) void ctl_filter_apply_kernel(uint32_t source, CtlLanes src, uint32_t n_src, uint64_t at_frame,
                                                                    const float* __restrict__ value, const uint32_t* __restrict__ captured,
                                                                    uint32_t kind, uint32_t control_index, double sr,
                                                                    float* __restrict__ shadow, double* __restrict__ coef, uint32_t n) {
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
  ctl_filter_store(kind, control_index, ctl_derived_param(control_index, v), sr, shadow, coef, n, e);
}

// ---- trip source --------------------------------------------------------------------------------------------------------------
// The device table of a trip link, SoA [step][source lane]: begin has n_steps + 1 rows (ctl_core.h: ctl_trip_begins).
struct CtlTrip {
  const double* __restrict__ begin;
  const double* __restrict__ start;
  const double* __restrict__ end;
  const double* __restrict__ beats;
  const uint32_t* __restrict__ kind;
  uint32_t n_steps;
};
// The value of source lane s at `now`, or false where the lane's trip has no step there.
__device__ __forceinline__ bool ctl_trip_lane_value(const CtlTrip& t, uint32_t n_src, uint32_t s, double now, double& v) {
  const int32_t i = ctl_trip_find(t.begin + s, n_src, t.n_steps, now);
  if (i < 0) return false;
  const size_t at = (size_t)i * n_src + s;
  v = ctl_trip_value(t.kind[at], t.start[at], t.end[at], t.begin[at], t.beats[at], now);
  return true;
}
// ctl_apply_kernel with a trip as the source: the f64 value through groove_fx_set_param's law (ctl_core.h: ctl_target_*_f64).
__global__ __launch_bounds__(kThreads) void ctl_trip_apply_kernel(CtlTrip trip, uint32_t n_src, uint64_t at_units, float* __restrict__ dst_f,
                                                                  uint32_t* __restrict__ dst_u, uint32_t n) {
  const uint32_t e = blockIdx.x * kThreads + threadIdx.x;
  if (e >= n) return;
  double v;
  if (!ctl_trip_lane_value(trip, n_src, n_src == 1u ? 0u : e, ctl_trip_now(at_units), v)) return;
  if (dst_u) dst_u[e] = ctl_target_bits_f64(v);
  else dst_f[e] = ctl_target_float_f64(v);
}
// ctl_filter_apply_kernel with a trip as the source.
__global__ __launch_bounds__(kThreads) void ctl_trip_filter_apply_kernel(CtlTrip trip, uint32_t n_src, uint64_t at_units, uint32_t kind,
                                                                         uint32_t control_index, double sr, float* __restrict__ shadow,
                                                                         double* __restrict__ coef, uint32_t n) {
  const uint32_t e = blockIdx.x * kThreads + threadIdx.x;
  if (e >= n) return;
  double v;
  if (!ctl_trip_lane_value(trip, n_src, n_src == 1u ? 0u : e, ctl_trip_now(at_units), v)) return;
  ctl_filter_store(kind, control_index, ctl_derived_param_f64(control_index, v), sr, shadow, coef, n, e);
}

// ---- bank target --------------------------------------------------------------------------------------------------------------
// A link onto a Welsh bank's dca-gain, dca-pan or filter-cutoff (groove_ctl_bank_link_create / groove_ctl_bank_trip_create).  The ONE
// source lane's value is broadcast to every voice, so voices that shared a parameter record before the apply share one after it: the
// wave-uniform kernels' records stay uniform.  The voice kernels read these words in two places and both are written here:
//   params[word * n + lane]   the per-lane SoA (per-lane, time-parallel and note-event kernels)
//   waves[w].p                the per-virtual-wave copy (wave-uniform kernels), w < n_vwaves; 0 waves on the per-lane form
// gl and gr depend on gain AND pan, which may differ between the voices of a bank: dca[CTL_DCA_WORDS][n] is the bank's per-lane shadow
// of the two (internal lane order), the apply stores its own word there and reads the other.
//
// This is a BETWEEN-BLOCKS mutation: the host orders the launch behind every render of the bank submitted so far and ahead of every
// later one (groove_hip.hip bank_link_apply: event join, fork), so no wavefront reads a record while it is written.  A write in the
// middle of a block would break the promise of welsh_wave_tables_up (kernels.h) — what a wave is at the start of a block it stays for the
// whole block: its record is in scalar registers, its tables are filled from it — and a padding wave that read a torn record is how a
// render once never finished (README.md on the stall of rounds 2-3).
struct CtlBank {
  uint32_t* __restrict__ params;
  WaveDesc* __restrict__ waves;
  float* __restrict__ dca; // nullptr on a cutoff link
  uint32_t n, n_vwaves, control_index;
};
// Thread e serves lane e (e < n) and virtual wave e (e < n_vwaves) with the parameter `mine`, the same in every thread.  A wave's lanes
// share a record, so the wave's words are those of its lane vbase; only the shadow word this link does NOT write is read from another
// lane's column, so the two halves need no order between them.  A padding wave (count == 0) is written like any other: its vbase is a
// valid voice of its kind and nothing reads its gains.
__device__ __forceinline__ void ctl_bank_store(const CtlBank& b, float mine, uint32_t e) {
  constexpr uint32_t kGl = offsetof(WelshParams, gl) / 4, kGr = offsetof(WelshParams, gr) / 4, kHz = offsetof(WelshParams, cutoff_hz) / 4;
  const size_t n = b.n;
  if (b.control_index == GROOVE_CTL_WELSH_CUTOFF) {
    if (e < b.n) b.params[kHz * n + e] = __float_as_uint(mine);
    if (e < b.n_vwaves) b.waves[e].p.cutoff_hz = mine;
    return;
  }
  const bool is_gain = b.control_index == GROOVE_CTL_WELSH_DCA_GAIN;
  const float* other = b.dca + (size_t)(is_gain ? CTL_DCA_PAN : CTL_DCA_GAIN) * n;
  if (e < b.n) {
    b.dca[(size_t)(is_gain ? CTL_DCA_GAIN : CTL_DCA_PAN) * n + e] = mine;
    float gl, gr;
    pan_gains((double)(is_gain ? mine : other[e]), (double)(is_gain ? other[e] : mine), gl, gr);
    b.params[kGl * n + e] = __float_as_uint(gl);
    b.params[kGr * n + e] = __float_as_uint(gr);
  }
  if (e < b.n_vwaves) {
    const uint32_t lane = b.waves[e].vbase;
    if (lane < b.n) {
      float gl, gr;
      pan_gains((double)(is_gain ? mine : other[lane]), (double)(is_gain ? other[lane] : mine), gl, gr);
      b.waves[e].p.gl = gl;
      b.waves[e].p.gr = gr;
    }
  }
}
// An LFO or signal source: the fp32 value01 widened, through groove_bank_set_param's law.
__global__ __launch_bounds__(kThreads) void ctl_bank_apply_kernel(uint32_t source, CtlLanes src, uint64_t at_frame, const float* __restrict__ value,
                                                                  const uint32_t* __restrict__ captured, CtlBank bank) {
  const uint32_t e = blockIdx.x * kThreads + threadIdx.x;
  if (e >= bank.n && e >= bank.n_vwaves) return;
  float v;
  if (source == GROOVE_CTL_SRC_LFO) {
    v = ctl_lfo_value01(src.waveform[0], src.delta64[0], src.duty64[0], at_frame);
  } else {
    if (*captured == 0u) return;
    v = ctl_signal_value01(src.law[0], value[0]);
  }
  ctl_bank_store(bank, ctl_bank_param_f64(bank.control_index, (double)v), e);
}
// A trip source: the f64 value.  No step at at_units: every word stays as it is.
__global__ __launch_bounds__(kThreads) void ctl_trip_bank_apply_kernel(CtlTrip trip, uint64_t at_units, CtlBank bank) {
  const uint32_t e = blockIdx.x * kThreads + threadIdx.x;
  if (e >= bank.n && e >= bank.n_vwaves) return;
  double v;
  if (!ctl_trip_lane_value(trip, 1u, 0u, ctl_trip_now(at_units), v)) return;
  ctl_bank_store(bank, ctl_bank_param_f64(bank.control_index, v), e);
}

// ---- FM and sampler bank targets ----------------------------------------------------------------------------------------------
// A link onto an FM bank's dca-gain, dca-pan, depth or beta, or onto a sampler (drumkit) bank's gain.  Every FM and sampler kernel — serial,
// time-parallel at one and at four voices per wavefront, the mixed one-launch form, the note-event kernels — loads its record from ONE
// place, the per-voice SoA params[word * n + voice]: there are no per-wave copies and no plan, so nothing is wave-uniform and the source
// may have one lane per voice (n_src == n: one drum, one lane) as well as one for all.  One thread per voice; the store is ctl_core.h's
// ctl_fm_store / ctl_sampler_store, the text the CPU tier holds against derive_fm.  shadow: the FM bank's [CTL_FM_WORDS][n] (nullptr on a
// sampler bank, whose gain is one word).  A between-blocks mutation ordered like the Welsh one (bank_link_apply).
struct CtlVoices {
  uint32_t* __restrict__ params;
  float* __restrict__ shadow;
  uint32_t n, control_index;
};
__device__ __forceinline__ void ctl_voices_store(const CtlVoices& b, double value, uint32_t e) {
  if (b.shadow) ctl_fm_store(b.params, b.shadow, b.n, e, b.control_index, ctl_fm_param_f64(b.control_index, value));
  else ctl_sampler_store(b.params, b.n, e, ctl_sampler_gain_f64(value));
}
// An LFO or signal source: the fp32 value01 widened, through groove_bank_set_param's law.
__global__ __launch_bounds__(kThreads) void ctl_voices_apply_kernel(uint32_t source, CtlLanes src, uint32_t n_src, uint64_t at_frame,
                                                                    const float* __restrict__ value, const uint32_t* __restrict__ captured,
                                                                    CtlVoices bank) {
  const uint32_t e = blockIdx.x * kThreads + threadIdx.x;
  if (e >= bank.n) return;
  const uint32_t s = n_src == 1u ? 0u : e;
  float v;
  if (source == GROOVE_CTL_SRC_LFO) {
    v = ctl_lfo_value01(src.waveform[s], src.delta64[s], src.duty64[s], at_frame);
  } else {
    if (*captured == 0u) return;
    v = ctl_signal_value01(src.law[s], value[s]);
  }
  ctl_voices_store(bank, (double)v, e);
}
// A trip source: the f64 value.  No step of the voice's lane at at_units: its words stay as they are.
__global__ __launch_bounds__(kThreads) void ctl_trip_voices_apply_kernel(CtlTrip trip, uint32_t n_src, uint64_t at_units, CtlVoices bank) {
  const uint32_t e = blockIdx.x * kThreads + threadIdx.x;
  if (e >= bank.n) return;
  double v;
  if (!ctl_trip_lane_value(trip, n_src, n_src == 1u ? 0u : e, ctl_trip_now(at_units), v)) return;
  ctl_voices_store(bank, v, e);
}

} // namespace groove
