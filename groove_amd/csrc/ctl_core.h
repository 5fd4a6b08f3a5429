// ctl_core.h — the value laws and target laws of a CONTROL LINK (docs/DSP_SPEC.md section 13): what a controller device
// (an LFO, a signal passthrough) hands to the parameter of the effect it is linked to, once per block.
//
// Plain inline functions like dsp_core.h's: the link kernels (ctl_link.h) evaluate them one target lane per thread, the host
// layer evaluates the f64 forms for the targets that only the host can derive (a filter's coefficients), and the CPU tests
// compile this text with g++ and hold it against closed forms.
#pragma once
#include "dsp_core.h"
#include "fx_coef.h"

namespace groove {

// ------------------------------------------------------------------ LFO source
// The increment the device oscillators derive from f / SR (derive.h: lfo_inc), and a waveform's duty in phase units
// (derive.h duty_to_u64: 2^64 - 2048 at duty 1 so that the product cannot overflow).
GROOVE_HD uint64_t ctl_lfo_delta64(double frequency_hz, double sr) { return turns_to_inc(frequency_hz / sr); }
GROOVE_HD uint64_t ctl_lfo_duty64(uint32_t waveform, float duty) {
  if (waveform != GROOVE_WAVE_PULSE_WIDTH) return 0x8000000000000000ull;
  return (uint64_t)(clamp01d((double)duty) * 18446744073709549568.0);
}
// A noise generator's state after n0 ticks has no closed form; "none" and the debug waveforms are no LFO.
GROOVE_HD bool ctl_lfo_waveform_ok(uint32_t waveform) {
  switch (waveform) {
    case GROOVE_WAVE_SINE: case GROOVE_WAVE_SQUARE: case GROOVE_WAVE_PULSE_WIDTH: case GROOVE_WAVE_TRIANGLE:
    case GROOVE_WAVE_SAWTOOTH: case GROOVE_WAVE_TRIANGLE_SINE: return true;
    default: return false;
  }
}
// The oscillator's phase at the first frame of a block, n0 frames after the start: frame 0 is at phase 0 (the first-tick rule),
// every later frame has taken one increment, and the 64-bit product wraps exactly as n0 additions would.
GROOVE_HD uint64_t ctl_lfo_phase(uint64_t delta64, uint64_t n0) { return delta64 * n0; }
GROOVE_HD float ctl_lfo_value01(uint32_t waveform, uint64_t delta64, uint64_t duty64, uint64_t n0) {
  const float v = osc_value(waveform, ctl_lfo_phase(delta64, n0), duty64, 0.0f);
  return (v + 1.0f) * 0.5f;
}
// The same law in f64, for the host layer's links onto parameters whose device form the host derives.
GROOVE_HD double ctl_lfo_value01_f64(uint32_t waveform, uint64_t delta64, uint64_t duty64, uint64_t n0) {
  return (osc_value_f64(waveform, ctl_lfo_phase(delta64, n0), duty64, 0.0f) + 1.0) * 0.5;
}

// ------------------------------------------------------------------ signal source
// What a signal passthrough keeps of the block it has just passed on: the mono sample of the block's last frame.
GROOVE_HD float ctl_signal_mono(float left, float right) { return fminf(fmaxf((left + right) * 0.5f, -1.0f), 1.0f); }
GROOVE_HD bool ctl_signal_law_ok(uint32_t law) { return law <= GROOVE_CTL_LAW_AMPLITUDE_INVERTED; }
GROOVE_HD float ctl_signal_value01(uint32_t law, float m) {
  switch (law) {
    case GROOVE_CTL_LAW_AMPLITUDE: return fabsf(m);
    case GROOVE_CTL_LAW_AMPLITUDE_INVERTED: return 1.0f - fabsf(m);
    default: return (m + 1.0f) * 0.5f; // GROOVE_CTL_LAW_BIPOLAR
  }
}

// ------------------------------------------------------------------ targets
// groove_fx_set_param's laws where the device form IS the value.  The others are derived on the host in f64 (cutoff, q,
// passband-ripple -> coefficients; a FILTER link derives them on the device instead, below) or choose a kernel path there
// (wet-dry-mix -> all_wet): a plain link cannot reach them.
GROOVE_HD bool ctl_target_linkable(uint32_t control_index) {
  switch (control_index) {
    case GROOVE_CTL_FX_CEILING: case GROOVE_CTL_FX_BITS: case GROOVE_CTL_FX_ATTENUATION: case GROOVE_CTL_FX_THRESHOLD: return true;
    default: return false;
  }
}
// The parameters a FILTER link (groove_ctl_filter_link_create) reaches: the link's kernel turns the value into the parameter by
// groove_fx_set_param's law and derives the lane's coefficients on the device (fx_coef.h).  cutoff: every IIR kind; q: the kinds whose
// formula reads it; passband-ripple: the 24 dB low-pass.
GROOVE_HD bool ctl_target_derived(uint32_t kind, uint32_t control_index) {
  switch (control_index) {
    case GROOVE_CTL_FX_CUTOFF: return fx_kind_is_filter(kind);
    case GROOVE_CTL_FX_Q: return kind == GROOVE_FX_BIQUAD_LP12 || kind == GROOVE_FX_BIQUAD_HP12 || kind == GROOVE_FX_BIQUAD_AP12;
    case GROOVE_CTL_FX_PASSBAND_RIPPLE: return kind == GROOVE_FX_BIQUAD_LP24;
    default: return false;
  }
}
// A filter lane's parameter shadow on the device, [word][lane]: what deriving its coefficients reads (groove_fx: d_shadow).
enum : uint32_t { CTL_SHADOW_CUTOFF = 0, CTL_SHADOW_Q = 1, CTL_SHADOW_RIPPLE = 2, CTL_SHADOW_BANDWIDTH = 3, CTL_SHADOW_DB_GAIN = 4, CTL_SHADOW_WORDS = 5 };
GROOVE_HD uint32_t ctl_shadow_word(uint32_t control_index) {
  return control_index == GROOVE_CTL_FX_CUTOFF ? CTL_SHADOW_CUTOFF : (control_index == GROOVE_CTL_FX_Q ? CTL_SHADOW_Q : CTL_SHADOW_RIPPLE);
}
// value01 (clamped like groove_fx_set_param's) -> the float groove_fx_params would hold
GROOVE_HD float ctl_derived_param(uint32_t control_index, float value01) {
  const double v = clamp01d((double)value01);
  return control_index == GROOVE_CTL_FX_CUTOFF ? (float)fx_percent_to_frequency(v) : (float)fx_q_law(v);
}
GROOVE_HD bool ctl_target_is_uint(uint32_t control_index) { return control_index == GROOVE_CTL_FX_BITS; }
GROOVE_HD float ctl_target_float(float value01) { return value01; } // ceiling, threshold, attenuation
GROOVE_HD uint32_t ctl_target_bits(float value01) {
  const uint32_t b = (uint32_t)(value01 * 16.0f);
  return b > 31u ? 31u : b;
}

} // namespace groove
