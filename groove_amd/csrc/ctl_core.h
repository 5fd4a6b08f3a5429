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

// ------------------------------------------------------------------ trip source
// A CONTROL TRIP (the host layer's ControlTrip): start_beat plus S steps {kind, start, end, beats}.  begin[0] = start_beat and
// begin[i + 1] = begin[i] + beats[i], accumulated in f64 in the order ControlTrip::work accumulates its `b` (ctl_trip_begins: the one
// place that does it); step i holds `now` iff begin[i] <= now < begin[i + 1].  The begins never decrease, so at most one step holds a
// given `now` and a binary search finds the step the host's first-match scan finds.
GROOVE_HD double ctl_trip_now(uint64_t at_units) { return (double)at_units / (double)GROOVE_CTL_UNITS_PER_BEAT; }
// begin[0 .. n_steps] from the beats of one source lane, `stride` elements apart in both arrays
GROOVE_HD void ctl_trip_begins(double start_beat, const double* beats, size_t beats_stride, uint32_t n_steps, double* begin, size_t stride) {
  double b = start_beat;
  begin[0] = b;
  for (uint32_t i = 0; i < n_steps; ++i) {
    b += beats[(size_t)i * beats_stride];
    begin[(size_t)(i + 1) * stride] = b;
  }
}
// The step that holds `now` among begin[0 .. n_steps] (stride elements apart: the device table is [step][lane]), or -1 outside
// [begin[0], begin[n_steps]).
GROOVE_HD int32_t ctl_trip_find(const double* begin, size_t stride, uint32_t n_steps, double now) {
  if (!(now >= begin[0]) || !(now < begin[(size_t)n_steps * stride])) return -1;
  uint32_t lo = 0, hi = n_steps; // begin[lo] <= now < begin[hi]
  while (hi - lo > 1u) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (now >= begin[(size_t)mid * stride]) lo = mid; else hi = mid;
  }
  return (int32_t)lo;
}
GROOVE_HD bool ctl_trip_kind_ok(uint32_t kind) { return kind <= GROOVE_CTL_STEP_EXPONENTIAL; }
// ControlTrip::value_at in f64: t = (now - begin) / beats clamped to 0..1; flat, slope, and the two MMA curves (convex / concave
// transforms of the linear ramp) with their threshold 10^(-12/5) as the double pow(10, -12 / 5) gives.  Every product and sum is
// rounded by itself: device code is built with contraction on, and a fused start + (end - start) * t would not give the host's bits.
GROOVE_HD double ctl_trip_value(uint32_t kind, double start, double end, double begin, double beats, double now) {
  GROOVE_NO_CONTRACT
  const double kThreshold = 0.003981071705534973; // 0x1.04e74cc73ee88p-8
  double t = (now - begin) / beats;
  t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
  double c;
  switch (kind) {
    case GROOVE_CTL_STEP_SLOPE: c = t; break;
    case GROOVE_CTL_STEP_LOGARITHMIC: c = t < kThreshold ? 0.0 : 1.0 + (5.0 / 12.0) * log10(t); break;
    case GROOVE_CTL_STEP_EXPONENTIAL: c = t > 1.0 - kThreshold ? 1.0 : -(5.0 / 12.0) * log10(1.0 - t); break;
    default: return start; // GROOVE_CTL_STEP_FLAT
  }
  const double span = end - start;
  const double rise = span * c;
  return start + rise;
}

// ------------------------------------------------------------------ routes
// THE routing rule (include/groove_hip.h, groove_ctl_*_create): which parameter of which kind of target a link reaches, and as what.
//   FLOAT, UINT  the device form IS the value: the float word (ceiling, attenuation, threshold: d_fa) or the uint word (bits: d_ua) the
//                effect kernels read (groove_ctl_link_create, groove_ctl_trip_create)
//   DERIVED      cutoff, q, passband-ripple: the link's kernel turns the value into the parameter by groove_fx_set_param's law and derives
//                the lane's coefficients on the device (fx_coef.h) (groove_ctl_filter_link_create, groove_ctl_trip_create)
//   WET          wet-dry-mix: the value itself into d_wet; the one host decision that hangs on it, a reverb's form, is made from the
//                reverb's count of live wet links (groove_ctl_wet_link_create, groove_ctl_wet_trip_create)
//   BANK         a word of a bank's voice records (groove_ctl_bank_link_create, groove_ctl_bank_trip_create)
// ctl_fx_class is the class of a control index whatever the effect, ctl_fx_route the class where the kind has that parameter: the
// library's creates, the host layer's orchestrator and the CPU tests all ask these two and ctl_bank_route.
enum CtlRoute : uint32_t { CTL_ROUTE_NONE = 0, CTL_ROUTE_FLOAT, CTL_ROUTE_UINT, CTL_ROUTE_DERIVED, CTL_ROUTE_WET, CTL_ROUTE_BANK };
enum BankKind { BANK_WELSH = 0, BANK_FM = 1, BANK_SAMPLER = 2 };
GROOVE_HD CtlRoute ctl_fx_class(uint32_t control_index) {
  switch (control_index) {
    case GROOVE_CTL_FX_CEILING: case GROOVE_CTL_FX_ATTENUATION: case GROOVE_CTL_FX_THRESHOLD: return CTL_ROUTE_FLOAT;
    case GROOVE_CTL_FX_BITS: return CTL_ROUTE_UINT;
    case GROOVE_CTL_FX_CUTOFF: case GROOVE_CTL_FX_Q: case GROOVE_CTL_FX_PASSBAND_RIPPLE: return CTL_ROUTE_DERIVED;
    case GROOVE_CTL_FX_WET: return CTL_ROUTE_WET;
    default: return CTL_ROUTE_NONE;
  }
}
GROOVE_HD CtlRoute ctl_fx_route(uint32_t fx_kind, uint32_t control_index) {
  bool has = false; // does the kind's kernel read the parameter?  (the arrays are shared between kinds: groove_fx d_fa)
  switch (control_index) {
    case GROOVE_CTL_FX_CEILING: has = fx_kind == GROOVE_FX_GAIN; break;
    case GROOVE_CTL_FX_BITS: has = fx_kind == GROOVE_FX_BITCRUSHER; break;
    case GROOVE_CTL_FX_ATTENUATION: has = fx_kind == GROOVE_FX_REVERB; break;
    case GROOVE_CTL_FX_THRESHOLD: has = fx_kind == GROOVE_FX_COMPRESSOR || fx_kind == GROOVE_FX_LIMITER; break;
    case GROOVE_CTL_FX_CUTOFF: has = fx_kind_is_filter(fx_kind); break; // every IIR kind
    case GROOVE_CTL_FX_Q: has = fx_kind == GROOVE_FX_BIQUAD_LP12 || fx_kind == GROOVE_FX_BIQUAD_HP12 || fx_kind == GROOVE_FX_BIQUAD_AP12; break; // the formulas that read it
    case GROOVE_CTL_FX_PASSBAND_RIPPLE: has = fx_kind == GROOVE_FX_BIQUAD_LP24; break;
    case GROOVE_CTL_FX_WET: has = fx_kind != GROOVE_FX_MIXER; break; // a Mixer is the identity and launches nothing
    default: break;
  }
  return has ? ctl_fx_class(control_index) : CTL_ROUTE_NONE;
}
// A Welsh bank's dca-gain, dca-pan and filter-cutoff; an FM bank's dca-gain, dca-pan, depth and beta; a sampler (drumkit) bank's gain.
GROOVE_HD CtlRoute ctl_bank_route(uint32_t bank_kind, uint32_t control_index) {
  bool has = false;
  switch (bank_kind) {
    case BANK_WELSH: has = control_index >= GROOVE_CTL_WELSH_DCA_GAIN && control_index <= GROOVE_CTL_WELSH_CUTOFF; break;
    case BANK_FM: has = control_index >= GROOVE_CTL_FM_DCA_GAIN && control_index <= GROOVE_CTL_FM_BETA; break;
    case BANK_SAMPLER: has = control_index == GROOVE_CTL_SAMPLER_GAIN; break;
    default: break;
  }
  return has ? CTL_ROUTE_BANK : CTL_ROUTE_NONE;
}

// ------------------------------------------------------------------ targets
// groove_fx_set_param's laws for the routes above, in the precision they have there.  (The predicates are the routes, asked the way the
// CPU tests' shims ask.)
GROOVE_HD bool ctl_target_linkable(uint32_t control_index) {
  return ctl_fx_class(control_index) == CTL_ROUTE_FLOAT || ctl_fx_class(control_index) == CTL_ROUTE_UINT;
}
GROOVE_HD bool ctl_target_derived(uint32_t kind, uint32_t control_index) { return ctl_fx_route(kind, control_index) == CTL_ROUTE_DERIVED; }
// A filter lane's parameter shadow on the device, [word][lane]: what deriving its coefficients reads (groove_fx: d_shadow).
enum : uint32_t { CTL_SHADOW_CUTOFF = 0, CTL_SHADOW_Q = 1, CTL_SHADOW_RIPPLE = 2, CTL_SHADOW_BANDWIDTH = 3, CTL_SHADOW_DB_GAIN = 4, CTL_SHADOW_WORDS = 5 };
GROOVE_HD uint32_t ctl_shadow_word(uint32_t control_index) {
  return control_index == GROOVE_CTL_FX_CUTOFF ? CTL_SHADOW_CUTOFF : (control_index == GROOVE_CTL_FX_Q ? CTL_SHADOW_Q : CTL_SHADOW_RIPPLE);
}
// value01 (clamped like groove_fx_set_param's) -> the float groove_fx_params would hold
GROOVE_HD float ctl_derived_param_f64(uint32_t control_index, double value01) {
  const double v = clamp01d(value01);
  return control_index == GROOVE_CTL_FX_CUTOFF ? (float)fx_percent_to_frequency(v) : (float)fx_q_law(v);
}
GROOVE_HD float ctl_derived_param(uint32_t control_index, float value01) { return ctl_derived_param_f64(control_index, (double)value01); }
GROOVE_HD bool ctl_target_is_uint(uint32_t control_index) { return ctl_fx_class(control_index) == CTL_ROUTE_UINT; }
GROOVE_HD float ctl_target_float(float value01) { return value01; } // ceiling, threshold, attenuation
GROOVE_HD uint32_t ctl_target_bits(float value01) {
  const uint32_t b = (uint32_t)(value01 * 16.0f);
  return b > 31u ? 31u : b;
}
// A trip hands on an f64 value that may lie outside 0..1 (a step's start and end are any finite numbers): groove_fx_set_param's clamp,
// then its law in the precision it has there — (float)v for the float targets, (uint32_t)(v * 16.0) capped like the upload for bits —
// so that a trip on the device gives the target word the host trip gives it.
GROOVE_HD float ctl_target_float_f64(double value) { return (float)clamp01d(value); }
GROOVE_HD uint32_t ctl_target_bits_f64(double value) {
  const uint32_t b = (uint32_t)(clamp01d(value) * 16.0);
  return b > 31u ? 31u : b;
}

// ------------------------------------------------------------------ targets on a Welsh bank
// A BANK link (groove_ctl_bank_link_create / groove_ctl_bank_trip_create) reaches the three controls groove_bank_set_param has, by that
// call's own laws in the precision they have there: the float groove_welsh_params would hold.
GROOVE_HD bool ctl_bank_target_ok(uint32_t control_index) { return ctl_bank_route(BANK_WELSH, control_index) != CTL_ROUTE_NONE; }
GROOVE_HD float ctl_bank_gain_f64(double value) { return (float)clamp01d(value); }
GROOVE_HD float ctl_bank_pan_f64(double value) { // ControlValue 0..1 -> BipolarNormal
  GROOVE_NO_CONTRACT
  const double twice = clamp01d(value) * 2.0;
  return (float)(twice - 1.0);
}
GROOVE_HD float ctl_bank_cutoff_f64(double value) { return (float)fx_percent_to_frequency(clamp01d(value)); } // WelshParams::cutoff_hz
GROOVE_HD float ctl_bank_param_f64(uint32_t control_index, double value) {
  return control_index == GROOVE_CTL_WELSH_DCA_GAIN ? ctl_bank_gain_f64(value)
                                                    : (control_index == GROOVE_CTL_WELSH_DCA_PAN ? ctl_bank_pan_f64(value) : ctl_bank_cutoff_f64(value));
}
// dca gain x pan law -> the per-channel gains a voice's last multiply reads (WelshParams / FmParams: gl, gr).  derive_welsh and derive_fm
// (derive.h) call this with the floats of the public params widened; a bank link's kernel with the floats of the bank's (gain, pan)
// shadow.  Every product and sum is rounded by itself, on both sides.
GROOVE_HD void pan_gains(double gain, double pan, float& gl, float& gr) {
  GROOVE_NO_CONTRACT
  gl = (float)(gain * (1.0 - 0.25 * (pan + 1.0) * (pan + 1.0)));
  gr = (float)(gain * (1.0 - (0.5 * pan - 0.5) * (0.5 * pan - 0.5)));
}
// The bank's (gain, pan) shadow on the device, [word][lane] in internal lane order (groove_bank: d_dca).
enum : uint32_t { CTL_DCA_GAIN = 0, CTL_DCA_PAN = 1, CTL_DCA_WORDS = 2 };

// ------------------------------------------------------------------ targets on an FM or a sampler bank
// The same two creates reach an FM bank's dca-gain, dca-pan, depth and beta and a sampler (or drumkit) bank's gain, by
// groove_bank_set_param's laws for those kinds: the float groove_fm_params / groove_sampler_params would hold.  gain and pan are the
// Welsh laws above; depth is a Normal and beta a plain ParameterType set from the ControlValue as it is — (float)clamp01(v) both (spec
// decisions, docs/DSP_SPEC.md section 13); `ratio` has no law anywhere and no control.
GROOVE_HD bool ctl_fm_target_ok(uint32_t control_index) { return ctl_bank_route(BANK_FM, control_index) != CTL_ROUTE_NONE; }
GROOVE_HD bool ctl_sampler_target_ok(uint32_t control_index) { return ctl_bank_route(BANK_SAMPLER, control_index) != CTL_ROUTE_NONE; }
GROOVE_HD float ctl_fm_depth_f64(double value) { return (float)clamp01d(value); }
GROOVE_HD float ctl_fm_beta_f64(double value) { return (float)clamp01d(value); }
GROOVE_HD float ctl_sampler_gain_f64(double value) { return (float)clamp01d(value); }
GROOVE_HD float ctl_fm_param_f64(uint32_t control_index, double value) {
  switch (control_index) {
    case GROOVE_CTL_FM_DCA_GAIN: return ctl_bank_gain_f64(value);
    case GROOVE_CTL_FM_DCA_PAN: return ctl_bank_pan_f64(value);
    case GROOVE_CTL_FM_DEPTH: return ctl_fm_depth_f64(value);
    default: return ctl_fm_beta_f64(value); // GROOVE_CTL_FM_BETA
  }
}
// An FM bank's per-voice shadow on the device, [word][voice] (groove_bank: d_dca with CTL_FM_WORDS rows): the four public floats the
// derived words come from.  The shadow word of an FM control index is its distance from the first.
enum : uint32_t { CTL_FM_GAIN = 0, CTL_FM_PAN = 1, CTL_FM_DEPTH = 2, CTL_FM_BETA = 3, CTL_FM_WORDS = 4 };
GROOVE_HD uint32_t ctl_fm_shadow_word(uint32_t control_index) { return control_index - GROOVE_CTL_FM_DCA_GAIN; }
// depth x beta -> the modulation index an FM voice multiplies with (FmParams::depth_beta); derive_fm (derive.h) calls this with the
// floats of the public params, a bank link's kernel with the floats of the shadow.
GROOVE_HD double fm_depth_beta(float depth, float beta) {
  GROOVE_NO_CONTRACT
  return (double)depth * (double)beta;
}
// What an apply onto voice e of an FM bank stores: `mine` into its shadow word, the partner word read (gain with pan, depth with beta),
// and the derived words into the rows of the word-major parameter SoA params[word * n + voice] that every FM kernel loads its FmParams
// from.  depth_beta is an f64 over TWO 32-bit rows: the low word to the first, the high word to the second.
GROOVE_HD void ctl_fm_store(uint32_t* params, float* shadow, uint32_t n_voices, uint32_t e, uint32_t control_index, float mine) {
  constexpr uint32_t kGl = offsetof(FmParams, gl) / 4, kGr = offsetof(FmParams, gr) / 4, kIdx = offsetof(FmParams, depth_beta) / 4;
  const size_t n = n_voices;
  const uint32_t word = ctl_fm_shadow_word(control_index), partner = word ^ 1u;
  shadow[(size_t)word * n + e] = mine;
  const float other = shadow[(size_t)partner * n + e];
  if (word <= CTL_FM_PAN) {
    const bool is_gain = word == CTL_FM_GAIN;
    float gl, gr;
    pan_gains((double)(is_gain ? mine : other), (double)(is_gain ? other : mine), gl, gr);
    params[kGl * n + e] = __builtin_bit_cast(uint32_t, gl);
    params[kGr * n + e] = __builtin_bit_cast(uint32_t, gr);
  } else {
    const bool is_depth = word == CTL_FM_DEPTH;
    const uint64_t bits = __builtin_bit_cast(uint64_t, fm_depth_beta(is_depth ? mine : other, is_depth ? other : mine));
    params[kIdx * n + e] = (uint32_t)bits;
    params[(kIdx + 1u) * n + e] = (uint32_t)(bits >> 32);
  }
}
// ... and onto voice e of a sampler bank: its gain is one word of the record.
GROOVE_HD void ctl_sampler_store(uint32_t* params, uint32_t n_voices, uint32_t e, float mine) {
  params[(size_t)(offsetof(SamplerParams, gain) / 4) * n_voices + e] = __builtin_bit_cast(uint32_t, mine);
}

// ------------------------------------------------------------------ the two device buffers of a link's source
// Byte offsets of the sections, 64-bit words first and the uint32 tail last; `bytes` is the allocation.  The host fills a staging copy
// through these and the kernels' views (ctl_link.h: CtlLanes, CtlTrip) are carved out by them: the one statement of each layout.
// An LFO / signal link: delta64[n_src], duty64[n_src] as uint64, then waveform[n_src], law[n_src] as uint32.
struct CtlLanesLayout { size_t delta64, duty64, waveform, law, bytes; };
GROOVE_HD CtlLanesLayout ctl_lanes_layout(uint32_t n_src) {
  const size_t n = n_src;
  return {0, 8 * n, 16 * n, 20 * n, 24 * n};
}
// A trip link, SoA [step][source lane]: begin[n_steps + 1][n_src], start, end, beats [n_steps][n_src] as f64, then kind[n_steps][n_src]
// as uint32, padded to a whole 64-bit word.
struct CtlTripLayout { size_t begin, start, end, beats, kind, bytes; };
GROOVE_HD CtlTripLayout ctl_trip_layout(uint32_t n_src, uint32_t n_steps) {
  const size_t rows = (size_t)n_steps * n_src, start = 8 * (rows + n_src);
  return {0, start, start + 8 * rows, start + 16 * rows, start + 24 * rows, start + 24 * rows + 8 * ((rows + 1) / 2)};
}

} // namespace groove
