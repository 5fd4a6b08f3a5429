// ctl_link.h — the kernels of a device-resident CONTROL LINK (include/groove_hip.h, groove_ctl_link_*).
//
// A controller's value reaches its target without the host: the capture kernel keeps the last frame of the block a signal
// passthrough has passed on, the apply kernel computes the control value (ctl_core.h) and writes it into the target's parameter
// words — the same words the effect and voice kernels read — both on the ctx stream, where stream order is the order of the
// calls.  ONE apply kernel, ctl_apply_kernel<Source, Target>: two sources (an LFO or captured signal; a trip) times four
// targets (an effect's plain words; a filter's shadow and coefficients; a Welsh bank; an FM or sampler bank's voices), each a
// small POD passed by value.  One thread per target element, kThreads per workgroup like the other per-lane kernels
// (kernels.h); a launch of either kernel is a few wavefronts and all latency.
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

// ---- sources --------------------------------------------------------------------------------------------------------------------
// Each yields the value of source lane s, or false where there is none: then the target stays as it is.
// An LFO or a captured signal: the fp32 value01.  A signal link that has captured nothing yet has no value.
struct CtlLive {
  using value_type = float;
  uint32_t source, n_src;
  CtlLanes lanes;
  uint64_t at_frame;
  const float* __restrict__ sample; // [n_src] what ctl_capture_kernel kept
  const uint32_t* __restrict__ captured;
  __device__ __forceinline__ bool value(uint32_t s, float& v) const {
    if (source == GROOVE_CTL_SRC_LFO) {
      v = ctl_lfo_value01(lanes.waveform[s], lanes.delta64[s], lanes.duty64[s], at_frame);
    } else {
      if (*captured == 0u) return false;
      v = ctl_signal_value01(lanes.law[s], sample[s]);
    }
    return true;
  }
};
// The device table of a trip link, SoA [step][source lane]: begin has n_steps + 1 rows (ctl_core.h: ctl_trip_begins, ctl_trip_layout).
struct CtlTrip {
  const double* __restrict__ begin;
  const double* __restrict__ start;
  const double* __restrict__ end;
  const double* __restrict__ beats;
  const uint32_t* __restrict__ kind;
  uint32_t n_steps;
};
// A trip: the f64 value at the musical time at_units, which may lie outside 0..1.  No step of the lane's trip holds that time: no value.
struct CtlTripAt {
  using value_type = double;
  CtlTrip trip;
  uint32_t n_src;
  uint64_t at_units;
  __device__ __forceinline__ bool value(uint32_t s, double& v) const {
    const double now = ctl_trip_now(at_units);
    const int32_t i = ctl_trip_find(trip.begin + s, n_src, trip.n_steps, now);
    if (i < 0) return false;
    const size_t at = (size_t)i * n_src + s;
    v = ctl_trip_value(trip.kind[at], trip.start[at], trip.end[at], trip.begin[at], trip.beats[at], now);
    return true;
  }
};

// ---- the apply kernel -----------------------------------------------------------------------------------------------------------
// Target element e = target law(the value of source lane e, or of the one source lane there is).  A target's store(float) takes a live
// source's value through the fp32 form of its law, store(double) a trip's through the f64 form: groove_fx_set_param's and
// groove_bank_set_param's laws in the precision each has there (ctl_core.h).
template <typename Source, typename Target>
__global__ __launch_bounds__(kThreads) void ctl_apply_kernel(Source src, Target dst) {
  const uint32_t e = blockIdx.x * kThreads + threadIdx.x;
  if (e >= dst.threads()) return;
  typename Source::value_type v;
  if (!src.value(src.n_src == 1u ? 0u : e, v)) return;
  dst.store(v, e);
}

// ---- effect targets -------------------------------------------------------------------------------------------------------------
// The per-lane parameter words the effect kernels read: exactly one of dst_f (d_fa, or d_wet for a wet link) and dst_u (d_ua) is set.
struct CtlPlain {
  float* __restrict__ dst_f;
  uint32_t* __restrict__ dst_u;
  uint32_t n;
  __host__ __device__ uint32_t threads() const { return n; }
  __device__ __forceinline__ void store(float v, uint32_t e) const {
    if (dst_u) dst_u[e] = ctl_target_bits(v);
    else dst_f[e] = ctl_target_float(v);
  }
  __device__ __forceinline__ void store(double v, uint32_t e) const {
    if (dst_u) dst_u[e] = ctl_target_bits_f64(v);
    else dst_f[e] = ctl_target_float_f64(v);
  }
};
// A filter's cutoff, q or passband-ripple (CTL_ROUTE_DERIVED): the parameter lands in the lane's word of the parameter shadow, and the
// lane's coefficients are derived from the five shadow words in f64 (fx_coef.h: the host's own text) and stored where the IIR kernels
// read them, coef[k * n + lane].  A second link onto the same effect runs behind this one on the ctx stream and loads what this one stored.
struct CtlFilter {
  uint32_t kind, control_index;
  double sr;
  float* __restrict__ shadow;
  double* __restrict__ coef;
  uint32_t n;
  __host__ __device__ uint32_t threads() const { return n; }
  __device__ __forceinline__ void store(float v, uint32_t e) const { put(ctl_derived_param(control_index, v), e); }
  __device__ __forceinline__ void store(double v, uint32_t e) const { put(ctl_derived_param_f64(control_index, v), e); }
  __device__ __forceinline__ void put(float mine, uint32_t e) const {
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
      return; // (not an IIR kind: the creates refuse it)
    }
#pragma unroll
    for (uint32_t k = 0; k < 6; ++k)
      if (k < nc) coef[(size_t)k * n + e] = c[k];
  }
};

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
// later one (groove_hip.hip link_apply: event join, fork), so no wavefront reads a record while it is written.  A write in the
// middle of a block would break the promise of welsh_wave_tables_up (kernels.h) — what a wave is at the start of a block it stays for the
// whole block: its record is in scalar registers, its tables are filled from it — and a padding wave that read a torn record is how a
// render once never finished (README.md on the stall of rounds 2-3).
// threads(): thread e serves lane e (e < n) and virtual wave e (e < n_vwaves), so a thread is idle only where e >= n && e >= n_vwaves;
// the create takes one source lane (n_src == 1), so every thread reads lane 0 and stores the same parameter `mine`.  A wave's lanes
// share a record, so the wave's words are those of its lane vbase; only the shadow word this link does NOT write is read from another
// lane's column, so the two halves need no order between them.  A padding wave (count == 0) is written like any other: its vbase is a
// valid voice of its kind and nothing reads its gains.
struct CtlBank {
  uint32_t* __restrict__ params;
  WaveDesc* __restrict__ waves;
  float* __restrict__ dca; // nullptr on a cutoff link
  uint32_t n, n_vwaves, control_index;
  __host__ __device__ uint32_t threads() const { return n > n_vwaves ? n : n_vwaves; }
  __device__ __forceinline__ void store(float v, uint32_t e) const { store((double)v, e); } // the fp32 value01 widened
  __device__ __forceinline__ void store(double v, uint32_t e) const { put(ctl_bank_param_f64(control_index, v), e); }
  __device__ __forceinline__ void put(float mine, uint32_t e) const {
    constexpr uint32_t kGl = offsetof(WelshParams, gl) / 4, kGr = offsetof(WelshParams, gr) / 4, kHz = offsetof(WelshParams, cutoff_hz) / 4;
    const size_t cols = n;
    if (control_index == GROOVE_CTL_WELSH_CUTOFF) {
      if (e < n) params[kHz * cols + e] = __float_as_uint(mine);
      if (e < n_vwaves) waves[e].p.cutoff_hz = mine;
      return;
    }
    const bool is_gain = control_index == GROOVE_CTL_WELSH_DCA_GAIN;
    const float* other = dca + (size_t)(is_gain ? CTL_DCA_PAN : CTL_DCA_GAIN) * cols;
    if (e < n) {
      dca[(size_t)(is_gain ? CTL_DCA_GAIN : CTL_DCA_PAN) * cols + e] = mine;
      float gl, gr;
      pan_gains((double)(is_gain ? mine : other[e]), (double)(is_gain ? other[e] : mine), gl, gr);
      params[kGl * cols + e] = __float_as_uint(gl);
      params[kGr * cols + e] = __float_as_uint(gr);
    }
    if (e < n_vwaves) {
      const uint32_t lane = waves[e].vbase;
      if (lane < n) {
        float gl, gr;
        pan_gains((double)(is_gain ? mine : other[lane]), (double)(is_gain ? other[lane] : mine), gl, gr);
        waves[e].p.gl = gl;
        waves[e].p.gr = gr;
      }
    }
  }
};

// ---- FM and sampler bank targets ----------------------------------------------------------------------------------------------
// A link onto an FM bank's dca-gain, dca-pan, depth or beta, or onto a sampler (drumkit) bank's gain.  Every FM and sampler kernel — serial,
// time-parallel at one and at four voices per wavefront, the mixed one-launch form, the note-event kernels — loads its record from ONE
// place, the per-voice SoA params[word * n + voice]: there are no per-wave copies and no plan, so nothing is wave-uniform and the source
// may have one lane per voice (n_src == n: one drum, one lane) as well as one for all.  One thread per voice; the store is ctl_core.h's
// ctl_fm_store / ctl_sampler_store, the text the CPU tier holds against derive_fm.  shadow: the FM bank's [CTL_FM_WORDS][n] (nullptr on a
// sampler bank, whose gain is one word).  A between-blocks mutation ordered like the Welsh one (link_apply).
struct CtlVoices {
  uint32_t* __restrict__ params;
  float* __restrict__ shadow;
  uint32_t n, control_index;
  __host__ __device__ uint32_t threads() const { return n; }
  __device__ __forceinline__ void store(float v, uint32_t e) const { store((double)v, e); } // the fp32 value01 widened
  __device__ __forceinline__ void store(double v, uint32_t e) const {
    if (shadow) ctl_fm_store(params, shadow, n, e, control_index, ctl_fm_param_f64(control_index, v));
    else ctl_sampler_store(params, n, e, ctl_sampler_gain_f64(v));
  }
};

} // namespace groove
