// dsp_probe.hip — the per-lane arithmetic of csrc/dsp_core.h, primitive by primitive (test infrastructure only; no part of
// libgroove_hip.so).  One element-wise kernel per primitive: lane i computes f(in0[i], in1[i], ...) into out[i] (or into the
// F::OUT words from out[i * F::OUT] on), 256 threads a block, guarded by i < n; plain loads and stores.
//
// The file is built twice (Makefile):
//   * by hipcc with the library's own flags into libdsp_probe.so: `int probe_<name>(in..., out, n)` allocates, copies in, launches,
//     synchronises, copies out, frees and returns the HIP error code — the device sides of dsp_core.h's branches;
//   * by g++ with the emulation tier's flags into libdsp_probe_host.so: `int probe_host_<name>(...)` runs the same functor over
//     the same arrays in a loop — the host sides.
// Host-only preparation (Lp24Consts from a ripple, RenderConsts from a rate) is derive.h's and dsp_core.h's own, on either side.
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include "../../groove_amd/csrc/dsp_core.h"
#include "../../groove_amd/csrc/derive.h" // host side only: derive_lp24_consts, lp24_coeffs_h

using namespace groove;

#if defined(__HIPCC__)
#define PROBE_NAME(name) probe_##name
#else
#define PROBE_NAME(name) probe_host_##name
#endif

namespace {

#if defined(__HIPCC__)
template <class F, class U, class... In>
__global__ void __launch_bounds__(256) probe_kernel(F f, size_t n, U* out, const In*... in) {
  const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (i < n) f(i, out, in...);
}
struct DevBuf { // one device allocation of the call; freed when the call returns
  void* p = nullptr;
  ~DevBuf() { if (p) (void)hipFree(p); }
};
template <class T>
hipError_t dev_in(DevBuf& b, const T* host, size_t count, const T*& dev) {
  hipError_t e = hipMalloc(&b.p, count * sizeof(T));
  if (e != hipSuccess) return e;
  dev = (const T*)b.p;
  return hipMemcpy(b.p, host, count * sizeof(T), hipMemcpyHostToDevice);
}
template <class K, class U>
int launch_and_fetch(K&& launch, U* out, size_t out_count, size_t n) {
  DevBuf o;
  hipError_t e = hipMalloc(&o.p, out_count * sizeof(U));
  if (e != hipSuccess) return (int)e;
  launch((U*)o.p, dim3((unsigned)((n + 255) / 256)), dim3(256));
  e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  e = hipDeviceSynchronize();
  if (e != hipSuccess) return (int)e;
  return (int)hipMemcpy(out, o.p, out_count * sizeof(U), hipMemcpyDeviceToHost);
}
#endif

// F: a functor `void operator()(size_t i, U* out, const In*... in) const` reading F::IN[k] words of input k and writing F::OUT words
// of lane i.  n lanes.
template <class F, class U, class... In>
int run(size_t n, U* out, const In*... in) {
  if (n == 0) return 0;
#if defined(__HIPCC__)
  constexpr size_t K = sizeof...(In);
  DevBuf bufs[K ? K : 1];
  size_t k = 0;
  hipError_t e = hipSuccess;
  auto up = [&](auto*& p) { // p: the host pointer, replaced by its device copy
    if (e == hipSuccess) e = dev_in(bufs[k], p, n * (size_t)F::IN[k], p);
    ++k;
  };
  (up(in), ...);
  if (e != hipSuccess) return (int)e;
  return launch_and_fetch([&](U* dout, dim3 grid, dim3 block) { probe_kernel<F, U, In...><<<grid, block>>>(F{}, n, dout, in...); }, out,
                          n * (size_t)F::OUT, n);
#else
  for (size_t i = 0; i < n; ++i) F{}(i, out, in...);
  return 0;
#endif
}

// ---- functors -------------------------------------------------------------------------------------------------------------------
#define PROBE_IO(nout, ...) static constexpr int OUT = nout; static constexpr int IN[] = {__VA_ARGS__}

#define UNARY(name, TI, TO, expr)                                                                 \
  struct F_##name { PROBE_IO(1, 1); GROOVE_HD void operator()(size_t i, TO* out, const TI* in) const { const TI x = in[i]; out[i] = (expr); } };

UNARY(fast_exp2, float, float, fast_exp2(x))
UNARY(fast_rcp, float, float, fast_rcp(x))
UNARY(f64_to_u64, double, uint64_t, f64_to_u64(x))
UNARY(fract_f64, double, double, fract_f64(x))
UNARY(turns_to_inc, double, uint64_t, turns_to_inc(x))
UNARY(turns_to_phase, double, uint64_t, turns_to_phase(x))
UNARY(fold_quarter, int32_t, int32_t, fold_quarter(x))
UNARY(fold_quarter64, int64_t, int64_t, fold_quarter64(x))
UNARY(env_frames, float, uint32_t, env_frames(x))
UNARY(sin_turns_folded, float, float, sin_turns_folded(x))
UNARY(sin_turns_folded_f64, double, double, sin_turns_folded_f64(x))
UNARY(exp2_small_f64, double, double, exp2_small_f64(x))
UNARY(exp_tiny_f64, double, double, exp_tiny_f64(x))
UNARY(tan_of_reduced, float, float, tan_of_reduced(x))

struct F_tan_reduced { // out: t, hi (1.0f / 0.0f)
  PROBE_IO(2, 1);
  GROOVE_HD void operator()(size_t i, float* out, const float* x) const {
    bool hi;
    out[2 * i] = tan_reduced(x[i], hi);
    out[2 * i + 1] = hi ? 1.0f : 0.0f;
  }
};
struct F_med3f {
  PROBE_IO(1, 1, 1, 1);
  GROOVE_HD void operator()(size_t i, float* out, const float* x, const float* lo, const float* hi) const { out[i] = med3f(x[i], lo[i], hi[i]); }
};
struct F_osc_value {
  PROBE_IO(1, 1, 1, 1);
  GROOVE_HD void operator()(size_t i, float* out, const uint32_t* wave, const uint64_t* phase, const uint64_t* duty) const {
    out[i] = osc_value(wave[i], phase[i], duty[i], 0.0f);
  }
};
struct F_osc_value_f64 {
  PROBE_IO(1, 1, 1, 1);
  GROOVE_HD void operator()(size_t i, double* out, const uint32_t* wave, const uint64_t* phase, const uint64_t* duty) const {
    out[i] = osc_value_f64(wave[i], phase[i], duty[i], 0.0f);
  }
};
struct F_noise_tick { // ticks[i] ticks from osc_reset (at most 4096 are run): the last tick's value (its bits), then x1 and x2
  PROBE_IO(3, 1);
  GROOVE_HD void operator()(size_t i, uint32_t* out, const uint32_t* ticks) const {
    OscState s;
    osc_reset(s);
    float v = 0.0f;
    const uint32_t count = ticks[i] < 4096u ? ticks[i] : 4096u;
    for (uint32_t k = 0; k < count; ++k) v = noise_tick(s);
    uint32_t bits;
    memcpy(&bits, &v, 4);
    out[3 * i] = bits; out[3 * i + 1] = s.x1; out[3 * i + 2] = s.x2;
  }
};
struct F_env_shape { // the value of frame n of a stage from A over D with 1 / len = inv_len: env_shape_consts, then env_shape (env_advance)
  PROBE_IO(1, 1, 1, 1, 1);
  GROOVE_HD void operator()(size_t i, float* out, const float* n, const float* A, const float* D, const float* inv_len) const {
    float c1, c2;
    env_shape_consts(D[i], inv_len[i], c1, c2);
    out[i] = env_shape(n[i], A[i], c1, c2);
  }
};
struct F_bitcrush {
  PROBE_IO(1, 1, 1);
  GROOVE_HD void operator()(size_t i, float* out, const float* x, const uint32_t* bits) const { out[i] = bitcrush(x[i], bits[i] & 31u); }
};
template <int MODE>
struct F_sample_interp { // taps: 4 words a lane, of which the mode reads its first N
  PROBE_IO(1, 4, 1);
  GROOVE_HD void operator()(size_t i, float* out, const float* taps, const float* t) const {
    float q[SampleTaps<MODE>::N];
    for (int k = 0; k < SampleTaps<MODE>::N; ++k) q[k] = taps[4 * i + k];
    out[i] = sample_interp<MODE>(q, t[i]);
  }
};
struct F_welsh_env_cutoff_pct {
  PROBE_IO(1, 1, 1, 1);
  GROOVE_HD void operator()(size_t i, float* out, const float* start, const float* end, const float* env) const {
    WelshParams p{};
    p.cutoff_start = start[i]; p.cutoff_end = end[i];
    out[i] = welsh_env_cutoff_pct(p, env[i]);
  }
};
struct F_welsh_lfo_cutoff_pct {
  PROBE_IO(1, 1, 1, 1);
  GROOVE_HD void operator()(size_t i, float* out, const float* start, const float* depth, const float* lfo) const {
    WelshParams p{};
    p.cutoff_start = start[i]; p.lfo_depth = depth[i];
    out[i] = welsh_lfo_cutoff_pct(p, lfo[i]);
  }
};

// The coefficient paths.  consts: c0, d1, c2, d3 of the lane (derive_lp24_consts on the host); rate: pi / SR and 0.49 SR as floats.
GROOVE_HD Lp24Consts consts_of(const float* consts, size_t i) { return Lp24Consts{consts[4 * i], consts[4 * i + 1], consts[4 * i + 2], consts[4 * i + 3]}; }
struct F_lp24_coefd_from_fc {
  PROBE_IO(6, 4, 1, 2);
  GROOVE_HD void operator()(size_t i, double* out, const float* consts, const float* fc, const float* rate) const {
    const Lp24CoefD d = lp24_coefd_from_fc(consts_of(consts, i), fc[i], rate[2 * i], rate[2 * i + 1]);
    double* o = out + 6 * i;
    o[0] = d.b0a; o[1] = d.a1a; o[2] = d.a2a; o[3] = d.b0b; o[4] = d.a1b; o[5] = d.a2b;
  }
};
struct F_lp24_coeff_from_fc { // lp24_t_from_fc, then lp24_coeff_from_t
  PROBE_IO(6, 4, 1, 2);
  GROOVE_HD void operator()(size_t i, float* out, const float* consts, const float* fc, const float* rate) const {
    const Lp24CoefF d = lp24_coeff_from_fc(consts_of(consts, i), fc[i], rate[2 * i], rate[2 * i + 1]);
    float* o = out + 6 * i;
    o[0] = d.b0a; o[1] = d.a1a; o[2] = d.a2a; o[3] = d.b0b; o[4] = d.a1b; o[5] = d.a2b;
  }
};
struct F_lp24_coefd_from_pct { // `wide` as derive_welsh sets it: c0 < 1 / 512
  PROBE_IO(6, 4, 1, 1);
  GROOVE_HD void operator()(size_t i, double* out, const float* consts, const float* pct, const RenderConsts* rc) const {
    const Lp24Consts c = consts_of(consts, i);
    const Lp24CoefD d = lp24_coefd_from_pct(c, pct[i], rc[i], c.c0 < 1.0f / 512.0f);
    double* o = out + 6 * i;
    o[0] = d.b0a; o[1] = d.a1a; o[2] = d.a2a; o[3] = d.b0b; o[4] = d.a1b; o[5] = d.a2b;
  }
};

// The recurrences: STEPS consecutive steps a lane.  coef: 6 words, state: 4 words, x: STEPS words a lane; out: STEPS records of
// (y, s0, s1, s2, s3) after the step.
constexpr int STEPS = 64;
struct F_lp24_step {
  PROBE_IO(5 * STEPS, 6, 4, STEPS);
  GROOVE_HD void operator()(size_t i, double* out, const double* coef, const double* state, const double* x) const {
    const double* k = coef + 6 * i;
    const Lp24CoefD c{k[0], k[1], k[2], k[3], k[4], k[5]};
    Lp24StateD s{state[4 * i], state[4 * i + 1], state[4 * i + 2], state[4 * i + 3]};
    for (int f = 0; f < STEPS; ++f) {
      double* o = out + ((size_t)STEPS * i + f) * 5;
      o[0] = lp24_step<false>(s, c, x[(size_t)STEPS * i + f]);
      o[1] = s.s0; o[2] = s.s1; o[3] = s.s2; o[4] = s.s3;
    }
  }
};
struct F_lp24_step_f32 {
  PROBE_IO(5 * STEPS, 6, 4, STEPS);
  GROOVE_HD void operator()(size_t i, float* out, const float* coef, const float* state, const float* x) const {
    const float* k = coef + 6 * i;
    const Lp24CoefF c{k[0], k[1], k[2], k[3], k[4], k[5]};
    Lp24StateF s{state[4 * i], state[4 * i + 1], state[4 * i + 2], state[4 * i + 3]};
    for (int f = 0; f < STEPS; ++f) {
      float* o = out + ((size_t)STEPS * i + f) * 5;
      o[0] = lp24_step_f32<false>(s, c, x[(size_t)STEPS * i + f]);
      o[1] = s.s0; o[2] = s.s1; o[3] = s.s2; o[4] = s.s3;
    }
  }
};
// ... and their SCALAR_COEF forms: ONE coefficient set a launch, as kernel arguments (wave-uniform), lanes differing in state and input.
// (On the host there is no such form: the same C body.)
template <class T> struct Coef6 { T v[6]; };
template <class T, class C, class S>
GROOVE_HD void scalar_steps_lane(size_t i, T* out, const Coef6<T>& k, const T* state, const T* x) {
  const C c{k.v[0], k.v[1], k.v[2], k.v[3], k.v[4], k.v[5]};
  S s{state[4 * i], state[4 * i + 1], state[4 * i + 2], state[4 * i + 3]};
  for (int f = 0; f < STEPS; ++f) {
    T* o = out + ((size_t)STEPS * i + f) * 5;
    if constexpr (sizeof(T) == 8) o[0] = lp24_step<true>(s, c, x[(size_t)STEPS * i + f]);
    else o[0] = lp24_step_f32<true>(s, c, x[(size_t)STEPS * i + f]);
    o[1] = s.s0; o[2] = s.s1; o[3] = s.s2; o[4] = s.s3;
  }
}
#if defined(__HIPCC__)
template <class T, class C, class S>
__global__ void __launch_bounds__(256) probe_scalar_steps_kernel(Coef6<T> k, size_t n, T* out, const T* state, const T* x) {
  const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (i < n) scalar_steps_lane<T, C, S>(i, out, k, state, x);
}
#endif
template <class T, class C, class S>
int run_scalar_steps(const T* coef6, const T* state, const T* x, T* out, size_t n) {
  if (n == 0) return 0;
  Coef6<T> k;
  for (int j = 0; j < 6; ++j) k.v[j] = coef6[j];
#if defined(__HIPCC__)
  DevBuf bs, bx;
  hipError_t e = dev_in(bs, state, n * 4, state);
  if (e == hipSuccess) e = dev_in(bx, x, n * (size_t)STEPS, x);
  if (e != hipSuccess) return (int)e;
  return launch_and_fetch([&](T* dout, dim3 grid, dim3 block) { probe_scalar_steps_kernel<T, C, S><<<grid, block>>>(k, n, dout, state, x); }, out,
                          n * (size_t)STEPS * 5, n);
#else
  for (size_t i = 0; i < n; ++i) scalar_steps_lane<T, C, S>(i, out, k, state, x);
  return 0;
#endif
}

// host preparation of the coefficient probes
void consts_and_rate(const double* ripple, const float* sr, size_t n, float* consts, float* rate, RenderConsts* rc) {
  for (size_t i = 0; i < n; ++i) {
    const Lp24Consts c = derive_lp24_consts(ripple[i]);
    consts[4 * i] = c.c0; consts[4 * i + 1] = c.d1; consts[4 * i + 2] = c.c2; consts[4 * i + 3] = c.d3;
    if (rate) { rate[2 * i] = (float)(3.14159265358979323846 / (double)sr[i]); rate[2 * i + 1] = (float)(0.49 * (double)sr[i]); }
    if (rc) rc[i] = render_consts((double)sr[i]);
  }
}
template <class T> struct HostArray { // (malloc, checked by the caller: no exception crosses the C boundary)
  T* p;
  explicit HostArray(size_t count) : p((T*)malloc((count ? count : 1) * sizeof(T))) {}
  ~HostArray() { free(p); }
};

} // namespace

#define ENTRY1(name, TI, TO) \
  extern "C" int PROBE_NAME(name)(const TI* in, TO* out, size_t n) { return run<F_##name>(n, out, in); }
#define ENTRY3(name, T0, T1, T2, TO) \
  extern "C" int PROBE_NAME(name)(const T0* a, const T1* b, const T2* c, TO* out, size_t n) { return run<F_##name>(n, out, a, b, c); }

ENTRY1(fast_exp2, float, float)
ENTRY1(fast_rcp, float, float)
ENTRY1(f64_to_u64, double, uint64_t)
ENTRY1(fract_f64, double, double)
ENTRY1(turns_to_inc, double, uint64_t)
ENTRY1(turns_to_phase, double, uint64_t)
ENTRY1(fold_quarter, int32_t, int32_t)
ENTRY1(fold_quarter64, int64_t, int64_t)
ENTRY1(env_frames, float, uint32_t)
ENTRY1(sin_turns_folded, float, float)
ENTRY1(sin_turns_folded_f64, double, double)
ENTRY1(exp2_small_f64, double, double)
ENTRY1(exp_tiny_f64, double, double)
ENTRY1(tan_of_reduced, float, float)
ENTRY1(tan_reduced, float, float)            // out: 2 words a lane
ENTRY1(noise_tick, uint32_t, uint32_t)       // out: 3 words a lane
ENTRY3(med3f, float, float, float, float)
ENTRY3(osc_value, uint32_t, uint64_t, uint64_t, float)
ENTRY3(osc_value_f64, uint32_t, uint64_t, uint64_t, double)
ENTRY3(welsh_env_cutoff_pct, float, float, float, float)
ENTRY3(welsh_lfo_cutoff_pct, float, float, float, float)
ENTRY3(lp24_step, double, double, double, double)       // coef 6, state 4, x 64 words a lane; out 320
ENTRY3(lp24_step_f32, float, float, float, float)

extern "C" {
int PROBE_NAME(env_shape)(const float* frame, const float* A, const float* D, const float* inv_len, float* out, size_t n) {
  return run<F_env_shape>(n, out, frame, A, D, inv_len);
}
int PROBE_NAME(bitcrush)(const float* x, const uint32_t* bits, float* out, size_t n) { return run<F_bitcrush>(n, out, x, bits); }
int PROBE_NAME(sample_interp_nearest)(const float* taps, const float* t, float* out, size_t n) { return run<F_sample_interp<GROOVE_SAMPLE_NEAREST>>(n, out, taps, t); }
int PROBE_NAME(sample_interp_linear)(const float* taps, const float* t, float* out, size_t n) { return run<F_sample_interp<GROOVE_SAMPLE_LINEAR>>(n, out, taps, t); }
int PROBE_NAME(sample_interp_cubic)(const float* taps, const float* t, float* out, size_t n) { return run<F_sample_interp<GROOVE_SAMPLE_CUBIC>>(n, out, taps, t); }
int PROBE_NAME(lp24_step_scalar)(const double* coef6, const double* state, const double* x, double* out, size_t n) {
  return run_scalar_steps<double, Lp24CoefD, Lp24StateD>(coef6, state, x, out, n);
}
int PROBE_NAME(lp24_step_f32_scalar)(const float* coef6, const float* state, const float* x, float* out, size_t n) {
  return run_scalar_steps<float, Lp24CoefF, Lp24StateF>(coef6, state, x, out, n);
}
// ripple (f64), cutoff in Hz, rate in Hz a lane -> 6 coefficients a lane (b0, a1, a2 of section a, then of section b)
int PROBE_NAME(lp24_coefd_from_fc)(const double* ripple, const float* fc, const float* sr, double* out, size_t n) {
  HostArray<float> consts(4 * n), rate(2 * n);
  if (!consts.p || !rate.p) return -1;
  consts_and_rate(ripple, sr, n, consts.p, rate.p, nullptr);
  return run<F_lp24_coefd_from_fc>(n, out, (const float*)consts.p, fc, (const float*)rate.p);
}
int PROBE_NAME(lp24_coeff_from_fc)(const double* ripple, const float* fc, const float* sr, float* out, size_t n) {
  HostArray<float> consts(4 * n), rate(2 * n);
  if (!consts.p || !rate.p) return -1;
  consts_and_rate(ripple, sr, n, consts.p, rate.p, nullptr);
  return run<F_lp24_coeff_from_fc>(n, out, (const float*)consts.p, fc, (const float*)rate.p);
}
int PROBE_NAME(lp24_coefd_from_pct)(const double* ripple, const float* pct, const float* sr, double* out, size_t n) {
  HostArray<float> consts(4 * n);
  HostArray<RenderConsts> rc(n);
  if (!consts.p || !rc.p) return -1;
  consts_and_rate(ripple, sr, n, consts.p, nullptr, rc.p);
  return run<F_lp24_coefd_from_pct>(n, out, (const float*)consts.p, pct, (const RenderConsts*)rc.p);
}
#if !defined(__HIPCC__)
// the reference of the coefficient paths: derive.h's lp24_coeffs_h, f64 throughout
int probe_ref_lp24_coeffs_h(const double* ripple, const double* fc, const double* sr, double* out, size_t n) {
  for (size_t i = 0; i < n; ++i) lp24_coeffs_h(fc[i], ripple[i], sr[i], out + 6 * i);
  return 0;
}
#endif
}
