// wave_probe.hip — the CROSS-LANE routines of csrc/welsh_tp.h and csrc/kernels.h, primitive by primitive (test infrastructure only; no
// part of libgroove_hip.so, and no kernel of the library runs here).  One small kernel per primitive: ONE WORKGROUP PER CASE, many cases
// a launch; every lane loads one value (or one record), calls the primitive and stores what it holds afterwards.  Workgroups have 64
// threads, or kThreads where the primitive needs the library's workgroup (FusedAcc's tile, tp_reduce_prev's "wavefront 0 only").
//
// `int wave_probe_<name>(...)` allocates, copies in, launches, synchronises, copies out, frees and returns the HIP error code (0: fine;
// -2: arguments that would index outside the buffers, checked on the host before anything is launched).
//
// The translation unit is welsh_tp.hip's: GROOVE_WELSH_CLASS_TU, kernels.h, welsh_tp.h.  wave_sum alone lives in the part of kernels.h
// that the define leaves out (the mix bus, defined once in groove_hip.hip); wave_probe_mix.hip includes this file with
// WAVE_PROBE_MIX_TU set, which builds the unit without the define and nothing but wave_sum's probe.
#include <stddef.h>
#include <stdint.h>
#if !defined(WAVE_PROBE_MIX_TU)
#define GROOVE_WELSH_CLASS_TU 1
#endif
#include "../../groove_amd/csrc/kernels.h"
#if !defined(WAVE_PROBE_MIX_TU)
#include "../../groove_amd/csrc/welsh_tp.h"
#include "../../groove_amd/csrc/fx_coef.h"
#endif

using namespace groove;

namespace {

struct DevBuf { // one device allocation of the call; freed when the call returns
  void* p = nullptr;
  ~DevBuf() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 1); }
  hipError_t upload(const void* host, size_t bytes) {
    const hipError_t e = alloc(bytes);
    return e != hipSuccess || !bytes ? e : hipMemcpy(p, host, bytes, hipMemcpyHostToDevice);
  }
  template <class T> T* as() const { return (T*)p; }
};
int fetch(const DevBuf& b, void* host, size_t bytes) { // after a launch
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  e = hipDeviceSynchronize();
  if (e != hipSuccess) return (int)e;
  return (int)hipMemcpy(host, b.p, bytes, hipMemcpyDeviceToHost);
}
#define UP(buf, host, bytes) { const hipError_t e_ = (buf).upload(host, bytes); if (e_ != hipSuccess) return (int)e_; }
#define ALLOC(buf, bytes) { const hipError_t e_ = (buf).alloc(bytes); if (e_ != hipSuccess) return (int)e_; }

#if defined(WAVE_PROBE_MIX_TU)
__global__ void __launch_bounds__(64) k_wave_sum(const float* in, float* out) {
  const size_t i = (size_t)blockIdx.x * 64u + threadIdx.x;
  out[i] = wave_sum(in[i]);
}
#else
// ---- welsh_tp.h: the DPP scans.  in / out: [cases][64] records
template <int LPV>
__global__ void __launch_bounds__(64) k_scan_add_u64(const uint64_t* in, uint64_t* out) {
  const size_t i = (size_t)blockIdx.x * 64u + threadIdx.x;
  uint64_t a = in[2 * i], b = in[2 * i + 1];
  tp_scan_add_u64<LPV>(a, b);
  out[2 * i] = a; out[2 * i + 1] = b;
}
template <int LPV>
__global__ void __launch_bounds__(64) k_scan_max_i32(const int* in, int* out) {
  const size_t i = (size_t)blockIdx.x * 64u + threadIdx.x;
  int x = in[i];
  tp_scan_max_i32<LPV>(x);
  out[i] = x;
}
// maps: 16 doubles a lane in Lp24Affine's order (c0[4], c1[4], c2[2], c3[2], z[4]); s0: the case's start state [cases][4];
// out: 20 doubles a lane, the scanned record and lp24_affine_mul(record, s0, with z) behind it
static_assert(sizeof(Lp24Affine) == 16 * sizeof(double), "a record is sixteen doubles");
template <int LPV>
__global__ void __launch_bounds__(64) k_scan_affine(const double* maps, const double* s0, double* out) {
  const size_t i = (size_t)blockIdx.x * 64u + threadIdx.x;
  Lp24Affine m;
  const double* r = maps + 16 * i;
#pragma unroll
  for (int k = 0; k < 4; ++k) { m.c0[k] = r[k]; m.c1[k] = r[4 + k]; m.z[k] = r[12 + k]; }
#pragma unroll
  for (int k = 0; k < 2; ++k) { m.c2[k] = r[8 + k]; m.c3[k] = r[10 + k]; }
  tp_scan_affine<LPV>(m);
  const double s_init[4] = {s0[4 * blockIdx.x], s0[4 * blockIdx.x + 1], s0[4 * blockIdx.x + 2], s0[4 * blockIdx.x + 3]};
  double s_end[4];
  lp24_affine_mul(m, s_init, s_end, true);
  double* o = out + 20 * i;
#pragma unroll
  for (int k = 0; k < 4; ++k) { o[k] = m.c0[k]; o[4 + k] = m.c1[k]; o[12 + k] = m.z[k]; o[16 + k] = s_end[k]; }
#pragma unroll
  for (int k = 0; k < 2; ++k) { o[8 + k] = m.c2[k]; o[10 + k] = m.c3[k]; }
}
// src = lane - d[case]
template <class T>
__global__ void __launch_bounds__(64) k_shfl(const T* in, const int* d, T* out) {
  const size_t i = (size_t)blockIdx.x * 64u + threadIdx.x;
  out[i] = tp_shfl(in[i], (int)threadIdx.x - d[blockIdx.x]);
}
// xf: [cases][64][CH] (lane l of a lane-channel holds frames CH l ..); par: twelve doubles per (case, lane-channel of the wavefront):
// frames, wet, b0, b1, b2, a1, a2, x1, x2, y1, y2, (unused); o: [cases][64][CH]; ns: five doubles a lane (holds_end, then ns[0..3],
// which keep the sentinel where holds_end is false)
constexpr double kNsSentinel = -7777.0;
template <int CH, int LPV>
__global__ void __launch_bounds__(64) k_bq_tp_wave(const float* xf_in, const double* par, float* o_out, double* ns_out) {
  const uint32_t lane = threadIdx.x, vl = lane & (uint32_t)(LPV - 1), sub = lane / (uint32_t)LPV;
  const size_t i = (size_t)blockIdx.x * 64u + lane;
  const double* q = par + ((size_t)blockIdx.x * 2 + sub) * 12;
  const uint32_t frames = (uint32_t)q[0];
  const float wm = (float)q[1];
  const BiquadCoefD c{q[2], q[3], q[4], q[5], q[6]};
  const uint32_t n0 = vl * CH;
  const uint32_t cnt = n0 < frames ? (frames - n0 < (uint32_t)CH ? frames - n0 : (uint32_t)CH) : 0u;
  float xf[CH], o[CH];
#pragma unroll
  for (uint32_t j = 0; j < (uint32_t)CH; ++j) xf[j] = j < cnt ? xf_in[i * CH + j] : 0.0f; // (as the callers hand them over)
  double ns[4] = {kNsSentinel, kNsSentinel, kNsSentinel, kNsSentinel};
  const bool holds_end = bq_tp_wave<CH, LPV>(xf, cnt, lane, frames, c, q[7], q[8], q[9], q[10], wm, o, ns);
#pragma unroll
  for (uint32_t j = 0; j < (uint32_t)CH; ++j) o_out[i * CH + j] = o[j];
  ns_out[5 * i] = holds_end ? 1.0 : 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) ns_out[5 * i + 1 + k] = ns[k];
}
// The generator's state is wave-uniform: the start states ride in the kernel's argument block, one pair a case.
constexpr uint32_t kNoiseCases = 256;
struct NoiseStarts { uint32_t x[kNoiseCases][2]; };
// out: 66 words a case: lanes 0 .. 63 of the accumulator (tick I's value in lane I), then x1, x2 after the 64 ticks
__global__ void __launch_bounds__(64) k_noise_ticks(NoiseStarts st, uint32_t* out) {
  uint32_t x1 = st.x[blockIdx.x][0], x2 = st.x[blockIdx.x][1];
  int acc = 0;
  tp_noise_ticks<64>(x1, x2, acc);
  uint32_t* o = out + (size_t)blockIdx.x * 66u;
  o[threadIdx.x] = (uint32_t)acc;
  if (threadIdx.x == 0) { o[64] = x1; o[65] = x2; }
}
// ---- kernels.h
__global__ void __launch_bounds__(64) k_wave_sum_lane63(const float* in, float* out) {
  const size_t i = (size_t)blockIdx.x * 64u + threadIdx.x;
  out[i] = wave_sum_lane63(in[i]);
}
__global__ void __launch_bounds__(64) k_wave_min_u32(const uint32_t* in, uint32_t* out) {
  const size_t i = (size_t)blockIdx.x * 64u + threadIdx.x;
  out[i] = wave_min_u32(in[i]);
}
// tile: [cases][8 frame slots][kThreads] (L, R) pairs; par: count, f0, prow, frames a case; partial: [cases][psize], prefilled by the caller
__global__ void __launch_bounds__(kThreads) k_fused_acc(const float2* tile, const uint32_t* par, float* partial, size_t psize) {
  const uint32_t count = par[4 * blockIdx.x], f0 = par[4 * blockIdx.x + 1], prow = par[4 * blockIdx.x + 2], frames = par[4 * blockIdx.x + 3];
  FusedAcc acc(prow);
  const float2* t = tile + (size_t)blockIdx.x * FusedAcc::kChunk * kThreads;
  for (uint32_t k = 0; k < count; ++k) {
    const uint32_t f = f0 + k;
    const float2 v = t[(f & (FusedAcc::kChunk - 1)) * kThreads + threadIdx.x];
    acc.add(v.x, v.y, f);
  }
  acc.flush(partial + (size_t)blockIdx.x * psize, frames, f0, count);
}
// desc: eight words a workgroup: offset of its rows, offset of its bus, n_rows, frames, accumulate, wg, n_wg, (unused)
__global__ void __launch_bounds__(kThreads) k_reduce_prev(const float* rows, float* bus, const uint32_t* desc) {
  const uint32_t* d = desc + (size_t)blockIdx.x * 8u;
  TpPrev pv;
  pv.rows = rows + d[0]; pv.bus = bus + d[1]; pv.n_rows = d[2]; pv.frames = d[3]; pv.accumulate = (int)d[4];
  tp_reduce_prev(pv, threadIdx.x, d[5], d[6]);
}
#endif

template <class T, class K>
int lanes_in_out(K kernel, const T* in, T* out, size_t cases, size_t words) {
  if (cases == 0) return 0;
  DevBuf bi, bo;
  UP(bi, in, cases * 64 * words * sizeof(T));
  ALLOC(bo, cases * 64 * words * sizeof(T));
  kernel<<<dim3((unsigned)cases), dim3(64)>>>(bi.as<const T>(), bo.as<T>());
  return fetch(bo, out, cases * 64 * words * sizeof(T));
}
#if !defined(WAVE_PROBE_MIX_TU)
template <class T>
int run_shfl(const T* in, const int* d, T* out, size_t cases) {
  if (cases == 0) return 0;
  DevBuf bi, bd, bo;
  UP(bi, in, cases * 64 * sizeof(T));
  UP(bd, d, cases * sizeof(int));
  ALLOC(bo, cases * 64 * sizeof(T));
  k_shfl<T><<<dim3((unsigned)cases), dim3(64)>>>(bi.as<const T>(), bd.as<const int>(), bo.as<T>());
  return fetch(bo, out, cases * 64 * sizeof(T));
}
#endif

} // namespace

extern "C" {
#if defined(WAVE_PROBE_MIX_TU)
int wave_probe_wave_sum(const float* in, float* out, size_t cases) { return lanes_in_out(k_wave_sum, in, out, cases, 1); }
#else
int wave_probe_scan_add_u64(int lpv, const uint64_t* in, uint64_t* out, size_t cases) {
  if (lpv == 64) return lanes_in_out(k_scan_add_u64<64>, in, out, cases, 2);
  if (lpv == 32) return lanes_in_out(k_scan_add_u64<32>, in, out, cases, 2);
  return -2;
}
int wave_probe_scan_max_i32(int lpv, const int* in, int* out, size_t cases) {
  if (lpv == 64) return lanes_in_out(k_scan_max_i32<64>, in, out, cases, 1);
  if (lpv == 32) return lanes_in_out(k_scan_max_i32<32>, in, out, cases, 1);
  return -2;
}
int wave_probe_scan_affine(int lpv, const double* maps, const double* s0, double* out, size_t cases) {
  if (lpv != 64 && lpv != 32) return -2;
  if (cases == 0) return 0;
  DevBuf bm, bs, bo;
  UP(bm, maps, cases * 64 * 16 * sizeof(double));
  UP(bs, s0, cases * 4 * sizeof(double));
  ALLOC(bo, cases * 64 * 20 * sizeof(double));
  if (lpv == 64) k_scan_affine<64><<<dim3((unsigned)cases), dim3(64)>>>(bm.as<const double>(), bs.as<const double>(), bo.as<double>());
  else k_scan_affine<32><<<dim3((unsigned)cases), dim3(64)>>>(bm.as<const double>(), bs.as<const double>(), bo.as<double>());
  return fetch(bo, out, cases * 64 * 20 * sizeof(double));
}
int wave_probe_shfl32(const uint32_t* in, const int* d, uint32_t* out, size_t cases) { return run_shfl(in, d, out, cases); }
int wave_probe_shfl64(const uint64_t* in, const int* d, uint64_t* out, size_t cases) { return run_shfl(in, d, out, cases); }
int wave_probe_bq_tp_wave(int lpv, const float* xf, const double* par, float* o, double* ns, size_t cases) {
  if (lpv != 64 && lpv != 32) return -2;
  if (cases == 0) return 0;
  const size_t ch = lpv == 64 ? 4 : 8;
  for (size_t i = 0; i < cases * 2; ++i) if (!(par[12 * i] >= 0.0 && par[12 * i] <= (double)(ch * (size_t)lpv))) return -2; // frames: up to the form's limit
  DevBuf bx, bp, bo, bn;
  UP(bx, xf, cases * 64 * ch * sizeof(float));
  UP(bp, par, cases * 2 * 12 * sizeof(double));
  ALLOC(bo, cases * 64 * ch * sizeof(float));
  ALLOC(bn, cases * 64 * 5 * sizeof(double));
  if (lpv == 64) k_bq_tp_wave<4, 64><<<dim3((unsigned)cases), dim3(64)>>>(bx.as<const float>(), bp.as<const double>(), bo.as<float>(), bn.as<double>());
  else k_bq_tp_wave<8, 32><<<dim3((unsigned)cases), dim3(64)>>>(bx.as<const float>(), bp.as<const double>(), bo.as<float>(), bn.as<double>());
  const int e = fetch(bo, o, cases * 64 * ch * sizeof(float));
  return e ? e : (int)hipMemcpy(ns, bn.p, cases * 64 * 5 * sizeof(double), hipMemcpyDeviceToHost);
}
int wave_probe_noise_ticks(const uint32_t* starts, uint32_t* out, size_t cases) {
  for (size_t c0 = 0; c0 < cases; c0 += kNoiseCases) {
    const size_t m = cases - c0 < kNoiseCases ? cases - c0 : kNoiseCases;
    NoiseStarts st = {};
    for (size_t i = 0; i < m; ++i) { st.x[i][0] = starts[2 * (c0 + i)]; st.x[i][1] = starts[2 * (c0 + i) + 1]; }
    DevBuf bo;
    ALLOC(bo, m * 66 * sizeof(uint32_t));
    k_noise_ticks<<<dim3((unsigned)m), dim3(64)>>>(st, bo.as<uint32_t>());
    const int e = fetch(bo, out + c0 * 66, m * 66 * sizeof(uint32_t));
    if (e) return e;
  }
  return 0;
}
int wave_probe_wave_sum_lane63(const float* in, float* out, size_t cases) { return lanes_in_out(k_wave_sum_lane63, in, out, cases, 1); }
int wave_probe_wave_min_u32(const uint32_t* in, uint32_t* out, size_t cases) { return lanes_in_out(k_wave_min_u32, in, out, cases, 1); }
// partial: [cases][psize] in and out
int wave_probe_fused_acc(const float* tile, const uint32_t* par, float* partial, size_t psize, size_t cases) {
  if (cases == 0) return 0;
  for (size_t i = 0; i < cases; ++i) {
    const uint64_t count = par[4 * i], f0 = par[4 * i + 1], prow = par[4 * i + 2], frames = par[4 * i + 3];
    if (count < 1 || count > FusedAcc::kChunk || (f0 & (FusedAcc::kChunk - 1)) || f0 + count > frames || (prow + 1) * 2 * frames > psize) return -2;
  }
  DevBuf bt, bp, bo;
  UP(bt, tile, cases * FusedAcc::kChunk * kThreads * 2 * sizeof(float));
  UP(bp, par, cases * 4 * sizeof(uint32_t));
  UP(bo, partial, cases * psize * sizeof(float));
  k_fused_acc<<<dim3((unsigned)cases), dim3(kThreads)>>>(bt.as<const float2>(), bp.as<const uint32_t>(), bo.as<float>(), psize);
  return fetch(bo, partial, cases * psize * sizeof(float));
}
// bus: [bus_count] in and out
int wave_probe_reduce_prev(const float* rows, size_t rows_count, float* bus, size_t bus_count, const uint32_t* desc, size_t wgs) {
  if (wgs == 0) return 0;
  for (size_t i = 0; i < wgs; ++i) {
    const uint32_t* d = desc + 8 * i;
    const uint64_t cols = 2 * (uint64_t)d[3];
    if (d[2] < 1 || d[3] < 1 || d[6] < 1 || d[5] >= d[6] || d[0] + d[2] * cols > rows_count || d[1] + cols > bus_count) return -2;
  }
  DevBuf br, bb, bd;
  UP(br, rows, rows_count * sizeof(float));
  UP(bb, bus, bus_count * sizeof(float));
  UP(bd, desc, wgs * 8 * sizeof(uint32_t));
  k_reduce_prev<<<dim3((unsigned)wgs), dim3(kThreads)>>>(br.as<const float>(), bb.as<float>(), bd.as<const uint32_t>());
  return fetch(bb, bus, bus_count * sizeof(float));
}

// ---- host side: the workgroup-to-voice-group mapping and the coefficient designs the real-coefficient cases are drawn from
uint32_t wave_probe_voices_per_workgroup(uint32_t vpw) { return (uint32_t)kTpWaves * vpw; }
uint32_t wave_probe_welsh_tp_grid(uint32_t n, uint32_t vpw) { return welsh_tp_grid(n, vpw); }
void wave_probe_groups_of_blocks(uint32_t grid, uint32_t* out) { for (uint32_t i = 0; i < grid; ++i) out[i] = tp_group_of_block(i, grid); }
int wave_probe_rbj_for_kind(uint32_t kind, double cutoff_hz, double q, double bandwidth_hz, double db_gain, double fs, double* c5) {
  return fx_rbj_for_kind(kind, cutoff_hz, q, bandwidth_hz, db_gain, fs, c5) ? 0 : -2;
}
void wave_probe_fx_lp24_coeffs(double fc, double ripple, double fs, double* out6) { fx_lp24_coeffs(fc, ripple, fs, out6); }
#endif
}
