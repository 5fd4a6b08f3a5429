// welsh_plan.h — how a Welsh bank's voices are laid out for the wave-uniform kernels (kernels.h, "Workgroup KINDS"):
// the lane order, the virtual waves, the workgroups and the lists the launches walk.  Host arithmetic only — no device call, no
// bank, no context — so the plan of any bank can be made and looked at without a GPU (tests/test_welsh_plan_cpu.py);
// groove_hip.hip welsh_upload_params derives the records, makes the plan and uploads its arrays as they stand.
//
//   derived records (caller's order) --welsh_patch_major_order--> perm (or none) --welsh_plan--> WelshPlan
#pragma once
#include "derive.h"
#include <algorithm>
#include <cstring>
#include <utility>
#include <vector>

namespace groove {

// A virtual wave: a run of at most 64 consecutive voices (internal lane order) with identical parameter records; one wavefront
// renders it with its parameters in scalar registers.  count 0: a padding wave (no lane active; vbase a valid voice).
struct WaveDesc {
  WelshParams p;
  uint32_t vbase, count;
};
constexpr int kPlanWaves = 4;                                          // virtual waves per workgroup (== kernels.h kWaves)
constexpr int kBaseKinds = 6;                                          // LFO mode x retune
constexpr int kClassCombos = LFO_CLASSES * OSC_CLASSES * OSC_CLASSES;  // (LFO class, oscillator 1 class, oscillator 2 class)
constexpr int kWgKinds = kBaseKinds * kClassCombos;                    // sort key of the workgroup list
GROOVE_HD constexpr int wg_base_kind_of(int lfo_mode, bool retune) {
  // cost order (cheap to expensive): F32 static, F32 retune, SMOOTH static, SMOOTH retune, F64 static, F64 retune
  return (lfo_mode == LFO_F32 ? 0 : (lfo_mode == LFO_F64_SMOOTH ? 2 : 4)) + (retune ? 1 : 0);
}
GROOVE_HD constexpr int wg_class_combo(int cl, int c1, int c2) { return (cl * OSC_CLASSES + c1) * OSC_CLASSES + c2; }
GROOVE_HD constexpr int wg_kind_of(int base_kind, int cl, int c1, int c2) { return base_kind * kClassCombos + wg_class_combo(cl, c1, c2); }

// THE virtual-wave cut: maximal runs of equal records in the lane order at(0), at(1), ..., cut at 64; emit(first lane, count).
template <class At, class Emit>
void for_each_virtual_wave(const std::vector<WelshParams>& P, uint32_t n, At&& at, Emit&& emit) {
  for (uint32_t i = 0; i < n;) {
    uint32_t e = i + 1;
    while (e < n && e - i < 64 && std::memcmp(&P[at(e)], &P[at(i)], sizeof(WelshParams)) == 0) ++e;
    emit(i, e - i);
    i = e;
  }
}
template <class At>
size_t count_virtual_waves(const std::vector<WelshParams>& P, uint32_t n, At&& at) {
  size_t waves = 0;
  for_each_virtual_wave(P, n, at, [&](uint32_t, uint32_t) { ++waves; });
  return waves;
}
inline bool runs_are_long(size_t virtual_waves, uint32_t n) {
  // Use the scalar-parameter kernels when the runs are long (at most 1.5x as many virtual waves as
  // physical ones), or when the bank is so small that even one short run per wave leaves the machine
  // (1,024 SIMDs) under-filled: there a partly filled fast wave beats a full slow one.
  const uint32_t phys_waves = (n + 63) / 64;
  return !(virtual_waves > (size_t)phys_waves + phys_waves / 2 + 8 && virtual_waves > 2048);
}

// The pieces of a wave-uniform bank: the per-base-kind slices of its kind-sorted workgroup list (the four class-specialised
// base kinds first, n_spec workgroups in all, then the two exact-f64 ones).
struct KindSlices { uint32_t count[kBaseKinds] = {}, offset[kBaseKinds] = {}, n_spec = 0; };
inline KindSlices kind_slices(const uint32_t (&wgs_of_kind)[kWgKinds]) {
  KindSlices p;
  for (uint32_t base = 0, at = 0; base < (uint32_t)kBaseKinds; ++base) {
    p.offset[base] = at;
    for (int c = 0; c < kClassCombos; ++c) p.count[base] += wgs_of_kind[base * kClassCombos + c];
    at += p.count[base];
  }
  p.n_spec = p.offset[4];
  return p;
}

// What the launches of a bank read of its plan, block after block (a bank keeps this part; the arrays of WelshPlan are uploaded).
struct WelshLayout {
  // Lane permutation.  A bank whose patches are interleaved voice by voice is kept patch-major inside the library (params, state,
  // cold values in INTERNAL lane order) so that it runs on the wave-uniform kernels; perm[internal lane] = caller's voice index,
  // inv = its inverse.  Empty = identity.
  std::vector<uint32_t> perm, inv;
  bool tp_pairs = false;      // every pair of adjacent voices (2i, 2i + 1) shares a record (welsh_tp_kernel<.., VPW = 2>)
  bool tp_full_coef = false;  // some voice routes the LFO to the resonance (welsh_tp_kernel<.., FULL_COEF>)
  uint32_t n_vwaves = 0;      // waves of the plan, padding included; 0: the bank runs on the per-lane kernel
  uint32_t wgs_of_kind[kWgKinds] = {};  // slice lengths of the sorted list, in kind order
  // The MIX kernel's three sections (kernels.h): entries [mix_off[s], + mix_cnt[s]) of the striped lists — the class-specialised
  // workgroups of the sorted list taken with a stride of three, each section kind-sorted itself.  All 0 on the per-lane kernel.
  uint32_t mix_off[3] = {}, mix_cnt[3] = {};
};
// Workgroup ids (a workgroup = kPlanWaves consecutive waves) and, entry by entry, the workgroup's class combination, base kind and
// whether its patches carry WF_FILTER_F32.
struct WgLists {
  std::vector<uint32_t> list;
  std::vector<uint8_t> cls, base, f32;
};
struct WelshPlan : WelshLayout {
  std::vector<WelshParams> records;  // internal lane order
  std::vector<double> cold;          // [4][n]: tune1, tune2, fixed1, fixed2, internal lane order
  std::vector<WaveDesc> waves;       // ordered by kind, every kind padded to whole workgroups; empty on the per-lane kernel
  WgLists sorted;                    // every workgroup, by (kind, fp32 flag)
  WgLists striped;                   // the first n_spec entries of `sorted`, section by section (mix_off / mix_cnt)
};

// The order decision of a bank whose state is (being) reset: the patch-major permutation (perm[internal lane] = caller's voice:
// a stable sort by a hash of the record) when the caller's order has short runs and that one has long ones; empty: keep the caller's.
inline std::vector<uint32_t> welsh_patch_major_order(const std::vector<WelshParams>& ext) {
  const uint32_t n = (uint32_t)ext.size();
  if (runs_are_long(count_virtual_waves(ext, n, [](uint32_t i) { return i; }), n)) return {};
  std::vector<uint64_t> h(n);
  for (uint32_t v = 0; v < n; ++v) { // FNV-1a
    uint64_t x = 1469598103934665603ull;
    const unsigned char* bytes = reinterpret_cast<const unsigned char*>(&ext[v]);
    for (size_t k = 0; k < sizeof(WelshParams); ++k) { x ^= bytes[k]; x *= 1099511628211ull; }
    h[v] = x;
  }
  std::vector<uint32_t> order(n);
  for (uint32_t v = 0; v < n; ++v) order[v] = v;
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t c) { return h[a] < h[c]; });
  if (!runs_are_long(count_virtual_waves(ext, n, [&](uint32_t i) { return order[i]; }), n)) order.clear(); // every voice its own patch
  return order;
}

// Which derived records carry WF_FILTER_F32.  The flag is a MEASURED property of the static cutoff (derive.h welsh_filter_f32_ok), and a
// device link onto the bank's cutoff (groove_ctl_bank_link_create, GROOVE_CTL_WELSH_CUTOFF) moves that cutoff where the host cannot
// measure: while the bank has `cutoff_links` > 0 of them no record carries the flag — the f64 recurrence is always safe.  Otherwise a
// record carries it iff measured(record) says so (the bank's memo of welsh_filter_f32_ok).  `enabled`: the context's f32_filter knob.
template <class Measured>
void welsh_flag_filter_f32(std::vector<WelshParams>& ext, bool enabled, uint32_t cutoff_links, Measured&& measured) {
  if (!enabled || cutoff_links) return; // (derive_welsh never sets the flag)
  for (WelshParams& o : ext)
    if (measured(o)) o.flags |= WF_FILTER_F32;
}

// The plan of a bank: `ext` / `cold_ext` are the derived records (WF_FILTER_F32 already decided) and cold values in the caller's
// order, `perm` the lane order to keep them in (empty: the caller's).
inline WelshPlan welsh_plan(const std::vector<WelshParams>& ext, const std::vector<WelshCold>& cold_ext, std::vector<uint32_t> perm) {
  WelshPlan plan;
  const uint32_t n = (uint32_t)ext.size();
  plan.perm = std::move(perm);
  if (!plan.perm.empty()) {
    plan.inv.resize(n);
    for (uint32_t i = 0; i < n; ++i) plan.inv[plan.perm[i]] = i;
  }
  // everything below is in INTERNAL lane order
  std::vector<WelshParams>& P = plan.records;
  P.resize(n);
  plan.cold.resize((size_t)4 * n);
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t v = plan.perm.empty() ? i : plan.perm[i];
    P[i] = ext[v];
    const WelshCold& c = cold_ext[v];
    plan.cold[i] = c.tune1; plan.cold[(size_t)n + i] = c.tune2; plan.cold[(size_t)2 * n + i] = c.fixed1; plan.cold[(size_t)3 * n + i] = c.fixed2;
  }
  plan.tp_pairs = true; // time-parallel form, two voices per wavefront: voices 2i and 2i + 1 share their parameter words
  for (uint32_t i = 0; i + 1 < n && plan.tp_pairs; i += 2) plan.tp_pairs = std::memcmp(&P[i], &P[i + 1], sizeof(WelshParams)) == 0;
  plan.tp_full_coef = false; // time-parallel form: a voice with the resonance routing keeps six f64 coefficients per frame (welsh_tp.h)
  for (uint32_t i = 0; i < n; ++i) if (P[i].flags & WF_LFO_RESO) { plan.tp_full_coef = true; break; } // (WF_COEF_WIDE patches: from the tangent like the rest, round 6)
  std::vector<WaveDesc> W;
  W.reserve((size_t)n / 64 + 64);
  for_each_virtual_wave(P, n, [](uint32_t i) { return i; }, [&](uint32_t v, uint32_t count) {
    WaveDesc d;
    d.p = P[v]; d.vbase = v; d.count = count;
    W.push_back(d);
  });
  // Otherwise (every voice its own patch, even patch-major) the per-lane kernel serves the whole bank.
  if (!runs_are_long(W.size(), n)) return plan;
  // A workgroup runs in ONE instantiation (kernels.h, "Workgroup KINDS"), so it is built from waves that
  // ask for the same one: the waves are ordered by the kind they need and every kind's last workgroup is
  // filled up with empty waves (count 0).  (Cutting the run order into fours made every workgroup of a
  // small many-patch bank a mixture, which runs in the most demanding base kind with the run-time
  // waveform switches: config #2's 32 waves took 0.21 ms per block where their slowest patch needs 0.16.)
  auto kind_of_wave = [](const WelshParams& p) -> uint16_t {
    const int base = welsh_base_kind(p); // == wg_base_kind_of(welsh_lfo_mode(p), welsh_retunes(p)); dsp_core.h
    int cl, c1, c2;
    welsh_body_classes(p, base, cl, c1, c2);
    return (uint16_t)wg_kind_of(base, cl, c1, c2);
  };
  std::vector<uint16_t> kind; // per workgroup
  std::vector<uint8_t> f32_of; // per workgroup: its waves' patches carry WF_FILTER_F32 (a workgroup is uniform in it too: sort key bit 0)
  {
    std::vector<uint32_t> wave_kind(W.size()); // (kind << 1) | fp32-filter flag
    std::vector<uint32_t> order(W.size());
    for (uint32_t w = 0; w < W.size(); ++w) { wave_kind[w] = ((uint32_t)kind_of_wave(W[w].p) << 1) | ((W[w].p.flags & WF_FILTER_F32) ? 1u : 0u); order[w] = w; }
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t c) { return wave_kind[a] < wave_kind[c]; });
    std::vector<WaveDesc>& packed = plan.waves;
    packed.reserve(W.size() + (size_t)kPlanWaves * 64);
    for (size_t i = 0; i < order.size();) {
      size_t e = i;
      while (e < order.size() && wave_kind[order[e]] == wave_kind[order[i]]) ++e;
      for (size_t j = i; j < e; ++j) {
        if ((j - i) % kPlanWaves == 0) { kind.push_back((uint16_t)(wave_kind[order[i]] >> 1)); f32_of.push_back((uint8_t)(wave_kind[order[i]] & 1u)); }
        packed.push_back(W[order[j]]);
      }
      while (packed.size() % kPlanWaves) { // empty waves: no lane active, the first wave's voice as the shadow address
        WaveDesc pad = W[order[i]];
        pad.count = 0;
        packed.push_back(pad);
      }
      i = e;
    }
  }
  plan.n_vwaves = (uint32_t)plan.waves.size();
  const uint32_t wgs = plan.n_vwaves / kPlanWaves;
  auto sized = [](WgLists& l, uint32_t entries) { l.list.resize(entries); l.cls.resize(entries); l.base.resize(entries); l.f32.resize(entries); };
  WgLists& s = plan.sorted;
  sized(s, wgs);
  {
    std::vector<uint32_t> at(kWgKinds + 1, 0);
    for (uint16_t k : kind) plan.wgs_of_kind[k] += 1;
    for (int k = 0; k < kWgKinds; ++k) at[k + 1] = at[k] + plan.wgs_of_kind[k];
    for (uint32_t g = 0; g < wgs; ++g) {
      const uint32_t slot = at[kind[g]]++;
      s.list[slot] = g;
      s.cls[slot] = (uint8_t)(kind[g] % kClassCombos);
      s.base[slot] = (uint8_t)(kind[g] / kClassCombos);
      s.f32[slot] = f32_of[g];
    }
  }
  // the mix kernel's sections: slots s, s + 3, s + 6 ... of the class-specialised part of the sorted list (the exact-f64 kinds, last in it, keep their own kernels)
  const uint32_t n_spec = kind_slices(plan.wgs_of_kind).n_spec;
  WgLists& m = plan.striped;
  sized(m, n_spec);
  uint32_t at = 0;
  for (uint32_t sec = 0; sec < 3; ++sec) {
    plan.mix_off[sec] = at;
    for (uint32_t g = sec; g < n_spec; g += 3, ++at) { m.list[at] = s.list[g]; m.cls[at] = s.cls[g]; m.base[at] = s.base[g]; m.f32[at] = s.f32[g]; }
    plan.mix_cnt[sec] = at - plan.mix_off[sec];
  }
  return plan;
}

} // namespace groove
