// sampler_interp_check.cpp — host build (g++) of groove_amd/csrc/dsp_core.h's interpolated sampler text, a program of its own
// (tests/test_sampler_interp_cpu.py builds and runs it, with the address and undefined-behaviour sanitizers):
//   1. sampler_chunk_interp<MODE, C> / _stereo over `count` frames give what `count` calls of sampler_frame_interp<MODE> / _stereo give —
//      values, idx, playing — in all three modes, and the mono forms give the stereo forms' left channel;
//   2. MODE NEAREST is sampler_frame / sampler_chunk bit for bit, and a frame whose fraction t is 0 plays NEAREST's bits in every mode;
//   3. the tap rule at both ends of a sample: the per-frame form against the formula written out here in double with the taps before
//      the first and past the last frame 0 — the sample lies between neighbours of 1e6, so a tap taken across its boundary is no
//      rounding error — and, for a sample that is the whole allocation, no address outside it (the sanitizer's part).
// TEST HARNESS ONLY.
#include "../groove_amd/csrc/dsp_core.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
using namespace groove;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static float noise() { const float x = (float)((double)(rnd() >> 11) / 9007199254740992.0 - 0.5); return x < 0 ? x - 0.1f : x + 0.1f; } // 0.1 <= |x| <= 0.6
static bool same(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }
static const char* kMode[3] = {"nearest", "linear", "cubic"};

// properties 1 and 2 for one (params, state, count)
template <int MODE, int C>
static int chunk_case(const std::vector<SamplePair>& bank, const std::vector<float>& left, SamplerParams p, SamplerState s0, uint32_t count, const char* what) {
  SamplerState a = s0, b = s0, m = s0, mf = s0, n = s0;
  float l[C], r[C], x[C];
  sampler_chunk_interp_stereo<MODE, C>(p, a, bank.data(), count, l, r);
  sampler_chunk_interp<MODE, C>(p, m, left.data(), count, x);
  for (uint32_t k = 0; k < (uint32_t)C; ++k) {
    float wl = 0.0f, wr = 0.0f, wm = 0.0f, wn = 0.0f;
    const bool whole = (mf.idx & ((1ull << 44) - 1)) >> 20 == 0; // t == 0 at this frame
    if (k < count) {
      sampler_frame_interp_stereo<MODE>(p, b, bank.data(), wl, wr);
      wm = sampler_frame_interp<MODE>(p, mf, left.data());
      wn = sampler_frame(p, n, left.data());
    }
    if (!same(wl, l[k]) || !same(wr, r[k]) || !same(wm, x[k]) || !same(wl, wm)) {
      std::printf("FAIL %s, %s: frame %u of %u: chunk %g %g, frames %g %g, mono %g / %g\n", kMode[MODE], what, k, count, l[k], r[k], wl, wr, x[k], wm);
      return 1;
    }
    if ((MODE == GROOVE_SAMPLE_NEAREST || whole) && !same(wm, wn)) {
      std::printf("FAIL %s, %s: frame %u of %u has t == 0 and plays %.9g where nearest plays %.9g\n", kMode[MODE], what, k, count, wm, wn);
      return 1;
    }
  }
  if (a.idx != b.idx || a.playing != b.playing || a.step != b.step || a.idx != m.idx || a.playing != m.playing || mf.idx != a.idx || mf.playing != a.playing ||
      n.idx != a.idx || n.playing != a.playing) {
    std::printf("FAIL %s, %s: state after %u frames: chunk idx %llu playing %u, frames idx %llu playing %u, nearest idx %llu playing %u\n", kMode[MODE], what, count,
                (unsigned long long)a.idx, a.playing, (unsigned long long)b.idx, b.playing, (unsigned long long)n.idx, n.playing);
    return 1;
  }
  if (MODE == GROOVE_SAMPLE_NEAREST) { // the chunk form of NEAREST too
    SamplerState c = s0;
    float y[C];
    sampler_chunk<C>(p, c, left.data(), count, y);
    for (int k = 0; k < C; ++k)
      if (!same(y[k], x[k])) { std::printf("FAIL nearest, %s: frame %d: sampler_chunk_interp %g, sampler_chunk %g\n", what, k, x[k], y[k]); return 1; }
  }
  return 0;
}

// property 3: one frame at cursor `pos` of a sample of `length` frames at `offset` of `bank`, against the formula in double
template <int MODE>
static int tap_case(const std::vector<float>& bank, uint32_t offset, uint32_t length, uint64_t pos, const char* what) {
  const SamplerParams p{offset, length, 440.0, 0.75f, 0u};
  SamplerState s{pos, 1ull << 43, 1u, 0u};
  const float got = sampler_frame_interp<MODE>(p, s, bank.data());
  const int64_t i = (int64_t)(pos >> 44);
  const double t = (double)((pos >> 20) & 0xFFFFFFu) / 16777216.0;
  auto tap = [&](int64_t j) { return j < 0 || j >= (int64_t)length ? 0.0 : (double)bank[offset + (size_t)j]; };
  double want, big;
  if (MODE == GROOVE_SAMPLE_LINEAR) {
    want = tap(i) + t * (tap(i + 1) - tap(i));
    big = std::fmax(std::fabs(tap(i)), std::fabs(tap(i + 1)));
  } else if (MODE == GROOVE_SAMPLE_CUBIC) {
    const double pm = tap(i - 1), p0 = tap(i), p1 = tap(i + 1), p2 = tap(i + 2);
    const double c1 = 0.5 * (p1 - pm), c2 = pm - 2.5 * p0 + 2.0 * p1 - 0.5 * p2, c3 = 0.5 * (p2 - pm) + 1.5 * (p0 - p1);
    want = ((c3 * t + c2) * t + c1) * t + p0;
    big = std::fmax(std::fmax(std::fabs(pm), std::fabs(p0)), std::fmax(std::fabs(p1), std::fabs(p2)));
  } else {
    want = tap(i);
    big = std::fabs(want);
  }
  want *= 0.75;
  const double bound = big * 0.75 / 262144.0 + std::fabs(want) / 16777216.0; // 2^-18 M gain + the rounding of `want` to fp32
  if (!(std::fabs((double)got - want) <= bound)) {
    std::printf("FAIL %s, %s: length %u, frame %lld, t %g: got %.9g, want %.9g (bound %g)\n", kMode[MODE], what, length, (long long)i, t, got, want, bound);
    return 1;
  }
  return 0;
}

int main() {
  constexpr int C = 16;
  const uint32_t frames = 6000;
  std::vector<SamplePair> bank(frames);
  std::vector<float> left(frames);
  for (uint32_t i = 0; i < frames; ++i) {
    bank[i].l = noise();
    bank[i].r = noise();
    left[i] = bank[i].l;
  }
  int bad = 0, cases = 0;
  auto run = [&](uint32_t offset, uint32_t length, uint64_t idx, uint64_t step, uint32_t playing, uint32_t count, const char* what) {
    SamplerParams p{offset, length, 440.0, 0.25f + (float)(rnd() % 1000) / 1000.0f, 0u};
    SamplerState s{idx, step, playing, 0u};
    bad += chunk_case<GROOVE_SAMPLE_NEAREST, C>(bank, left, p, s, count, what);
    bad += chunk_case<GROOVE_SAMPLE_LINEAR, C>(bank, left, p, s, count, what);
    bad += chunk_case<GROOVE_SAMPLE_CUBIC, C>(bank, left, p, s, count, what);
    cases += 3;
  };
  const uint64_t one = 1ull << 44;
  // the named cases: count < C, a sample that ends inside the chunk, step 0, lengths 1 - 3, samples at either end of the allocation
  // (the sanitizer's part: no tap address outside the sample), not playing, count 0
  for (uint32_t count = 0; count <= (uint32_t)C; ++count) {
    run(10, 100, 0, one, 1, count, "count");
    run(10, 100, 0, one / 2, 1, count, "step 1/2");
    run(10, 100, 95 * one, one, 1, count, "ends inside the chunk");
    run(10, 100, 97 * one + one / 3, one / 2 + 12345, 1, count, "ends inside the chunk, step < 1");
    run(10, 100, 90 * one + one / 5, 2 * one + one / 7, 1, count, "ends inside the chunk, step > 2");
    run(10, 100, 3 * one + one / 2, 0, 1, count, "step 0");
    run(5999, 1, 0, one, 1, count, "length 1, last frame of the allocation");
    run(5999, 1, one / 3, one / 4, 1, count, "length 1, step 1/4");
    run(0, 1, one / 3, one / 4, 1, count, "length 1, first frame of the allocation");
    run(0, 2, 0, one / 4 + 999, 1, count, "length 2, start of the allocation");
    run(5998, 2, 0, one / 4 + 999, 1, count, "length 2, end of the allocation");
    run(0, 3, 0, one / 3, 1, count, "length 3, start of the allocation");
    run(5997, 3, 0, one / 3, 1, count, "length 3, end of the allocation");
    run(0, 6000, 5990 * one, one - 4321, 1, count, "the whole allocation, its end");
    run(10, 100, 5 * one, one, 0, count, "not playing");
    run(10, 100, 100 * one, one, 1, count, "already at the end");
  }
  for (int it = 0; it < 20000; ++it) { // random (idx, step, length, count)
    const uint32_t length = 1 + (uint32_t)(rnd() % (it % 3 == 0 ? 40 : 5000));
    const uint32_t offset = (uint32_t)(rnd() % (frames - length + 1));
    const uint64_t step = it % 7 == 0 ? 0 : (it % 5 == 0 ? (1 + rnd() % 3) * one : rnd() % (4 * one));
    const uint64_t idx = it % 5 == 0 ? (rnd() % ((uint64_t)length + 2)) << 44 : rnd() % (((uint64_t)length + 2) << 44);
    run(offset, length, idx, step, it % 11 != 0, (uint32_t)(rnd() % (C + 1)), "random");
  }
  // property 3: samples of 1, 2, 3, 4 and 100 frames between neighbours of 1e6, every frame of them at several fractions
  for (uint32_t length : {1u, 2u, 3u, 4u, 100u}) {
    std::vector<float> b(length + 8, 1.0e6f);
    for (uint32_t i = 0; i < length; ++i) b[4 + i] = noise();
    for (uint32_t i = 0; i < length; ++i) {
      const uint64_t fracs[] = {0, 1ull << 20, one / 4, one / 2, one - (1ull << 20), one - 1};
      for (const uint64_t frac : fracs) {
        bad += tap_case<GROOVE_SAMPLE_NEAREST>(b, 4, length, i * one + frac, "between loud neighbours");
        bad += tap_case<GROOVE_SAMPLE_LINEAR>(b, 4, length, i * one + frac, "between loud neighbours");
        bad += tap_case<GROOVE_SAMPLE_CUBIC>(b, 4, length, i * one + frac, "between loud neighbours");
        cases += 3;
      }
    }
  }
  std::printf("%s: %d cases, %d failed\n", bad ? "FAIL" : "ok", cases, bad);
  return bad ? 1 : 0;
}
