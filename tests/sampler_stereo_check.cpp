// sampler_stereo_check.cpp — host build (g++) of groove_amd/csrc/dsp_core.h's stereo sampler text, a program of its own
// (tests/test_wav_stereo_cpu.py builds and runs it): sampler_chunk_stereo<C> over `count` frames must give what `count` calls of
// sampler_frame_stereo give — values, idx, playing — and the mono forms must give the left channel's.  TEST HARNESS ONLY.
#include "../groove_amd/csrc/dsp_core.h"
#include <cstdio>
#include <cstring>
#include <vector>
using namespace groove;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

template <int C>
static int one_case(const std::vector<SamplePair>& bank, const std::vector<float>& left, SamplerParams p, SamplerState s0, uint32_t count, const char* what) {
  SamplerState a = s0, b = s0, m = s0, mf = s0;
  float l[C], r[C], x[C];
  sampler_chunk_stereo<C>(p, a, bank.data(), count, l, r);
  sampler_chunk<C>(p, m, left.data(), count, x);
  for (uint32_t k = 0; k < (uint32_t)C; ++k) {
    float wl = 0.0f, wr = 0.0f, wm = 0.0f;
    if (k < count) { sampler_frame_stereo(p, b, bank.data(), wl, wr); wm = sampler_frame(p, mf, left.data()); }
    if (std::memcmp(&wl, &l[k], 4) || std::memcmp(&wr, &r[k], 4) || std::memcmp(&wm, &x[k], 4) || std::memcmp(&wl, &wm, 4)) {
      std::printf("FAIL %s: frame %u of %u: chunk %g %g, frames %g %g, mono %g / %g\n", what, k, count, l[k], r[k], wl, wr, x[k], wm);
      return 1;
    }
  }
  if (a.idx != b.idx || a.playing != b.playing || a.step != b.step || a.idx != m.idx || a.playing != m.playing || mf.idx != a.idx || mf.playing != a.playing) {
    std::printf("FAIL %s: state after %u frames: chunk idx %llu playing %u, frames idx %llu playing %u, mono idx %llu playing %u\n", what, count,
                (unsigned long long)a.idx, a.playing, (unsigned long long)b.idx, b.playing, (unsigned long long)m.idx, m.playing);
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
    bank[i].l = (float)((double)(rnd() >> 11) / 9007199254740992.0 - 0.5);
    bank[i].r = (float)((double)(rnd() >> 11) / 9007199254740992.0 - 0.5);
    left[i] = bank[i].l;
  }
  int bad = 0, cases = 0;
  auto run = [&](uint32_t offset, uint32_t length, uint64_t idx, uint64_t step, uint32_t playing, uint32_t count, const char* what) {
    SamplerParams p{offset, length, 440.0, 0.25f + (float)(rnd() % 1000) / 1000.0f, 0u};
    SamplerState s{idx, step, playing, 0u};
    bad += one_case<C>(bank, left, p, s, count, what);
    ++cases;
  };
  const uint64_t one = 1ull << 44;
  // the named cases: count < C, a sample that ends inside the chunk, step 0, length 1, not playing, count 0
  for (uint32_t count = 0; count <= (uint32_t)C; ++count) {
    run(10, 100, 0, one, 1, count, "count");
    run(10, 100, 95 * one, one, 1, count, "ends inside the chunk");
    run(10, 100, 97 * one + one / 3, one / 2 + 12345, 1, count, "ends inside the chunk, step < 1");
    run(10, 100, 3 * one, 0, 1, count, "step 0");
    run(5999, 1, 0, one, 1, count, "length 1");
    run(5999, 1, 0, one / 4, 1, count, "length 1, step 1/4");
    run(10, 100, 5 * one, one, 0, count, "not playing");
    run(10, 100, 100 * one, one, 1, count, "already at the end");
  }
  for (int it = 0; it < 20000; ++it) { // random (idx, step, length, count)
    const uint32_t length = 1 + (uint32_t)(rnd() % (it % 3 == 0 ? 40 : 5000));
    const uint32_t offset = (uint32_t)(rnd() % (frames - length + 1));
    const uint64_t step = it % 7 == 0 ? 0 : rnd() % (4 * one);
    const uint64_t idx = rnd() % (((uint64_t)length + 2) << 44);
    run(offset, length, idx, step, it % 11 != 0, (uint32_t)(rnd() % (C + 1)), "random");
  }
  std::printf("%s: %d cases, %d failed\n", bad ? "FAIL" : "ok", cases, bad);
  return bad ? 1 : 0;
}
