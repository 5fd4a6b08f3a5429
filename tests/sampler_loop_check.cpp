// sampler_loop_check.cpp — host build (g++) of groove_amd/csrc/dsp_core.h's looped sampler text and of the host layer's read_wav_loop,
// a program of its own (tests/test_sampler_loop_cpu.py builds and runs it, with the address and undefined-behaviour sanitizers):
//   1. sample_loop_fold against a loop of repeated subtraction, and F(F(x) + y) == F(x + y) (sample_loop_advance) on random and
//      edge values, in 128-bit integers where x + y passes 2^64;
//   2. sampler_chunk_loop<MODE, C> / _stereo over `count` frames give what `count` calls of sampler_frame_loop<MODE> / _stereo give —
//      values, idx, playing — in all three modes, for voices that loop and voices that do not; a voice that does not loop (no loop, a
//      one-shot voice) is sampler_frame_interp's bits; a frame whose fraction is 0 plays NEAREST's bits;
//   3. the tap rule at loops of 1, 2 and 3 frames, start == 0 and end == length: the per-frame form against the formula written out
//      in double over the taps start + (j - start) mod (end - start); every sample is an allocation of exactly `end` frames where it
//      can be (the sanitizer's part: no address outside [offset, offset + end)), and lies between neighbours of 1e6 where it cannot;
//      the chunk forms run on the same allocations, so a fetch past `end` that a select would drop is found too;
//   4. the wrap case: length 2^20 - 1, end == length, step 2^51;
//   5. read_wav_loop on WAV files written here: a forward loop, a ping-pong loop, a truncated chunk, dwEnd at and past the frame
//      count, a file without the chunk, and chunks of two records (the first forward one is taken, wherever it stands).
// TEST HARNESS ONLY.
#include "../groove_amd/csrc/dsp_core.h"
#include "../groove_amd/host/project.hpp"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
using namespace groove;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static float noise() { const float x = (float)((double)(rnd() >> 11) / 9007199254740992.0 - 0.5); return x < 0 ? x - 0.1f : x + 0.1f; } // 0.1 <= |x| <= 0.6
static bool same(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }
static const char* kMode[3] = {"nearest", "linear", "cubic"};
static const uint64_t one = 1ull << 44;
typedef unsigned __int128 u128;

// F(x) for x of any size, by the definition
static uint64_t fold_ref(u128 x, uint32_t start, uint32_t end) {
  const u128 S = (u128)start << 44, E = (u128)end << 44, L = E - S;
  return (uint64_t)(x < E ? x : S + (x - S) % L);
}

static int fold_cases(int& cases) {
  int bad = 0;
  // repeated subtraction, on loops short enough for it
  for (int it = 0; it < 2000; ++it) {
    const uint32_t start = (uint32_t)(rnd() % 50), end = start + 1 + (uint32_t)(rnd() % 9);
    uint64_t x = rnd() % ((uint64_t)(end + 200) << 44);
    const uint64_t got = sample_loop_fold(x, start, end);
    const uint64_t E = (uint64_t)end << 44, L = (uint64_t)(end - start) << 44;
    while (x >= E) x -= L;
    ++cases;
    if (got != x) { std::printf("FAIL fold: loop [%u, %u): got %llu, repeated subtraction %llu\n", start, end, (unsigned long long)got, (unsigned long long)x); ++bad; }
  }
  // F(F(x) + y) == F(x + y), random and edge values
  const uint32_t lens[] = {1u, 2u, 3u, 7u, 100u, 5000u, (1u << 20) - 1};
  for (int it = 0; it < 40000; ++it) {
    const uint32_t length = lens[it % 7];
    uint32_t start, end;
    switch (it % 5) {
      case 0: start = 0; end = length; break;
      case 1: end = length; start = end - 1; break;
      case 2: start = 0; end = 1; break;
      default: start = (uint32_t)(rnd() % length); end = start + 1 + (uint32_t)(rnd() % (length - start)); break;
    }
    uint64_t x, y;
    switch (it % 4) {
      case 0: x = rnd(); y = rnd(); break;                                    // anything: x + y passes 2^64 half of the time
      case 1: x = ((uint64_t)end << 44) - 1; y = rnd() % 3; break;            // the last cursor below E
      case 2: x = rnd() % ((uint64_t)length << 44); y = 1ull << 51; break;
      default: x = (uint64_t)(rnd() % (length + 1)) << 44; y = (rnd() % 4) * one; break; // whole frames
    }
    const uint64_t fx = sample_loop_fold(x, start, end);
    const uint64_t got = sample_loop_advance(fx, y, start, end);
    const uint64_t want = fold_ref((u128)x + y, start, end);
    ++cases;
    if (fx != fold_ref(x, start, end) || got != want || got >= ((uint64_t)end << 44)) {
      std::printf("FAIL F(F(x) + y): loop [%u, %u), x %llu, y %llu: F(x) %llu, got %llu, want %llu\n", start, end, (unsigned long long)x, (unsigned long long)y,
                  (unsigned long long)fx, (unsigned long long)got, (unsigned long long)want);
      ++bad;
    }
  }
  return bad;
}

// property 2 for one (params, loop, state, count)
template <int MODE, int C>
static int chunk_case(const std::vector<SamplePair>& bank, const std::vector<float>& left, SamplerParams p, SampleLoop lp, SamplerState s0, uint32_t count, const char* what) {
  SamplerState a = s0, b = s0, m = s0, mf = s0, n = s0, plain = s0;
  float l[C], r[C], x[C];
  sampler_chunk_loop_stereo<MODE, C>(p, lp, a, bank.data(), count, l, r);
  sampler_chunk_loop<MODE, C>(p, lp, m, left.data(), count, x);
  const bool loops = sampler_voice_loops(p, s0, lp);
  for (uint32_t k = 0; k < (uint32_t)C; ++k) {
    float wl = 0.0f, wr = 0.0f, wm = 0.0f, wn = 0.0f, wp = 0.0f;
    bool whole = false;
    if (k < count) {
      const uint64_t c = loops ? sample_loop_fold(mf.idx, lp.start, lp.end) : mf.idx;
      whole = (c & ((1ull << 44) - 1)) >> 20 == 0; // t == 0 at this frame
      sampler_frame_loop_stereo<MODE>(p, lp, b, bank.data(), wl, wr);
      wm = sampler_frame_loop<MODE>(p, lp, mf, left.data());
      wn = sampler_frame_loop<GROOVE_SAMPLE_NEAREST>(p, lp, n, left.data());
      if (!loops) wp = sampler_frame_interp<MODE>(p, plain, left.data());
    }
    if (!same(wl, l[k]) || !same(wr, r[k]) || !same(wm, x[k]) || !same(wl, wm)) {
      std::printf("FAIL %s, %s: frame %u of %u: chunk %g %g, frames %g %g, mono %g / %g\n", kMode[MODE], what, k, count, l[k], r[k], wl, wr, x[k], wm);
      return 1;
    }
    if (whole && !same(wm, wn)) { std::printf("FAIL %s, %s: frame %u has t == 0 and plays %.9g where nearest plays %.9g\n", kMode[MODE], what, k, wm, wn); return 1; }
    if (!loops && !same(wm, wp)) { std::printf("FAIL %s, %s: frame %u of a voice that does not loop: %.9g, sampler_frame_interp %.9g\n", kMode[MODE], what, k, wm, wp); return 1; }
  }
  if (a.idx != b.idx || a.playing != b.playing || a.step != b.step || a.idx != m.idx || a.playing != m.playing || mf.idx != a.idx || mf.playing != a.playing ||
      n.idx != a.idx || n.playing != a.playing || (!loops && (plain.idx != a.idx || plain.playing != a.playing)) || (loops && count && a.idx >= ((uint64_t)lp.end << 44))) {
    std::printf("FAIL %s, %s: state after %u frames: chunk idx %llu playing %u, frames idx %llu playing %u, nearest idx %llu playing %u\n", kMode[MODE], what, count,
                (unsigned long long)a.idx, a.playing, (unsigned long long)b.idx, b.playing, (unsigned long long)n.idx, n.playing);
    return 1;
  }
  return 0;
}

// property 3: one frame of a looping voice at cursor `pos`, against the formula in double over the looped taps
template <int MODE>
static int tap_case(const std::vector<float>& bank, uint32_t offset, uint32_t length, SampleLoop lp, uint64_t pos, const char* what) {
  const SamplerParams p{offset, length, 440.0, 0.75f, 0u};
  SamplerState s{pos, 1ull << 43, 1u, 0u};
  const float got = sampler_frame_loop<MODE>(p, lp, s, bank.data());
  const uint64_t c = fold_ref(pos, lp.start, lp.end);
  const int64_t i = (int64_t)(c >> 44);
  const double t = (double)((c >> 20) & 0xFFFFFFu) / 16777216.0;
  int outside = 0;
  auto tap = [&](int64_t j) {
    if (j < 0) return 0.0;
    if (j >= (int64_t)lp.end) j = lp.start + (j - lp.start) % (int64_t)(lp.end - lp.start);
    if (j < 0 || j >= (int64_t)lp.end) ++outside;
    return (double)bank[offset + (size_t)j];
  };
  for (int k = SampleTaps<MODE>::FIRST; k < SampleTaps<MODE>::FIRST + SampleTaps<MODE>::N; ++k) { // the index rule itself, against the modulo
    const int64_t j = i + k;
    const int64_t want = j < (int64_t)lp.end ? j : lp.start + (j - lp.start) % (int64_t)(lp.end - lp.start);
    const int32_t gotj = sample_loop_tap((uint32_t)i, k, lp.start, lp.end);
    if (gotj != want || gotj >= (int32_t)lp.end) { std::printf("FAIL %s, %s: tap %lld + %d of loop [%u, %u): index %d, want %lld\n", kMode[MODE], what, (long long)i, k, lp.start, lp.end, gotj, (long long)want); return 1; }
  }
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
  const uint64_t next = fold_ref((u128)c + (1ull << 43), lp.start, lp.end); // (the step above)
  if (outside || !(std::fabs((double)got - want) <= bound) || s.idx != next) {
    std::printf("FAIL %s, %s: length %u, loop [%u, %u), frame %lld, t %g: got %.9g, want %.9g (bound %g), idx %llu, want %llu\n", kMode[MODE], what, length, lp.start, lp.end,
                (long long)i, t, got, want, bound, (unsigned long long)s.idx, (unsigned long long)next);
    return 1;
  }
  return 0;
}

// property 5: WAV files written here
static void put32(std::string& s, uint32_t v) { for (int i = 0; i < 4; ++i) s.push_back((char)((v >> (8 * i)) & 0xFF)); }
static void put16(std::string& s, uint32_t v) { s.push_back((char)(v & 0xFF)); s.push_back((char)((v >> 8) & 0xFF)); }
// a 16-bit mono file of `frames` frames; smpl_bytes < 0: no smpl chunk, otherwise the chunk cut to that many bytes (60: whole, one loop)
// type2 >= 0: a second loop record of that type over [first2, last2] (the whole chunk is then 84 bytes)
static std::string wav_file(uint32_t frames, int smpl_bytes, uint32_t type, uint32_t first, uint32_t last, int type2 = -1, uint32_t first2 = 0, uint32_t last2 = 0) {
  std::string body = "WAVE";
  body += "fmt "; put32(body, 16); put16(body, 1); put16(body, 1); put32(body, 44100); put32(body, 88200); put16(body, 2); put16(body, 16);
  if (smpl_bytes >= 0) {
    std::string c;
    put32(c, 0); put32(c, 0); put32(c, 22675); put32(c, 60); put32(c, 0); put32(c, 0); put32(c, 0); put32(c, type2 >= 0 ? 2 : 1); put32(c, 0); // header: the number of loops
    put32(c, 0); put32(c, type); put32(c, first); put32(c, last); put32(c, 0); put32(c, 0);
    if (type2 >= 0) { put32(c, 1); put32(c, (uint32_t)type2); put32(c, first2); put32(c, last2); put32(c, 0); put32(c, 0); }
    c.resize((size_t)smpl_bytes);
    body += "smpl"; put32(body, (uint32_t)c.size()); body += c;
    if (c.size() & 1) body.push_back(0);
  }
  body += "data"; put32(body, frames * 2);
  for (uint32_t i = 0; i < frames; ++i) put16(body, (uint32_t)(int16_t)(i * 37 % 2000 - 1000) & 0xFFFFu);
  std::string file = "RIFF"; put32(file, (uint32_t)body.size()); file += body;
  return file;
}
static int wav_case(const std::string& dir, const char* name, const std::string& file, bool want_ok, uint32_t want_start, uint32_t want_end, bool want_warning) {
  const std::string path = dir + "/" + name;
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f || std::fwrite(file.data(), 1, file.size(), f) != file.size()) { std::printf("FAIL cannot write %s\n", path.c_str()); if (f) std::fclose(f); return 1; }
  std::fclose(f);
  uint32_t s = 77, e = 77;
  std::string warning;
  const bool ok = groove_host::read_wav_loop(path, &s, &e, &warning);
  if (ok != want_ok || s != want_start || e != want_end || warning.empty() == want_warning) {
    std::printf("FAIL read_wav_loop(%s): %d [%u, %u) warning '%s'; want %d [%u, %u), %s\n", name, (int)ok, s, e, warning.c_str(), (int)want_ok, want_start, want_end,
                want_warning ? "a warning" : "no warning");
    return 1;
  }
  return 0;
}

int main(int argc, char** argv) {
  constexpr int C = 16;
  int bad = 0, cases = 0;
  bad += fold_cases(cases);

  const uint32_t frames = 6000;
  std::vector<SamplePair> bank(frames);
  std::vector<float> left(frames);
  for (uint32_t i = 0; i < frames; ++i) { bank[i].l = noise(); bank[i].r = noise(); left[i] = bank[i].l; }
  auto run = [&](uint32_t offset, uint32_t length, SampleLoop lp, uint32_t one_shot, uint64_t idx, uint64_t step, uint32_t playing, uint32_t count, const char* what) {
    SamplerParams p{offset, length, 440.0, 0.25f + (float)(rnd() % 1000) / 1000.0f, one_shot};
    SamplerState s{idx, step, playing, 0u};
    bad += chunk_case<GROOVE_SAMPLE_NEAREST, C>(bank, left, p, lp, s, count, what);
    bad += chunk_case<GROOVE_SAMPLE_LINEAR, C>(bank, left, p, lp, s, count, what);
    bad += chunk_case<GROOVE_SAMPLE_CUBIC, C>(bank, left, p, lp, s, count, what);
    cases += 3;
  };
  for (uint32_t count = 0; count <= (uint32_t)C; ++count) {
    run(10, 100, {90, 100}, 0, 0, one, 1, count, "loop at the end");
    run(10, 100, {90, 100}, 0, 95 * one, one / 2 + 12345, 1, count, "inside the loop, step < 1");
    run(10, 100, {90, 100}, 0, 85 * one + one / 5, 2 * one + one / 7, 1, count, "runs into the loop, step > 2");
    run(10, 100, {90, 100}, 0, 3 * one, 37 * one + one / 3, 1, count, "step > the loop: a frame wraps several times");
    run(10, 100, {90, 100}, 0, 99 * one + 5, 0, 1, count, "step 0");
    run(10, 100, {20, 50}, 0, 70 * one + one / 3, one, 1, count, "cursor past end when the loop was set");
    run(10, 100, {20, 50}, 0, 100 * one, one, 1, count, "cursor at the sample's end when the loop was set");
    run(10, 100, {90, 100}, 1, 95 * one, one, 1, count, "one-shot voice on a looped sample");
    run(10, 100, {0, 0}, 0, 95 * one, one, 1, count, "no loop");
    run(10, 100, {90, 100}, 0, 95 * one, one, 0, count, "not playing");
    run(5999, 1, {0, 1}, 0, one / 3, one / 4, 1, count, "loop [0, 1) of one frame, last frame of the allocation");
    run(0, 1, {0, 1}, 0, 0, one * 3, 1, count, "loop [0, 1), first frame of the allocation");
    run(0, 2, {0, 2}, 0, 0, one / 4 + 999, 1, count, "loop [0, 2)");
    run(5998, 2, {1, 2}, 0, 0, one / 4 + 999, 1, count, "loop [1, 2) at the end of the allocation");
    run(5994, 6, {1, 4}, 0, 0, one / 3, 1, count, "loop [1, 4) of six frames");
    run(0, 6000, {5990, 6000}, 0, 5980 * one, one - 4321, 1, count, "the whole allocation, loop at its end");
  }
  for (int it = 0; it < 20000; ++it) { // random (loop, idx, step, length, count)
    const uint32_t length = 1 + (uint32_t)(rnd() % (it % 3 == 0 ? 40 : 5000));
    const uint32_t offset = (uint32_t)(rnd() % (frames - length + 1));
    SampleLoop lp{0, 0};
    if (it % 9 != 0) { lp.start = (uint32_t)(rnd() % length); lp.end = lp.start + 1 + (uint32_t)(rnd() % (it % 2 ? std::min(length - lp.start, 4u) : length - lp.start)); }
    const uint64_t step = it % 7 == 0 ? 0 : (it % 5 == 0 ? (1 + rnd() % 3) * one : rnd() % (it % 4 == 0 ? 600 * one : 4 * one));
    const uint64_t idx = it % 5 == 0 ? (rnd() % ((uint64_t)length + 2)) << 44 : rnd() % (((uint64_t)length + 2) << 44);
    run(offset, length, lp, it % 13 == 0, idx, step, it % 11 != 0, (uint32_t)(rnd() % (C + 1)), "random");
  }

  // property 3: the allocation is offset + end frames long (nothing readable past the loop's end); the frames before `offset` are 1e6
  struct TapShape { uint32_t length, start, end; };
  for (const TapShape sh : {TapShape{1, 0, 1}, TapShape{2, 0, 2}, TapShape{2, 1, 2}, TapShape{6, 1, 4}, TapShape{3, 0, 3}, TapShape{100, 90, 100}, TapShape{100, 0, 100},
                            TapShape{100, 99, 100}, TapShape{100, 0, 1}, TapShape{100, 40, 42}}) {
    std::vector<float> b(4 + sh.end, 1.0e6f);
    for (uint32_t i = 0; i < sh.end; ++i) b[4 + i] = noise();
    for (uint32_t i = 0; i < sh.end + 5; ++i) { // (cursors past `end` too: folded first)
      const uint64_t fracs[] = {0, 1ull << 20, one / 4, one / 2, one - (1ull << 20), one - 1};
      for (const uint64_t frac : fracs) {
        bad += tap_case<GROOVE_SAMPLE_NEAREST>(b, 4, sh.length, {sh.start, sh.end}, i * one + frac, "loop at the allocation's end");
        bad += tap_case<GROOVE_SAMPLE_LINEAR>(b, 4, sh.length, {sh.start, sh.end}, i * one + frac, "loop at the allocation's end");
        bad += tap_case<GROOVE_SAMPLE_CUBIC>(b, 4, sh.length, {sh.start, sh.end}, i * one + frac, "loop at the allocation's end");
        cases += 3;
      }
    }
    // the chunk forms — what the serial kernel runs — on the same kind of allocation: a fetch past `end` that a select would drop is a
    // read outside the allocation, the sanitizer's to find; values and state against the per-frame form as everywhere
    std::vector<SamplePair> pairs(4 + sh.end, SamplePair{1.0e6f, 1.0e6f});
    for (uint32_t i = 0; i < sh.end; ++i) pairs[4 + i] = SamplePair{b[4 + i], noise()};
    const uint64_t steps[] = {0, one / 3, one - 1, one, 2 * one + one / 7, 8 * one, 37 * one + 5};
    for (uint32_t i = 0; i < sh.end + 5; i += (sh.end > 10 ? 7 : 1)) {
      for (const uint64_t step : steps) {
        for (const uint32_t count : {1u, 5u, (uint32_t)C}) {
          const SamplerParams p{4, sh.length, 440.0, 0.5f, 0u};
          const SamplerState st{i * one + one / 5, step, 1u, 0u};
          bad += chunk_case<GROOVE_SAMPLE_NEAREST, C>(pairs, b, p, {sh.start, sh.end}, st, count, "chunk on an allocation that ends at the loop's end");
          bad += chunk_case<GROOVE_SAMPLE_LINEAR, C>(pairs, b, p, {sh.start, sh.end}, st, count, "chunk on an allocation that ends at the loop's end");
          bad += chunk_case<GROOVE_SAMPLE_CUBIC, C>(pairs, b, p, {sh.start, sh.end}, st, count, "chunk on an allocation that ends at the loop's end");
          cases += 3;
        }
      }
    }
  }

  { // property 4: the wrap case.  A sample of 2^20 - 1 frames looped at its end, step 2^51: idx + k * step passes 2^64
    const uint32_t length = (1u << 20) - 1;
    std::vector<float> big(length);
    for (uint32_t i = 0; i < length; ++i) big[i] = (float)(int)(i % 2001) / 1000.0f - 1.0f;
    for (const SampleLoop lp : {SampleLoop{length - 5, length}, SampleLoop{0, length}, SampleLoop{length - 1, length}}) {
      for (int MODEi = 0; MODEi < 3; ++MODEi) {
        const SamplerParams p{0, length, 8.18, 1.0f, 0u};
        SamplerState a{((uint64_t)length << 44) - (1ull << 50) - 12345, 1ull << 51, 1u, 0u}, b = a;
        u128 exact = a.idx;
        for (int chunk = 0; chunk < 40; ++chunk) {
          float x[C], w[C];
          if (MODEi == 0) sampler_chunk_loop<GROOVE_SAMPLE_NEAREST, C>(p, lp, a, big.data(), C, x);
          else if (MODEi == 1) sampler_chunk_loop<GROOVE_SAMPLE_LINEAR, C>(p, lp, a, big.data(), C, x);
          else sampler_chunk_loop<GROOVE_SAMPLE_CUBIC, C>(p, lp, a, big.data(), C, x);
          for (int k = 0; k < C; ++k) {
            const uint64_t c = fold_ref(exact, lp.start, lp.end);
            if (MODEi == 0) { w[k] = sampler_frame_loop<GROOVE_SAMPLE_NEAREST>(p, lp, b, big.data()); if (!same(w[k], big[c >> 44])) { std::printf("FAIL wrap: frame not at the exact cursor\n"); ++bad; } }
            else if (MODEi == 1) w[k] = sampler_frame_loop<GROOVE_SAMPLE_LINEAR>(p, lp, b, big.data());
            else w[k] = sampler_frame_loop<GROOVE_SAMPLE_CUBIC>(p, lp, b, big.data());
            exact += (u128)1 << 51;
            if (!same(w[k], x[k])) { std::printf("FAIL wrap, %s: chunk %d frame %d: %g, frames %g\n", kMode[MODEi], chunk, k, x[k], w[k]); ++bad; }
          }
          const uint64_t want = fold_ref(exact, lp.start, lp.end);
          ++cases;
          if (a.idx != want || b.idx != want || !a.playing) {
            std::printf("FAIL wrap, %s: loop [%u, %u) after chunk %d: idx %llu / %llu, exact %llu, playing %u\n", kMode[MODEi], lp.start, lp.end, chunk, (unsigned long long)a.idx,
                        (unsigned long long)b.idx, (unsigned long long)want, a.playing);
            ++bad;
            break;
          }
        }
      }
    }
  }

  // property 5
  const std::string dir = argc > 1 ? argv[1] : ".";
  bad += wav_case(dir, "forward.wav", wav_file(1000, 60, 0, 200, 899), true, 200, 900, false);
  bad += wav_case(dir, "whole.wav", wav_file(1000, 60, 0, 0, 999), true, 0, 1000, false);
  bad += wav_case(dir, "pingpong.wav", wav_file(1000, 60, 1, 200, 899), false, 0, 0, true);
  bad += wav_case(dir, "reverse.wav", wav_file(1000, 60, 2, 200, 899), false, 0, 0, true);
  bad += wav_case(dir, "truncated.wav", wav_file(1000, 47, 0, 200, 899), false, 0, 0, true);
  bad += wav_case(dir, "truncated_header.wav", wav_file(1000, 20, 0, 200, 899), false, 0, 0, true);
  bad += wav_case(dir, "end_at_count.wav", wav_file(1000, 60, 0, 200, 1000), false, 0, 0, true);
  bad += wav_case(dir, "end_past_count.wav", wav_file(1000, 60, 0, 200, 5000), false, 0, 0, true);
  bad += wav_case(dir, "start_past_end.wav", wav_file(1000, 60, 0, 900, 200), false, 0, 0, true);
  bad += wav_case(dir, "no_chunk.wav", wav_file(1000, -1, 0, 0, 0), false, 0, 0, false);
  bad += wav_case(dir, "pingpong_then_forward.wav", wav_file(1000, 84, 1, 200, 899, 0, 300, 799), true, 300, 800, false);
  bad += wav_case(dir, "forward_then_pingpong.wav", wav_file(1000, 84, 0, 200, 899, 1, 300, 799), true, 200, 900, false);
  bad += wav_case(dir, "pingpong_then_reverse.wav", wav_file(1000, 84, 1, 200, 899, 2, 300, 799), false, 0, 0, true);
  bad += wav_case(dir, "pingpong_then_cut.wav", wav_file(1000, 70, 1, 200, 899, 0, 300, 799), false, 0, 0, true);
  bad += wav_case(dir, "pingpong_then_forward_past_the_end.wav", wav_file(1000, 84, 1, 200, 899, 0, 300, 1000), false, 0, 0, true);
  cases += 15;

  std::printf("%s: %d cases, %d failed\n", bad ? "FAIL" : "ok", cases, bad);
  return bad ? 1 : 0;
}
