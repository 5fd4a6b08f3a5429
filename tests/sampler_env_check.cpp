// sampler_env_check.cpp — host build (g++) of the enveloped sampler text of groove_amd/csrc/dsp_core.h, derive.h and welsh_tp.h, a
// program of its own (tests/test_sampler_env_cpu.py builds and runs it, with the address and undefined-behaviour sanitizers).  One voice
// at a time is rendered through a timeline of note events in three forms, and every frame and every block-end state is compared:
//   A. the per-frame DEFINITION: sampler_frame_env<MODE> / _stereo, one call per frame;
//   B. the serial kernel's form: sampler_chunk_env<MODE, 16> / _stereo over the block's chunks;
//   C. the time-parallel body's form: lanes are frames — `valid` from sampler_env_valid (env_idle_at), every lane's factors from
//      sampler_env_lane (env_seek to its first frame, then its ticks), the frame read at its closed-form position, the stored record
//      from sampler_env_block_end.
// What is checked:
//   1. B == A and C == A, bit for bit: values (both channels in B), SamplerState and all seven EnvState words at every block end, in the
//      three modes, for two splits of the same timeline into blocks (so the split changes nothing either), on a sample that ends during
//      its release, a looped one, a loop of one frame, a sample without an envelope and a one-shot voice on an enveloped sample;
//   2. the same where the sample's end and the release's end fall on the same frame, one and two frames apart either way, with the idle
//      frame on every position of a block, its last frame included;
//   3. the gate envelope (0, 0, 1, 0) plays sampler_frame_loop's bits under sampler_note and leaves its SamplerState words;
//   4. no tap is read outside the voice's sample: every sample is an allocation of exactly its length (the sanitizer's part).
// TEST HARNESS ONLY.
#include "../groove_amd/csrc/derive.h"
#include "../groove_amd/csrc/welsh_tp.h"
#include <cstdio>
#include <cstring>
#include <vector>
using namespace groove;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static float noise() { const float x = (float)((double)(rnd() >> 11) / 9007199254740992.0 - 0.5); return x < 0 ? x - 0.2f : x + 0.2f; } // 0.2 <= |x| <= 0.7
static bool same(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }
static bool same_env(const EnvState& a, const EnvState& b) { return std::memcmp(&a, &b, sizeof(EnvState)) == 0; }
static bool same_state(const SamplerState& a, const SamplerState& b) { return a.idx == b.idx && a.step == b.step && a.playing == b.playing; }
static const char* kMode[3] = {"nearest", "linear", "cubic"};
constexpr double kSr = 44100.0;

struct Sample { // an allocation of exactly `length` frames, mono and stereo
  std::vector<float> mono;
  std::vector<SamplePair> pair;
  explicit Sample(uint32_t length) : mono(length), pair(length) {
    for (uint32_t i = 0; i < length; ++i) { mono[i] = noise(); pair[i].l = mono[i]; pair[i].r = noise(); }
  }
};
struct Event { uint32_t frame; bool on; uint32_t key; };
struct Voice { SamplerState s; EnvState es; };

// One block of the time-parallel form, mono: the text of welsh_tp.h sampler_tp_body with a loop over the lanes.
template <int MODE>
static void block_tp(const SamplerParams& p, const SampleLoop& lp, const EnvParams& ep, Voice& v, const float* bank, uint32_t frames, float* out) {
  SamplerState s0 = v.s;
  uint32_t ls = 0, le = 0;
  if (sampler_voice_loops(p, s0, lp)) { ls = lp.start; le = lp.end; s0.idx = sample_loop_fold(s0.idx, ls, le); }
  uint32_t valid = 0;
  if (le) valid = frames;
  else if (s0.playing && frames) {
    const uint64_t lim = (uint64_t)p.length << 44;
    if (s0.idx < lim) {
      const uint64_t room = lim - s0.idx - 1;
      const uint64_t fmax = s0.step ? room / s0.step : (uint64_t)frames;
      valid = fmax >= frames ? frames : (uint32_t)fmax + 1u;
    }
  }
  const uint32_t valid_sample = valid;
  const bool env_on = s0.playing && sampler_voice_enveloped(p, ep);
  if (env_on) valid = sampler_env_valid(v.es, ep, valid_sample, frames);
  for (uint32_t lane = 0; lane < kTpLanes; ++lane) {
    const uint32_t n0 = lane * kTpChunk;
    float e[kTpChunk] = {1.0f, 1.0f, 1.0f, 1.0f};
    if (env_on) sampler_env_lane(v.es, ep, n0, e);
    for (uint32_t j = 0; j < kTpChunk; ++j) {
      const uint32_t f = n0 + j;
      if (f >= frames) continue;
      const uint64_t pos = sample_loop_pos(s0.idx, (uint64_t)f * s0.step, ls, le);
      const bool ok = s0.playing && (uint32_t)(pos >> 44) < p.length && f < valid;
      float x = 0.0f;
      if (ok) {
        SamplerState t = s0;
        t.idx = pos;
        x = sampler_frame_loop<MODE>(p, le ? lp : SampleLoop{0, 0}, t, bank);
        if (env_on) x = x * e[j];
      }
      out[f] = x;
    }
  }
  if (frames) {
    SamplerState s = s0;
    s.idx = sample_loop_pos(s0.idx, (uint64_t)valid * s0.step, ls, le);
    if (s0.playing && valid < frames) s.playing = 0;
    v.s = s;
    if (env_on) sampler_env_block_end(v.es, ep, valid_sample, frames);
  }
}

// One voice through a timeline, the three forms side by side.  `gate_ref`: also against sampler_frame_loop under sampler_note.
template <int MODE>
static int run(const Sample& smp, SamplerParams p, SampleLoop lp, EnvParams ep, const std::vector<Event>& events, const std::vector<uint32_t>& blocks, bool gate_ref, const char* what) {
  constexpr int C = 16;
  Voice a{SamplerState{0, 0, 0, 0}, EnvState{}}, b = a, bs = a, as = a, c = a;
  env_init(a.es); b = bs = as = c = a;
  SamplerState g{0, 0, 0, 0};
  uint32_t frame = 0;
  for (size_t bi = 0; bi < blocks.size(); ++bi) {
    const uint32_t frames = blocks[bi];
    for (const Event& ev : events) {
      if (ev.frame != frame) continue;
      for (Voice* v : {&a, &b, &bs, &as, &c}) sampler_note_env(p, ep, v->s, v->es, ev.key, ev.on);
      sampler_note(p, g, ev.key, ev.on);
    }
    std::vector<float> wa(frames), wl(frames), wr(frames), wc(frames), wg(frames);
    for (uint32_t f = 0; f < frames; ++f) {
      wa[f] = sampler_frame_env<MODE>(p, lp, ep, a.s, a.es, smp.mono.data());
      sampler_frame_env_stereo<MODE>(p, lp, ep, as.s, as.es, smp.pair.data(), wl[f], wr[f]);
      wg[f] = sampler_frame_loop<MODE>(p, lp, g, smp.mono.data());
    }
    block_tp<MODE>(p, lp, ep, c, smp.mono.data(), frames, wc.data());
    for (uint32_t f0 = 0; f0 < frames; f0 += C) {
      const uint32_t count = frames - f0 < (uint32_t)C ? frames - f0 : (uint32_t)C;
      float x[C], l[C], r[C];
      sampler_chunk_env<MODE, C>(p, lp, ep, b.s, b.es, smp.mono.data(), count, x);
      sampler_chunk_env_stereo<MODE, C>(p, lp, ep, bs.s, bs.es, smp.pair.data(), count, l, r);
      for (uint32_t k = 0; k < (uint32_t)C; ++k) {
        const float ea = k < count ? wa[f0 + k] : 0.0f, el = k < count ? wl[f0 + k] : 0.0f, er = k < count ? wr[f0 + k] : 0.0f;
        if (!same(x[k], ea) || !same(l[k], el) || !same(r[k], er) || !same(el, ea)) {
          std::printf("FAIL %s, %s: block %zu frame %u: chunk %.9g (%.9g, %.9g), per frame %.9g (%.9g, %.9g)\n", kMode[MODE], what, bi, f0 + k, x[k], l[k], r[k], ea, el, er);
          return 1;
        }
      }
    }
    for (uint32_t f = 0; f < frames; ++f) {
      if (!same(wc[f], wa[f])) { std::printf("FAIL %s, %s: block %zu frame %u: closed form %.9g, per frame %.9g\n", kMode[MODE], what, bi, f, wc[f], wa[f]); return 1; }
      if (gate_ref && !same(wg[f], wa[f])) { std::printf("FAIL %s, %s: block %zu frame %u: gate envelope %.9g, no envelope %.9g\n", kMode[MODE], what, bi, f, wa[f], wg[f]); return 1; }
    }
    // a looping voice's cursor is stored folded by both kernel forms and left unfolded by a per-frame walk of zero frames only
    if (!same_state(a.s, b.s) || !same_state(a.s, bs.s) || !same_state(a.s, as.s) || !same_state(a.s, c.s) || !same_env(a.es, b.es) || !same_env(a.es, bs.es) ||
        !same_env(a.es, as.es) || !same_env(a.es, c.es)) {
      std::printf("FAIL %s, %s: state after block %zu (%u frames): per frame idx %llu playing %u env %u n %u N %u value %.9g; chunk idx %llu playing %u env %u n %u N %u value %.9g; "
                  "closed form idx %llu playing %u env %u n %u N %u value %.9g\n", kMode[MODE], what, bi, frames,
                  (unsigned long long)a.s.idx, a.s.playing, a.es.state, a.es.n, a.es.N, a.es.value, (unsigned long long)b.s.idx, b.s.playing, b.es.state, b.es.n, b.es.N, b.es.value,
                  (unsigned long long)c.s.idx, c.s.playing, c.es.state, c.es.n, c.es.N, c.es.value);
      return 1;
    }
    if (gate_ref && !same_state(a.s, g)) {
      std::printf("FAIL %s, %s: state after block %zu: gate envelope idx %llu playing %u, no envelope idx %llu playing %u\n", kMode[MODE], what, bi,
                  (unsigned long long)a.s.idx, a.s.playing, (unsigned long long)g.idx, g.playing);
      return 1;
    }
    frame += frames;
  }
  return 0;
}

static groove_envelope_params env_of(double a, double d, double s, double r) { groove_envelope_params e; e.attack = a; e.decay = d; e.sustain = s; e.release = r; return e; }

template <int MODE>
static int mode_cases(int& cases) {
  int bad = 0;
  const Sample s300(300), s5000(5000), s7(7);
  const std::vector<uint32_t> split1 = {64, 37, 17, 256, 64, 37, 17, 256, 64, 37, 17, 256}, split2 = {101, 17, 256, 101, 17, 256, 101, 17, 256};
  const groove_envelope_params envs[] = {env_of(0.002, 0.003, 0.6, 0.005), env_of(0.0, 0.0, 0.0, 0.001), env_of(0.001, 0.0, 1.0, 1.0), env_of(0.0, 0.0, 1.0, 0.0),
                                         env_of(0.0005, 0.02, 0.3, 0.0101)};
  const uint32_t keys[] = {57, 69, 81, 105}; // an octave below the root (440 Hz), on it, an octave and three octaves above
  for (size_t ei = 0; ei < sizeof(envs) / sizeof(envs[0]); ++ei) {
    const EnvParams ep = derive_env(envs[ei], kSr);
    const bool gate = ei == 3;
    for (uint32_t key : keys) {
      const std::vector<Event> events = {{0, true, key}, {101, false, key}, {118, true, key}, {475, false, key}};
      for (const std::vector<uint32_t>* split : {&split1, &split2}) {
        bad += run<MODE>(s300, SamplerParams{0, 300, 440.0, 0.75f, 0u}, SampleLoop{0, 0}, ep, events, *split, gate, "300 frames, no loop"); ++cases;
        bad += run<MODE>(s5000, SamplerParams{0, 5000, 440.0, 0.5f, 0u}, SampleLoop{1000, 3000}, ep, events, *split, gate, "5,000 frames looped [1000, 3000)"); ++cases;
        bad += run<MODE>(s7, SamplerParams{0, 7, 440.0, 1.25f, 0u}, SampleLoop{3, 4}, ep, events, *split, gate, "a loop of one frame"); ++cases;
        bad += run<MODE>(s5000, SamplerParams{0, 5000, 440.0, 0.5f, 0u}, SampleLoop{1000, 3000}, sample_env_none(), events, *split, true, "no envelope"); ++cases;
        bad += run<MODE>(s300, SamplerParams{0, 300, 0.0, 0.5f, 1u}, SampleLoop{0, 0}, ep, events, *split, true, "a one-shot voice on an enveloped sample"); ++cases;
        if (bad) return bad;
      }
    }
  }
  // the sample's end against the release's end: key on the root (one frame per frame), note-on at frame 0, note-off at frame `off`, a
  // release of 41 frames from the plateau at 1: idle on frame off + 41; samples of off + 41 + d frames end on frame off + 41 + d
  const EnvParams rel = derive_env(env_of(0.0, 0.0, 1.0, 40.3 / kSr), kSr);
  if (env_frames(rel.release_len) != 41) { std::printf("FAIL: the release of the end cases is %u frames, not 41\n", env_frames(rel.release_len)); return 1; }
  for (uint32_t bl : {1u, 5u, 16u, 17u, 21u, 41u, 42u, 64u, 256u}) {
    for (uint32_t blocks_before = 1; blocks_before <= 3; ++blocks_before) {
      const uint32_t off = bl * blocks_before;
      for (int d = -2; d <= 2; ++d) {
        const uint32_t length = (uint32_t)((int)off + 41 + d);
        const Sample smp(length);
        const std::vector<Event> events = {{0, true, 69}, {off, false, 69}};
        std::vector<uint32_t> split((off + 41 + 4) / bl + 3, bl);
        bad += run<MODE>(smp, SamplerParams{0, length, 440.0, 0.75f, 0u}, SampleLoop{0, 0}, rel, events, split, false, "the sample's end beside the release's end"); ++cases;
        // and with the block boundary moved so that the idle frame is the block's last and the next block's first
        std::vector<uint32_t> last = {off, 42, 7}, first = {off, 41, 7}, before = {off, 40, 7};
        for (const std::vector<uint32_t>* sp : {&last, &first, &before})
          if (off <= 256) { bad += run<MODE>(smp, SamplerParams{0, length, 440.0, 0.75f, 0u}, SampleLoop{0, 0}, rel, events, *sp, false, "the idle frame at a block's edge"); ++cases; }
        if (bad) return bad;
      }
    }
  }
  return bad;
}

int main() {
  int cases = 0, bad = 0;
  bad += mode_cases<GROOVE_SAMPLE_NEAREST>(cases);
  bad += mode_cases<GROOVE_SAMPLE_LINEAR>(cases);
  bad += mode_cases<GROOVE_SAMPLE_CUBIC>(cases);
  if (bad) { std::printf("FAILED: %d of %d cases\n", bad, cases); return 1; }
  std::printf("ok: %d cases\n", cases);
  return 0;
}
