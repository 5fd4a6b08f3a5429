// groove_host.hpp — compiled host layer above the C ABI (include/groove_hip.h).
//
// The reference's host code is Rust; no Rust toolchain exists in the build image, so the
// host side that sits above the FFI is written in C++ and mirrors the reference's
// operator surface for this path, name for name:
//
//   Orchestrator::{add, patch, patch_chain_to_main_mixer, unpatch_all,
//                  connect_midi_downstream, tick, gather_audio, run, run_performance,
//                  update_sample_rate}      /root/reference/orchestration/src/orchestrator.rs
//                                           :136-142, 263-325, 472-490, 367-470, 788-877
//   Performance{sample_rate, worker}        orchestrator.rs:32-46
//   IsInstrument / IsEffect / IsController  proc-macros/src/entity.rs:29-139
//   IOHelper::send_performance_to_file      orchestration/src/helpers.rs:74-97
//
// Block semantics.  The reference evaluates the patch graph once per FRAME
// (gather_audio, orchestrator.rs:367-470); here the same post-order traversal runs once
// per BLOCK on device blocks, which is equivalent because entities never reference each
// other and events are block-granular already (tick(): handle_work once, then gather).
// A node's output is a device block with `lanes` lanes.  A WelshSynth with 8 voices is
// one entity whose voices are summed to ONE lane (the reference's Synthesizer sums its
// voice store); "batched" instruments (`sum_voices = false`) keep one lane per voice so
// that per-voice effect chains (BASELINE config #3) run as wide effect banks.  An effect
// sums ALL its sources, then transforms the sum once (orchestrator.rs:438-457, pinned by
// the fan-in test :1642-1668); sources with more lanes than the sink are lane-summed.
#pragma once
#include "../../include/groove_hip.h"
#include "../csrc/ctl_core.h" // the control links' route table (ctl_fx_route, ctl_bank_route) and value laws
#include <cstdint>
#include <memory>
#include <string>
#include <vector>
#include <map>

namespace groove_host {

using Uid = size_t;
constexpr Uid kMainMixerUid = 0; // MAIN_MIXER_UVID, orchestrator.rs:104, 543-546

struct StereoSample { float l, r; };

// Performance, orchestrator.rs:32-46 (the FIFO worker is a plain vector here).
struct Performance {
  uint32_t sample_rate = GROOVE_DEFAULT_SAMPLE_RATE;
  std::vector<StereoSample> worker;
};

// MusicalTime: 65,536 units per beat (src/mini/transport.rs:157-176, doc/designs/time.md:94-98).
struct MusicalTime {
  static constexpr uint64_t UNITS_IN_BEAT = 65536;
  uint64_t units = 0;
  static MusicalTime from_beats(double beats) { return {(uint64_t)(beats * UNITS_IN_BEAT + 0.5)}; }
  static uint64_t frames_to_units(double bpm, uint32_t sr, uint64_t frames) {
    return (uint64_t)((double)frames * bpm / 60.0 / (double)sr * (double)UNITS_IN_BEAT);
  }
  double beats() const { return (double)units / UNITS_IN_BEAT; }
};

class Orchestrator;
class ControlSource;
class ControlTrip;

class Entity {
 public:
  virtual ~Entity() = default;
  Uid uid = 0;
  std::string name;
  virtual bool is_instrument() const { return false; }
  virtual bool is_effect() const { return false; }
  virtual bool is_controller() const { return false; }
  // the source side of `controls` links, if the entity is a controller DEVICE (an LFO, a signal passthrough)
  virtual ControlSource* control_source() { return nullptr; }
  virtual ControlTrip* control_trip() { return nullptr; } // the entity itself, if it is a ControlTrip
};

// #[derive(Control)] kebab-case names of the effects' parameters (proc-macros/src/control.rs:127-131, 165) -> groove_control_index; -1: none.
inline int fx_control_index_for_name(const std::string& name) {
  static const std::pair<const char*, int> table[] = {
      {"ceiling", GROOVE_CTL_FX_CEILING}, {"bits", GROOVE_CTL_FX_BITS}, {"bits-to-crush", GROOVE_CTL_FX_BITS},
      {"cutoff", GROOVE_CTL_FX_CUTOFF}, {"q", GROOVE_CTL_FX_Q}, {"passband-ripple", GROOVE_CTL_FX_PASSBAND_RIPPLE},
      {"attenuation", GROOVE_CTL_FX_ATTENUATION}, {"wet-dry-mix", GROOVE_CTL_FX_WET}, {"threshold", GROOVE_CTL_FX_THRESHOLD}};
  for (auto& t : table) if (name == t.first) return t.second;
  return -1;
}
// The same for the controls the library's banks expose, per kind of bank (include/groove_types.h: each kind has its own indices).
//   Welsh: the `dca` field gives dca-gain / dca-pan; the filter's cutoff is the one Welsh voice parameter the reference's demos automate
//   on effects.  FM: dca-gain / dca-pan, depth and beta (`ratio` has no law and no control).  Sampler and drumkit: gain.  Toy: the
//   ToyInstrument is an FM bank of one voice behind a Dca — its gain and pan, as before (through groove_bank_set_param, which serves its
//   bank now; a deliberate exception to `anything else: -1`).  Anything else: -1.
enum class BankControls { NONE, WELSH, FM, SAMPLER, TOY };
inline int bank_control_index_for_name(BankControls kind, const std::string& name) {
  static const std::pair<const char*, int> welsh[] = {
      {"dca-gain", GROOVE_CTL_WELSH_DCA_GAIN}, {"gain", GROOVE_CTL_WELSH_DCA_GAIN}, {"dca-pan", GROOVE_CTL_WELSH_DCA_PAN}, {"pan", GROOVE_CTL_WELSH_DCA_PAN},
      {"filter-cutoff", GROOVE_CTL_WELSH_CUTOFF}, {"cutoff", GROOVE_CTL_WELSH_CUTOFF}};
  static const std::pair<const char*, int> fm[] = {
      {"dca-gain", GROOVE_CTL_FM_DCA_GAIN}, {"gain", GROOVE_CTL_FM_DCA_GAIN}, {"dca-pan", GROOVE_CTL_FM_DCA_PAN}, {"pan", GROOVE_CTL_FM_DCA_PAN},
      {"depth", GROOVE_CTL_FM_DEPTH}, {"beta", GROOVE_CTL_FM_BETA}};
  switch (kind) {
    case BankControls::WELSH: for (auto& t : welsh) if (name == t.first) return t.second; return -1;
    case BankControls::FM: for (auto& t : fm) if (name == t.first) return t.second; return -1;
    case BankControls::TOY: for (size_t i = 0; i < 4; ++i) if (name == fm[i].first) return fm[i].second; return -1;
    case BankControls::SAMPLER: return name == "gain" ? (int)GROOVE_CTL_SAMPLER_GAIN : -1;
    default: return -1;
  }
}
// ... of a project file's device kind (project.cpp)
inline BankControls bank_controls_of_device(const std::string& device_kind) {
  if (device_kind == "welsh" || device_kind == "welsh-raw") return BankControls::WELSH;
  if (device_kind == "fm-synthesizer") return BankControls::FM;
  if (device_kind == "drumkit" || device_kind == "sampler") return BankControls::SAMPLER;
  if (device_kind == "toy-instrument") return BankControls::TOY;
  return BankControls::NONE;
}
// The controls of an instrument a BANK link reaches (groove_ctl_bank_link_create / groove_ctl_bank_trip_create, which have the last word):
// every control its kind of bank has.  The toy instrument's gain and pan keep the host path: its names resolve because project files use
// them (tests/test_project_controllers.py), nothing more is built for it.
inline bool bank_control_device_linkable(BankControls kind, int index) {
  switch (kind) {
    case BankControls::WELSH: return groove::ctl_bank_route(groove::BANK_WELSH, (uint32_t)index) != groove::CTL_ROUTE_NONE;
    case BankControls::FM: return groove::ctl_bank_route(groove::BANK_FM, (uint32_t)index) != groove::CTL_ROUTE_NONE;
    case BankControls::SAMPLER: return groove::ctl_bank_route(groove::BANK_SAMPLER, (uint32_t)index) != groove::CTL_ROUTE_NONE;
    default: return false;
  }
}
// How a control link onto this parameter of this kind of effect can stay on the device (ctl_core.h: ctl_fx_route; the creates have the
// last word).  linkable: the parameters whose device form IS the value, on the kind whose kernels read them (groove_ctl_link_create).
// derived: a filter's cutoff, q and passband-ripple, through a filter link, where the orchestrator has been asked to
// (Orchestrator::set_filter_links_on_device).  wet: wet-dry-mix onto every kind but the Mixer, which launches nothing
// (groove_ctl_wet_link_create / groove_ctl_wet_trip_create), where asked to (Orchestrator::set_wet_links_on_device).
inline groove::CtlRoute fx_control_route(uint32_t fx_kind, int index) { return groove::ctl_fx_route(fx_kind, (uint32_t)index); }
inline bool fx_control_device_linkable(uint32_t fx_kind, int index) {
  return fx_control_route(fx_kind, index) == groove::CTL_ROUTE_FLOAT || fx_control_route(fx_kind, index) == groove::CTL_ROUTE_UINT;
}
inline bool fx_control_device_wet(uint32_t fx_kind, int index) { return fx_control_route(fx_kind, index) == groove::CTL_ROUTE_WET; }
inline bool fx_control_device_derived(uint32_t fx_kind, int index) { return fx_control_route(fx_kind, index) == groove::CTL_ROUTE_DERIVED; }

// IsInstrument: Generates<StereoSample> + Ticks + HandlesMidi.
class Instrument : public Entity {
 public:
  bool is_instrument() const override { return true; }
  virtual uint32_t lanes() const = 0;          // lanes of the block it outputs
  virtual groove_block* output() = 0;
  virtual int tick(uint32_t frames) = 0;       // render `frames` into output()
  // Does every tick / finish write the whole of output() anew?  Then a chain that is the block's only listener may
  // transform it where it lies; a source that keeps a constant block (ToyAudioSource) must be copied first.
  virtual bool output_is_scratch() const { return true; }
  // HandlesMidi::handle_midi_message (note on/off only on this path)
  virtual void note_on(uint8_t key, uint8_t velocity, uint64_t now_frame) = 0;
  virtual void note_off(uint8_t key, uint8_t velocity, uint64_t now_frame) = 0;
  // Render-ahead protocol of the offline runs (Orchestrator::run / run_performance): render_ahead()
  // starts the NEXT block's render beside whatever the ctx stream does (groove_bank_render_async)
  // without disturbing output(); finish() makes that block the current output().
  virtual bool supports_render_ahead() const { return false; }
  virtual bool render_ahead_pays() const { return true; }
  virtual int render_ahead(uint32_t frames) { (void)frames; return 0; }
  virtual int finish(uint32_t frames) { return tick(frames); }
  // The library bank behind the instrument, if all it does is render that bank: patched STRAIGHT into the main mixer and heard by
  // nothing else, such an instrument needs no voice block at all — the orchestrator renders it fused onto the bus
  // (Orchestrator::gather_audio's fast path).
  virtual groove_bank* fused_bank() { return nullptr; }
  virtual BankControls bank_controls() const { return BankControls::NONE; } // which controls that bank's kind has
  // Controllable (proc-macros/src/control.rs:171-249: generated for EVERY entity, instruments included): a ControlTrip whose target
  // is an instrument drives these (entities/src/controllers/control_trip.rs:184-254).  -1 / 1: no such control.
  virtual int control_index_for_name(const std::string&) const { return -1; }
  virtual int control_set_param(uint32_t index, double value01) { (void)index; (void)value01; return 1; }
};

// IsEffect: TransformsAudio.
class Effect : public Entity {
 public:
  bool is_effect() const override { return true; }
  virtual uint32_t lanes() const = 0;
  virtual int transform_audio(groove_block* inout, uint32_t frames) = 0;
  virtual groove_fx* library_fx() { return nullptr; } // the library effect behind it, if it is one (chains of those are fused)
  virtual int control_set_param(uint32_t index, double value01) { (void)index; (void)value01; return 1; }
  virtual int control_index_for_name(const std::string&) const { return -1; }
};

// IsController: Controls (update_time / work / is_finished), src/mini/transport.rs:116-151.
struct MidiEvent { uint8_t channel, key, velocity; bool on; };
class Controller : public Entity {
 public:
  bool is_controller() const override { return true; }
  // events that fall inside [start, end) musical-time units, appended to `out`
  virtual void work(uint64_t start_units, uint64_t end_units, std::vector<MidiEvent>& out,
                    Orchestrator& o) = 0;
  virtual bool is_finished(uint64_t end_units) const = 0;
  virtual uint64_t end_units() const = 0;
  virtual void skip_to_start() {}
};

// ---- concrete entities -------------------------------------------------------------------
// A synth = ONE patch + a voice store (first-idle allocation, A.6); voices summed to 1 lane.
class VoiceBankInstrument : public Instrument {
 public:
  VoiceBankInstrument(groove_ctx* ctx, groove_bank* bank, BankControls controls, uint32_t voices, bool sum_voices,
                      double release_seconds, bool one_voice_per_key);
  ~VoiceBankInstrument() override;
  uint32_t lanes() const override { return sum_voices_ ? 1 : voices_; }
  groove_block* output() override { return sum_voices_ ? summed_ : block_; }
  int tick(uint32_t frames) override;
  bool supports_render_ahead() const override { return true; }
  // A bank the library renders time-parallel (one wavefront per voice: ~20 us per block) is shorter than what the
  // side-stream hand-over costs (event packets, a cross-queue wait): render-ahead only pays for the serial forms.
  bool render_ahead_pays() const override { return !short_render_; }
  int render_ahead(uint32_t frames) override;
  int finish(uint32_t frames) override;
  void note_on(uint8_t key, uint8_t velocity, uint64_t now_frame) override;
  void note_off(uint8_t key, uint8_t velocity, uint64_t now_frame) override;
  groove_bank* bank() { return bank_; }
  groove_bank* fused_bank() override { return bank_; }
  BankControls bank_controls() const override { return controls_; }
  // the controls the library's banks expose (include/groove_types.h GROOVE_CTL_WELSH_*, _FM_*, _SAMPLER_GAIN: by kind of bank), for every
  // voice of the instrument
  int control_index_for_name(const std::string& name) const override;
  int control_set_param(uint32_t index, double value01) override;
  uint32_t last_allocated_voice() const { return last_voice_; }
 private:
  groove_ctx* ctx_;
  groove_bank* bank_;
  BankControls controls_;
  uint32_t voices_;
  bool sum_voices_;
  double release_seconds_;
  bool per_key_; // Drumkit: one voice per note (A.10)
  bool short_render_ = false;
  groove_block* block_ = nullptr;
  groove_block* block_next_ = nullptr; // render-ahead: the block being rendered while block_ is consumed
  groove_block* summed_ = nullptr;
  std::vector<int> key_of_voice_;        // -1 = free
  std::vector<uint64_t> busy_until_;     // frame until which the voice may still sound
  std::vector<uint64_t> started_;
  uint32_t last_voice_ = 0;
};

// ToyAudioSource{level}: constant-level instrument used by the reference's mix-bus tests.
class ToyAudioSource : public Instrument {
 public:
  ToyAudioSource(groove_ctx* ctx, double level);
  ~ToyAudioSource() override;
  uint32_t lanes() const override { return 1; }
  groove_block* output() override { return block_; }
  int tick(uint32_t frames) override;
  bool supports_render_ahead() const override { return true; } // constant block: nothing to render
  bool output_is_scratch() const override { return false; }
  void note_on(uint8_t, uint8_t, uint64_t) override {}
  void note_off(uint8_t, uint8_t, uint64_t) override {}
 private:
  groove_ctx* ctx_;
  float level_;
  groove_block* block_ = nullptr;
  std::vector<float> host_;
};

class FxEffect : public Effect {
 public:
  FxEffect(groove_ctx* ctx, uint32_t kind, const groove_fx_params* p, uint32_t lanes);
  ~FxEffect() override;
  uint32_t lanes() const override { return lanes_; }
  int transform_audio(groove_block* inout, uint32_t frames) override;
  groove_fx* library_fx() override { return fx_; }
  int control_set_param(uint32_t index, double value01) override;
  int control_index_for_name(const std::string& name) const override;
  uint32_t kind() const { return kind_; }
 private:
  groove_ctx* ctx_;
  groove_fx* fx_ = nullptr;
  uint32_t kind_;
  uint32_t lanes_;
};

// Timer: finishes after N beats (groove-toys Timer, orchestrator.rs:1408-1415).
class Timer : public Controller {
 public:
  explicit Timer(double beats) : end_(MusicalTime::from_beats(beats).units) {}
  void work(uint64_t, uint64_t, std::vector<MidiEvent>&, Orchestrator&) override {}
  bool is_finished(uint64_t end_units) const override { return end_units >= end_; }
  uint64_t end_units() const override { return end_; }
 private:
  uint64_t end_;
};

// Sequencer: notes at musical-time positions on a MIDI channel (settings/src/songs.rs:210-249
// inserts pattern notes; the beat sequencer finishes at the end of its last full measure).
class Sequencer : public Controller {
 public:
  void insert(uint8_t channel, uint8_t key, double start_beat, double duration_beats);
  void set_end_beats(double beats) { end_ = MusicalTime::from_beats(beats).units; explicit_end_ = true; }
  void work(uint64_t start_units, uint64_t end_units, std::vector<MidiEvent>& out, Orchestrator&) override;
  bool is_finished(uint64_t end_units) const override { return end_units >= end_; }
  uint64_t end_units() const override { return end_; }
 private:
  struct Ev { uint64_t at; uint8_t channel, key; bool on; };
  std::vector<Ev> events_;
  uint64_t end_ = 0;
  bool explicit_end_ = false;
};

// ControlTrip: automation of one Controllable parameter along a path of steps
// (entities/src/controllers/control_trip.rs:7-26, 99-142, 257-264).
struct ControlStep {
  enum Kind { FLAT, SLOPE, LOGARITHMIC, EXPONENTIAL, TRIGGERED } kind = FLAT;
  double start = 0.0, end = 0.0; // FLAT uses start as its value
  double beats = 1.0;            // duration of this step
};
// A trip works through Orchestrator::control_effect — one groove_fx_set_param, with its host wait, per block in which the value moves —
// unless the orchestrator has made it DEVICE-RESIDENT when the performance started (Orchestrator::set_trips_on_device, skip_to_start):
// then its steps live in the library (groove_ctl_trip_create) and work() only names the block's start time (Orchestrator::control_link).
class ControlTrip : public Controller {
 public:
  ControlTrip(Uid target, uint32_t control_index, double start_beat) : target_(target), index_(control_index), start_(start_beat) {}
  ~ControlTrip() override { set_device_link(nullptr); }
  ControlTrip* control_trip() override { return this; }
  void add_step(const ControlStep& s) { steps_.push_back(s); }
  Uid target() const { return target_; }
  uint32_t control_index() const { return index_; }
  double start_beat() const { return start_; }
  const std::vector<ControlStep>& steps() const { return steps_; }
  bool on_device() const { return dev_ != nullptr; }
  // takes ownership; destroys the link it had.  on_instrument: a bank link — its applies are never held back (Orchestrator::control_link)
  void set_device_link(groove_ctl_link* link, bool on_instrument = false);
  void work(uint64_t start_units, uint64_t end_units, std::vector<MidiEvent>& out, Orchestrator& o) override;
  bool is_finished(uint64_t end_units) const override { return end_units >= end_units_(); }
  uint64_t end_units() const override { return end_units_(); }
  static double value_at(const ControlStep& s, double t01);
 private:
  uint64_t end_units_() const;
  Uid target_;
  uint32_t index_;
  double start_;
  std::vector<ControlStep> steps_;
  double last_sent_ = -1.0;
  groove_ctl_link* dev_ = nullptr; // device-resident: the trip link
  bool dev_instrument_ = false;    // device-resident: the link's target is an instrument's bank
  int last_step_ = -1;             // device-resident: the step of the last apply (a FLAT step is applied once)
};

// ---- controller devices ------------------------------------------------------------------------
// The source side of the project's `controls` links (ControllerSettings, settings/src/controllers.rs:103-112): worked once per block,
// before gather_audio, in the order the entities were added (handle_work, orchestrator.rs:631-708).  A link onto a parameter whose device
// form is the value lives in the library (groove_ctl_link: no host wait); an LFO's link onto anything else goes through
// Orchestrator::control_effect with the same law evaluated on the host in f64 (docs/DSP_SPEC.md section 13).
class ControlSource {
 public:
  virtual ~ControlSource();
  struct Link { groove_ctl_link* dev; Uid target; uint32_t index; bool instrument = false; }; // dev == nullptr: through Orchestrator::control_effect; instrument: dev is a bank link
  virtual groove_ctl_source source_desc() const = 0;
  void add_link(const Link& l) { links_.push_back(l); }
  const std::vector<Link>& link_list() const { return links_; }
  size_t links() const { return links_.size(); }
  void work_controls(Orchestrator& o, uint64_t at_frame);
  void reset_controls(); // Resets::reset: a signal source forgets what it captured
 protected:
  virtual double host_value01(uint64_t at_frame, uint32_t sample_rate) const { (void)at_frame; (void)sample_rate; return 0.0; }
  std::vector<Link> links_;
};

// LfoController{waveform, frequency} (settings/src/controllers.rs:108-109).
class LfoController : public Controller, public ControlSource {
 public:
  LfoController(uint32_t waveform, float duty, double frequency_hz) : waveform_(waveform), duty_(duty), frequency_(frequency_hz) {}
  ControlSource* control_source() override { return this; }
  void work(uint64_t start_units, uint64_t end_units, std::vector<MidiEvent>& out, Orchestrator& o) override;
  bool is_finished(uint64_t) const override { return true; } // an LFO keeps no performance going
  uint64_t end_units() const override { return 0; }
  groove_ctl_source source_desc() const override;
 protected:
  double host_value01(uint64_t at_frame, uint32_t sample_rate) const override;
 private:
  uint32_t waveform_;
  float duty_;
  double frequency_;
};

// SignalPassthroughController (settings/src/controllers.rs:110-111): an effect that is the identity on its one lane (so that it can sit in
// a patch cable), and a controller whose value is the last sample it has passed on — what a sidechain is built from.
class SignalPassthrough : public Effect, public ControlSource {
 public:
  explicit SignalPassthrough(uint32_t law = GROOVE_CTL_LAW_BIPOLAR) : law_(law) {}
  ControlSource* control_source() override { return this; }
  uint32_t lanes() const override { return 1; }
  int transform_audio(groove_block* inout, uint32_t frames) override; // the block is only read
  groove_ctl_source source_desc() const override;
 private:
  uint32_t law_;
};

// ---- the orchestrator ----------------------------------------------------------------------
class Orchestrator {
 public:
  Orchestrator(int device, uint32_t sample_rate, double bpm);
  ~Orchestrator();
  Orchestrator(const Orchestrator&) = delete;

  groove_ctx* ctx() { return ctx_; }
  const std::string& last_error() const { return err_; }
  uint32_t sample_rate() const { return sr_; }
  double bpm() const { return bpm_; }
  void set_bpm(double bpm) { bpm_ = bpm; } // Clock::set_bpm (orchestrator.rs:888-890)
  int update_sample_rate(uint32_t hz);

  // Orchestrator::add (orchestrator.rs:136-142): takes ownership, returns the Uid.
  Uid add(std::unique_ptr<Entity> e);
  Entity* get(Uid uid);
  // Orchestrator::patch (orchestrator.rs:263-304): source output → sink input.  0 on success.
  int patch(Uid source, Uid sink);
  int patch_chain_to_main_mixer(const std::vector<Uid>& uids);
  void unpatch_all();
  // Orchestrator::connect_midi_downstream (orchestrator.rs:472-490)
  int connect_midi_downstream(Uid receiver, uint8_t channel);

  // Orchestrator::tick (orchestrator.rs:856-877): events for this block, gather_audio, clock
  // advance.  Writes frames into `out` and returns ticks_completed (< frames ends the run).
  int tick(StereoSample* out, uint32_t frames, uint32_t* ticks_completed);
  // Orchestrator::gather_audio (orchestrator.rs:367-470) for one block into the device bus.
  int gather_audio(uint32_t frames);
  // Orchestrator::run / run_performance (orchestrator.rs:788-846).  `run` keeps the final
  // partial block, `run_performance` drops it (quirk, :827-836).
  int run(uint32_t buffer_frames, std::vector<StereoSample>& out);
  int run_performance(uint32_t buffer_frames, Performance& perf);
  void skip_to_start();
  // Offline runs render the instruments of block b+1 on the library's side streams while the effect
  // graph of block b runs (same samples; DESIGN.md "Render-ahead").  On by default; off = block by block.
  // 0 = block by block, 1 = where it pays (default), 2 = whenever the graph allows it (tests).
  void set_render_ahead(int mode) { render_ahead_ = mode; }
  // Instruments patched straight into the main mixer (and heard by nothing else) render FUSED onto the bus — no voice block, one
  // launch for all of them when they are small (groove_banks_render_mix_deferred) — instead of block by block through the mixer's
  // accumulator.  Same sum to fp32 rounding.  On by default; off = the entity-boundary walk for every source (tests, A/B).
  void set_fused_direct(bool on) { fused_direct_ = on; }
  // ControlTrip -> effect parameter.  While the controllers are run one block ahead of the effects
  // the update is held back until the effects have processed the current block.
  int control_effect(Uid target, uint32_t index, double value01);
  // Orchestrator::link_control (orchestrator.rs:1279-1294): `source` is a controller device, `param` one of the target's control names.
  // 0: linked; 1: error; 2: dropped — a signal source onto a parameter only the host can derive would need a download per block
  // (last_error() says so; the project loader turns it into a warning).
  int link_control(Uid source, Uid target, const std::string& param);
  // A link onto a filter's cutoff, q or passband-ripple derives the coefficients on the device (groove_ctl_filter_link_create: no host wait)
  // instead of going through control_effect once per block — and so a signal source onto one of them is linked (0) where it is dropped (2)
  // with the switch off.  Off by default; it affects the links made after it is set.
  void set_filter_links_on_device(bool on) { filter_links_on_device_ = on; }
  bool filter_links_on_device() const { return filter_links_on_device_; }
  // A device-resident link's value for the block at `at`: applied now, or — like control_effect — held back while the controllers
  // are run one block ahead of the effects.  `at` is the block's first frame (an LFO or signal link: groove_ctl_link_apply) or, for a
  // trip link, its start in musical-time units (groove_ctl_trip_apply).
  // A link onto an INSTRUMENT (a bank link) is applied at once even then, as control_effect's instrument branch is: the instruments are
  // the block being sequenced.
  int control_link(groove_ctl_link* link, uint64_t at, bool trip_units = false, bool on_instrument = false);
  // ControlTrips onto effect parameters the library can reach (groove_ctl_trip_create) stay on the device: no groove_fx_set_param, and so
  // no host wait, per automated block.  Decided for all trips at once when a performance starts (skip_to_start): a trip is device-resident
  // iff the switch is on, its target is an effect, the library accepts the parameter for that kind, and EVERY other control onto the same
  // effect (trips and `controls` links) is device-resident too — one host-path groove_fx_set_param re-uploads the host's stale copy of the
  // parameter the device trip owns.  Everything else (instruments, wet-dry-mix) takes the host path unchanged.  Off by default.
  void set_trips_on_device(bool on) { trips_on_device_ = on; }
  // Controls onto an effect's wet-dry-mix stay on the device (groove_ctl_wet_link_create, groove_ctl_wet_trip_create).  link_control then
  // links an LFO or a signal-passthrough source onto it there — a sidechain onto the mix is linked (0) where it is dropped (2) with the
  // switch off — and place_trips counts a trip onto it as reachable when set_trips_on_device is on as well, so that it no longer forces
  // the effect's other trips onto the host.  Alone it moves no trip.  Off by default; it affects the links made after it is set.
  void set_wet_links_on_device(bool on) { wet_links_on_device_ = on; }
  bool wet_links_on_device() const { return wet_links_on_device_; }
  // The library's groove_set_fx_wet_reverb_run: a partly wet reverb (and one with a live wet link) keeps the fused run's forms.  Off by default.
  int set_wet_reverb_run(bool on);
  bool wet_reverb_run() const;
  bool trips_on_device() const { return trips_on_device_; }
  // Controls onto a Welsh synth's dca-gain / gain, dca-pan / pan or filter-cutoff / cutoff — and onto an FM synth's gain, pan, depth or beta
  // and a sampler's or drumkit's gain (bank_control_device_linkable) — stay on the device (groove_ctl_bank_trip_create,
  // groove_ctl_bank_link_create): no groove_bank_set_param — a re-derivation, a re-plan and a re-upload of the bank, with their host waits —
  // per automated block.  Off by default and independent of set_trips_on_device.  Trips are placed when a performance starts
  // (skip_to_start), by the effects' rule per instrument: if ANY control reaches the instrument through the host — a parameter or a bank
  // the library refuses, an LFO link without a device link, a create that fails — ALL its trips stay on the host, because a host
  // set_param re-uploads the host's copy over the device's value.  LFO `controls` links are made by link_control, so the switch has to be
  // set before the project's controls are linked.  A signal-passthrough source onto an instrument stays dropped (status 2) either way:
  // in the render-ahead walk the instruments of block b + 1 render before block b's effects have captured anything, so the reference's
  // "value captured in the previous tick" cannot be honoured there (the library call takes signal sources; the host layer does not use it).
  void set_instrument_controls_on_device(bool on) { instrument_controls_on_device_ = on; }
  bool instrument_controls_on_device() const { return instrument_controls_on_device_; }
  // Samplers and drumkits keep the channels of two-channel sample files (groove_sampler_create_stereo) instead of averaging them before
  // upload.  Read when a project is instantiated (project.hpp instantiate).  Off by default: a stereo file is then the mean of its channels.
  void set_stereo_samples(bool on) { stereo_samples_ = on; }
  bool stereo_samples() const { return stereo_samples_; }
  // How the sampler and drumkit banks added from here on read their samples between frames (groove_bank_set_sample_interpolation: a
  // groove_sample_interpolation), every bank a project's instantiation creates among them.  GROOVE_SAMPLE_NEAREST by default: the
  // reference's reading.  An unknown mode is refused (last_error) and changes nothing.
  int set_sample_interpolation(uint32_t mode);
  uint32_t sample_interpolation() const { return sample_interpolation_; }
  // A `sampler` a project's instantiation creates from here on takes the forward sustain loop its WAV file carries (project.hpp
  // read_wav_loop; groove_bank_set_sample_loops): a held note then outlasts the file.  Drumkits never do: their voices are one-shots.
  // Off by default: a sampler plays its file once, as the reference does.
  void set_sample_loops(bool on) { sample_loops_ = on; }
  bool sample_loops() const { return sample_loops_; }
  // A `sampler` created from here on gets this amplitude envelope on its sample (groove_bank_set_sample_envelopes: an attack, and a
  // release tail after note-off) and is busy until note-off + the envelope's release, the rule Welsh and FM synths follow: the next
  // note takes another voice while the tail sounds.  Drumkits never do: their voices are one-shots.  NULL: none, the default — a
  // sampler voice starts at full level and stops at its note-off, as the reference's does.  A negative or non-finite time or a sustain
  // outside [0, 1] is refused (last_error) and changes nothing.
  int set_sample_envelope(const groove_envelope_params* env);
  const groove_envelope_params* sample_envelope() const { return sample_envelope_on_ ? &sample_envelope_ : nullptr; }
  uint64_t sequencing_frame() const { return sequencing_frame_; } // first frame of the block whose controllers are being worked
  uint64_t clock_frames() const { return frames_; }
  uint64_t performance_frames() const; // ceil(end of the last controller)

  // IOHelper::send_performance_to_file (helpers.rs:74-97): 16-bit stereo PCM WAV, quantised on the device.
  int send_performance_to_file(const Performance& perf, const std::string& path);

  int fail(const std::string& msg) { err_ = msg; return 1; }

 private:
  struct Node {
    std::unique_ptr<Entity> entity;
    std::vector<Uid> sources;          // audio_sink_uid_to_source_uids
    groove_block* accum = nullptr;     // effect input sum / output block
    uint32_t accum_lanes = 0;
  };
  int eval(Uid uid, uint32_t frames, groove_block** out_block, uint32_t* out_lanes);
  int ensure_accum(Node& n, uint32_t lanes);
  uint32_t fanout(Uid uid); // how many sinks hear this node
  // handle_work + broadcast_midi_messages for the block [at_frame, at_frame + frames)
  void sequence_block(uint64_t at_frame, uint32_t frames);
  // the instruments the main mixer hears, if every one of them is heard exactly once and can render ahead
  bool ahead_instruments(std::vector<Instrument*>& out);
  // the main mixer's sources split into banks that can render fused onto the bus and the rest (chains, toy sources, shared instruments)
  bool direct_banks(std::vector<groove_bank*>& direct, std::vector<Uid>& rest);
  int tick_ahead(StereoSample* out, uint32_t frames, uint32_t* ticks_completed, const std::vector<Instrument*>& instruments);
  int tick_offline(StereoSample* out, uint32_t frames, uint32_t* ticks_completed);

  groove_ctx* ctx_ = nullptr;
  uint32_t sr_;
  double bpm_;
  std::string err_;
  std::vector<Node> nodes_;
  std::vector<uint32_t> fanout_; // per node, rebuilt after a patch change
  bool fanout_valid_ = false;
  std::multimap<uint8_t, Uid> midi_receivers_;
  float* bus_ = nullptr; // device [block][2]
  uint32_t bus_frames_ = 0;
  uint64_t frames_ = 0;
  bool performing_ = false;
  int render_ahead_ = 1;
  bool fused_direct_ = true;
  bool filter_links_on_device_ = false;
  bool trips_on_device_ = false;
  bool wet_links_on_device_ = false;
  bool instrument_controls_on_device_ = false;
  bool stereo_samples_ = false;
  bool sample_loops_ = false;
  bool sample_envelope_on_ = false;
  groove_envelope_params sample_envelope_{};
  uint32_t sample_interpolation_ = GROOVE_SAMPLE_NEAREST;
  void place_trips(); // skip_to_start: which trips are device-resident for this performance
  bool ahead_primed_ = false;   // the current block's instruments were rendered by the previous tick_ahead
  bool ahead_eval_ = false;     // eval(): instruments already hold their block
  bool deferring_ = false;      // controllers are being run for the NEXT block
  struct Deferred { Uid target; uint32_t index; double value; groove_ctl_link* link; uint64_t at; bool trip_units; }; // link set: a device-resident link's apply at `at`
  std::vector<Deferred> deferred_;
  uint64_t sequencing_frame_ = 0;
};

// BusStation (src/mini/bus_station.rs:7-52): which track sends how much of its signal to which aux
// track.  At the reference commit it is a routing table only (nothing renders through it yet), so
// this is the table, with the behaviour of its code and unit test (:55-140): adding a route appends
// (the test's "should replace the prior one" only counts tracks; the code pushes, so does this),
// removing a route drops every route to that aux and leaves the track's (possibly empty) list in
// place, removing a track's sends leaves an empty list for it.
struct BusRoute { uint32_t aux_track_uid; double amount; };
class BusStation {
 public:
  void add_send_route(uint32_t track_uid, const BusRoute& route) {
    send_routes_[track_uid].push_back(route);
  }
  void remove_send_route(uint32_t track_uid, uint32_t aux_track_uid) {
    auto it = send_routes_.find(track_uid);
    if (it == send_routes_.end()) return;
    std::vector<BusRoute>& routes = it->second;
    for (size_t i = 0; i < routes.size();)
      if (routes[i].aux_track_uid == aux_track_uid) routes.erase(routes.begin() + (long)i); else ++i;
  }
  void remove_track_sends(uint32_t track_uid) { send_routes_[track_uid].clear(); }
  const std::vector<BusRoute>* sends_for(uint32_t track_uid) const {
    auto it = send_routes_.find(track_uid);
    return it == send_routes_.end() ? nullptr : &it->second;
  }
  size_t tracks() const { return send_routes_.size(); }
 private:
  std::map<uint32_t, std::vector<BusRoute>> send_routes_;
};

} // namespace groove_host
