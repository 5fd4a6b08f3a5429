// groove-cli-hip — offline renderer, the GPU-path counterpart of the reference's `groove-cli`
// (/root/reference/src/bin/groove-cli.rs:24-53 args, :56-158 main; gated at the reference commit).
//
//   groove-cli-hip [--wav] [--assets DIR] [--device N] [--synthetic-kit] [--device-filter-links] [--device-trips] [--device-instrument-controls] [--device-wet-links] [--wet-reverb-run] [--stereo-samples] [--sample-interpolation nearest|linear|cubic] [--sample-loops] [--sample-envelope A,D,S,R] [--quiet] [--perf] [--debug] FILE...
//
// --device-filter-links: `controls` onto a filter's cutoff, q or passband-ripple stay on the device (Orchestrator::set_filter_links_on_device),
// a signal source's among them, which are dropped with a warning otherwise.
// --device-trips: control trips onto effect parameters the library can reach stay on the device (Orchestrator::set_trips_on_device): no
// host wait per automated block.
// --device-instrument-controls: control trips and LFO `controls` onto a Welsh synth's dca-gain, dca-pan or filter-cutoff, an FM synth's gain, pan, depth or beta, a sampler's or drumkit's gain stay on the device
// (Orchestrator::set_instrument_controls_on_device): no re-plan and re-upload of the synth's bank per automated block.
//
// --device-wet-links: `controls` onto an effect's wet-dry-mix stay on the device (Orchestrator::set_wet_links_on_device), a signal source's
// among them; with --device-trips, control trips onto it do too.
// --wet-reverb-run: a partly wet reverb keeps the fused run's kernel forms (Orchestrator::set_wet_reverb_run; same bits).
// --stereo-samples: samplers and drumkits keep the channels of two-channel sample files (Orchestrator::set_stereo_samples); without it a
// stereo file is the mean of its channels.
// --sample-interpolation nearest|linear|cubic: how samplers and drumkits read their samples between frames
// (Orchestrator::set_sample_interpolation); nearest, the reference's reading, by default.
// --sample-loops: a sampler whose WAV file carries a forward sustain loop (`smpl` chunk) repeats it while a note is held
// (Orchestrator::set_sample_loops); without it a sampler plays its file once.
// --sample-envelope A,D,S,R: samplers get an amplitude envelope — attack, decay in seconds, sustain 0..1, release in seconds — so a
// note fades in and has a release tail after its note-off (Orchestrator::set_sample_envelope); without it a sampler voice starts at
// full level and stops at its note-off.  Drumkits get none.
//
// For each project file: SongSettings::new_from_project_file → instantiate → update_sample_rate(44100)
// → run_performance(buffer) → (with --wav) send_performance_to_file(<input with .json5/.json → .wav>).
#include "project.hpp"
#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace groove_host;

static std::string wav_name(const std::string& in) {
  // groove-cli.rs:144-148 rewrites ".json5" → ".wav"; the shipped demo is ".json" (SURVEY F6), so accept both
  for (const char* ext : {".json5", ".json"}) {
    const size_t n = std::strlen(ext);
    if (in.size() > n && in.compare(in.size() - n, n, ext) == 0) return in.substr(0, in.size() - n) + ".wav";
  }
  return in + ".wav";
}

int main(int argc, char** argv) {
  bool wav = false, quiet = false, perf = false, debug = false, synthetic = false, filter_links = false, device_trips = false, instrument_controls = false, wet_links = false, wet_run = false, stereo_samples = false, sample_loops = false;
  int device = 0;
  uint32_t sample_interpolation = GROOVE_SAMPLE_NEAREST;
  bool sample_envelope_on = false;
  groove_envelope_params sample_envelope{};
  std::string assets = "assets";
  std::vector<std::string> inputs;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    if (a == "--wav" || a == "-w") wav = true;
    else if (a == "--quiet" || a == "-q") quiet = true;
    else if (a == "--perf" || a == "-p") perf = true;
    else if (a == "--debug" || a == "-d") debug = true;
    else if (a == "--synthetic-kit") synthetic = true;
    else if (a == "--device-filter-links") filter_links = true;
    else if (a == "--device-trips") device_trips = true;
    else if (a == "--device-instrument-controls") instrument_controls = true;
    else if (a == "--device-wet-links") wet_links = true;
    else if (a == "--wet-reverb-run") wet_run = true;
    else if (a == "--stereo-samples") stereo_samples = true;
    else if (a == "--sample-loops") sample_loops = true;
    else if (a == "--sample-envelope" && i + 1 < argc) {
      char extra = 0;
      if (std::sscanf(argv[++i], "%lf,%lf,%lf,%lf%c", &sample_envelope.attack, &sample_envelope.decay, &sample_envelope.sustain, &sample_envelope.release, &extra) != 4) {
        std::fprintf(stderr, "--sample-envelope takes four numbers A,D,S,R (seconds, seconds, 0..1, seconds), got '%s'\n", argv[i]); return 2;
      }
      sample_envelope_on = true;
    }
    else if (a == "--sample-interpolation" && i + 1 < argc) {
      const std::string m = argv[++i];
      if (m == "nearest") sample_interpolation = GROOVE_SAMPLE_NEAREST;
      else if (m == "linear") sample_interpolation = GROOVE_SAMPLE_LINEAR;
      else if (m == "cubic") sample_interpolation = GROOVE_SAMPLE_CUBIC;
      else { std::fprintf(stderr, "--sample-interpolation: nearest, linear or cubic, not '%s'\n", m.c_str()); return 2; }
    }
    else if (a == "--assets" && i + 1 < argc) assets = argv[++i];
    else if (a == "--device" && i + 1 < argc) device = std::atoi(argv[++i]);
    else if (a == "--version" || a == "-v") { std::printf("groove-cli-hip 0.1 (MI355X render path)\n"); return 0; }
    else if (a == "--help" || a == "-h") {
      std::printf("usage: groove-cli-hip [--wav] [--assets DIR] [--device N] [--synthetic-kit] [--device-filter-links] [--device-trips] [--device-instrument-controls] [--device-wet-links] [--wet-reverb-run] [--stereo-samples] [--sample-interpolation nearest|linear|cubic] [--sample-loops] [--sample-envelope A,D,S,R] [--quiet] [--perf] [--debug] FILE...\n");
      return 0;
    } else inputs.push_back(a);
  }
  if (inputs.empty()) { std::fprintf(stderr, "no input files\n"); return 2; }
  for (const std::string& in : inputs) {
    ProjectDesc desc;
    try { desc = parse_project_file(in, assets); }
    catch (const std::exception& e) { std::fprintf(stderr, "%s: %s\n", in.c_str(), e.what()); return 1; }
    for (size_t i = 0; i < desc.warnings.size(); ++i) {
      bool linked = false; // a control that --device-filter-links or --device-wet-links links after all is not "dropped"
      for (const auto& h : desc.held_controls) linked = linked || ((held_control_is_wet(h.control) ? wet_links : filter_links) && h.warning == i);
      if (!linked) std::fprintf(stderr, "Warning: %s\n", desc.warnings[i].c_str());
    }
    if (debug) std::printf("%s\n", describe(desc, assets, stereo_samples).c_str());
    Orchestrator o(device, GROOVE_DEFAULT_SAMPLE_RATE, desc.bpm);
    if (!o.ctx()) { std::fprintf(stderr, "no HIP device: %s (this renderer has no CPU path)\n", o.last_error().c_str()); return 1; }
    o.set_filter_links_on_device(filter_links);
    o.set_trips_on_device(device_trips);
    o.set_instrument_controls_on_device(instrument_controls);
    o.set_wet_links_on_device(wet_links);
    o.set_stereo_samples(stereo_samples);
    o.set_sample_loops(sample_loops);
    if (sample_envelope_on && o.set_sample_envelope(&sample_envelope)) { std::fprintf(stderr, "%s: %s\n", in.c_str(), o.last_error().c_str()); return 1; }
    if (o.set_sample_interpolation(sample_interpolation)) { std::fprintf(stderr, "%s: %s\n", in.c_str(), o.last_error().c_str()); return 1; }
    if (o.set_wet_reverb_run(wet_run)) { std::fprintf(stderr, "%s: %s\n", in.c_str(), o.last_error().c_str()); return 1; }
    if (instantiate(o, desc, assets, synthetic)) { std::fprintf(stderr, "%s: %s\n", in.c_str(), o.last_error().c_str()); return 1; }
    if (!quiet) std::printf("Performing to queue %s\n", in.c_str());
    const auto t0 = std::chrono::steady_clock::now();
    Performance perf_out;
    if (o.run_performance(GROOVE_BLOCK_FRAMES, perf_out)) { std::fprintf(stderr, "%s: %s\n", in.c_str(), o.last_error().c_str()); return 1; }
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    const size_t frames = perf_out.worker.size();
    if (perf || !quiet) {
      // the same figures groove-cli --perf prints (groove-cli.rs:123-139)
      std::printf("Orchestrator performance:\n Elapsed    : %.6f s\n Frames     : %zu\n Samples per msec (goal > %.1f): %.1f\n usec per sample (goal < %.2f): %.4f\n x real time: %.1f\n",
                  secs, frames, perf_out.sample_rate / 1000.0, frames / (secs * 1000.0), 1e6 / perf_out.sample_rate,
                  secs * 1e6 / (frames ? frames : 1), frames / (double)perf_out.sample_rate / secs);
    }
    if (debug) { // the library's counters after the run (host_waits, host_wait_ms, ...: groove_debug_info)
      std::vector<char> info(1 << 16);
      if (!groove_debug_info(o.ctx(), info.data(), info.size())) std::printf("debug_info: %s\n", info.data());
    }
    if (wav) {
      const std::string out = wav_name(in);
      if (o.send_performance_to_file(perf_out, out)) { std::fprintf(stderr, "%s\n", o.last_error().c_str()); return 1; }
      if (!quiet) std::printf("Rendered %s (%zu frames)\n", out.c_str(), frames);
    }
  }
  return 0;
}
