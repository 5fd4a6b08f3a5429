/* groove_hip.h — C ABI of libgroove_hip.so, the MI355X (gfx950) render path that
 * drops in behind the reference's instrument/effect trait surface.
 *
 * The reference has no FFI of its own: its "plugin" boundary is the
 * set of Rust traits an entity implements (`ensnare_core::traits`, glued by
 * /root/reference/proc-macros/src/entity.rs:29-139).  Each entry point below names the
 * trait method(s) it replaces and the call site in the reference that drives it.  All
 * citations are relative to /root/reference.  INTEGRATION.md shows the Rust `extern "C"`
 * block and the `entities`-crate wrappers a maintainer would add.
 *
 * Conventions
 *   - every call returns 0 on success, non-zero on failure; groove_last_error() gives the
 *     message (audio-path trait methods are infallible in the reference; graph edits
 *     return anyhow::Result, orchestrator.rs:263-304 — the library never aborts);
 *   - the caller owns host memory; the library owns device memory behind opaque handles;
 *   - handles are not thread-safe: one HIP stream per ctx, matching the reference's
 *     single-threaded audio path (orchestrator.rs:367-470).  A ctx and everything created
 *     from it belong to one thread at a time; different contexts are independent and may be
 *     driven from different threads at once (tests/test_gpu_deferred.py::test_two_contexts_*);
 *   - device blocks are planar, frame-major fp32:  block[ch][frame][voice], ch 0 = left,
 *     so one wavefront's store is 64 consecutive floats; the bus is bus[frame][2];
 *   - note events and parameter changes take effect at the next block start, exactly the
 *     granularity of Orchestrator::tick (orchestrator.rs:856-859: handle_work once per
 *     tick, then gather_audio over the whole buffer).
 */
#ifndef GROOVE_HIP_H
#define GROOVE_HIP_H

#include "groove_types.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct groove_ctx groove_ctx;     /* one device + one stream                       */
typedef struct groove_bank groove_bank;   /* an instrument: N homogeneous voices, one lane each */
typedef struct groove_fx groove_fx;       /* an effect applied per lane to an N-lane block  */
typedef struct groove_block groove_block; /* device stereo block [2][frames_cap][n] fp32    */
typedef struct groove_ctl_link groove_ctl_link; /* a controller linked to one parameter of an effect */

/* ---- context ------------------------------------------------------------------------ */
/* Orchestrator::new_with + device selection (orchestrator.rs:522-568). */
int groove_init(int device_ordinal, groove_ctx** out);
/* groove_init for one rank of a multi-GPU job: the rank's RCCL communicator is created FIRST (id from
 * groove_comm_unique_id(NULL, ...) on rank 0, broadcast by the launcher), the library's own streams after it, so
 * that RCCL's internal streams do not land between them.  Equivalent to groove_init followed by
 * groove_comm_init otherwise — which is the faster order on this part (measured, DESIGN.md section 6: the communicator first
 * costs the million-voice path 19 %) and the one bench.py's ranks use.  GROOVE_SAFE_STREAMS=1 in the environment selects the conservative stream layout (one
 * priority, four streams in all) for either form. */
int groove_init_comm(int device_ordinal, const uint8_t id[128], int rank, int world_size, groove_ctx** out);
void groove_shutdown(groove_ctx* ctx);
/* ctx may be NULL: returns the last error of the calling thread. */
const char* groove_last_error(groove_ctx* ctx);
/* Use the caller's hipStream_t (e.g. a torch stream) instead of the ctx's own. */
int groove_set_stream(groove_ctx* ctx, void* hip_stream);
/* Waits for everything submitted so far (every stream of the library).  Like every blocking call of this API
 * (downloads, groove_bus_to_i16, groove_event_elapsed_ms ...) it polls with a DEADLINE: if the work has not completed
 * after groove_sync_timeout_ms() milliseconds the call returns non-zero and groove_last_error() names the streams
 * that are still busy — a stalled kernel surfaces as an error, never as a hang and never as an abort.  Nothing is
 * cancelled; the caller may wait again or tear the process down.  Default 60,000 ms (GROOVE_SYNC_TIMEOUT_MS in the
 * environment at groove_init), 0 = wait for ever.  No reference counterpart (the reference's audio path is
 * synchronous CPU code, orchestrator.rs:367-470). */
int groove_synchronize(groove_ctx* ctx);
int groove_set_sync_timeout_ms(groove_ctx* ctx, uint32_t ms);
uint32_t groove_sync_timeout_ms(groove_ctx* ctx);
/* Test / diagnosis hooks.  groove_debug_spin: one idle kernel that occupies a library stream for `ms` milliseconds
 * (side_stream = -1: the ctx stream; 0..5 kind streams; 6.. bank streams) — how the tests block a stream on purpose.
 * groove_debug_info: a JSON object with the stream layout of this ctx and `zero_segments` — how often a Welsh kernel's wave
 * found that its ACTIVE lanes had zero frames to their next envelope boundary (csrc/diag.h: the counted assertion behind
 * DESIGN.md section 7; it must read 0, and the GPU tests, smoke() and bench.py require that).  It waits for the ctx stream;
 * call groove_synchronize first for a figure that includes the side streams' latest kernels.  `host_waits`,
 * `host_waits_blocked`, `host_wait_ms`: how often the library's own waits (groove_synchronize, the paced calls, ...) ran, how
 * many of them found the device still busy, and for how long in total the calling thread was blocked in them — a paced walk
 * that is never blocked is bound by the host's submission, not by the device. */
int groove_debug_spin(groove_ctx* ctx, int side_stream, uint32_t ms);
int groove_debug_info(groove_ctx* ctx, char* out, size_t cap);
/* Configurable::update_sample_rate fan-out (orchestrator.rs:125-127, 1019-1022, 1389-1394).
 * Re-derives every bank/effect created on this ctx and resets their state. */
int groove_update_sample_rate(groove_ctx* ctx, uint32_t hz);
uint32_t groove_sample_rate(groove_ctx* ctx);
/* Tuning: Welsh banks of up to this many voices render a block (of up to 256 frames) TIME-PARALLEL, one
 * wavefront per voice with the frames spread over its lanes (csrc/welsh_tp.h), instead of one voice per
 * lane walking the frames serially — the form that is latency-bound below ~250,000 voices.  Same results
 * to f64 rounding of the filter.  0 = always the serial kernels.  Default 16,384 (GROOVE_TP_MAX_VOICES in
 * the environment overrides it at groove_init).  No reference counterpart. */
int groove_set_time_parallel_max_voices(groove_ctx* ctx, uint32_t max_voices);
uint32_t groove_time_parallel_max_voices(groove_ctx* ctx);
/* Tuning: time-parallel Welsh banks of at least this many voices, whose adjacent voices (2i, 2i + 1) share a patch, render
 * TWO voices per wavefront (32 lanes x 8 frames each) instead of one (64 lanes x 4 frames): half the wavefronts, 25 % less
 * issue per voice, the right trade once the one-voice form needs more wavefronts than the SIMDs hold at once; such banks stay
 * time-parallel up to 11/8 of groove_set_time_parallel_max_voices' limit (22,528 voices by default).  Default 3,073;
 * 0 = never; 1 = whenever the pairs allow (tests).
 * No reference counterpart. */
int groove_set_time_parallel_pair_min_voices(groove_ctx* ctx, uint32_t min_voices);
uint32_t groove_time_parallel_pair_min_voices(groove_ctx* ctx);
/* Tuning: Welsh banks of at least this many (virtual) wavefronts — 64 voices each; default 3,800 = ~243,000 voices — run
 * the mix kernel (three launches over thirds of the workgroups, and one kernel per exact-f64 base kind) and pipeline
 * consecutive fused blocks; smaller ones take one launch for all kinds.  1 forces that big-bank form for every size (tests
 * and bench.py's parity sample use it to run the kernels of the million-voice path on a small bank).  GROOVE_PIPELINE_MIN_WAVES in the environment sets it at groove_init. */
int groove_set_pipeline_min_waves(groove_ctx* ctx, uint32_t waves);
uint32_t groove_pipeline_min_waves(groove_ctx* ctx);
/* Which look-aheads the wave-uniform Welsh kernels may use (csrc/kernels.h): bit 0 — a wave whose live voices share the filter
 * envelope's stage computes 64 frames' filter coefficients in one pass, lane = frame (bit-identical to the per-lane retune); bit 1 —
 * a wave whose live voices share the LFO's phase evaluates what the LFO does to the oscillators (pitch / pulse-width routing) the same
 * way, exactly, where each lane would advance recurrences (within 1e-6 of them).  Default 3; GROOVE_LOOK_AHEAD in the environment
 * sets it at groove_init.  Tests render the same bank with and without.  Bit 2 (tests): count the waves that take the FAST copy of
 * their block body (groove_debug_info: fast_waves). */
int groove_set_look_ahead(groove_ctx* ctx, uint32_t bits);
uint32_t groove_look_ahead(groove_ctx* ctx);
/* Tuning, for a render-ahead walk of blocks through an effect chain that ENDS in a reverb (config #3): on = the reverb's two
 * all-passes — the chain's last kernel, which nothing on the ctx stream reads behind — are launched on a side stream of the
 * library, so that the NEXT block's fused run follows this block's run directly and the all-passes overlap it (0.0489 -> 0.044 ms
 * per block of config #3).  Semantics are unchanged: the block is "pending" like one a groove_bank_render_async is filling
 * (every call that reads it orders itself behind the kernel; groove_block_wait_ready / groove_block_wait_released wait for it);
 * its lane sums reach the bus through groove_mix, or — deferred — through groove_mix_deferred, in which case the next all-pass
 * launch (or any flush point) sums them.  Only blocks that have been through groove_block_release or an asynchronous render
 * (they have their events) take the side stream; everything else runs as before.  Results are bit-identical either way.
 * Default off.  No reference counterpart (the reference transforms one sample at a time, orchestrator.rs:446-454). */
int groove_set_fx_allpass_stream(groove_ctx* ctx, int on);
int groove_fx_allpass_stream(groove_ctx* ctx);
/* Tuning: on = a reverb that is only PARTLY wet (a lane's wet-dry-mix below 1, or a live wet link onto it: groove_ctl_wet_link_create)
 * keeps the forms of an all-wet one — its combs a stage of the fused run, the all-pass kernels behind it, the all-pass stream, the
 * block's lane sums left for groove_mix — where, off, it walks the block's frames serially (fx_reverb_kernel) and cuts the chain's
 * fused run in front of it.  The run's reverb stage then also keeps its input, and the kernel that writes the reverb's final value
 * applies the serial kernel's own `wet < 1 ? fma(out, wet, dry * (1 - wet)) : out` per lane: results are bit-identical either way.
 * groove_fx_kernel_form reports the all-wet reverb's form strings for it.  An all-wet reverb launches exactly what it launches with
 * the knob off.  Default off; GROOVE_FX_WET_REVERB_RUN=1 in the environment sets it at groove_init.  May be changed between any two
 * blocks.  No reference counterpart (the reference transforms one sample at a time, orchestrator.rs:446-454). */
int groove_set_fx_wet_reverb_run(groove_ctx* ctx, int on);
int groove_fx_wet_reverb_run(groove_ctx* ctx);
/* Tuning: Welsh banks of up to this many (virtual) wavefronts that are too big for the time-parallel form render ROLE-SPLIT:
 * four wavefronts per 64 voices — envelopes + LFO, oscillators, cutoff tangent + coefficient quotients, filter + gains — pipelined
 * over the block's frames through LDS, so that a bank which cannot fill the chip with voices fills it with the parts of a voice's
 * frame (csrc/welsh_split.h).  Same results bit for bit as the serial kernels run without their LFO look-ahead (groove_set_look_ahead),
 * within 2e-6 of them with.  Default 1,024 (65,536 voices: one workgroup per CU); larger banks take the all-kinds kernel; 0 = never.
 * No reference counterpart. */
int groove_set_split_max_waves(groove_ctx* ctx, uint32_t waves);
uint32_t groove_split_max_waves(groove_ctx* ctx);
/* HIP events on the ctx stream, for measurement (bench.py): create / record / elapsed. */
int groove_event_create(groove_ctx* ctx, void** out_event);
int groove_event_destroy(groove_ctx* ctx, void* event);
int groove_event_record(groove_ctx* ctx, void* event);
int groove_event_elapsed_ms(groove_ctx* ctx, void* start, void* stop, float* out_ms);

/* ---- blocks --------------------------------------------------------------------------- */
/* The buffer a `generate_batch_values(&mut [StereoSample])` call fills
 * (entities/src/instruments/metronome.rs:23-35), for n lanes at once. */
int groove_block_create(groove_ctx* ctx, uint32_t n, uint32_t frames_cap, groove_block** out);
int groove_block_destroy(groove_block* b);
/* The raw device pointer.  Handing it out invalidates the lane sums the last render left with the block (groove_mix
 * then reads the block itself); a caller that keeps the pointer and writes the block again later calls
 * groove_block_mark_dirty (or groove_block_acquire) before the next groove_mix. */
float* groove_block_device_ptr(groove_block* b);
int groove_block_mark_dirty(groove_block* b);
uint32_t groove_block_lanes(groove_block* b);
uint32_t groove_block_frames_cap(groove_block* b);
/* host [2][frames][n] fp32 <-> device */
int groove_block_upload(groove_block* b, const float* host, uint32_t frames);
int groove_block_download(groove_block* b, float* host, uint32_t frames);

/* dst (+)= src.  Equal lane counts: element-wise.  dst with ONE lane: the lanes of src are summed
 * (a Synthesizer summing its voice store; an effect summing its sources, orchestrator.rs:438-457). */
int groove_block_accumulate(groove_block* dst, groove_block* src, uint32_t frames, int accumulate);
int groove_block_zero(groove_block* b);

/* ---- instruments (Ticks + Generates<StereoSample> + HandlesMidi + Controllable) --------- */
/* WelshSynth::new_with(&WelshSynthParams) (settings/src/instruments.rs:71-76) for n voices. */
int groove_welsh_create(groove_ctx* ctx, const groove_welsh_params* p, uint32_t n, groove_bank** out);
/* FmSynth::new_with(&FmSynthParams) (settings/src/instruments.rs:89-92). */
int groove_fm_create(groove_ctx* ctx, const groove_fm_params* p, uint32_t n, groove_bank** out);
/* Sampler::new_with / Drumkit::new_with (settings/src/instruments.rs:81-88); the shared
 * mono sample bank is uploaded once and stays resident. */
int groove_sampler_create(groove_ctx* ctx, const float* bank_pcm, uint64_t bank_frames,
                          const groove_sample_desc* descs, uint32_t n_samples,
                          const groove_sampler_params* p, uint32_t n, groove_bank** out);
/* The same bank over STEREO sample memory: bank_pcm_lr is [bank_frames][2] fp32, interleaved left, right; groove_sample_desc is
 * unchanged (offset and length in frames).  A voice steps and ends exactly as a mono bank's does (same parameter and state records,
 * same groove_bank_state_words / _download_state), and its output is L = left[offset + i] * gain, R = right[offset + i] * gain.
 * Stereo is a property of the bank: a kit that mixes mono and stereo files is a stereo bank whose mono files the caller writes into
 * both channels.  Everything that takes a sampler bank takes this one (note events, reset, groove_bank_set_param and links onto
 * GROOVE_CTL_SAMPLER_GAIN, the four render entries, groove_bank_kernel_form: same strings and thresholds).  Same argument checks as
 * groove_sampler_create, reported under this function's name. */
int groove_sampler_create_stereo(groove_ctx* ctx, const float* bank_pcm_lr, uint64_t bank_frames,
                                 const groove_sample_desc* descs, uint32_t n_samples,
                                 const groove_sampler_params* p, uint32_t n, groove_bank** out);
/* Channels of a sampler bank's sample memory: 1 (groove_sampler_create) or 2 (groove_sampler_create_stereo); 0 for any other bank. */
uint32_t groove_bank_sample_channels(groove_bank* bank);
/* How a sampler or drumkit bank reads its sample BETWEEN frames (docs/DSP_SPEC.md section 7): a groove_sample_interpolation.
 * GROOVE_SAMPLE_NEAREST (the default) plays pcm[floor(idx)] as the reference does; GROOVE_SAMPLE_LINEAR and GROOVE_SAMPLE_CUBIC
 * (Catmull-Rom) weigh 2 and 4 frames around the cursor by the top 24 bits of its fraction, per channel on a stereo bank.  A tap before
 * a sample's first or past its last frame is 0 and is never read from memory: neighbouring samples of the bank are not heard.  Only
 * the value a frame plays changes: cursor, end rule, note rules, parameters and state are the same in every mode (the same events
 * leave the same groove_bank_download_state words), and a voice whose step is an integer — a drumkit, a key on the root — plays
 * NEAREST's bits.  The setter is refused with a message for a bank of another kind and for an unknown mode; it joins the bank's
 * earlier work first, like groove_bank_set_param, may be called between any two renders and touches neither parameters nor state.
 * Everything that takes a sampler bank takes an interpolated one (the four render entries, reset, a sample-rate change,
 * groove_bank_set_param, links onto the gain); groove_bank_kernel_form names the mode after the form.  The getter reports
 * GROOVE_SAMPLE_NEAREST for a bank of another kind. */
int groove_bank_set_sample_interpolation(groove_bank* bank, uint32_t mode);
uint32_t groove_bank_sample_interpolation(groove_bank* bank);
/* FORWARD LOOPS: a held note outlasts the recording (docs/DSP_SPEC.md section 7).  loops[i] is the loop of the bank's i-th sample,
 * n_samples the bank's sample count; loops == NULL clears every loop.  A voice loops while its sample has a loop, it is no one_shot
 * voice (a drumkit voice ignores note-off and would never end) and it plays: its Q20.44 cursor is folded into [0, end) — F(x) = x
 * below end << 44, start + (x - start) mod (end - start) from there on, exact 64-bit integers, for every length the create calls
 * accept — so the end rule is never met and note-off stops it at the next block start as it stops any sampler voice (a release tail:
 * groove_bank_set_sample_envelopes).
 * The split of a render into blocks changes no bit of output or state.  Interpolation taps at or past `end` are read as the loop
 * repeats, taps before the sample's first frame are silence; no tap of a looping voice lies outside [0, end).  Every other voice —
 * on a sample without a loop, or a one_shot voice on a looped one — plays what it played before, bit for bit.  Like the interpolation
 * mode a property of the bank: settable between any two renders (a cursor at or past `end` is folded at its next frame), kept by
 * groove_bank_reset, a sample-rate change and groove_bank_set_param, touching neither parameters nor state.  The setter joins the
 * bank's earlier work first, like groove_bank_set_param.  It is refused with a message for a bank of another kind, n_samples other
 * than the bank's sample count, start >= end unless both are 0, and end beyond the sample's length.  groove_bank_kernel_form says
 * ", looped" while a sample of the bank has a loop.  The getter writes the first min(cap, sample count) loops to `out` (NULL: none)
 * and returns the number of looped samples; 0 for a bank of another kind. */
int groove_bank_set_sample_loops(groove_bank* bank, const groove_sample_loop* loops, uint32_t n_samples);
uint32_t groove_bank_sample_loops(groove_bank* bank, groove_sample_loop* out, uint32_t cap);
/* AMPLITUDE ENVELOPES: a note gets an attack and a release tail (docs/DSP_SPEC.md section 7).  env[i] is the envelope of the bank's
 * i-th sample (times in seconds, sustain 0..1; the shape and stage rules are section 3's, the Welsh and FM voices'), n_samples the
 * bank's sample count; enabled[i] == 0 leaves sample i without one (enabled == NULL: every sample has one); env == NULL clears all.
 * A voice is ENVELOPED when its sample has an envelope and it is no one_shot voice; every other voice plays what it played before,
 * bit for bit.  For an enveloped voice note-on starts the sample and attacks (a retrigger from the envelope's current value),
 * note-off releases and leaves the cursor running — a looping voice loops through its release — and each frame is the plain frame
 * times the envelope's value, one fp32 multiply; the voice stops on the frame whose tick finds the envelope idle, or at the sample's
 * end.  The split of a render into blocks changes no bit of output or state, and the gate envelope (0, 0, 1, 0) plays the bank's
 * bits without envelopes.  SamplerParams, SamplerState and groove_bank_state_words do not change: the envelope records live in a
 * buffer of their own, allocated by the first call and freed with the bank.  The setter joins the bank's earlier work first, like
 * groove_bank_set_sample_loops, and may be called between any two renders: every record becomes idle, that of a voice that plays a
 * SUSTAIN plateau at its sustain level; on clearing, a voice whose envelope is in its release stops (it would play on without one)
 * and a held voice plays on.  A property of the bank: kept by groove_bank_set_param and gain links, by groove_bank_reset (every
 * record idle) and by a sample-rate change (parameters derived again, records idle like the state).  Refused with a message for a
 * bank of another kind, n_samples other than the bank's sample count, a negative or non-finite time, a sustain outside [0, 1].
 * groove_bank_kernel_form says ", enveloped" while a sample of the bank has an envelope.  The getter writes the first
 * min(cap, sample count) envelopes and flags (either may be NULL) and returns the number of enveloped samples; 0 for a bank of
 * another kind.  groove_bank_download_sample_envelope_state copies the voices' envelope state words, [7][n] word-major (state, n, N,
 * A, D, inv_len, value), for tests and hosts that checkpoint; refused on a bank without envelopes. */
int groove_bank_set_sample_envelopes(groove_bank* bank, const groove_envelope_params* env, const uint32_t* enabled, uint32_t n_samples);
uint32_t groove_bank_sample_envelopes(groove_bank* bank, groove_envelope_params* out, uint32_t* enabled_out, uint32_t cap);
int groove_bank_download_sample_envelope_state(groove_bank* bank, uint32_t* words);
int groove_bank_destroy(groove_bank* bank);
uint32_t groove_bank_voices(groove_bank* bank);
/* HandlesMidi::handle_midi_message → PlaysNotes::note_on/note_off (orchestrator.rs:737-739;
 * settings/src/patches.rs:928, 821).  Applied in order, at the start of the next render. */
int groove_bank_note_events(groove_bank* bank, const groove_note_event* ev, uint32_t n_ev);
/* Controllable::control_set_param_by_index (proc-macros/src/control.rs:211-226); value01 is a
 * ControlValue in 0..1 (orchestration/src/lib.rs:43-47).  voice = GROOVE_ALL_VOICES for all.
 * Each bank kind has its own indices (groove_types.h): a Welsh bank GROOVE_CTL_WELSH_* (32 - 34), an FM bank GROOVE_CTL_FM_* (48 - 51:
 * dca-gain, dca-pan, depth, beta; `ratio` has no control), a sampler or drumkit bank GROOVE_CTL_SAMPLER_GAIN (64).  An index of another
 * kind is refused with a message that names the kind's own.  The host's copy of the voice's parameters is updated, the ctx stream is
 * joined and waited for, and the derived parameter records are uploaded again; the voices' state stays where it is. */
int groove_bank_set_param(groove_bank* bank, uint32_t voice, uint32_t control_index, double value01);
/* Ticks::tick(frames) + Generates::generate_batch_values: fills out[2][frames][n]. */
int groove_bank_render(groove_bank* bank, uint32_t frames, groove_block* out);
/* The same render submitted to the library's own side streams: it starts once everything submitted
 * to the ctx stream so far has finished (the previous users of `out` and of the bank), and runs BESIDE
 * what the ctx stream is given next.  Operations that take `out` (groove_fx_process, groove_mix,
 * groove_block_accumulate / download / upload / zero, another render into it) wait for it by
 * themselves; a caller that hands groove_block_device_ptr(out) to its own kernels on the ctx stream
 * calls groove_block_acquire(out) first.  Purpose: the per-entity walk of Orchestrator::run
 * (orchestrator.rs:397-457) has the instruments of block b+1 depend on nothing the effect chains of
 * block b produce, so a host that keeps two blocks per instrument submits render(b+1) before the
 * effects of block b and the two overlap (bench.py --workload chain-4096).  Results are identical to
 * groove_bank_render's. */
int groove_bank_render_async(groove_bank* bank, uint32_t frames, groove_block* out);
/* Orders the ctx stream after the asynchronous render that last filled `b` (no-op otherwise). */
int groove_block_acquire(groove_block* b);
/* HOST PACING (no reference counterpart; the reference's audio path is synchronous).  A device-side wait for another queue's
 * event costs the waiting stream 7 - 9 us whether or not the event has completed when the stream gets there, but a wait whose
 * event is already complete WHEN THE CALL IS MADE is dropped.  An offline host that has nothing else to do waits itself:
 * groove_block_wait_ready blocks the host (with the deadline of groove_synchronize) until the asynchronous render — and chain
 * head — that last filled `b` has finished, after which the ctx-stream operations on `b` carry no wait;
 * groove_block_wait_released blocks it until the point marked by the last groove_block_release(b) has passed, after which the
 * next groove_bank_render_async into `b` carries none.  With four blocks per instrument in rotation and the renders submitted
 * two blocks ahead both return at once in steady state (bench.py --workload chain-4096). */
int groove_block_wait_ready(groove_block* b);
int groove_block_wait_released(groove_block* b);
/* Marks the end of the block's consumers so far (one event on the ctx stream).  The next
 * groove_bank_render_async into `b` then waits for this point only — not for everything submitted to
 * the ctx stream by the time of that call — provided nothing uses the block on the ctx stream in
 * between.  With three blocks per instrument in rotation the released block's consumers are a whole
 * step in the past, the render needs no cross-queue wait and follows the previous one directly. */
int groove_block_release(groove_block* b);
/* Fused form of "tick every leaf and add its value to the running sum"
 * (orchestrator.rs:397-410) for instruments patched straight into the main mixer: renders
 * and accumulates into bus_dev[frames][2] (device) without materialising the block.
 * accumulate = 0 overwrites the bus, 1 adds to it.
 * Asynchronous like every call here: the bus is complete for anything ordered after this call on the
 * ctx stream (groove_download, groove_bus_to_i16, groove_bus_reduce, groove_synchronize ...).  Large
 * Welsh banks pipeline consecutive calls (block b+1's voice kernels, on the library's own side
 * streams, do not wait for block b's bus sum); calls that touch the bank in between (note events,
 * groove_bank_set_param, groove_bank_render, groove_bank_download_state) join that pipeline first, so
 * the order of effects is the order of calls.  The voices' lane order inside the library is its own
 * business (a bank whose patches are interleaved voice by voice is kept patch-major): every index in
 * this API is the caller's voice index. */
int groove_bank_render_mix(groove_bank* bank, uint32_t frames, float* bus_dev, int accumulate);
/* groove_bank_render_mix whose bus reduction is DEFERRED: the block's partial rows are put on the bus by the bank's next deferred
 * render (its workgroups each add up a slice while their parameter loads are under way: no reduction launch), or — at the latest —
 * by the next call that waits for the ctx stream (groove_synchronize, downloads), records an event on it, or touches a bus
 * (groove_mix, groove_bank_render_mix, groove_bus_zero / _to_i16 / _reduce, groove_bus_flush).  For a host that renders a lone
 * small bank block after block (the reference's offline loop, orchestrator.rs:367-470, with one instrument): a time-parallel
 * bank's step is then one launch instead of two (256 Welsh voices 0.016 -> 0.013 ms per block).  The banks of a small project may
 * also take turns this way — each render carries the reduction of the one before it, in submission order, all on the ctx stream —
 * instead of running side by side with their cross-queue waits (config #5's 16,384-voice share of a GPU).  Banks it does not apply to
 * (not time-parallel, more than 2,048 partial rows — 16,384 paired Welsh voices) are rendered by groove_bank_render_mix.  The bus
 * is the same sum to fp32 rounding, but NOT the same bits as groove_bank_render_mix's, nor from one call pattern to another: the
 * order in which a column's rows are added depends on which launch carries them (a following deferred render adds them in batches
 * of eight rows per lane, partitioned by ITS grid; groove_bus_flush and the flush points add them in segments of 64 rows).  A
 * host that needs bit-reproducible buses calls groove_bank_render_mix. */
int groove_bank_render_mix_deferred(groove_bank* bank, uint32_t frames, float* bus_dev, int accumulate);
/* One block of a project of several SMALL banks of different kinds — Orchestrator::gather_audio's one sum over all instruments
 * (orchestrator.rs:397-410) — in ONE launch: the workgroups of one grid dispatch on their index into the Welsh / FM / sampler
 * time-parallel bodies (the most expensive kind first), they share one buffer of partial rows, and the block's one bus reduction is
 * deferred exactly as above (carried by the next such call, or flushed).  For projects with at most one time-parallel bank of each
 * kind and at most 2,048 partial rows in all (config #5's share of one of eight GPUs: 8,192 Welsh + 4,096 FM + 4,096 sampler
 * voices, three launches whose durations added -> one); anything else is rendered bank by bank by groove_bank_render_mix_deferred in
 * the order given (bus = banks[0] (+)= ... ); a STEREO sampler bank among them, one whose sample
 * interpolation is not GROOVE_SAMPLE_NEAREST, or one with a looped or enveloped sample always takes that bank-by-bank path (the one launch's
 * sampler body is the mono, nearest, loop-free one).  Bit-reproducible from run to run; the same sum as bank by bank to fp32 rounding, not
 * the same bits (one reduction over all rows instead of one per bank).  No reference counterpart as a call: the reference ticks
 * every instrument inside gather_audio. */
int groove_banks_render_mix_deferred(groove_ctx* ctx, groove_bank* const* banks, uint32_t n_banks, uint32_t frames, float* bus_dev, int accumulate);
int groove_bus_flush(groove_ctx* ctx);
/* groove_bank_render_mix for a project whose banks render SIDE BY SIDE on the library's streams, PACED by the host (see
 * groove_block_wait_ready): the call blocks the host, as needed, until the reduction that frees this bank's slot of partial rows
 * (two of its blocks back) and the render of its PREVIOUS block have finished, so that neither the render streams nor the ctx
 * stream ever carry a cross-queue wait; the reduction of the block rendered by THIS call is launched by the bank's next paced
 * call, or by whatever flushes a bus (groove_bus_flush, groove_synchronize, a download, groove_event_record, any unpaced render
 * or mix).  The banks' sums reach a bus in the order of the calls, as with groove_bank_render_mix; same bits.  For the offline
 * host that renders several instruments patched straight into the main mixer block after block (orchestrator.rs:397-410):
 * config #5 on one GPU and its per-GPU share of eight.  No reference counterpart. */
int groove_bank_render_mix_paced(groove_bank* bank, uint32_t frames, float* bus_dev, int accumulate);
/* Every voice back to its freshly created state (oscillator phases, envelopes idle, filter memory,
 * sampler cursors); parameters stay; queued note events are dropped.  What the reference gets by
 * re-running a project from the top: Orchestrator::skip_to_start (orchestrator.rs:971-983) followed by
 * the Configurable::update_sample_rate fan-out that resets every entity (orchestrator.rs:125-127) —
 * without re-deriving or re-uploading the parameter tables. */
int groove_bank_reset(groove_bank* bank);
/* Which kernel form a render of `frames` frames of this bank takes right now (a static string; diagnosis: bench.py
 * prints it beside every parity figure so that the figure names the kernels it checked). */
const char* groove_bank_kernel_form(groove_bank* bank, uint32_t frames, int fused);
/* Raw state snapshot (checkpoint / debugging): words = groove_bank_state_words(). */
uint32_t groove_bank_state_words(groove_bank* bank);
int groove_bank_download_state(groove_bank* bank, uint32_t* host_words /* [words][n] */);

/* ---- effects (TransformsAudio) ---------------------------------------------------------- */
/* `Foo::new_with(&FooParams)` for n lanes (settings/src/effects.rs:59-117).  p has n entries. */
int groove_fx_create(groove_ctx* ctx, uint32_t kind, const groove_fx_params* p, uint32_t n, groove_fx** out);
int groove_fx_destroy(groove_fx* fx);
/* Clears the effect's memory (IIR state, delay lines, ring positions); parameters stay. */
int groove_fx_reset(groove_fx* fx);
/* TransformsAudio::transform_audio over a block, in place (orchestrator.rs:438-457). */
int groove_fx_process(groove_fx* fx, groove_block* inout, uint32_t frames);
/* The effects patched behind one instrument, in patch order, over one block: what the reference's gather walk does when
 * it meets a chain of TransformsAudio entities above a source (orchestrator.rs:438-457: each effect transforms the sum
 * of what is patched into it).  Same result, bit for bit, as groove_fx_process on chain[0] .. chain[n_fx-1] in turn;
 * the library fuses the stages that have no feedback inside a block (element-wise kinds, delay lines at least a block
 * long) into one pass over the block.  An effect may appear once. */
int groove_fx_chain_process(groove_fx* const* chain, uint32_t n_fx, groove_block* inout, uint32_t frames);
/* The chain's LEADING stages that have feedback inside a block (the IIR filters; delay lines shorter than the block),
 * submitted to the side stream that carries `inout`'s pending groove_bank_render_async, right behind that render:
 * *n_done stages are taken — IIR filters only (0 when the block has no pending render on one side stream, or when the chain
 * starts with another kind of stage); an effect that is processed ahead like this must be processed ahead in EVERY block
 * (its blocks would otherwise be submitted out of order); the caller hands chain + *n_done to groove_fx_chain_process when it reaches the block.  Same
 * bits as processing the whole chain there.  Purpose: in the render-ahead walk (groove_bank_render_async above) these
 * narrow, latency-bound kernels then run beside the wide stages of the PREVIOUS block instead of in front of them on
 * the ctx stream.  Parameter changes of those effects must be made before this call for the block it processes
 * (the effect is one block ahead of the ctx stream's walk).  No reference counterpart. */
int groove_fx_chain_process_async(groove_fx* const* chain, uint32_t n_fx, groove_block* inout, uint32_t frames, uint32_t* n_done);
/* groove_bank_render_async(bank, frames, out) followed by groove_fx_chain_process_async(chain, n_fx, out, frames, n_done) as ONE
 * call — which lets the library fuse the chain's first stage into the render kernel itself when it can: a 12 dB BiQuad
 * behind a bank that renders time-parallel (the frames of a voice's block are then already spread over a wavefront's lanes,
 * and the filter is one more scan on values that sit in registers: no separate launch, and the block is not read and
 * written a second time).  Same results as the two calls to f64 rounding of the filter's start states.  *n_done as above. */
int groove_bank_render_chain_async(groove_bank* bank, uint32_t frames, groove_block* out, groove_fx* const* chain, uint32_t n_fx,
                                   uint32_t* n_done);
/* Which kernel form groove_fx_process(fx, block, frames) takes right now (a static string; diagnosis and tests).  The form
 * follows from the effect's kind, its lane count, the block length and its line lengths; a reverb's direct all-pass form also
 * depends on the block's capacity (its staging block), hence the block.  The answer is the one for an effect that is the LAST
 * launch of its chain: a reverb further up a chain never rides the all-pass stream.  groove_fx_kernel_form_name(i) lists every
 * string the query can return, i = 0, 1, ... until it returns NULL (the one list of them: the library's table, in enum order). */
const char* groove_fx_kernel_form(groove_fx* fx, groove_block* block, uint32_t frames);
const char* groove_fx_kernel_form_name(uint32_t index);
/* Controllable for effects; lane = GROOVE_ALL_VOICES for all lanes. */
int groove_fx_set_param(groove_fx* fx, uint32_t lane, uint32_t control_index, double value01);
/* Replace all per-lane parameters (non-UNIFORM fields only may change). */
int groove_fx_set_params(groove_fx* fx, const groove_fx_params* p, uint32_t n);

/* ---- control links (IsController -> Controllable, resident on the device) ------------------ */
/* A controller device (ControllerSettings::LfoController / SignalPassthroughController, settings/src/controllers.rs:103-112)
 * linked to one parameter of an effect: the `controls` entry `source -> target.param` that Orchestrator::link_control
 * records (orchestrator.rs:1279-1294).  The reference works every controller once per tick and dispatches the ControlValue it
 * emits to the linked Controllable::control_set_param_by_index before gather_audio (orchestrator.rs:631-708, 856-877); here
 * a small kernel on the ctx stream writes the value into the target's device parameters, with NO host wait and no copy
 * (groove_fx_set_param re-uploads whole parameter arrays and waits for the ctx stream around each copy: fine for a change
 * now and then, not for one in every block).  docs/DSP_SPEC.md section 13 defines the value and target laws.
 *   src[n_src]: n_src equals the target's lane count, or is 1 and is broadcast to every lane; all of one `source` kind.
 *   control_index: GROOVE_CTL_FX_CEILING (Gain), _BITS (Bitcrusher), _ATTENUATION (Reverb), _THRESHOLD (Compressor / Limiter)
 *   — the parameters whose device form IS the value.  _CUTOFF, _Q, _PASSBAND_RIPPLE (coefficients derived on the host in f64)
 *   and _WET (it chooses a reverb's kernel path on the host) are refused here — the first three have groove_ctl_filter_link_create,
 *   _WET has groove_ctl_wet_link_create, both below — as are noise / none waveforms (no closed form for the state
 *   of a noise generator after n ticks).
 * A link does not update the host's copy of the target's parameters: a later groove_fx_set_param / groove_fx_set_params on the
 * target re-uploads that copy and so overwrites the linked parameter until the link's next apply. */
int groove_ctl_link_create(groove_ctx* ctx, const groove_ctl_source* src, uint32_t n_src, groove_fx* target, uint32_t control_index,
                           groove_ctl_link** out);
/* A FILTER link: the same kind of link onto a parameter that becomes filter coefficients.  Its apply computes the control value as
 * above, turns it into the parameter by groove_fx_set_param's law (cutoff: 25 * 800^v Hz; q and passband-ripple: 10 v^2 + 0.707,
 * each rounded to the float groove_fx_params holds), and derives the lane's five or six f64 coefficients ON THE DEVICE from the
 * effect's per-lane parameter shadow — the formulas of groove_fx_create, one text for both sides (csrc/fx_coef.h) — again with no
 * host wait and no copy.  The shadow (five floats per lane) is allocated with the first filter link onto an effect; from then on
 * groove_fx_set_param(s) refresh it with the coefficients, so the staleness rule above holds unchanged, and two links onto one
 * effect (cutoff and q) see each other's last value in the order of their applies.
 *   control_index: GROOVE_CTL_FX_CUTOFF onto any of the nine filter kinds, _Q onto low-pass / high-pass / all-pass 12 dB,
 *   _PASSBAND_RIPPLE onto low-pass 24 dB.  Everything else is refused (_WET included: groove_ctl_wet_link_create).  The sources are checked as above.
 * The link it returns is an ordinary one: capture, apply, reset and destroy below. */
int groove_ctl_filter_link_create(groove_ctx* ctx, const groove_ctl_source* src, uint32_t n_src, groove_fx* target, uint32_t control_index,
                                  groove_ctl_link** out);
/* TransformsAudio::transform_audio of a SignalPassthroughController: the identity on `block` (it is only read), which keeps, per
 * lane, clamp((L + R) / 2, -1, 1) of frame `frames - 1` for the next groove_ctl_link_apply.  Signal links only; the block has
 * n_src lanes.  Ordered behind whatever fills the block, like every call that reads one. */
int groove_ctl_link_capture(groove_ctl_link* link, groove_block* block, uint32_t frames);
/* IsController::work for the block whose first frame is `at_frame` (frames since Orchestrator::skip_to_start), followed by the
 * dispatch of its ControlValue: an LFO link evaluates its oscillator at at_frame; a signal link hands on what it captured last
 * (nothing captured yet, or since a reset: the target is left untouched).  Ordered like groove_fx_set_param — behind every use of
 * the target submitted so far, ahead of every later one.  An error once the target has been destroyed. */
int groove_ctl_link_apply(groove_ctl_link* link, uint64_t at_frame);
/* A TRIP link: a control trip (start_beat plus n_steps steps {kind, start, end, beats}, include/groove_types.h) as the source of a
 * link — a closed form of musical time, evaluated in f64 by the link's kernel (csrc/ctl_core.h: the host trip's law restated).
 *   steps[n_src][n_steps], start_beat[n_src]: n_src equals the target's lane count, or is 1 and is broadcast; every source lane has the
 *   same step count and its own steps.  The steps' begins (begin[0] = start_beat, begin[i + 1] = begin[i] + beats[i], in f64) are
 *   uploaded once; they do not depend on the sample rate.
 *   control_index: ONE create for both forms — a parameter whose device form is the value (groove_ctl_link_create's list) makes a
 *   plain link, a filter's cutoff, q or passband-ripple (groove_ctl_filter_link_create's list) a filter link with the parameter shadow.
 * Refused: _WET (groove_ctl_wet_trip_create takes it); a parameter the target's kind does not have; n_steps == 0 or > 65,536; a step with beats <= 0 or a non-finite
 * beats, start or end; a non-finite start_beat; an unknown step kind; a target that is not a live effect.
 * The value is clamped to 0..1 and goes through groove_fx_set_param's law in the precision it has there, so the target word is the one
 * that call would give it (flat and slope steps: bit for bit; the two curves read log10 from the device's math library).  The link it
 * returns takes groove_ctl_trip_apply, groove_ctl_link_reset (nothing to forget: a no-op) and groove_ctl_link_destroy;
 * groove_ctl_link_apply and groove_ctl_link_capture on it are errors, as is groove_ctl_trip_apply on any other link. */
int groove_ctl_trip_create(groove_ctx* ctx, const groove_ctl_step* steps, uint32_t n_steps, const double* start_beat, uint32_t n_src,
                           groove_fx* target, uint32_t control_index, groove_ctl_link** out);
/* IsController::work of a trip for the block that starts at musical time `at_units` (GROOVE_CTL_UNITS_PER_BEAT units per beat): each
 * lane finds the step that holds at_units / 65536 and writes its value; a lane whose trip has no step there (before start_beat, at or
 * after the end) leaves its target word untouched, as the host trip sends nothing outside its steps.  Ordered like
 * groove_ctl_link_apply: one launch on the ctx stream, no wait, no copy.  The staleness rule above holds — and where the host trip
 * re-sends only when its value changes, an apply inside a step ALWAYS writes, so it also restores a linked parameter that a
 * groove_fx_set_param(s) on the target has overwritten since. */
int groove_ctl_trip_apply(groove_ctl_link* link, uint64_t at_units);
/* A BANK link: a controller linked to a Welsh synth's dca-gain, dca-pan or filter-cutoff — Controllable on the instrument, which
 * groove_bank_set_param(bank, GROOVE_ALL_VOICES, ...) serves by re-deriving, re-planning and re-uploading the whole bank with host
 * waits around each copy.  The link's apply is one small kernel on the ctx stream instead: it computes the control value, turns it
 * into the parameter by groove_bank_set_param's law (gain: clamp01(v); pan: clamp01(v) * 2 - 1; cutoff: 25 * 800^clamp01(v) Hz, each
 * rounded to the float groove_welsh_params holds) and writes the words the voice kernels read at the start of a block — gl and gr
 * (the pan law of the bank's per-voice gain and pan, csrc/ctl_core.h pan_gains) or cutoff_hz — into the per-lane parameter array AND
 * the per-virtual-wave copies.  No host wait, no copy.
 *   src[1] / steps[1][n_steps], start_beat[1]: ONE source, broadcast to every voice (what GROOVE_ALL_VOICES does).  n_src != 1 is
 *   refused: per-voice values would break the wave-uniform parameter records; per-voice changes keep groove_bank_set_param.
 *   control_index: GROOVE_CTL_WELSH_DCA_GAIN, _DCA_PAN or _CUTOFF on a Welsh bank (FM and sampler banks: below).  Refused: any other index,
 *   a bank that is not live, and whatever groove_ctl_link_create / groove_ctl_trip_create refuse of their sources and steps.
 * Gain and pan share two words, so the bank gets a per-voice (gain, pan) shadow on the device with its first gain or pan link;
 * groove_bank_set_param, a sample-rate change and a reset refresh it from the host's copy.  The staleness rule of the effect links
 * holds unchanged: a link does not update the host's copy, a later groove_bank_set_param re-uploads it and overwrites the linked
 * parameter until the link's next apply (a trip's apply inside a step always writes), and two links onto one bank (gain and pan) see
 * each other's last value in the order of their applies.
 * Cutoff and the fp32 filter: whether a patch's filter may run in fp32 is MEASURED on the host for its static cutoff, and a link moves
 * that cutoff where the host cannot measure.  While a bank has a live cutoff link its voices run the f64 recurrence (always safe);
 * the bank is re-planned — like a groove_bank_set_param, host's copy re-uploaded — when the first such link is created and when the
 * last one is destroyed.  A cutoff link onto a patch whose filter is retuned by its envelope or LFO is accepted and inaudible, as the
 * host path is: those bodies do not read the static cutoff.
 * Ordering: the apply runs behind every render of the bank submitted so far and ahead of every later one, joined and forked by
 * events; it is a between-blocks change like a note event.  A signal link's capture block has one lane.  (The compiled host layer
 * does not make signal links onto instruments: in its render-ahead walk the instruments of block b + 1 render before block b's
 * effects have captured anything, so "the value captured in the previous tick" does not exist there.)
 * FM and sampler banks: the same two creates take GROOVE_CTL_FM_DCA_GAIN, _DCA_PAN, _DEPTH and _BETA on an FM bank and
 * GROOVE_CTL_SAMPLER_GAIN on a sampler or drumkit bank, by groove_bank_set_param's laws for those kinds (gain and pan as above; depth,
 * beta and a sampler's gain: clamp01(v) rounded to float).  Every FM and sampler kernel loads its record from the per-voice parameter
 * array alone — no per-wave copies, nothing wave-uniform — so here n_src may be 1 (broadcast) OR the bank's voice count: one source
 * lane per voice, the natural form for a drumkit, where a voice is a drum.  The apply is one thread per voice.  An FM bank gets a
 * per-voice shadow of (gain, pan, depth, beta) with its first link: gl and gr come from gain and pan, the modulation index
 * depth * beta — an f64 held in two 32-bit rows of the array — from depth and beta, and each apply writes its own word and reads its
 * partner.  groove_bank_set_param, a sample-rate change and a reset upload shadow and records again from the host's copy; so
 * groove_bank_reset of an FM bank that has a link waits on the host for that upload, which a reset of any other bank does not.  A
 * sampler's gain is one word and needs no shadow: a reset leaves its records as they are, the link's last value included.  The staleness rule and the ordering are the ones above.  A Welsh index on these
 * banks, an FM index on a sampler bank and the reverse are refused, each with its message.
 * The link returned is an ordinary one: capture, apply / trip apply, reset and destroy under their own rules.  groove_bank_destroy
 * leaves it without a target: its next apply is an error. */
int groove_ctl_bank_link_create(groove_ctx* ctx, const groove_ctl_source* src, uint32_t n_src, groove_bank* target, uint32_t control_index,
                                groove_ctl_link** out);
int groove_ctl_bank_trip_create(groove_ctx* ctx, const groove_ctl_step* steps, uint32_t n_steps, const double* start_beat, uint32_t n_src,
                                groove_bank* target, uint32_t control_index, groove_ctl_link** out);
/* A WET link / WET trip: a controller linked to an effect's wet-dry-mix (GROOVE_CTL_FX_WET), which the three creates above refuse.
 * Every effect kernel reads the per-lane mix from device memory at launch and selects `wet < 1` per lane, so the link's apply is the
 * plain link's kernel writing that array: groove_fx_set_param's law, (float)clamp01(v), no host wait, no copy.  The one decision the
 * HOST takes from the value is a reverb's kernel form, so a reverb counts its live wet links: while it has one it is treated as not
 * all wet whatever the host's copy says — serial with groove_set_fx_wet_reverb_run off, the fused run's forms with it on — and it is
 * all wet again once the last link is destroyed and the host's copy says so.
 *   Targets: every kind but GROOVE_FX_MIXER (the identity launches nothing and reads no mix).  Sources, steps and n_src are checked
 *   as by groove_ctl_link_create / groove_ctl_trip_create.
 * The staleness rule holds unchanged: a later groove_fx_set_param(s) re-uploads the host's copy, the link's next apply overwrites it.
 * The link returned is an ordinary one: capture, apply / trip apply, reset and destroy under their own rules. */
int groove_ctl_wet_link_create(groove_ctx* ctx, const groove_ctl_source* src, uint32_t n_src, groove_fx* target, groove_ctl_link** out);
int groove_ctl_wet_trip_create(groove_ctx* ctx, const groove_ctl_step* steps, uint32_t n_steps, const double* start_beat, uint32_t n_src,
                               groove_fx* target, groove_ctl_link** out);
/* Resets::reset (Orchestrator::skip_to_start, orchestrator.rs:971-983): a signal link forgets what it captured. */
int groove_ctl_link_reset(groove_ctl_link* link);
/* Orchestrator::unlink_control (orchestrator.rs:1296-1320).  groove_shutdown frees the links that are still alive. */
int groove_ctl_link_destroy(groove_ctl_link* link);

/* ---- mix bus (Orchestrator::gather_audio, orchestrator.rs:367-470) ------------------------ */
/* bus_dev[f][ch] (+)= sum over blocks and lanes of block[ch][f][lane]. */
int groove_mix(groove_ctx* ctx, groove_block* const* blocks, uint32_t n_blocks, uint32_t frames,
               float* bus_dev, int accumulate);
/* groove_mix of ONE block that a render or an effect chain has just filled (its lane sums are still valid: a few short rows),
 * with the reduction of those rows DEFERRED the way groove_bank_render_mix_deferred defers a render's: the next effect-chain
 * launch on the ctx stream (or the next deferred render) sums them onto the bus in passing, and groove_bus_flush — or any call
 * that waits for the ctx stream, records an event on it or touches a bus — does it at the latest.  For the host that walks a
 * chain block after block (render, effects, main-mixer sum: orchestrator.rs:397-457): the step loses a launch that is all
 * latency.  A block without valid lane sums (or with more than 2,048 rows) is mixed by groove_mix at once.  No reference
 * counterpart. */
int groove_mix_deferred(groove_ctx* ctx, groove_block* block, uint32_t frames, float* bus_dev, int accumulate);
/* Device scratch the caller can use as a bus: frames*2 floats, zeroed. */
int groove_bus_create(groove_ctx* ctx, size_t frames, float** out_dev);
int groove_bus_destroy(groove_ctx* ctx, float* bus_dev);
int groove_bus_zero(groove_ctx* ctx, float* bus_dev, size_t frames);
int groove_download(groove_ctx* ctx, const float* dev, float* host, size_t n_floats);
int groove_upload(groove_ctx* ctx, float* dev, const float* host, size_t n_floats);
/* WAV sink quantisation (orchestration/src/helpers.rs:79-91): interleaved i16 = (x*32767) as i16
 * (truncate toward zero, saturating), computed on the device from bus_dev[frames][2]. */
int groove_bus_to_i16(groove_ctx* ctx, const float* bus_dev, size_t frames, int16_t* host_out);

/* ---- multi-GPU (no reference counterpart) ----------------------------------- */
/* One process per GPU.  Rank 0 calls groove_comm_unique_id, the launcher broadcasts the 128
 * bytes, every rank calls groove_comm_init; groove_bus_reduce sums bus_dev[frames_total][2]
 * (fp32) onto `root` with one RCCL reduce over xGMI. */
int groove_comm_unique_id(groove_ctx* ctx /* may be NULL */, uint8_t id_out[128]);
int groove_comm_init(groove_ctx* ctx, const uint8_t id[128], int rank, int world_size);
/* Ranks that joined the communicator (ncclCommCount); 1 when no communicator has been set up.  The
 * launcher checks it against the number of GPUs it asked for (bench.py: `rccl_ranks`). */
int groove_comm_ranks(groove_ctx* ctx, int* out_ranks);
int groove_comm_destroy(groove_ctx* ctx);
int groove_bus_reduce(groove_ctx* ctx, float* bus_dev, size_t frames_total, int root);

#ifdef __cplusplus
}
#endif
#endif /* GROOVE_HIP_H */
