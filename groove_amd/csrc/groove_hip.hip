// groove_hip.hip — implementation of the C ABI in include/groove_hip.h.
//
// Host side of the MI355X render path: owns device memory, derives packed per-lane
// parameters (derive.h), queues block-granular note events, launches the kernels in
// kernels.h (voice kernels on per-kind / per-bank side streams, everything else on the ctx stream).
// Nothing here falls back to a CPU path: every entry point
// either launches HIP work or returns an error.
#include "../../include/groove_hip.h"
#include "kernels.h"
#include "welsh_tp.h"
#include "welsh_split.h"
#include "fx_tp.h"
#include "ctl_link.h"
#include <dlfcn.h>
#include <hip/hip_ext.h> // hipExtLaunchKernelGGL: an event bound to a kernel's own completion signal (launch_reduce, launch_welsh_tp)
#include <rccl/rccl.h> // types, enumerators and prototypes only: the library itself is dlopen'ed (rccl_open)
#include <string>
#include <map>
#include <vector>
#include <algorithm>
#include <cstring>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <memory>
#include <thread>
#include <new>

using namespace groove;

namespace {
thread_local std::string g_last_error;
}

// The lane order of a bank that keeps its voices in another order than the caller gave them (patch-major regrouping,
// welsh_plan.h welsh_patch_major_order): src_lane[caller's lane] = the library's lane.  Shared by the bank and by every block its renders
// filled, so that a block outlives a re-grouping (or the bank) with the order its content has.
struct LaneOrder {
  uint32_t n = 0;
  uint32_t* d_src_lane = nullptr;
  ~LaneOrder() { if (d_src_lane) (void)hipFree(d_src_lane); }
};

struct groove_block {
  groove_ctx* ctx;
  uint32_t n, cap;
  float* d;
  // LAZY LANE ORDER.  A render of a regrouped bank fills `d_alt` in the LIBRARY's lane order (coalesced rows) and tags the
  // block with that order; `d` — the pointer the caller can ask for — is only produced (one gather pass, block_normalise)
  // when something needs the caller's order: an effect (per-lane parameters), an element-wise accumulate, a download,
  // groove_block_device_ptr.  The mix bus never does (a sum over the lanes has no order), so render + mix of a regrouped
  // bank costs what it costs for a grouped one (round 2 gathered every block: 2.85 ms against 0.97 at 1,000,000 voices).
  float* d_alt = nullptr;
  std::shared_ptr<LaneOrder> order; // set: the block's current content is d_alt, in this order
  uint32_t order_frames = 0;
  // groove_bank_render_async: the producer kernels run on side streams; ev_ready[k] is recorded on
  // side stream k behind them, ready_mask says which are outstanding (block_acquire clears it).
  hipEvent_t ev_free = nullptr, ev_ready[16] = {};
  uint32_t ready_mask = 0;
  bool released = false; // groove_block_release: ev_free marks the end of the block's consumers so far
  bool free_marked = false; // ev_free already completes with the block's last consumer (groove_mix bound it to its last kernel): a release needs no record
  // The lane sums of the block, as the render that filled it left them: sums[row][ch][frame], `sum_rows` rows whose
  // column totals are the block's bus contribution (the fused path's partial rows).  groove_mix reduces these 8 MB
  // instead of reading 2 GB of voice block back; anything else that writes the block clears sums_valid.
  float* d_sums = nullptr;
  size_t sums_cap = 0;
  uint32_t sum_rows = 0, sum_frames = 0;
  bool sums_valid = false;
  // The all-pass stream (groove_set_fx_allpass_stream; fx_launch_run): a chain that ends in a reverb leaves the block's last
  // kernel — the reverb's two all-passes — on a side stream, beside the next block's fused run.  That kernel reads the comb sum
  // from the BLOCK's own staging buffer (no other block's kernels touch it) and writes the lane sums into one of two buffers the
  // block keeps for that stream alone (only all-pass kernels, all on that one stream, and flushes that order themselves against
  // it, ever touch them): nothing here needs a cross-stream wait in the steady state.
  float* d_stage = nullptr;
  uint32_t stage_cap = 0; // frames
  float* d_sums_ap[2] = {nullptr, nullptr};
  size_t sums_ap_cap[2] = {0, 0};
  int ap_flip = 0;
  bool sums_on_ap = false; // the valid lane sums are d_sums_ap[ap_flip], written on the all-pass stream
};

// (BankKind — BANK_WELSH, BANK_FM, BANK_SAMPLER — is ctl_core.h's: the control links' route table is asked by it)

// One distinct filter description of a Welsh patch: what derive.h welsh_filter_f32_error depends on (welsh_upload_params).
struct F32FilterKey {
  float c0, d1, c2, d3, hz, start, end, depth;
  uint32_t bits;
  bool operator<(const F32FilterKey& o) const { return std::memcmp(this, &o, sizeof(F32FilterKey)) < 0; }
};
struct groove_bank {
  groove_ctx* ctx;
  BankKind kind;
  std::map<F32FilterKey, bool> f32_memo; // WF_FILTER_F32 verdicts measured so far at f32_memo_sr (0.6 ms each: not again for every control change)
  double f32_memo_sr = 0.0;
  uint32_t n;
  uint32_t pw, sw; // param / state words per lane
  uint32_t* d_params = nullptr;
  uint32_t* d_state = nullptr;
  double* d_cold = nullptr; // welsh: [4][n]; fm: ratio [n]
  WaveDesc* d_waves = nullptr;   // welsh: virtual waves (runs of <= 64 voices sharing a patch)
  size_t vwaves_cap = 0;
  // welsh, fused path: block pipeline (render_mix_pipelined).  Two slots of partial rows / segment sums and
  // the events that order slot reuse: a base kind's render of block b+2 waits for the reduce of block b.
  float* d_pipe_part[2] = {nullptr, nullptr};
  float* d_pipe_seg[2] = {nullptr, nullptr};
  size_t pipe_part_cap[2] = {0, 0}, pipe_seg_cap[2] = {0, 0};
  hipEvent_t ev_render_done[kBaseKinds + 4][2] = {};
  hipEvent_t ev_reduce_done[2] = {nullptr, nullptr};
  bool reduce_recorded[2] = {false, false};
  int pipe_slot = 0;
  // groove_bank_render_mix_paced: the reduction of the block rendered by the last paced call, launched by the next one (or a flush)
  struct { bool active = false; int slot = 0; uint32_t rows = 0, frames = 0, used = 0; float* bus = nullptr; int accumulate = 0; } paced;
  int stream_slot = 0; // side stream of a single-kernel bank (FM, sampler, per-lane Welsh) in the asynchronous fused path
  bool ctx_touched = true; // the ctx stream has worked on this bank's state since its last asynchronous render waited for it
  int side_mode = 0;    // which side streams carried this bank's last asynchronous work: 0 none, 1 one per base kind, 2 stream_slot
  // welsh: what the launches read of the bank's plan (welsh_plan.h): the lane permutation, the number of virtual waves (0: the per-lane
  // kernel), the time-parallel form's two conditions, the slice lengths of the sorted lists and the mix kernel's sections of the striped ones
  WelshLayout plan;
  std::shared_ptr<LaneOrder> order; // device copy of plan.inv, shared with the blocks this bank's renders fill (groove_block: lazy lane order)
  uint8_t* d_wg_cls = nullptr;   // welsh: oscillator class pair of each entry of d_wg_list
  uint8_t* d_wg_base = nullptr;  // welsh: base kind of each entry of d_wg_list (the all-kinds kernel of small banks)
  uint8_t* d_wg_f32 = nullptr;   // welsh: 1 where the entry's patches carry WF_FILTER_F32 (read by the fused mix kernel)
  // welsh: workgroup ids (groups of 4 virtual waves) sorted by kind (kernels.h).  All four d_wg_ arrays hold 2 * wg_list_cap entries: plan.sorted
  // from entry 0, plan.striped — the mix kernel's sections, [wg_list_cap + mix_off[s], + mix_cnt[s]) — from entry wg_list_cap
  uint32_t* d_wg_list = nullptr;
  size_t wg_list_cap = 0;
  float* d_pcm = nullptr;   // sampler bank: [bank_frames] values, or [bank_frames] interleaved left, right pairs ...
  bool pcm_stereo = false;  // ... of a stereo bank (groove_sampler_create_stereo): picks the kernels' STEREO instantiations
  uint32_t pcm_interp = GROOVE_SAMPLE_NEAREST; // sampler bank: a groove_sample_interpolation, read at every launch (picks the kernels' MODE instantiations)
  // sampler bank: the samples' forward loops (groove_bank_set_sample_loops; empty: never set), whether any sample has one (picks the
  // kernels' LOOP instantiations) and, allocated with the first loop, each VOICE's loop words [2][n] — start row, end row, its sample's
  std::vector<groove_sample_loop> loops;
  bool looped = false;
  uint32_t* d_loops = nullptr;
  // sampler bank: the samples' amplitude envelopes (groove_bank_set_sample_envelopes; empty: none) and which samples have one, whether
  // any has (picks the kernels' ENV instantiations, which are built on the LOOP text: d_loops is then allocated too, zeros for no loop)
  // and, allocated by the first setter call, each VOICE's EnvParams and EnvState words [13][n] (dsp_core.h kSampleEnvWords)
  std::vector<groove_envelope_params> envs;
  std::vector<uint32_t> env_enabled;
  bool enveloped = false;
  uint32_t* d_env = nullptr;
  std::string form_text; // groove_bank_kernel_form's answer for an enveloped bank (the others are literals)
  // welsh: the bank links' per-lane shadow [CTL_DCA_WORDS][n] of dca gain and pan (internal lane order; ctl_link.h), allocated with the first
  // gain or pan link onto the bank and refreshed by welsh_upload_params from then on; and how many live links reach the filter cutoff
  // (welsh_plan.h welsh_flag_filter_f32: no WF_FILTER_F32 while there is one).  fm: the same owner with CTL_FM_WORDS rows — gain, pan, depth,
  // beta per voice in the caller's order — refreshed by fm_upload_params; a sampler bank has none (its gain is one word of the record)
  float* d_dca = nullptr;
  uint32_t cutoff_links = 0;
  groove_note_event* d_ev[2] = {nullptr, nullptr};
  // pinned staging of queued note events, two slots in rotation: flush_events hands the events to the ctx
  // stream and returns without a host synchronisation (a project with note events in every block would
  // otherwise serialise host and GPU once per block)
  groove_note_event* h_ev[2] = {nullptr, nullptr};
  size_t h_ev_cap[2] = {0, 0};
  hipEvent_t ev_staged[2] = {nullptr, nullptr};
  bool staged[2] = {false, false};
  int ev_slot = 0;
  std::vector<groove_note_event> pending;
  InlineEvents inline_ev{};  // sampler: this block's events, to ride in the next time-parallel render's arguments (flush_events)
  std::vector<groove_welsh_params> welsh;
  std::vector<groove_fm_params> fm;
  std::vector<groove_sampler_params> sampler;
  std::vector<groove_sample_desc> descs;
};

struct groove_fx {
  groove_ctx* ctx;
  uint32_t kind, n;
  std::vector<groove_fx_params> p;
  float* d_fa = nullptr;   // per-lane float param A (ceiling / limit_min / attenuation)
  float* d_fb = nullptr;   // per-lane float param B (limit_max / ratio)
  uint32_t* d_ua = nullptr; // per-lane uint param (bits)
  float* d_wet = nullptr;
  double* d_coef = nullptr; // [5|6][n]
  float* d_shadow = nullptr; // [CTL_SHADOW_WORDS][n]: the filter parameters the coefficients derive from; only once a filter link has been made onto the effect
  double* d_st = nullptr;   // [4][2n]
  float* d_ring = nullptr;  // rows of 2n floats
  size_t ring_rows = 0;
  // uniform geometry
  uint32_t N = 0, w = 0, voices = 1, spacing = 0;
  bool all_wet = true; // every lane of the HOST's copy has wet == 1 (enables the split reverb path)
  uint32_t wet_links = 0; // live wet links (groove_ctl_wet_link_create / groove_ctl_wet_trip_create): above zero the device's wet values are not the host's, so a reverb counts as not all wet (fx_needs_dry)
  ReverbGeom geo{};
  // reverb, direct all-pass form (kernels.h): second copies of the two all-pass rings (read one, write the other, swap)
  // and a staging block for the comb sum, allocated at first use
  uint64_t ap_alt[2] = {0, 0};
  float* d_tmp = nullptr;
  uint32_t tmp_cap = 0; // frames
  bool ap_busy = false;         // the all-pass lines' last kernel went to the all-pass stream (ap_join before the ctx stream touches them)
  int last_side = -1;           // side stream whose kernels touched this effect last (-1: the ctx stream); fx_acquire_ctx
  hipEvent_t ev_done = nullptr; // end of that use
  bool done_recorded = true;    // false: the last use was a kernel whose end another event marks (a fused render's): ev_done is recorded on demand
};

// A controller linked to one parameter of one target (groove_ctl_*; csrc/ctl_link.h).  The target is one of four, by the route of
// (target kind, control_index) (ctl_core.h: ctl_fx_route, ctl_bank_route): an effect's plain parameter words (d_fa, d_ua, or d_wet for a
// wet link), a filter's parameter shadow and coefficients, a Welsh bank's records, an FM or sampler bank's voices.  Everything the apply
// kernel reads of the SOURCE lives on the device: an LFO's or signal's per-source-lane description (uploaded once, and again when the
// sample rate changes), the captured samples and the flag that says there are any; or a trip's step table.
struct groove_ctl_link {
  groove_ctx* ctx;
  uint32_t source, n_src, control_index;
  groove_fx* target; // nullptr once the target has been destroyed (groove_fx_destroy clears it), and on a bank link
  groove_bank* bank = nullptr; // a bank link's target (groove_ctl_bank_link_create); on_bank stays set when groove_bank_destroy clears it
  bool on_bank = false;
  std::vector<groove_ctl_source> src;
  uint64_t* d_lanes = nullptr; // the LFO / signal lanes (ctl_core.h: ctl_lanes_layout)
  float* d_value = nullptr;    // [n_src] captured samples (signal source)
  uint32_t* d_captured = nullptr;
  // a trip link's step table (ctl_core.h: ctl_trip_layout) — uploaded once: nothing in it depends on the sample rate
  double* d_trip = nullptr;
  uint32_t n_steps = 0;
};

// Events that only order the library's own streams on one device: no timing, and no system-scope fence
// (cache writeback + invalidate) when they are recorded — the host reads results through
// hipMemcpy / hipStreamSynchronize, which fence by themselves.
#ifndef GROOVE_SOURCE_HASH
#define GROOVE_SOURCE_HASH "unknown" /* groove_amd/Makefile: sha256 of the library's sources, first 16 hex digits */
#endif
constexpr unsigned kSyncEventFlags = hipEventDisableTiming | hipEventDisableSystemFence;
constexpr int kBankStreams = 4;                         // shared round-robin by single-kernel banks (FM, sampler, per-lane Welsh)
constexpr int kSideStreams = kBaseKinds + kBankStreams;
static_assert(kBaseKinds == 6 && kBankStreams == 4, "groove_init lists the side streams in creation order"); // + one per Welsh base kind; the ctx stream carries events, reductions and the rest
static_assert(kSideStreams <= 16, "groove_block::ev_ready holds one event per side stream");
struct groove_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = true;
  hipStream_t side_stream[kSideStreams] = {}; // kernels of the other workgroup kinds run beside the main one
  hipStream_t placeholder_stream = nullptr;   // created, never used (groove_init)
  unsigned long long* hb = nullptr;           // -DGROOVE_HEARTBEAT (diagnostic build): [workgroups started, finished] of the per-kind kernels, in coherent host memory
  uint32_t* d_diag = nullptr;                 // DiagCounters (diag.h): the segment guard's counter, read by groove_debug_info
  hipEvent_t ev_fork = nullptr, ev_join[kSideStreams] = {};
  bool side_busy[kSideStreams] = {};    // work enqueued on the side stream since the last join
  bool fork_pending[kSideStreams] = {}; // the side stream has not yet waited for ev_fork
  bool need_fork = true;                // ctx-stream work since the last fork that side streams must wait for
  uint32_t tp_max_voices = kTpMaxVoices; // Welsh banks up to this size render time-parallel (welsh_tp.h); GROOVE_TP_MAX_VOICES overrides, 0 = never
  uint32_t fx_tp_max_lanes = 4096;       // IIR effect banks of up to this many lane-channels (half as many for the 24 dB low-pass) run time-parallel (fx_tp.h: measured crossovers, tools/fx_bench.py)
  // Mid-size Welsh banks (too big for the time-parallel form, too small to fill the chip with one voice-wave per wavefront):
  // the ROLE-SPLIT kernel (welsh_split.h: four wavefronts per 64 voices, pipelined over the block's frames) for banks of up
  // to this many virtual waves; 0 = never.  groove_set_split_max_waves.
  uint32_t split_max_waves = 1024;      // 65,536 voices = one workgroup (sixteen wavefronts) per CU; measured (round 3, blocks 5-24): 20,000 voices 0.120 -> 0.090 ms per block, 32,768 0.119 -> 0.090, 65,536 0.123 -> 0.095; 80,000 (a second round of workgroups) 0.135 -> 0.153: not above
  uint32_t pipeline_min_waves = 3800;   // banks at least this long (~243,000 voices; 7,000 = ~450,000 until the end of round 6: with the FAST copies of the bodies in both kernels the crossover moved down — in one job, tools/ab_env.sh, mix kernel against all-kinds kernel: 200,000 voices 0.114 against 0.110 ms per block, 250,000 0.120 against 0.121 - 0.123, 300,000 0.125 against 0.158, 400,000 0.139 against 0.188, 500,000 0.164 against 0.212) run the mix kernel (one launch per base kind before round 6) and pipeline their fused blocks; smaller ones take the all-kinds kernel (round 2, blocks 5-44 of the timeline: 300,000 voices 0.275 -> 0.250 ms per block, 500,000 0.357 -> 0.342; 600,000 0.372 against 0.400.  Round 5: the per-kind kernels alone carry the fp32 filter kind and the crossover moved down from ~550,000 — the driver's window, in-job, per-kind against all-kinds: 500,000 voices 0.271 against 0.281, 420,000 0.246 against 0.244, 350,000 0.223 against 0.225: profiles/r05_pipeline_threshold_ab.log)
  // How many of the bank streams exist and are handed out.  Three: with the ctx stream and the four
  // kind streams that is eight streams; a ninth lands on a hardware queue that already carries one of the others, and a
  // project with a bank on it ran three times slower (mixed-131072: 0.12 -> 0.39 ms per block whenever a bank had the
  // fourth bank stream, whichever bank it was; tools/micro/slot_probe.py).
  int bank_streams = 3;
  // Normal-priority streams for the class-specialised Welsh kinds.  Three: the fourth kind shares the first kind's stream
  // (1,000,000 voices: 0.511 against 0.515 ms per block with four).  docs/STREAMS.md item 10: the k-th stream a process
  // creates lands on hardware queue (k - 1) mod 4, so the fifth (and the ninth) shares the ctx stream's queue; the fifth
  // used to be the fourth kind stream and is now a placeholder nobody uses.
  int kind_streams = 3;
  uint32_t look_ahead = 3u; // RenderConsts::look: bit 0 the coefficient look-ahead, bit 1 the LFO look-ahead (kernels.h); GROOVE_LOOK_AHEAD=<bits>, groove_set_look_ahead (tests render the same bank with and without)
  int next_stream_slot = 0;             // round-robin side-stream assignment of single-kernel banks
  uint32_t fm_tp_max_voices = kFmTpMaxVoices;
  // Welsh banks of at least this many voices whose adjacent pairs share a patch render two voices per wavefront
  // (welsh_tp_kernel<.., VPW = 2>): above 3,072 voices the one-voice form no longer fits the SIMDs in one round
  uint32_t tp_vpw2_min_voices = 3073; // groove_set_time_parallel_pair_min_voices (0 = never)
  // events that mark the end of ONE kernel (a block's render, a block's last reduction) are bound to that dispatch's own
  // completion signal instead of being recorded behind it (a barrier packet each, ~5 us of the stream's timeline)
  uint32_t fm_tp_vpw4_min_voices = 4096; // GROOVE_FM_TP_VPW4_MIN_VOICES (0 = never): FM banks of at least this many voices, four voices per wavefront
  // (Round 3 switched this off when fresh runs stalled with it on; the stall was the zero-frame segment of DESIGN.md section 7,
  // which had nothing to do with events.  On again in round 4; GROOVE_BIND_EVENTS=0 for A/B.)
  bool bind_events = true;
  uint32_t fx_seg_max_lanes = 49152;     // biquad banks of up to this many lane-channels take the four-segment kernel (measured, tools/fx_bench.py: 8,192 lane-channels 17.5 -> 9.3 us, 32,768 19.4 -> 15.6, 131,072 42.9 -> 58.4; 0 = never)
  // groove_set_fx_allpass_stream: the side stream that carries the all-passes of chains that END in a reverb (-1: the ctx stream
  // carries them, behind the run).  deferred_ap: lane sums written on that stream that groove_mix_deferred has taken and the NEXT
  // all-pass launch (same stream: ordered) puts on their bus.
  int fx_ap_stream = -1;
  TpPrev deferred_ap;
  hipEvent_t ev_ap_run = nullptr, ev_ap_x = nullptr;
  bool seq_allpass = false;             // GROOVE_FX_SEQ_ALLPASS=1: the sequential all-pass kernel (A/B and bit-identity tests)
  bool fx_wet_reverb_run = false;       // groove_set_fx_wet_reverb_run / GROOVE_FX_WET_REVERB_RUN=1: a partly wet reverb keeps the fused run (fx_form_of)
  bool chunked_allpass = false;         // GROOVE_FX_CHUNKED_ALLPASS=1: the chunk-parallel all-pass kernel instead of the direct one
  uint32_t sr = GROOVE_DEFAULT_SAMPLE_RATE;
  // Blocking waits (groove_synchronize and every call that hands data to the host) poll the stream with a deadline
  // instead of sleeping inside hipStreamSynchronize: a kernel that does not complete then comes
  // back as an ERROR that names the streams still busy, not as a hang.  0 = wait for ever.  GROOVE_SYNC_TIMEOUT_MS.
  uint32_t sync_timeout_ms = 60000;
  unsigned long long host_waits = 0, host_waits_blocked = 0, host_wait_ns = 0; // wait_deadline: calls, calls that found work pending, time blocked (groove_debug_info)
  bool safe_streams = false;            // GROOVE_SAFE_STREAMS=1: one priority, four streams in all (ctx + three that kinds and banks share)
  bool comm_before_streams = false;     // groove_init_comm: the RCCL communicator (and its streams) existed before the library's own
  int streams_created = 0;              // hipStreamCreate* calls of this ctx, in order: ctx, kind streams, placeholder, bank streams
  std::string err;
  std::vector<groove_bank*> banks;
  std::vector<groove_fx*> fxs;
  std::vector<groove_ctl_link*> links;
  float* d_partial = nullptr;
  size_t partial_cap = 0;
  float* d_fpart = nullptr;  // fused path: partial[workgroup][2][frames]
  size_t fpart_cap = 0;
  // groove_bank_render_mix_deferred: two more row buffers in alternation, and the block whose rows are waiting for the next
  // deferred render (or bus_flush) to put them on the bus
  float* d_dpart[2] = {nullptr, nullptr};
  size_t dpart_cap[2] = {0, 0};
  int dpart_next = 0;
  TpPrev deferred; // (all zero when nothing is pending: a launch takes it as its `prev` as it stands)
  size_t deferred_owned_cap = 0;
  // groove_mix_deferred takes the block's row-sum buffer AWAY from the block (owned_cap != 0: the pending rows live in a buffer
  // nobody else can write) and hands the block one of these instead; a consumed buffer comes back here (deferred_taken)
  std::vector<std::pair<float*, size_t>> spare_sums;
  bool f32_filter = true; // WF_FILTER_F32: patches whose 24 dB filter is measured safe in fp32 take the fp32 recurrence in the fused mix kernel (GROOVE_F32_FILTER=0: never)
  std::vector<groove_bank*> paced_order; // banks with a pending paced reduction, in call order (= the order of their sums on a bus)
  float* d_fseg = nullptr;   // fused path: seg[segments][2*frames]
  size_t fseg_cap = 0;
  int16_t* d_i16 = nullptr;
  size_t i16_cap = 0;
  // RCCL (dlopen'ed lazily)
  void* rccl = nullptr;
  void* comm = nullptr;
  int rank = 0, world = 1;
};

namespace {

// Returned through hipError_t-typed helpers whose failure is already described in ctx->err: GHIP passes it on untouched.
constexpr hipError_t kGrooveFailed = hipErrorAssert;
int fail(groove_ctx* ctx, const std::string& msg) {
  g_last_error = msg;
  if (ctx) ctx->err = msg;
  return 1;
}
#define GHIP(ctx, expr)                                                                    \
  do {                                                                                     \
    hipError_t e_ = (expr);                                                                \
    if (e_ == hipErrorNotReady) return 2; /* a deadline passed: wait_deadline wrote the message */ \
    if (e_ == kGrooveFailed) return 1;    /* the callee has written the message (ctx_wait: bus_flush) */ \
    if (e_ != hipSuccess)                                                                  \
      return fail(ctx, std::string(#expr) + ": " + hipGetErrorString(e_));                 \
  } while (0)

// Synchronous copies go through the CTX stream, never the null stream: the null stream is one more normal-priority
// stream for the runtime to map, and with the four kind streams it made five on four hardware queues — the fourth kind
// stream shared its queue with it (rocprofv3 trace, round 2).
RenderConsts render_consts_of(const groove_ctx* ctx) { RenderConsts rc = render_consts(ctx->sr); rc.look = ctx->look_ahead; return rc; }
const char* side_stream_name(int k) {
  static const char* names[] = {"kind stream 0 (Welsh F32 static; also kinds 3 and 4)", "kind stream 1 (Welsh F32 retune; also kind 5)",
                                "kind stream 2 (Welsh smooth-LFO static)", "kind stream 3 (Welsh smooth-LFO retune)",
                                "kind stream 4", "kind stream 5", "bank stream 0", "bank stream 1", "bank stream 2", "bank stream 3"};
  return k >= 0 && k < 10 ? names[k] : "side stream";
}
// Wait for `st` (or, if `ev` is given, for that event) with the ctx's deadline.  hipSuccess when it completed;
// hipErrorNotReady when the deadline passed — ctx->err then names every library stream that still has work.  Nothing is
// cancelled: the work stays queued and a later wait may still see it complete.
hipError_t wait_deadline(groove_ctx* ctx, hipStream_t st, hipEvent_t ev, const char* what) {
  if (ctx->sync_timeout_ms == 0) return ev ? hipEventSynchronize(ev) : hipStreamSynchronize(st);
  const auto t0 = std::chrono::steady_clock::now();
  const auto limit = std::chrono::milliseconds(ctx->sync_timeout_ms);
  for (uint32_t spins = 0;; ++spins) {
    const hipError_t q = ev ? hipEventQuery(ev) : hipStreamQuery(st);
    if (q != hipErrorNotReady) {
      ctx->host_waits += 1;
      if (spins) { ctx->host_waits_blocked += 1; ctx->host_wait_ns += (unsigned long long)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count(); }
      return q;
    }
    const auto waited = std::chrono::steady_clock::now() - t0;
    if (waited > limit) break;
    // the first ~100 us busy-poll (most waits of this path are that short), then yield, then sleep in growing steps.  (A sleep of
    // 50 us returns after 100 - 150: with sleeps from 2 ms on, a 2.5 ms wait — the end of a 20-block window of a 125,000-voice shard —
    // came back up to 0.1 ms late, 5 us per block of a 0.12 ms block; waits of up to 20 ms now yield.)
    if (spins < 64) continue;
    if (waited < std::chrono::milliseconds(20)) std::this_thread::yield();
    else std::this_thread::sleep_for(std::chrono::microseconds(waited < std::chrono::milliseconds(200) ? 50 : 500));
  }
  std::string busy;
  if (hipStreamQuery(ctx->stream) == hipErrorNotReady) busy += "ctx stream";
  for (int k = 0; k < kSideStreams; ++k) {
    hipStream_t s = ctx->side_stream[k];
    if (!s) continue;
    bool dup = false;
    for (int j = 0; j < k; ++j) dup = dup || ctx->side_stream[j] == s;
    if (dup) continue;
    if (hipStreamQuery(s) == hipErrorNotReady) { if (!busy.empty()) busy += ", "; busy += side_stream_name(k); }
  }
  // which events of the block pipelines are still pending (render_mix_pipelined): a render that is pending although the
  // reduction it waited for is done is a kernel that does not finish; pending reductions behind done renders would be the ctx
  // stream itself
  std::string pipes;
  for (size_t bi = 0; bi < ctx->banks.size() && bi < 4; ++bi) {
    const groove_bank* bk = ctx->banks[bi];
    for (int slot = 0; slot < 2; ++slot) {
      if (!bk->ev_reduce_done[slot]) continue;
      pipes += "; bank " + std::to_string(bi) + " slot " + std::to_string(slot) + ": reduction " + (hipEventQuery(bk->ev_reduce_done[slot]) == hipSuccess ? "done" : "PENDING") + ", renders";
      for (int k = 0; k < kSideStreams; ++k)
        if (bk->ev_render_done[k][slot]) pipes += std::string(" ") + std::to_string(k) + (hipEventQuery(bk->ev_render_done[k][slot]) == hipSuccess ? ":done" : ":PENDING");
    }
  }
  (void)hipGetLastError(); // hipErrorNotReady is sticky in the runtime's last-error slot
  busy += pipes;
#ifdef GROOVE_HEARTBEAT
  if (ctx->hb) {
    const unsigned long long s0 = ((volatile unsigned long long*)ctx->hb)[0], f0 = ((volatile unsigned long long*)ctx->hb)[1];
    std::this_thread::sleep_for(std::chrono::milliseconds(500));
    const unsigned long long s1 = ((volatile unsigned long long*)ctx->hb)[0], f1 = ((volatile unsigned long long*)ctx->hb)[1];
    busy += "; heartbeat of the per-kind kernels: workgroups started " + std::to_string(s0) + " finished " + std::to_string(f0) + ", half a second later started " + std::to_string(s1) + " finished " + std::to_string(f1);
  }
#endif
  fail(ctx, std::string(what) + ": not complete after " + std::to_string(ctx->sync_timeout_ms) + " ms (GROOVE_SYNC_TIMEOUT_MS / groove_set_sync_timeout_ms); still busy: " +
                (busy.empty() ? "nothing (the wait itself raced the completion)" : busy) +
                ".  The work stays queued and a later wait may still see it complete; if it does not, tear the process down (DESIGN.md section 7: the one stall this path has known was an endless loop in a render kernel, fixed in round 4; groove_debug_info's zero_segments counts its trigger).");
  return hipErrorNotReady;
}
int bus_flush(groove_ctx* ctx); // a deferred block's rows onto its bus (groove_bank_render_mix_deferred), defined with the reductions below
hipError_t ctx_wait(groove_ctx* ctx, const char* what = "wait for the ctx stream") {
  if (bus_flush(ctx)) return kGrooveFailed; // (its own message stands.)  Whoever waits for the ctx stream expects every bus to be complete behind it
  return wait_deadline(ctx, ctx->stream, nullptr, what);
}
hipError_t ctx_memcpy(groove_ctx* ctx, void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
  // (a copy from or to pageable host memory blocks INSIDE hipMemcpyAsync until the stream gets to it: the deadline has to
  // be applied to the stream first)
  hipError_t e = ctx_wait(ctx, "copy on the ctx stream");
  if (e != hipSuccess) return e;
  e = hipMemcpyAsync(dst, src, bytes, kind, ctx->stream);
  if (e != hipSuccess) return e;
  return ctx_wait(ctx, "copy on the ctx stream");
}
hipStream_t side_stream_of(groove_ctx* ctx, int k) {
  if (!ctx->side_stream[k] && hipStreamCreateWithFlags(&ctx->side_stream[k], hipStreamNonBlocking) != hipSuccess) {
    ctx->side_stream[k] = nullptr;
    fail(ctx, "side stream: hipStreamCreate failed");
    return ctx->stream; // degrade to the ctx stream: still ordered, just not concurrent
  }
  return ctx->side_stream[k];
}
// Order the ctx stream after everything enqueued on the side streams, and make later side-stream work
// wait for whatever the ctx stream does next.  Called by every operation that touches bank state or
// parameters outside the pipelined fused render (note events, controls, state download, destroy...).
int ctx_join(groove_ctx* ctx) {
  for (int k = 0; k < kSideStreams; ++k) {
    if (!ctx->side_busy[k]) continue;
    GHIP(ctx, hipEventRecord(ctx->ev_join[k], side_stream_of(ctx, k)));
    GHIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_join[k], 0));
    ctx->side_busy[k] = false;
  }
  ctx->need_fork = true;
  return 0;
}

// Order the ctx stream after the asynchronous render that produced `blk` (groove_bank_render_async).
// Every ctx-stream operation that reads or writes a block calls this first.
int block_acquire(groove_block* blk) {
  blk->released = false; // the ctx stream is about to use the block again
  blk->free_marked = false;
  if (!blk->ready_mask) return 0;
  groove_ctx* ctx = blk->ctx;
  for (int k = 0; k < kSideStreams; ++k)
    if (blk->ready_mask & (1u << k)) GHIP(ctx, hipStreamWaitEvent(ctx->stream, blk->ev_ready[k], 0));
  blk->ready_mask = 0;
  return 0;
}
// The block's current content, whichever lane order it is in (for readers that do not care: lane sums).
inline const float* block_data(const groove_block* blk) { return blk->order ? blk->d_alt : blk->d; }
// Where a render of bank order `order` (null: the caller's own order) writes; tags the block.
int block_render_target(groove_block* blk, const std::shared_ptr<LaneOrder>& order, uint32_t frames, float** out) {
  if (!order) { blk->order.reset(); *out = blk->d; return 0; }
  if (!blk->d_alt) {
    hipError_t e = hipMalloc(&blk->d_alt, (size_t)2 * blk->cap * blk->n * 4);
    if (e != hipSuccess) return fail(blk->ctx, std::string("block (library lane order): hipMalloc: ") + hipGetErrorString(e));
  }
  blk->order = order;
  blk->order_frames = frames;
  *out = blk->d_alt;
  return 0;
}
// Produce the caller's lane order in blk->d (ctx stream; the caller has acquired the block).
int block_normalise(groove_block* blk) {
  if (!blk->order) return 0;
  groove_ctx* ctx = blk->ctx;
  const uint32_t frames = std::min(blk->order_frames, blk->cap);
  const size_t chs = (size_t)blk->cap * blk->n;
  if (frames) {
    hipLaunchKernelGGL(block_gather_kernel, dim3((blk->n + kThreads - 1) / kThreads, std::min<uint32_t>(frames, 64)), dim3(kThreads), 0, ctx->stream, blk->d, chs,
                       blk->d_alt, chs, blk->order->d_src_lane, blk->n, frames);
    GHIP(ctx, hipGetLastError());
  }
  blk->order.reset();
  return 0;
}
// An effect's memory (IIR state, rings, parameter arrays) is touched by one stream at a time: the ctx stream, or — for the
// stages groove_fx_chain_process_async runs behind a block's asynchronous render — that render's side stream.  ev_done
// marks the end of its last side-stream use; the ctx stream waits for it before it touches the effect again.
// ev_done of an effect whose last side-stream use was not followed by a record of its own: the CURRENT end of that stream
// (later than needed, never earlier: the stream runs in order)
int fx_done_event(groove_fx* fx) {
  if (fx->done_recorded) return 0;
  GHIP(fx->ctx, hipEventRecord(fx->ev_done, side_stream_of(fx->ctx, fx->last_side)));
  fx->done_recorded = true;
  return 0;
}
int fx_acquire_ctx(groove_fx* fx) {
  if (fx->last_side < 0) return 0;
  if (fx_done_event(fx)) return 1;
  GHIP(fx->ctx, hipStreamWaitEvent(fx->ctx->stream, fx->ev_done, 0));
  fx->last_side = -1;
  return 0;
}
// A bank's state is touched by one set of side streams at a time; changing the set joins first.
int bank_side_mode(groove_bank* b, int mode) {
  if (b->side_mode && b->side_mode != mode && ctx_join(b->ctx)) return 1;
  b->side_mode = mode;
  return 0;
}

template <class T>
std::vector<uint32_t> to_soa(const std::vector<T>& aos) {
  const size_t n = aos.size(), W = sizeof(T) / 4;
  std::vector<uint32_t> soa(W * n);
  for (size_t v = 0; v < n; ++v) {
    uint32_t w[sizeof(T) / 4];
    std::memcpy(w, &aos[v], sizeof(T));
    for (size_t i = 0; i < W; ++i) soa[i * n + v] = w[i];
  }
  return soa;
}
template <class T>
int upload_soa(groove_ctx* ctx, uint32_t* dst, const std::vector<T>& aos) {
  std::vector<uint32_t> soa = to_soa(aos);
  GHIP(ctx, hipMemcpyAsync(dst, soa.data(), soa.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  GHIP(ctx, ctx_wait(ctx));
  return 0;
}
inline uint32_t blocks_for(size_t items) { return (uint32_t)((items + kThreads - 1) / kThreads); }

// The bank links' (gain, pan) shadow from the host's copy of the parameters, in internal lane order (ctl_link.h: CtlBank::dca).
int welsh_upload_dca(groove_bank* b) {
  groove_ctx* ctx = b->ctx;
  const uint32_t n = b->n;
  std::vector<float> w((size_t)CTL_DCA_WORDS * n);
  for (uint32_t i = 0; i < n; ++i) {
    const groove_welsh_params& p = b->welsh[b->plan.perm.empty() ? i : b->plan.perm[i]];
    w[(size_t)CTL_DCA_GAIN * n + i] = p.dca_gain;
    w[(size_t)CTL_DCA_PAN * n + i] = p.dca_pan;
  }
  GHIP(ctx, ctx_memcpy(ctx, b->d_dca, w.data(), w.size() * 4, hipMemcpyHostToDevice));
  return 0;
}
// Welsh: derive + upload parameters only (SoA, cold values, per-wave table, workgroup lists): derive -> flag -> order -> plan
// (welsh_plan.h) -> grow -> upload.  `regroup`: the state is (being) reset, so the lane order may be chosen afresh.
int welsh_upload_params(groove_bank* b, bool regroup) {
  groove_ctx* ctx = b->ctx;
  const double sr = ctx->sr;
  const uint32_t n = b->n;
  std::vector<WelshParams> Pext(n);
  std::vector<WelshCold> Cext(n);
  for (uint32_t v = 0; v < n; ++v) Pext[v] = derive_welsh(b->welsh[v], sr, Cext[v]);
  { // WF_FILTER_F32 (derive.h welsh_filter_f32_ok): measured once per distinct filter description; none while a link moves the cutoff
    using Key = F32FilterKey;
    if (b->f32_memo_sr != sr) { b->f32_memo.clear(); b->f32_memo_sr = sr; } // (kept across uploads: a control change re-derives the bank, groove_bank_set_param)
    std::map<Key, bool>& memo = b->f32_memo;
    welsh_flag_filter_f32(Pext, ctx->f32_filter, b->cutoff_links, [&](const WelshParams& o) {
      Key k{};
      k.c0 = o.fc.c0; k.d1 = o.fc.d1; k.c2 = o.fc.c2; k.d3 = o.fc.d3; k.hz = o.cutoff_hz; k.start = o.cutoff_start; k.end = o.cutoff_end;
      k.depth = (o.flags & WF_LFO_CUTOFF) ? o.lfo_depth : 0.0f; k.bits = o.flags & (WF_RETUNE_ENV | WF_LFO_CUTOFF | WF_LFO_RESO | WF_COEF_WIDE);
      auto it = memo.find(k);
      // (~0.6 ms per distinct filter description: a bank of more than 4,096 of them — no project of the reference's shape, one patch
      // per synth — keeps the f64 recurrence, always safe, for the descriptions beyond, instead of seconds of measuring at upload)
      if (it == memo.end()) it = memo.emplace(k, memo.size() < 4096 ? welsh_filter_f32_ok(o, sr) : false).first;
      return it->second;
    });
  }
  WelshPlan plan = welsh_plan(Pext, Cext, regroup ? welsh_patch_major_order(Pext) : std::move(b->plan.perm));
  b->plan = std::move(static_cast<WelshLayout&>(plan)); // what the launches read stays with the bank; the arrays of `plan` are uploaded below
  if (regroup) {
    b->order.reset(); // blocks filled under the old order keep it alive for as long as they hold that content
    if (!b->plan.perm.empty()) {
      auto o = std::make_shared<LaneOrder>();
      o->n = n;
      GHIP(ctx, hipMalloc(&o->d_src_lane, (size_t)n * sizeof(uint32_t)));
      GHIP(ctx, ctx_memcpy(ctx, o->d_src_lane, b->plan.inv.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice));
      b->order = std::move(o);
    }
  }
  if (upload_soa(ctx, b->d_params, plan.records)) return 1;
  GHIP(ctx, ctx_memcpy(ctx, b->d_cold, plan.cold.data(), plan.cold.size() * 8, hipMemcpyHostToDevice));
  if (b->d_dca && welsh_upload_dca(b)) return 1; // the bank links' shadow follows the host's copy, in the lane order just decided
  if (plan.waves.empty()) return 0; // the per-lane kernel reads no wave and no list
  const size_t wgs = plan.sorted.list.size(), n_spec = plan.striped.list.size();
  if (b->vwaves_cap < plan.waves.size()) {
    if (b->d_waves) GHIP(ctx, hipFree(b->d_waves));
    b->vwaves_cap = plan.waves.size() + plan.waves.size() / 8 + 16;
    GHIP(ctx, hipMalloc(&b->d_waves, b->vwaves_cap * sizeof(WaveDesc)));
  }
  GHIP(ctx, ctx_memcpy(ctx, b->d_waves, plan.waves.data(), plan.waves.size() * sizeof(WaveDesc), hipMemcpyHostToDevice));
  // The four lists, each of twice the capacity: the kind-sorted list from entry 0, the mix kernel's striped copy of it from wg_list_cap.
  const bool grow = b->wg_list_cap < wgs;
  if (grow) b->wg_list_cap = wgs + wgs / 8 + 16;
  struct { void** d; const void* sorted; const void* striped; size_t entry; } lists[4] = {
      {(void**)&b->d_wg_list, plan.sorted.list.data(), plan.striped.list.data(), sizeof(uint32_t)}, {(void**)&b->d_wg_cls, plan.sorted.cls.data(), plan.striped.cls.data(), 1},
      {(void**)&b->d_wg_base, plan.sorted.base.data(), plan.striped.base.data(), 1}, {(void**)&b->d_wg_f32, plan.sorted.f32.data(), plan.striped.f32.data(), 1}};
  for (auto& l : lists) {
    if (grow) {
      if (*l.d) GHIP(ctx, hipFree(*l.d));
      GHIP(ctx, hipMalloc(l.d, 2 * b->wg_list_cap * l.entry));
    }
    GHIP(ctx, ctx_memcpy(ctx, *l.d, l.sorted, wgs * l.entry, hipMemcpyHostToDevice));
    if (n_spec) GHIP(ctx, ctx_memcpy(ctx, (char*)*l.d + b->wg_list_cap * l.entry, l.striped, n_spec * l.entry, hipMemcpyHostToDevice));
  }
  return 0;
}

// FM / sampler: derive + upload the parameter SoA only — the state and d_cold stay where they are (groove_bank_set_param).  An FM bank
// that has a link keeps its (gain, pan, depth, beta) shadow beside the records, from the same host copy.
std::vector<FmParams> fm_derive_params(const groove_bank* b) {
  std::vector<FmParams> P(b->n);
  for (uint32_t v = 0; v < b->n; ++v) P[v] = derive_fm(b->fm[v], b->ctx->sr);
  return P;
}
std::vector<SamplerParams> sampler_derive_params(const groove_bank* b) {
  std::vector<SamplerParams> P(b->n);
  for (uint32_t v = 0; v < b->n; ++v) {
    const groove_sampler_params& sp = b->sampler[v];
    const groove_sample_desc& d = b->descs[sp.sample_index < b->descs.size() ? sp.sample_index : 0];
    P[v] = SamplerParams{(uint32_t)d.offset, d.length, (double)d.root_hz, sp.gain, sp.one_shot};
  }
  return P;
}
int fm_upload_shadow(groove_bank* b) {
  groove_ctx* ctx = b->ctx;
  const uint32_t n = b->n;
  std::vector<float> w((size_t)CTL_FM_WORDS * n);
  for (uint32_t i = 0; i < n; ++i) {
    const groove_fm_params& p = b->fm[i];
    w[(size_t)CTL_FM_GAIN * n + i] = p.dca_gain;
    w[(size_t)CTL_FM_PAN * n + i] = p.dca_pan;
    w[(size_t)CTL_FM_DEPTH * n + i] = p.depth;
    w[(size_t)CTL_FM_BETA * n + i] = p.beta;
  }
  GHIP(ctx, ctx_memcpy(ctx, b->d_dca, w.data(), w.size() * 4, hipMemcpyHostToDevice));
  return 0;
}
int fm_upload_params(groove_bank* b) {
  if (upload_soa(b->ctx, b->d_params, fm_derive_params(b))) return 1;
  return b->d_dca ? fm_upload_shadow(b) : 0;
}
int sampler_upload_params(groove_bank* b) { return upload_soa(b->ctx, b->d_params, sampler_derive_params(b)); }
// An enveloped sampler bank's records [13][n] from the kept groove_envelope_params: the parameters derived at the ctx's rate and spread
// over the voices by sample_index (release_len < 0 for a voice whose sample has none), every envelope idle.
int sampler_upload_envelopes(groove_bank* b) {
  groove_ctx* ctx = b->ctx;
  const uint32_t n = b->n;
  std::vector<uint32_t> w((size_t)kSampleEnvWords * n);
  EnvState idle;
  env_init(idle);
  for (uint32_t v = 0; v < n; ++v) {
    const uint32_t i = b->sampler[v].sample_index;
    const EnvParams ep = i < b->envs.size() && b->env_enabled[i] ? derive_env(b->envs[i], ctx->sr) : sample_env_none();
    uint32_t rec[kSampleEnvWords];
    std::memcpy(rec, &ep, sizeof(ep));
    std::memcpy(rec + kSampleEnvParamWords, &idle, sizeof(idle));
    for (uint32_t k = 0; k < kSampleEnvWords; ++k) w[(size_t)k * n + v] = rec[k];
  }
  GHIP(ctx, ctx_memcpy(ctx, b->d_env, w.data(), w.size() * 4, hipMemcpyHostToDevice));
  return 0;
}

int bank_derive_and_upload(groove_bank* b) {
  groove_ctx* ctx = b->ctx;
  const uint32_t n = b->n;
  GHIP(ctx, hipSetDevice(ctx->device));
  if (b->kind == BANK_WELSH) {
    std::vector<WelshState> S(n, initial_welsh_state()); // every voice starts from the same state: any lane order will do
    if (welsh_upload_params(b, true)) return 1;
    if (upload_soa(ctx, b->d_state, S)) return 1;
  } else if (b->kind == BANK_FM) {
    std::vector<FmState> S(n, initial_fm_state());
    std::vector<double> ratio(n);
    for (uint32_t v = 0; v < n; ++v) ratio[v] = b->fm[v].ratio;
    if (fm_upload_params(b)) return 1;
    if (upload_soa(ctx, b->d_state, S)) return 1;
    GHIP(ctx, ctx_memcpy(ctx, b->d_cold, ratio.data(), ratio.size() * 8, hipMemcpyHostToDevice));
  } else {
    std::vector<SamplerState> S(n, SamplerState{0, 0, 0, 0});
    if (sampler_upload_params(b)) return 1;
    if (upload_soa(ctx, b->d_state, S)) return 1;
    if (b->enveloped && sampler_upload_envelopes(b)) return 1; // re-derived at the new rate, idle like the state
  }
  b->pending.clear();
  return 0;
}

int bank_alloc(groove_bank* b) {
  groove_ctx* ctx = b->ctx;
  GHIP(ctx, hipSetDevice(ctx->device));
  // soa_load / soa_store (kernels.h) address a record through ONE buffer resource: its byte size and the
  // row offsets are 32-bit, so words * n * 4 must stay below 4 GiB (26.8 M Welsh voices per bank).
  if ((uint64_t)std::max(b->pw, b->sw) * b->n * 4ull >= (1ull << 32))
    return fail(ctx, "bank too large: parameter/state record x voices must stay below 4 GiB per bank (split the voices over several banks)");
  GHIP(ctx, hipMalloc(&b->d_params, (size_t)b->pw * b->n * 4));
  GHIP(ctx, hipMalloc(&b->d_state, (size_t)b->sw * b->n * 4));
  return 0;
}

// Launch one note-event round resident at ev[0..count) on the device.
int launch_events(groove_bank* b, const groove_note_event* ev, uint32_t count, int all_event, hipStream_t st) {
  groove_ctx* ctx = b->ctx;
  const uint32_t items = all_event >= 0 ? b->n : count;
  const dim3 grid(blocks_for(items)), blk(kThreads);
  if (b->kind == BANK_WELSH)
    hipLaunchKernelGGL(welsh_events_kernel, grid, blk, 0, st, ev, count, all_event, b->d_params,
                       b->d_state, b->d_cold, b->n, (double)ctx->sr);
  else if (b->kind == BANK_FM)
    hipLaunchKernelGGL(fm_events_kernel, grid, blk, 0, st, ev, count, all_event, b->d_params,
                       b->d_state, b->d_cold, b->n, (double)ctx->sr);
  else
    hipLaunchKernelGGL(sampler_events_kernel, grid, blk, 0, st, ev, count, all_event, b->d_params,
                       b->d_state, b->n, b->enveloped ? b->d_env : (uint32_t*)nullptr);
  GHIP(ctx, hipGetLastError());
  return 0;
}

// Apply queued events in order.  Events are cut into rounds in which every voice appears
// at most once, so one thread per event is race-free and order is preserved across rounds.
// `inline_ok`: the caller is about to launch the bank's time-parallel render, which can take a short sorted list of
// events in its arguments (welsh_tp.h, InlineEvents).
int flush_events(groove_bank* b, bool inline_ok = false) {
  if (b->inline_ev.n) { // handed to a render that never ran: they come first, through the ordinary path
    b->pending.insert(b->pending.begin(), b->inline_ev.ev, b->inline_ev.ev + b->inline_ev.n);
    b->inline_ev.n = 0;
    inline_ok = false;
  }
  if (b->pending.empty()) return 0;
  groove_ctx* ctx = b->ctx;
  if (inline_ok && b->kind == BANK_SAMPLER && b->plan.inv.empty() && b->pending.size() <= kInlineEvents) {
    bool sorted = b->pending[0].voice != GROOVE_ALL_VOICES;
    for (size_t i = 1; sorted && i < b->pending.size(); ++i) sorted = b->pending[i].voice != GROOVE_ALL_VOICES && b->pending[i].voice > b->pending[i - 1].voice;
    if (sorted) {
      b->inline_ev.n = (uint32_t)b->pending.size();
      std::memcpy(b->inline_ev.ev, b->pending.data(), b->pending.size() * sizeof(groove_note_event));
      b->pending.clear();
      return 0;
    }
  }
  // Which stream applies the events.  A bank whose renders all run on ONE side stream (side_mode 2: FM,
  // sampler, small or per-lane Welsh banks in the asynchronous forms) and whose state the ctx stream has not
  // touched since gets its events on that same stream: they are ordered with its renders, nothing else reads
  // its state, and the other banks' streams never notice (a project with note events in every block —
  // config #4's staggered starts inside config #5 — would otherwise join and re-fork every stream once per
  // block: mixed-131072 0.229 -> 0.13 ms per block).  Otherwise: the ctx stream, after joining the side streams.
  hipStream_t st = ctx->stream;
  const bool own_stream = b->side_mode == 2 && !b->ctx_touched;
  if (own_stream) {
    st = side_stream_of(ctx, b->stream_slot);
    ctx->side_busy[b->stream_slot] = true;
  } else {
    b->ctx_touched = true;
    if (ctx_join(ctx)) return 1;
  }
  // caller's voice index -> internal lane, into a copy: a failure below leaves `pending` as it was queued,
  // so the next flush maps it exactly once
  std::vector<groove_note_event> ev = b->pending;
  if (!b->plan.inv.empty())
    for (groove_note_event& e : ev)
      if (e.voice != GROOVE_ALL_VOICES) e.voice = b->plan.inv[e.voice];
  // Device and pinned host staging, two slots each in rotation: the events of this flush are handed to the
  // stream and the call returns without a host synchronisation.
  const int hs = b->ev_slot;
  b->ev_slot ^= 1;
  if (b->staged[hs]) GHIP(ctx, wait_deadline(ctx, nullptr, b->ev_staged[hs], "note-event staging slot")); // two flushes ago: long done
  if (b->h_ev_cap[hs] < ev.size()) {
    if (b->h_ev[hs]) GHIP(ctx, hipHostFree(b->h_ev[hs]));
    if (b->d_ev[hs]) GHIP(ctx, hipFree(b->d_ev[hs]));
    b->h_ev_cap[hs] = std::max<size_t>(ev.size() * 2, 1024);
    GHIP(ctx, hipHostMalloc(&b->h_ev[hs], b->h_ev_cap[hs] * sizeof(groove_note_event), hipHostMallocDefault));
    GHIP(ctx, hipMalloc(&b->d_ev[hs], b->h_ev_cap[hs] * sizeof(groove_note_event)));
  }
  if (!b->ev_staged[hs]) GHIP(ctx, hipEventCreateWithFlags(&b->ev_staged[hs], hipEventDisableTiming));
  std::memcpy(b->h_ev[hs], ev.data(), ev.size() * sizeof(groove_note_event));
  groove_note_event* d_ev = b->d_ev[hs];
  GHIP(ctx, hipMemcpyAsync(d_ev, b->h_ev[hs], ev.size() * sizeof(groove_note_event), hipMemcpyHostToDevice, st));
  // fast path: strictly increasing voices, no ALL events → one round
  bool sorted = true;
  for (size_t i = 0; i < ev.size(); ++i) {
    if (ev[i].voice == GROOVE_ALL_VOICES || (i && ev[i].voice <= ev[i - 1].voice)) { sorted = false; break; }
  }
  if (sorted) {
    if (launch_events(b, d_ev, (uint32_t)ev.size(), -1, st)) return 1;
  } else {
    // general path: contiguous runs; a run ends at an ALL event or at a repeated voice
    std::vector<uint32_t> seen_round(b->n, 0);
    uint32_t round = 1;
    size_t start = 0;
    auto launch_run = [&](size_t lo, size_t hi) -> int {
      if (hi <= lo) return 0;
      return launch_events(b, d_ev + lo, (uint32_t)(hi - lo), -1, st);
    };
    for (size_t i = 0; i < ev.size(); ++i) {
      if (ev[i].voice == GROOVE_ALL_VOICES) {
        if (launch_run(start, i)) return 1;
        if (launch_events(b, d_ev, (uint32_t)ev.size(), (int)i, st)) return 1;
        start = i + 1; ++round;
      } else if (ev[i].voice < b->n) {
        if (seen_round[ev[i].voice] == round) {
          if (launch_run(start, i)) return 1;
          start = i; ++round;
        }
        seen_round[ev[i].voice] = round;
      }
    }
    if (launch_run(start, ev.size())) return 1;
  }
  GHIP(ctx, hipEventRecord(b->ev_staged[hs], st));
  b->staged[hs] = true;
  b->pending.clear(); // (the device reads the pinned copy, not this vector)
  return 0;
}

int ensure_partial(groove_ctx* ctx, size_t floats) {
  if (ctx->partial_cap >= floats) return 0;
  if (ctx->d_partial) GHIP(ctx, hipFree(ctx->d_partial));
  GHIP(ctx, hipMalloc(&ctx->d_partial, floats * 4));
  ctx->partial_cap = floats;
  return 0;
}

// The segment buffer of a bus reduction: seg[segs][cols].
int ensure_seg_buffer(groove_ctx* ctx, float** buf, size_t* cap, size_t seg_floats) {
  if (*buf && *cap >= seg_floats) return 0;
  if (*buf) { GHIP(ctx, hipFree(*buf)); *buf = nullptr; *cap = 0; }
  GHIP(ctx, hipMalloc(buf, seg_floats * 4));
  *cap = seg_floats;
  return 0;
}
// bus[f][ch] (+)= column sums of partial[row][ch][frame] on the ctx stream (fixed order: segments of 64 rows, then the
// segments in index order; a single segment's sums go straight to the bus).
constexpr uint32_t kRowsPerSeg = 64;
constexpr uint32_t reduce_segs(uint32_t rows) { return (rows + kRowsPerSeg - 1) / kRowsPerSeg; }
constexpr size_t reduce_seg_floats(uint32_t rows, uint32_t frames) { return (size_t)reduce_segs(rows) * 2 * frames; } // what launch_reduce needs of seg_buf
constexpr size_t kMaxSpareSums = 8; // lane-sum buffers groove_mix_deferred keeps for blocks to take (deferred_taken)
// `done` (optional): an event that completes with the LAST kernel of the reduction — bound to that dispatch's own completion
// signal (hipExtLaunchKernelGGL), not recorded behind it: a recorded event is a barrier packet of its own, ~5 us of the
// stream's timeline (docs/STREAMS.md).
void launch_reduce(groove_ctx* ctx, const float* partial, uint32_t rows, uint32_t frames, float* seg_buf, float* bus_dev, int accumulate, hipEvent_t done = nullptr) {
  const uint32_t cols = 2 * frames, segs = reduce_segs(rows);
  const dim3 blk(kThreads);
  if (segs == 1) {
    if (done) hipExtLaunchKernelGGL(partial_rows_kernel, dim3(blocks_for(cols), 1), blk, 0, ctx->stream, nullptr, done, 0, partial, rows, cols, kRowsPerSeg, seg_buf, bus_dev, accumulate);
    else hipLaunchKernelGGL(partial_rows_kernel, dim3(blocks_for(cols), 1), blk, 0, ctx->stream, partial, rows, cols, kRowsPerSeg, seg_buf, bus_dev, accumulate);
  } else {
    hipLaunchKernelGGL(partial_rows_kernel, dim3(blocks_for(cols), segs), blk, 0, ctx->stream, partial, rows, cols, kRowsPerSeg, seg_buf, (float*)nullptr, 0);
    if (done) hipExtLaunchKernelGGL(partial_final_kernel, dim3(blocks_for(cols)), blk, 0, ctx->stream, nullptr, done, 0, seg_buf, segs, frames, bus_dev, accumulate);
    else hipLaunchKernelGGL(partial_final_kernel, dim3(blocks_for(cols)), blk, 0, ctx->stream, seg_buf, segs, frames, bus_dev, accumulate);
  }
}
// The pending rows have been handed to a launch (or to bus_flush's reduction): a buffer groove_mix_deferred took from a block is
// a spare from now on (stream order protects it: whoever is given it next writes it behind that launch — DESIGN.md section 5).
void deferred_taken(groove_ctx* ctx) {
  if (ctx->deferred.rows && ctx->deferred_owned_cap) {
    ctx->spare_sums.emplace_back(const_cast<float*>(ctx->deferred.rows), ctx->deferred_owned_cap);
    if (ctx->spare_sums.size() > kMaxSpareSums) { // (a rotation holds one spare per block in flight; beyond that the list only grows when blocks die)
      // the smallest goes; hipFree waits for the device, which is why this only happens past the cap
      auto it = std::min_element(ctx->spare_sums.begin(), ctx->spare_sums.end(), [](const auto& x, const auto& y) { return x.second < y.second; });
      if (it->first != ctx->deferred.rows) { (void)hipFree(it->first); ctx->spare_sums.erase(it); }
    }
  }
  ctx->deferred = TpPrev{};
  ctx->deferred_owned_cap = 0;
}
// The pending reduction of a bank's last paced block onto its bus (ctx stream).  host_wait: the HOST waits for the block's render
// kernels (they were submitted a whole call ago), so that the ctx stream carries no cross-queue wait; otherwise (flush points) the
// ctx stream waits for them itself.
int paced_reduce(groove_bank* b, bool host_wait) {
  if (!b->paced.active) return 0;
  groove_ctx* ctx = b->ctx;
  const auto p = b->paced;
  // The fallible steps FIRST: a wait whose deadline passes (return code 2) leaves the record pending — the next call, or any flush
  // point, tries again — so a caller that carries on after a timeout never gets a bus that silently lacks this block.
  for (int k = 0; k < kSideStreams; ++k) {
    if (!(p.used & (1u << k))) continue;
    if (host_wait) GHIP(ctx, wait_deadline(ctx, nullptr, b->ev_render_done[k][p.slot], "groove_bank_render_mix_paced: the previous block's render"));
    else GHIP(ctx, hipStreamWaitEvent(ctx->stream, b->ev_render_done[k][p.slot], 0));
  }
  b->paced.active = false;
  ctx->paced_order.erase(std::remove(ctx->paced_order.begin(), ctx->paced_order.end(), b), ctx->paced_order.end());
  launch_reduce(ctx, b->d_pipe_part[p.slot], p.rows, p.frames, b->d_pipe_seg[p.slot], p.bus, p.accumulate, nullptr);
  GHIP(ctx, hipEventRecord(b->ev_reduce_done[p.slot], ctx->stream));
  b->reduce_recorded[p.slot] = true;
  GHIP(ctx, hipGetLastError());
  return 0;
}
// ---- the all-pass stream (groove_set_fx_allpass_stream)
static hipStream_t ap_stream(groove_ctx* ctx) { return side_stream_of(ctx, ctx->fx_ap_stream); }
static int ap_events(groove_ctx* ctx) {
  if (!ctx->ev_ap_run) GHIP(ctx, hipEventCreateWithFlags(&ctx->ev_ap_run, kSyncEventFlags));
  if (!ctx->ev_ap_x) GHIP(ctx, hipEventCreateWithFlags(&ctx->ev_ap_x, kSyncEventFlags));
  return 0;
}
// The ctx stream behind everything the all-pass stream has been given ...
int ap_join(groove_ctx* ctx) {
  if (ctx->fx_ap_stream < 0 || !ctx->side_busy[ctx->fx_ap_stream]) return 0;
  if (ap_events(ctx)) return 1;
  GHIP(ctx, hipEventRecord(ctx->ev_ap_x, ap_stream(ctx)));
  GHIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_ap_x, 0));
  return 0;
}
// ... and the all-pass stream behind everything the ctx stream has been given.
static int ap_follow(groove_ctx* ctx) {
  if (ctx->fx_ap_stream < 0) return 0;
  if (ap_events(ctx)) return 1;
  GHIP(ctx, hipEventRecord(ctx->ev_ap_run, ctx->stream));
  GHIP(ctx, hipStreamWaitEvent(ap_stream(ctx), ctx->ev_ap_run, 0));
  return 0;
}
// Lane sums that wait for the next all-pass launch and will not get one: the ctx stream reduces them itself, behind the kernel that
// wrote them and ahead of whichever all-pass writes that buffer next.
int bus_flush_ap(groove_ctx* ctx) {
  if (!ctx->deferred_ap.rows) return 0;
  const TpPrev d = ctx->deferred_ap;
  ctx->deferred_ap = TpPrev{};
  if (ap_join(ctx)) return 1;
  if (ensure_seg_buffer(ctx, &ctx->d_fseg, &ctx->fseg_cap, reduce_seg_floats(d.n_rows, d.frames))) return 1;
  launch_reduce(ctx, d.rows, d.n_rows, d.frames, ctx->d_fseg, d.bus, d.accumulate, nullptr);
  if (hipGetLastError() != hipSuccess) return fail(ctx, "bus_flush: launch failed");
  return ap_follow(ctx);
}
int bus_flush_deferred(groove_ctx* ctx) {
  if (!ctx->deferred.rows) return 0;
  const TpPrev d = ctx->deferred;
  deferred_taken(ctx);
  if (ensure_seg_buffer(ctx, &ctx->d_fseg, &ctx->fseg_cap, reduce_seg_floats(d.n_rows, d.frames))) return 1;
  launch_reduce(ctx, d.rows, d.n_rows, d.frames, ctx->d_fseg, d.bus, d.accumulate);
  return hipGetLastError() == hipSuccess ? 0 : fail(ctx, "bus_flush: launch failed");
}
// Pending PACED reductions of any bank go onto their buses before a call of another form adds to a bus (include/groove_hip.h: "any
// unpaced render or mix flushes them"): call order is the order of a bus's sums.
static int flush_paced(groove_ctx* ctx) {
  if (bus_flush_ap(ctx)) return 1; // (lane sums waiting on the all-pass stream: the order of a bus's sums is the order of the calls)
  while (!ctx->paced_order.empty()) // (call order: the order of the banks' sums on a bus)
    if (const int rc = paced_reduce(ctx->paced_order.front(), false)) return rc;
  return 0;
}
int bus_flush(groove_ctx* ctx) { return bus_flush_deferred(ctx) ? 1 : flush_paced(ctx); }
int reduce_rows(groove_ctx* ctx, const float* rows_dev, uint32_t rows, uint32_t frames, float* bus_dev, int accumulate, hipEvent_t done = nullptr) {
  if (ensure_seg_buffer(ctx, &ctx->d_fseg, &ctx->fseg_cap, reduce_seg_floats(rows, frames))) return 1;
  launch_reduce(ctx, rows_dev, rows, frames, ctx->d_fseg, bus_dev, accumulate, done);
  GHIP(ctx, hipGetLastError());
  return 0;
}

constexpr uint32_t kMixSeg = 16384; // floats of one row summed by one workgroup

int mix_one(groove_ctx* ctx, const groove_block* b, uint32_t frames, float* bus, int accumulate, size_t planar_stride = 0) {
  const uint32_t n_seg = (b->n + kMixSeg - 1) / kMixSeg;
  const uint32_t rows = 2 * frames;
  if (ensure_partial(ctx, (size_t)rows * n_seg)) return 1;
  if (n_seg == 1) { // one segment per row: the partial sums are the totals
    hipLaunchKernelGGL(mix_partial_kernel, dim3(1, rows), dim3(kThreads), 0, ctx->stream, block_data(b), b->n, frames,
                       (size_t)b->cap * b->n, kMixSeg, ctx->d_partial, 1u, bus, accumulate, planar_stride);
    GHIP(ctx, hipGetLastError());
    return 0;
  }
  hipLaunchKernelGGL(mix_partial_kernel, dim3(n_seg, rows), dim3(kThreads), 0, ctx->stream, block_data(b), b->n, frames,
                     (size_t)b->cap * b->n, kMixSeg, ctx->d_partial, n_seg, (float*)nullptr, 0, (size_t)0);
  hipLaunchKernelGGL(mix_final_kernel, dim3(blocks_for(rows)), dim3(kThreads), 0, ctx->stream, ctx->d_partial,
                     frames, n_seg, bus, accumulate, planar_stride);
  GHIP(ctx, hipGetLastError());
  return 0;
}

// ---- effects -------------------------------------------------------------------------
// The device's copy of the filter parameters of every lane, for the filter links' kernel (ctl_link.h) to derive coefficients from.
int fx_upload_shadow(groove_fx* fx) {
  groove_ctx* ctx = fx->ctx;
  const uint32_t n = fx->n;
  std::vector<float> w((size_t)CTL_SHADOW_WORDS * n);
  for (uint32_t i = 0; i < n; ++i) {
    const groove_fx_params& p = fx->p[i];
    w[(size_t)CTL_SHADOW_CUTOFF * n + i] = p.cutoff_hz;
    w[(size_t)CTL_SHADOW_Q * n + i] = p.q;
    w[(size_t)CTL_SHADOW_RIPPLE * n + i] = p.passband_ripple;
    w[(size_t)CTL_SHADOW_BANDWIDTH * n + i] = p.bandwidth_hz;
    w[(size_t)CTL_SHADOW_DB_GAIN * n + i] = p.db_gain;
  }
  GHIP(ctx, ctx_memcpy(ctx, fx->d_shadow, w.data(), w.size() * 4, hipMemcpyHostToDevice));
  return 0;
}
int fx_upload_params(groove_fx* fx) {
  groove_ctx* ctx = fx->ctx;
  const uint32_t n = fx->n;
  const double sr = ctx->sr;
  std::vector<float> fa(n), fb(n), wet(n);
  std::vector<uint32_t> ua(n);
  fx->all_wet = true;
  for (uint32_t i = 0; i < n; ++i) {
    const groove_fx_params& p = fx->p[i];
    wet[i] = p.wet;
    if (p.wet < 1.0f) fx->all_wet = false;
    ua[i] = p.bits > 31 ? 31 : p.bits;
    switch (fx->kind) {
      case GROOVE_FX_GAIN: fa[i] = p.ceiling; break;
      case GROOVE_FX_LIMITER:
      case GROOVE_FX_COMPRESSOR: fa[i] = p.limit_min; fb[i] = p.limit_max; break;
      case GROOVE_FX_REVERB: fa[i] = p.attenuation; break;
      default: break;
    }
  }
  GHIP(ctx, ctx_memcpy(ctx, fx->d_fa, fa.data(), n * 4, hipMemcpyHostToDevice));
  GHIP(ctx, ctx_memcpy(ctx, fx->d_fb, fb.data(), n * 4, hipMemcpyHostToDevice));
  GHIP(ctx, ctx_memcpy(ctx, fx->d_ua, ua.data(), n * 4, hipMemcpyHostToDevice));
  GHIP(ctx, ctx_memcpy(ctx, fx->d_wet, wet.data(), n * 4, hipMemcpyHostToDevice));
  double probe[5];
  if (rbj_for_kind_h(fx->kind, fx->p[0], sr, probe)) { // any BiQuad 12 dB mode
    std::vector<double> c((size_t)5 * n);
    for (uint32_t i = 0; i < n; ++i) {
      double c5[5];
      rbj_for_kind_h(fx->kind, fx->p[i], sr, c5);
      for (int k = 0; k < 5; ++k) c[(size_t)k * n + i] = c5[k];
    }
    GHIP(ctx, ctx_memcpy(ctx, fx->d_coef, c.data(), c.size() * 8, hipMemcpyHostToDevice));
  } else if (fx->kind == GROOVE_FX_BIQUAD_LP24) {
    std::vector<double> c((size_t)6 * n);
    for (uint32_t i = 0; i < n; ++i) {
      double c6[6];
      lp24_coeffs_h(fx->p[i].cutoff_hz, fx->p[i].passband_ripple, sr, c6);
      for (int k = 0; k < 6; ++k) c[(size_t)k * n + i] = c6[k];
    }
    GHIP(ctx, ctx_memcpy(ctx, fx->d_coef, c.data(), c.size() * 8, hipMemcpyHostToDevice));
  }
  if (fx->d_shadow) return fx_upload_shadow(fx); // a filter link's value is gone with its coefficients, until its next apply
  return 0;
}

int fx_setup_state(groove_fx* fx) { // (re)allocate and zero state for the current sample rate
  groove_ctx* ctx = fx->ctx;
  const uint32_t n = fx->n;
  const double sr = ctx->sr;
  const size_t ln = 2 * (size_t)n;
  if (fx->d_st) { GHIP(ctx, hipFree(fx->d_st)); fx->d_st = nullptr; }
  if (fx->d_ring) { GHIP(ctx, hipFree(fx->d_ring)); fx->d_ring = nullptr; }
  fx->ring_rows = 0; fx->w = 0;
  const groove_fx_params& p0 = fx->p[0];
  switch (fx->kind) {
    case GROOVE_FX_BIQUAD_LP12:
    case GROOVE_FX_BIQUAD_HP12:
    case GROOVE_FX_BIQUAD_BP12:
    case GROOVE_FX_BIQUAD_BS12:
    case GROOVE_FX_BIQUAD_AP12:
    case GROOVE_FX_BIQUAD_PEAK12:
    case GROOVE_FX_BIQUAD_LSHELF12:
    case GROOVE_FX_BIQUAD_HSHELF12:
    case GROOVE_FX_BIQUAD_LP24:
      GHIP(ctx, hipMalloc(&fx->d_st, 4 * ln * 8));
      GHIP(ctx, hipMemsetAsync(fx->d_st, 0, 4 * ln * 8, ctx->stream)); // on the ctx stream: a null-stream memset is not ordered with it
      break;
    case GROOVE_FX_DELAY:
      fx->N = delay_frames_h(p0.delay_seconds, sr);
      fx->ring_rows = fx->N;
      break;
    case GROOVE_FX_CHORUS:
      fx->N = delay_frames_h(p0.delay_seconds, sr);
      if (p0.voices > 64) return fail(ctx, "groove_fx: chorus voices > 64"); // the taps are a per-frame loop on the device
      fx->voices = p0.voices < 1 ? 1 : p0.voices;
      fx->spacing = fx->N / fx->voices;
      fx->ring_rows = fx->N;
      break;
    case GROOVE_FX_REVERB: {
      uint64_t base = 0;
      for (int i = 0; i < 6; ++i) {
        const double d = i < 4 ? kCombDelaysH[i] : kAllpassDelaysH[i - 4];
        fx->geo.N[i] = delay_frames_h(d, sr);
        fx->geo.w[i] = 0;
        fx->geo.base[i] = base;
        fx->geo.g[i] = (float)(i < 4 ? decay_gain_h(d, p0.reverb_seconds) : decay_gain_h(d, kAllpassDecaysH[i - 4]));
        base += fx->geo.N[i];
      }
      for (int i = 0; i < 2; ++i) { fx->ap_alt[i] = base; base += fx->geo.N[4 + i]; }
      fx->ring_rows = base;
      break;
    }
    default: break;
  }
  if (fx->ring_rows > (1ull << 26)) return fail(ctx, "groove_fx: delay line longer than 2^26 frames");
  if (fx->ring_rows) {
    GHIP(ctx, hipMalloc(&fx->d_ring, fx->ring_rows * ln * 4));
    GHIP(ctx, hipMemsetAsync(fx->d_ring, 0, fx->ring_rows * ln * 4, ctx->stream));
  }
  return 0;
}

int fx_check_uniform(groove_fx* fx) {
  const groove_fx_params& a = fx->p[0];
  for (uint32_t i = 1; i < fx->n; ++i) {
    const groove_fx_params& b = fx->p[i];
    if ((fx->kind == GROOVE_FX_CHORUS && (a.voices != b.voices || a.delay_seconds != b.delay_seconds)) ||
        (fx->kind == GROOVE_FX_DELAY && a.delay_seconds != b.delay_seconds) ||
        (fx->kind == GROOVE_FX_REVERB && a.reverb_seconds != b.reverb_seconds))
      return fail(fx->ctx, "groove_fx: delay-line geometry (voices / delay_seconds / reverb_seconds) must be uniform across the lanes of one effect bank");
  }
  return 0;
}

// ---- control links ----------------------------------------------------------------------
// The sections of a link's two source buffers, on the device or in a host staging copy: ctl_core.h's layouts are the only offsets.
template <typename T> T* ctl_section(void* base, size_t byte_offset) { return reinterpret_cast<T*>(static_cast<char*>(base) + byte_offset); }
CtlLanes ctl_lanes_view(const groove_ctl_link* l) {
  const CtlLanesLayout at = ctl_lanes_layout(l->n_src);
  return {ctl_section<uint64_t>(l->d_lanes, at.delta64), ctl_section<uint64_t>(l->d_lanes, at.duty64), ctl_section<uint32_t>(l->d_lanes, at.waveform),
          ctl_section<uint32_t>(l->d_lanes, at.law)};
}
CtlTrip ctl_trip_view(const groove_ctl_link* l) {
  const CtlTripLayout at = ctl_trip_layout(l->n_src, l->n_steps);
  return {ctl_section<double>(l->d_trip, at.begin), ctl_section<double>(l->d_trip, at.start), ctl_section<double>(l->d_trip, at.end),
          ctl_section<double>(l->d_trip, at.beats), ctl_section<uint32_t>(l->d_trip, at.kind), l->n_steps};
}
// The device copy of a link's source lanes at the current sample rate (creation, groove_update_sample_rate: the caller has
// waited for the ctx stream, or nothing has used the buffer yet).
int ctl_upload_lanes(groove_ctl_link* l) {
  groove_ctx* ctx = l->ctx;
  const CtlLanesLayout at = ctl_lanes_layout(l->n_src);
  std::vector<uint64_t> w(at.bytes / 8);
  uint64_t *delta64 = ctl_section<uint64_t>(w.data(), at.delta64), *duty64 = ctl_section<uint64_t>(w.data(), at.duty64);
  uint32_t *waveform = ctl_section<uint32_t>(w.data(), at.waveform), *law = ctl_section<uint32_t>(w.data(), at.law);
  for (uint32_t i = 0; i < l->n_src; ++i) {
    const groove_ctl_source& s = l->src[i];
    delta64[i] = ctl_lfo_delta64(s.frequency_hz, (double)ctx->sr);
    duty64[i] = ctl_lfo_duty64(s.waveform, s.duty);
    waveform[i] = s.waveform;
    law[i] = s.law;
  }
  GHIP(ctx, ctx_memcpy(ctx, l->d_lanes, w.data(), at.bytes, hipMemcpyHostToDevice));
  return 0;
}

// ---- RCCL via dlopen -----------------------------------------------------------------
// Function-pointer types are taken from the prototypes in <rccl/rccl.h>, so a change of the ABI is a
// compile error here instead of a silently wrong call.
using nccl_get_uid_fn = decltype(&ncclGetUniqueId);
using nccl_init_rank_fn = decltype(&ncclCommInitRank);
using nccl_reduce_fn = decltype(&ncclReduce);
using nccl_destroy_fn = decltype(&ncclCommDestroy);
using nccl_count_fn = decltype(&ncclCommCount);
using nccl_errstr_fn = decltype(&ncclGetErrorString);
static_assert(sizeof(ncclUniqueId) == 128, "groove_comm_unique_id hands out a 128-byte id");

void* g_rccl = nullptr; // one RCCL per process, whichever ctx asks first
int rccl_open(groove_ctx* ctx) {
  if (!g_rccl) {
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char* nm : names) {
      g_rccl = dlopen(nm, RTLD_NOW | RTLD_GLOBAL);
      if (g_rccl) break;
    }
  }
  if (!g_rccl) return fail(ctx, std::string("dlopen(librccl) failed: ") + dlerror());
  if (ctx) ctx->rccl = g_rccl;
  return 0;
}

// Test hook (groove_debug_spin): one wave that sleeps until `ticks` of the constant-rate wall clock have passed.
__global__ void debug_spin_kernel(uint64_t ticks) {
  const uint64_t t0 = wall_clock64();
  while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(64);
}

} // namespace

extern "C" {

// ============================================================================ context
// The library's streams, in the order the design of DESIGN.md section 7 wants them created: ctx (highest priority),
// three normal-priority kind streams, the placeholder in fifth place, then the low-priority bank streams.
static bool create_streams(groove_ctx* ctx) {
  // The runtime spreads the streams of one priority over a handful of hardware queues, and streams that
  // share a queue run one after the other.  The ctx stream is created at the highest priority: that
  // gives it a hardware queue of its own, so that a bank's side stream can never land behind it (as a
  // normal-priority stream it shared a queue with the first bank stream and the render-ahead overlap of
  // config #3 was gone: 0.25 ms per block against 0.14), and its short bus reductions, which every
  // pipelined block waits for, are dispatched ahead of the long render kernels.
  int prio_least = 0, prio_greatest = 0;
  bool ok = hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest) == hipSuccess;
  if (ok && ctx->safe_streams) prio_least = prio_greatest = 0;
  auto make = [&](hipStream_t* st, int prio) {
    const bool made = hipStreamCreateWithPriority(st, hipStreamNonBlocking, prio) == hipSuccess;
    if (made) ctx->streams_created += 1;
    return made;
  };
  ok = ok && make(&ctx->stream, prio_greatest) && hipEventCreateWithFlags(&ctx->ev_fork, kSyncEventFlags) == hipSuccess;
  // Normal-priority streams for the four class-specialised Welsh kinds (side by side in every block
  // of a big bank; the two exact-f64-LFO kinds, rare, share the first two), and three LOW-priority streams
  // for the single-kernel banks (side by side in a mixed project): never more streams than hardware queues,
  // so no two of them are serialised behind each other by the runtime (see bank_streams).
  // SAFE layout (GROOVE_SAFE_STREAMS=1): one priority and four streams in all — the ctx stream and three side streams
  // that kinds and banks share — so that no two streams of this library ever share a hardware queue and nothing rests
  // on the order in which the process created its streams.  Measured cost: about 8 % at 1,000,000 voices in round 3; none since the
  // walks are paced by the host (profiles/r05_layout_ab.log).
  for (int i = 0; ok && i < kSideStreams; ++i) {
    if (i >= kBaseKinds + ctx->bank_streams) { ok = hipEventCreateWithFlags(&ctx->ev_join[i], kSyncEventFlags) == hipSuccess; continue; }
    if (i == 4 || i == 5) ctx->side_stream[i] = ctx->side_stream[i - 4]; // (safe layout; otherwise re-pointed below)
    else if (i == 3 && ctx->kind_streams == 3) { // three normal-priority streams (see kind_streams); the fifth stream the
      // process creates lands on the ctx stream's hardware queue (so does the ninth): that place is taken by a stream nobody uses
      if (!ctx->safe_streams) ok = make(&ctx->placeholder_stream, 0);
      ctx->side_stream[3] = ctx->side_stream[0];
    }
    else if (i < kBaseKinds) ok = make(&ctx->side_stream[i], 0);
    else if (ctx->safe_streams) ctx->side_stream[i] = ctx->side_stream[(i - kBaseKinds) % 3];
    else ok = make(&ctx->side_stream[i], prio_least);
    ok = ok && hipEventCreateWithFlags(&ctx->ev_join[i], kSyncEventFlags) == hipSuccess;
  }
  // The two exact-f64-LFO kinds run on a stream of their own (round 6; they shared the first two kind streams before): behind another
  // kind's kernel on its stream their kernel's time per block was added to that stream's — the step's long pole with the
  // library-proportioned table (profiles/r06_*).  Which stream: the normal-priority PLACEHOLDER (created so that no working stream shares
  // the ctx stream's hardware queue; the exact kinds' kernel and the ctx stream's two short reductions per block get along on it) —
  // 0.382 / 0.382 ms per block against 0.392 / 0.389 on the first (low-priority) bank stream, in one job, tools/ab_exact_stream.sh, once the
  // kind's register budget let its workgroups be placed at all (kernels.h GROOVE_WAVES_F64).  GROOVE_EXACT_STREAM=bank: the bank stream.
  if (ok && !ctx->safe_streams) {
    const char* e = std::getenv("GROOVE_EXACT_STREAM");
    const bool bank = e && e[0] == 'b';
    if (!bank && ctx->placeholder_stream) ctx->side_stream[4] = ctx->side_stream[5] = ctx->placeholder_stream;
    else if (ctx->bank_streams > 0 && ctx->side_stream[kBaseKinds]) ctx->side_stream[4] = ctx->side_stream[5] = ctx->side_stream[kBaseKinds];
  }
  return ok;
}
static bool side_stream_owned(const groove_ctx* ctx, int i) {
  if (!ctx->side_stream[i] || i == 4 || i == 5 || (i == 3 && ctx->kind_streams == 3)) return false;
  return !(ctx->safe_streams && i >= kBaseKinds);
}
static int comm_init_rank(groove_ctx* ctx, const uint8_t id[128], int rank, int world_size);
static int init_impl(int device_ordinal, const uint8_t* comm_id, int rank, int world_size, groove_ctx** out) {
  if (!out) return fail(nullptr, "groove_init: out is NULL");
  *out = nullptr;
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0)
    return fail(nullptr, std::string("groove_init: no HIP device available (") + hipGetErrorString(e) +
                             "); this library has no CPU path");
  if (device_ordinal < 0 || device_ordinal >= count) return fail(nullptr, "groove_init: bad device ordinal");
  groove_ctx* ctx = new (std::nothrow) groove_ctx();
  if (!ctx) return fail(nullptr, "groove_init: out of memory");
  ctx->device = device_ordinal;
  if (const char* e = std::getenv("GROOVE_FX_SEQ_ALLPASS")) ctx->seq_allpass = e[0] == '1';
  if (const char* e = std::getenv("GROOVE_SAFE_STREAMS")) ctx->safe_streams = e[0] == '1';
  if (const char* e = std::getenv("GROOVE_LOOK_AHEAD")) ctx->look_ahead = (uint32_t)std::strtoul(e, nullptr, 10) & 7u;
  if (const char* e = std::getenv("GROOVE_SYNC_TIMEOUT_MS")) ctx->sync_timeout_ms = (uint32_t)std::strtoul(e, nullptr, 10);
  if (const char* e = std::getenv("GROOVE_FM_TP_VPW4_MIN_VOICES")) ctx->fm_tp_vpw4_min_voices = (uint32_t)std::strtoul(e, nullptr, 10);
  if (const char* e = std::getenv("GROOVE_BIND_EVENTS")) ctx->bind_events = std::atoi(e) != 0;
  if (const char* e = std::getenv("GROOVE_FX_CHUNKED_ALLPASS")) ctx->chunked_allpass = e[0] == '1';
  if (const char* e = std::getenv("GROOVE_FX_WET_REVERB_RUN")) ctx->fx_wet_reverb_run = e[0] == '1';
  if (const char* e = std::getenv("GROOVE_TP_MAX_VOICES")) ctx->tp_max_voices = (uint32_t)std::strtoul(e, nullptr, 10);
  if (const char* e = std::getenv("GROOVE_SPLIT_MAX_WAVES")) ctx->split_max_waves = (uint32_t)std::strtoul(e, nullptr, 10);   // (A/B runs: tools/ab_env.sh)
  if (const char* e = std::getenv("GROOVE_F32_FILTER")) ctx->f32_filter = e[0] != '0'; // (A/B and the bit-identity tests between kernel forms)
  if (const char* e = std::getenv("GROOVE_PIPELINE_MIN_WAVES")) ctx->pipeline_min_waves = (uint32_t)std::strtoul(e, nullptr, 10); // tests force the pipeline on small banks
  bool ok = hipSetDevice(device_ordinal) == hipSuccess;
  // groove_init_comm: the rank's RCCL communicator first, so that whatever streams RCCL creates for itself exist BEFORE
  // the library's five, which then follow each other in the process's creation order as section 7's layout assumes
  // (with groove_comm_init after groove_init, RCCL's streams became the ctx stream's queue-mates in every rank).
  if (ok && comm_id) {
    if (comm_init_rank(ctx, comm_id, rank, world_size)) { const std::string m = ctx->err; delete ctx; return fail(nullptr, m); }
    ctx->comm_before_streams = true;
  }
  ok = ok && create_streams(ctx);
  ok = ok && hipMalloc(reinterpret_cast<void**>(&ctx->d_diag), sizeof(DiagCounters)) == hipSuccess && hipMemsetAsync(ctx->d_diag, 0, sizeof(DiagCounters), ctx->stream) == hipSuccess;
#ifdef GROOVE_HEARTBEAT
  if (ok && hipHostMalloc(reinterpret_cast<void**>(&ctx->hb), 64, hipHostMallocCoherent | hipHostMallocMapped) == hipSuccess) { ctx->hb[0] = 0; ctx->hb[1] = 0; }
#endif
  if (!ok) {
    groove_shutdown(ctx);
    return fail(nullptr, "groove_init: hipSetDevice/hipStreamCreate failed");
  }
  *out = ctx;
  return 0;
}
int groove_init(int device_ordinal, groove_ctx** out) { return init_impl(device_ordinal, nullptr, 0, 1, out); }
int groove_init_comm(int device_ordinal, const uint8_t id[128], int rank, int world_size, groove_ctx** out) {
  if (!id) return fail(nullptr, "groove_init_comm: id is NULL");
  return init_impl(device_ordinal, id, rank, world_size, out);
}
void groove_shutdown(groove_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  (void)ctx_join(ctx);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  for (groove_ctl_link* l : ctx->links) l->bank = nullptr; // (no bank is re-planned for the links it loses here: it goes next)
  while (!ctx->links.empty()) groove_ctl_link_destroy(ctx->links.back());
  while (!ctx->banks.empty()) groove_bank_destroy(ctx->banks.back());
  while (!ctx->fxs.empty()) groove_fx_destroy(ctx->fxs.back());
  groove_comm_destroy(ctx);
  if (ctx->d_partial) (void)hipFree(ctx->d_partial);
  if (ctx->d_fpart) (void)hipFree(ctx->d_fpart);
  for (float* q : ctx->d_dpart) if (q) (void)hipFree(q);
  if (ctx->d_fseg) (void)hipFree(ctx->d_fseg);
  if (ctx->d_i16) (void)hipFree(ctx->d_i16);
  if (ctx->d_diag) (void)hipFree(ctx->d_diag);
  if (ctx->deferred.rows && ctx->deferred_owned_cap) (void)hipFree(const_cast<float*>(ctx->deferred.rows));
  for (auto& sp : ctx->spare_sums) (void)hipFree(sp.first);
  if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
  for (int i = 0; i < kSideStreams; ++i) {
    if (side_stream_owned(ctx, i)) { (void)hipStreamSynchronize(ctx->side_stream[i]); (void)hipStreamDestroy(ctx->side_stream[i]); }
    if (ctx->ev_join[i]) (void)hipEventDestroy(ctx->ev_join[i]);
  }
  if (ctx->placeholder_stream) (void)hipStreamDestroy(ctx->placeholder_stream);
  if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
  if (ctx->ev_ap_run) (void)hipEventDestroy(ctx->ev_ap_run);
  if (ctx->ev_ap_x) (void)hipEventDestroy(ctx->ev_ap_x);
  delete ctx;
}
const char* groove_last_error(groove_ctx* ctx) { return ctx ? ctx->err.c_str() : g_last_error.c_str(); }
int groove_set_stream(groove_ctx* ctx, void* hip_stream) {
  if (!ctx) return fail(nullptr, "groove_set_stream: ctx is NULL");
  if (ctx_join(ctx)) return 1;
  GHIP(ctx, ctx_wait(ctx));
  if (ctx->own_stream && ctx->stream) GHIP(ctx, hipStreamDestroy(ctx->stream));
  ctx->stream = (hipStream_t)hip_stream;
  ctx->own_stream = false;
  return 0;
}
int groove_synchronize(groove_ctx* ctx) {
  if (!ctx) return fail(nullptr, "groove_synchronize: ctx is NULL");
  if (ctx_join(ctx)) return 1;
  GHIP(ctx, ctx_wait(ctx, "groove_synchronize"));
  return 0;
}
int groove_set_sync_timeout_ms(groove_ctx* ctx, uint32_t ms) {
  if (!ctx) return fail(nullptr, "groove_set_sync_timeout_ms: ctx is NULL");
  ctx->sync_timeout_ms = ms;
  return 0;
}
uint32_t groove_sync_timeout_ms(groove_ctx* ctx) { return ctx ? ctx->sync_timeout_ms : 0; }
int groove_debug_spin(groove_ctx* ctx, int side_stream, uint32_t ms) {
  if (!ctx) return fail(nullptr, "groove_debug_spin: ctx is NULL");
  if (side_stream >= kSideStreams) return fail(ctx, "groove_debug_spin: no such side stream");
  int khz = 0;
  GHIP(ctx, hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, ctx->device));
  if (khz <= 0) khz = 100000; // 100 MHz
  hipStream_t st = side_stream < 0 ? ctx->stream : side_stream_of(ctx, side_stream);
  hipLaunchKernelGGL(debug_spin_kernel, dim3(1), dim3(64), 0, st, (uint64_t)ms * (uint64_t)khz);
  GHIP(ctx, hipGetLastError());
  if (side_stream >= 0) ctx->side_busy[side_stream] = true;
  return 0;
}
int groove_debug_info(groove_ctx* ctx, char* out, size_t cap) {
  if (!ctx || !out || cap == 0) return fail(ctx, "groove_debug_info: NULL argument");
  int distinct = 0;
  for (int k = 0; k < kSideStreams; ++k) {
    bool dup = !ctx->side_stream[k];
    for (int j = 0; j < k && !dup; ++j) dup = ctx->side_stream[j] == ctx->side_stream[k];
    distinct += dup ? 0 : 1;
  }
  // the segment guard's counter (diag.h): what the kernels have counted so far (groove_synchronize first for a final figure)
  DiagCounters dc{};
  GHIP(ctx, ctx_memcpy(ctx, &dc, ctx->d_diag, sizeof(dc), hipMemcpyDeviceToHost));
  std::string diag = "\"host_waits\": " + std::to_string(ctx->host_waits) + ", \"host_waits_blocked\": " + std::to_string(ctx->host_waits_blocked) + ", \"host_wait_ms\": " + std::to_string((double)ctx->host_wait_ns * 1e-6) +
                     ", \"zero_segments\": " + std::to_string(dc.zero_segments) + ", \"fast_table_misses\": " + std::to_string(dc.fast_table_misses) + ", \"fast_waves\": " + std::to_string(dc.fast_waves) + ", \"source_hash\": \"" GROOVE_SOURCE_HASH "\"";
#ifdef GROOVE_DIAG_SHADOW_IN_MIN
  diag += ", \"diag_build\": \"GROOVE_DIAG_SHADOW_IN_MIN\", \"shadow_zero_lanes\": " + std::to_string(dc.shadow_zero_lanes) + ", \"shadow_zero_waves\": " + std::to_string(dc.shadow_zero_waves) + ", \"records\": [";
  for (uint32_t i = 0; i < std::min(dc.records, kDiagRecords); ++i) {
    const DiagRecord& r = dc.rec[i];
    diag += std::string(i ? ", " : "") + "{\"wg\": " + std::to_string(r.wg) + ", \"wave\": " + std::to_string(r.wave) + ", \"lane\": " + std::to_string(r.lane) + ", \"active\": " + std::to_string(r.active) +
            ", \"count\": " + std::to_string(r.count) + ", \"frame\": " + std::to_string(r.frame) + ", \"amp\": [" + std::to_string(r.amp_state) + ", " + std::to_string(r.amp_n) + ", " + std::to_string(r.amp_N) +
            "], \"fil\": [" + std::to_string(r.fil_state) + ", " + std::to_string(r.fil_n) + ", " + std::to_string(r.fil_N) + "]}";
  }
  diag += "]";
#endif
  std::snprintf(out, cap,
                "{\"layout\": \"%s\", \"streams_created\": %d, \"distinct_side_streams\": %d, \"kind_streams\": %d, \"bank_streams\": %d, "
                "\"placeholder_fifth\": %s, \"comm_before_streams\": %s, \"own_ctx_stream\": %s, \"sync_timeout_ms\": %u, %s}",
                ctx->safe_streams ? "safe (one priority, ctx + 3 shared side streams)" : "default (ctx high, 3 kind streams normal, placeholder, bank streams low)",
                ctx->streams_created, distinct, ctx->kind_streams, ctx->safe_streams ? 0 : ctx->bank_streams, ctx->placeholder_stream ? "true" : "false",
                ctx->comm_before_streams ? "true" : "false", ctx->own_stream ? "true" : "false", ctx->sync_timeout_ms, diag.c_str());
  return 0;
}
uint32_t groove_sample_rate(groove_ctx* ctx) { return ctx ? ctx->sr : 0; }
int groove_set_time_parallel_max_voices(groove_ctx* ctx, uint32_t max_voices) {
  if (!ctx) return fail(nullptr, "groove_set_time_parallel_max_voices: ctx is NULL");
  if (ctx_join(ctx)) return 1; // banks change kernels (and side streams) at their next render
  GHIP(ctx, ctx_wait(ctx));
  ctx->tp_max_voices = max_voices;
  return 0;
}
uint32_t groove_time_parallel_max_voices(groove_ctx* ctx) { return ctx ? ctx->tp_max_voices : 0; }
int groove_set_time_parallel_pair_min_voices(groove_ctx* ctx, uint32_t min_voices) {
  if (!ctx) return fail(nullptr, "groove_set_time_parallel_pair_min_voices: ctx is NULL");
  if (ctx_join(ctx)) return 1; // the partial-row count of a bank's renders changes with the form
  GHIP(ctx, ctx_wait(ctx));
  ctx->tp_vpw2_min_voices = min_voices;
  return 0;
}
uint32_t groove_time_parallel_pair_min_voices(groove_ctx* ctx) { return ctx ? ctx->tp_vpw2_min_voices : 0; }
int groove_set_look_ahead(groove_ctx* ctx, uint32_t bits) {
  if (!ctx) return fail(nullptr, "groove_set_look_ahead: ctx is NULL");
  ctx->look_ahead = bits & 7u;
  return 0;
}
uint32_t groove_look_ahead(groove_ctx* ctx) { return ctx ? ctx->look_ahead : 0; }
int groove_set_pipeline_min_waves(groove_ctx* ctx, uint32_t waves) {
  if (!ctx) return fail(nullptr, "groove_set_pipeline_min_waves: ctx is NULL");
  if (ctx_join(ctx)) return 1; // banks change kernels (and side streams) at their next render
  GHIP(ctx, ctx_wait(ctx));
  ctx->pipeline_min_waves = waves;
  return 0;
}
uint32_t groove_pipeline_min_waves(groove_ctx* ctx) { return ctx ? ctx->pipeline_min_waves : 0; }
int groove_set_fx_allpass_stream(groove_ctx* ctx, int on) {
  if (!ctx) return fail(nullptr, "groove_set_fx_allpass_stream: ctx is NULL");
  if (bus_flush(ctx) || ctx_join(ctx)) return 1; // nothing of the old arrangement is in flight when the next chain is submitted
  GHIP(ctx, ctx_wait(ctx));
  for (groove_fx* fx : ctx->fxs) fx->ap_busy = false;
  const int k_ap = kBaseKinds + 1;
  if (on && ctx->bank_streams > 1) // banks that render on that stream move to the others (everything is idle here; their next events go through the ctx stream)
    for (groove_bank* b : ctx->banks)
      if (b->stream_slot == k_ap) { b->stream_slot = kBaseKinds + (ctx->next_stream_slot++ % 2 ? 2 % ctx->bank_streams : 0); b->ctx_touched = true; }
  // the second of the low-priority bank streams: a lone bank renders on the first (measured, tools/ap_stream_ab.sh: 0.0489 -> 0.044
  // ms per block of config #3 there, 0.045 - 0.048 on a normal-priority kind stream, 0.063 - 0.070 on the first kind stream)
  ctx->fx_ap_stream = on ? k_ap : -1;
  return 0;
}
int groove_fx_allpass_stream(groove_ctx* ctx) { return ctx ? (ctx->fx_ap_stream >= 0 ? 1 : 0) : 0; }
// Host-side only: the form is decided per launch (fx_form_of), and a reverb's lines mean the same to every form (the all-pass rings'
// live copies are geo.base[4..5] whichever kernel wrote them last), so nothing in flight has to finish first.
int groove_set_fx_wet_reverb_run(groove_ctx* ctx, int on) {
  if (!ctx) return fail(nullptr, "groove_set_fx_wet_reverb_run: ctx is NULL");
  ctx->fx_wet_reverb_run = on != 0;
  return 0;
}
int groove_fx_wet_reverb_run(groove_ctx* ctx) { return ctx ? (ctx->fx_wet_reverb_run ? 1 : 0) : 0; }
int groove_set_split_max_waves(groove_ctx* ctx, uint32_t waves) {
  if (!ctx) return fail(nullptr, "groove_set_split_max_waves: ctx is NULL");
  if (ctx_join(ctx)) return 1;
  GHIP(ctx, ctx_wait(ctx));
  ctx->split_max_waves = waves;
  return 0;
}
uint32_t groove_split_max_waves(groove_ctx* ctx) { return ctx ? ctx->split_max_waves : 0; }
int groove_update_sample_rate(groove_ctx* ctx, uint32_t hz) {
  if (!ctx) return fail(nullptr, "groove_update_sample_rate: ctx is NULL");
  if (hz < 1000 || hz > 768000) return fail(ctx, "groove_update_sample_rate: unsupported rate");
  if (ctx_join(ctx)) return 1;
  GHIP(ctx, ctx_wait(ctx));
  ctx->sr = hz;
  for (groove_bank* b : ctx->banks)
    if (bank_derive_and_upload(b)) return 1;
  for (groove_fx* fx : ctx->fxs) {
    fx->last_side = -1; // joined above
    if (fx_setup_state(fx)) return 1;
    if (fx_upload_params(fx)) return 1;
  }
  for (groove_ctl_link* l : ctx->links) // an LFO's increment is f / SR (a trip's table is in beats: it stays)
    if (l->source != GROOVE_CTL_SRC_TRIP && ctl_upload_lanes(l)) return 1;
  return 0;
}
int groove_event_create(groove_ctx* ctx, void** out_event) {
  if (!ctx || !out_event) return fail(ctx, "groove_event_create: NULL argument");
  hipEvent_t ev;
  GHIP(ctx, hipEventCreate(&ev));
  *out_event = (void*)ev;
  return 0;
}
int groove_event_destroy(groove_ctx* ctx, void* event) {
  if (!ctx || !event) return fail(ctx, "groove_event_destroy: NULL argument");
  GHIP(ctx, hipEventDestroy((hipEvent_t)event));
  return 0;
}
int groove_event_record(groove_ctx* ctx, void* event) {
  if (!ctx || !event) return fail(ctx, "groove_event_record: NULL argument");
  if (bus_flush(ctx)) return 1; // the event marks the end of everything asked for so far
  GHIP(ctx, hipEventRecord((hipEvent_t)event, ctx->stream));
  return 0;
}
int groove_event_elapsed_ms(groove_ctx* ctx, void* start, void* stop, float* out_ms) {
  if (!ctx || !start || !stop || !out_ms) return fail(ctx, "groove_event_elapsed_ms: NULL argument");
  GHIP(ctx, wait_deadline(ctx, nullptr, (hipEvent_t)stop, "groove_event_elapsed_ms"));
  GHIP(ctx, hipEventElapsedTime(out_ms, (hipEvent_t)start, (hipEvent_t)stop));
  return 0;
}

// ============================================================================ blocks
int groove_block_create(groove_ctx* ctx, uint32_t n, uint32_t frames_cap, groove_block** out) {
  if (!ctx || !out) return fail(ctx, "groove_block_create: NULL argument");
  if (n == 0 || frames_cap == 0) return fail(ctx, "groove_block_create: empty block");
  GHIP(ctx, hipSetDevice(ctx->device));
  groove_block* b = new groove_block();
  b->ctx = ctx; b->n = n; b->cap = frames_cap; b->d = nullptr;
  const size_t bytes = (size_t)2 * frames_cap * n * 4;
  hipError_t e = hipMalloc(&b->d, bytes);
  if (e != hipSuccess) { delete b; return fail(ctx, std::string("groove_block_create: hipMalloc: ") + hipGetErrorString(e)); }
  (void)hipMemsetAsync(b->d, 0, bytes, ctx->stream);
  *out = b;
  return 0;
}
int groove_block_destroy(groove_block* b) {
  if (!b) return 0;
  // lane sums of this block that still wait for the next all-pass launch: onto their bus first (the buffer dies with the block)
  if (b->ctx->deferred_ap.rows && (b->ctx->deferred_ap.rows == b->d_sums_ap[0] || b->ctx->deferred_ap.rows == b->d_sums_ap[1])) (void)bus_flush_ap(b->ctx);
  if (b->ready_mask) (void)ctx_join(b->ctx);
  (void)hipStreamSynchronize(b->ctx->stream);
  (void)hipFree(b->d);
  (void)hipFree(b->d_alt);
  (void)hipFree(b->d_sums);
  (void)hipFree(b->d_stage); (void)hipFree(b->d_sums_ap[0]); (void)hipFree(b->d_sums_ap[1]);
  if (b->ev_free) (void)hipEventDestroy(b->ev_free);
  for (hipEvent_t e : b->ev_ready) if (e) (void)hipEventDestroy(e);
  delete b;
  return 0;
}
float* groove_block_device_ptr(groove_block* b) {
  // The pointer escapes: whatever the caller's own kernels do to the block, the row sums the last render left no
  // longer describe it (groove_mix would put the pre-modification audio on the bus).
  if (!b) return nullptr;
  if (b->order && (block_acquire(b) || block_normalise(b))) return nullptr; // the caller's lane order, now that somebody looks
  b->sums_valid = false;
  return b->d;
}
int groove_block_mark_dirty(groove_block* b) {
  if (!b) return fail(nullptr, "groove_block_mark_dirty: block is NULL");
  b->sums_valid = false;
  return 0;
}
uint32_t groove_block_lanes(groove_block* b) { return b ? b->n : 0; }
uint32_t groove_block_frames_cap(groove_block* b) { return b ? b->cap : 0; }
int groove_block_upload(groove_block* b, const float* host, uint32_t frames) {
  if (!b || !host) return fail(nullptr, "groove_block_upload: NULL argument");
  groove_ctx* ctx = b->ctx;
  if (frames > b->cap) return fail(ctx, "groove_block_upload: frames > capacity");
  if (block_acquire(b)) return 1;
  b->sums_valid = false;
  b->order.reset(); // the content is replaced
  const size_t per = (size_t)frames * b->n;
  for (int ch = 0; ch < 2; ++ch)
    GHIP(ctx, hipMemcpyAsync(b->d + (size_t)ch * b->cap * b->n, host + ch * per, per * 4, hipMemcpyHostToDevice, ctx->stream));
  GHIP(ctx, ctx_wait(ctx));
  return 0;
}
int groove_block_download(groove_block* b, float* host, uint32_t frames) {
  if (!b || !host) return fail(nullptr, "groove_block_download: NULL argument");
  groove_ctx* ctx = b->ctx;
  if (frames > b->cap) return fail(ctx, "groove_block_download: frames > capacity");
  if (block_acquire(b) || block_normalise(b)) return 1;
  GHIP(ctx, ctx_wait(ctx, "copy on the ctx stream"));
  const size_t per = (size_t)frames * b->n;
  for (int ch = 0; ch < 2; ++ch)
    GHIP(ctx, hipMemcpyAsync(host + ch * per, b->d + (size_t)ch * b->cap * b->n, per * 4, hipMemcpyDeviceToHost, ctx->stream));
  GHIP(ctx, ctx_wait(ctx));
  return 0;
}

// ============================================================================ instruments
// Round-robin side-stream assignment of single-kernel banks; the all-pass stream (groove_set_fx_allpass_stream), while there is
// one, is left to the all-passes: a bank that rendered on it would queue its renders behind them.
static int next_bank_slot(groove_ctx* ctx) {
  int slot = kBaseKinds + ctx->next_stream_slot++ % ctx->bank_streams;
  if (slot == ctx->fx_ap_stream && ctx->bank_streams > 1) slot = kBaseKinds + ctx->next_stream_slot++ % ctx->bank_streams;
  return slot;
}
static int bank_finish_create(groove_bank* b, groove_bank** out) {
  b->stream_slot = next_bank_slot(b->ctx);
  if (bank_alloc(b) || bank_derive_and_upload(b)) { groove_bank_destroy(b); return 1; }
  b->ctx->banks.push_back(b);
  *out = b;
  return 0;
}
int groove_welsh_create(groove_ctx* ctx, const groove_welsh_params* p, uint32_t n, groove_bank** out) {
  if (!ctx || !p || !out) return fail(ctx, "groove_welsh_create: NULL argument");
  if (n == 0) return fail(ctx, "groove_welsh_create: n == 0");
  for (uint32_t v = 0; v < n; ++v) // every kernel form must see the same, canonical enumerators
    if (p[v].oscillator_1.waveform >= GROOVE_WAVEFORM_COUNT || p[v].oscillator_2.waveform >= GROOVE_WAVEFORM_COUNT ||
        p[v].lfo_waveform >= GROOVE_WAVEFORM_COUNT || p[v].lfo_routing >= GROOVE_LFO_ROUTING_COUNT)
      return fail(ctx, "groove_welsh_create: waveform or LFO routing enumerator out of range (voice " + std::to_string(v) + ")");
  groove_bank* b = new groove_bank();
  b->ctx = ctx; b->kind = BANK_WELSH; b->n = n;
  b->pw = sizeof(WelshParams) / 4; b->sw = sizeof(WelshState) / 4;
  b->welsh.assign(p, p + n);
  if (hipMalloc(&b->d_cold, (size_t)4 * n * 8) != hipSuccess) { delete b; return fail(ctx, "groove_welsh_create: hipMalloc failed"); }
  return bank_finish_create(b, out);
}
int groove_fm_create(groove_ctx* ctx, const groove_fm_params* p, uint32_t n, groove_bank** out) {
  if (!ctx || !p || !out) return fail(ctx, "groove_fm_create: NULL argument");
  if (n == 0) return fail(ctx, "groove_fm_create: n == 0");
  groove_bank* b = new groove_bank();
  b->ctx = ctx; b->kind = BANK_FM; b->n = n;
  b->pw = sizeof(FmParams) / 4; b->sw = sizeof(FmState) / 4;
  b->fm.assign(p, p + n);
  if (hipMalloc(&b->d_cold, (size_t)n * 8) != hipSuccess) { delete b; return fail(ctx, "groove_fm_create: hipMalloc failed"); }
  return bank_finish_create(b, out);
}
// groove_sampler_create (channels 1) and groove_sampler_create_stereo (channels 2: the host's interleaved L, R frames are the device's)
static int sampler_create(const char* who, uint32_t channels, groove_ctx* ctx, const float* bank_pcm, uint64_t bank_frames,
                          const groove_sample_desc* descs, uint32_t n_samples,
                          const groove_sampler_params* p, uint32_t n, groove_bank** out) {
  const std::string w = std::string(who) + ": ";
  if (!ctx || !bank_pcm || !descs || !p || !out) return fail(ctx, w + "NULL argument");
  if (n == 0 || n_samples == 0 || bank_frames == 0) return fail(ctx, w + "empty bank");
  if (bank_frames >= (1ull << 32)) return fail(ctx, w + "bank too large");
  for (uint32_t i = 0; i < n_samples; ++i) {
    if (descs[i].offset > bank_frames || descs[i].length > bank_frames - descs[i].offset)
      return fail(ctx, w + "sample descriptor exceeds bank");
    if (descs[i].length == 0) return fail(ctx, w + "empty sample"); // the fetch clamps to length - 1
    if (descs[i].length >= (1u << 20)) return fail(ctx, w + "sample longer than 2^20 frames");
  }
  for (uint32_t i = 0; i < n; ++i)
    if (p[i].sample_index >= n_samples) return fail(ctx, w + "sample_index out of range");
  groove_bank* b = new groove_bank();
  b->ctx = ctx; b->kind = BANK_SAMPLER; b->n = n;
  b->pw = sizeof(SamplerParams) / 4; b->sw = sizeof(SamplerState) / 4;
  b->sampler.assign(p, p + n);
  b->descs.assign(descs, descs + n_samples);
  b->pcm_stereo = channels == 2;
  const size_t bytes = (size_t)bank_frames * 4 * channels;
  if (hipMalloc(&b->d_pcm, bytes) != hipSuccess) { delete b; return fail(ctx, w + "hipMalloc failed"); }
  if (ctx_memcpy(ctx, b->d_pcm, bank_pcm, bytes, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(b->d_pcm); delete b; return fail(ctx, w + "upload failed"); }
  return bank_finish_create(b, out);
}
int groove_sampler_create(groove_ctx* ctx, const float* bank_pcm, uint64_t bank_frames,
                          const groove_sample_desc* descs, uint32_t n_samples,
                          const groove_sampler_params* p, uint32_t n, groove_bank** out) {
  return sampler_create("groove_sampler_create", 1, ctx, bank_pcm, bank_frames, descs, n_samples, p, n, out);
}
int groove_sampler_create_stereo(groove_ctx* ctx, const float* bank_pcm_lr, uint64_t bank_frames,
                                 const groove_sample_desc* descs, uint32_t n_samples,
                                 const groove_sampler_params* p, uint32_t n, groove_bank** out) {
  return sampler_create("groove_sampler_create_stereo", 2, ctx, bank_pcm_lr, bank_frames, descs, n_samples, p, n, out);
}
uint32_t groove_bank_sample_channels(groove_bank* b) { return b && b->kind == BANK_SAMPLER ? (b->pcm_stereo ? 2u : 1u) : 0u; }
// A host-side switch between kernel instantiations: neither parameters nor state are touched.  Joined first like groove_bank_set_param,
// so that the order of effects is the order of calls whatever streams the bank's earlier blocks run on.
int groove_bank_set_sample_interpolation(groove_bank* b, uint32_t mode) {
  if (!b) return fail(nullptr, "groove_bank_set_sample_interpolation: bank is NULL");
  groove_ctx* ctx = b->ctx;
  if (b->kind != BANK_SAMPLER) return fail(ctx, "groove_bank_set_sample_interpolation: only sampler and drumkit banks play samples");
  if (mode != GROOVE_SAMPLE_NEAREST && mode != GROOVE_SAMPLE_LINEAR && mode != GROOVE_SAMPLE_CUBIC)
    return fail(ctx, "groove_bank_set_sample_interpolation: unknown mode (0 nearest, 1 linear, 2 cubic)");
  if (ctx_join(ctx)) return 1;
  b->pcm_interp = mode;
  return 0;
}
uint32_t groove_bank_sample_interpolation(groove_bank* b) { return b && b->kind == BANK_SAMPLER ? b->pcm_interp : (uint32_t)GROOVE_SAMPLE_NEAREST; }
// Like the mode a property of the bank beside parameters and state: reset, a sample-rate change and groove_bank_set_param upload the
// records and leave d_loops alone.  The kernels read a voice's loop by its index, so the samples' loops are spread over the voices here.
int groove_bank_set_sample_loops(groove_bank* b, const groove_sample_loop* loops, uint32_t n_samples) {
  if (!b) return fail(nullptr, "groove_bank_set_sample_loops: bank is NULL");
  groove_ctx* ctx = b->ctx;
  if (b->kind != BANK_SAMPLER) return fail(ctx, "groove_bank_set_sample_loops: only sampler and drumkit banks play samples");
  if (loops) {
    if (n_samples != b->descs.size()) return fail(ctx, "groove_bank_set_sample_loops: n_samples is not the bank's sample count (" + std::to_string(b->descs.size()) + ")");
    for (uint32_t i = 0; i < n_samples; ++i) {
      if (loops[i].start == 0 && loops[i].end == 0) continue;
      if (loops[i].start >= loops[i].end) return fail(ctx, "groove_bank_set_sample_loops: start >= end (sample " + std::to_string(i) + ")");
      if (loops[i].end > b->descs[i].length) return fail(ctx, "groove_bank_set_sample_loops: end beyond the sample's length (sample " + std::to_string(i) + ")");
    }
  }
  if (ctx_join(ctx)) return 1;
  bool any = false;
  for (uint32_t i = 0; loops && i < n_samples; ++i) any = any || loops[i].end != 0;
  if (any) {
    const uint32_t n = b->n;
    std::vector<uint32_t> w((size_t)2 * n);
    for (uint32_t v = 0; v < n; ++v) {
      const groove_sample_loop& l = loops[b->sampler[v].sample_index];
      w[v] = l.start; w[(size_t)n + v] = l.end;
    }
    GHIP(ctx, hipSetDevice(ctx->device));
    GHIP(ctx, ctx_wait(ctx)); // (the last launch that read d_loops has finished)
    if (!b->d_loops && hipMalloc(&b->d_loops, w.size() * 4) != hipSuccess) { b->d_loops = nullptr; return fail(ctx, "groove_bank_set_sample_loops: hipMalloc failed"); }
    GHIP(ctx, ctx_memcpy(ctx, b->d_loops, w.data(), w.size() * 4, hipMemcpyHostToDevice));
    b->loops.assign(loops, loops + n_samples);
  } else {
    b->loops.clear();
    if (b->d_loops) { // (an enveloped bank's kernels go on reading the table: zeros, no loop)
      GHIP(ctx, hipSetDevice(ctx->device));
      GHIP(ctx, ctx_wait(ctx));
      GHIP(ctx, hipMemsetAsync(b->d_loops, 0, (size_t)2 * b->n * 4, ctx->stream));
    }
  }
  b->looped = any;
  return 0;
}
uint32_t groove_bank_sample_loops(groove_bank* b, groove_sample_loop* out, uint32_t cap) {
  if (!b || b->kind != BANK_SAMPLER) return 0;
  uint32_t looped = 0;
  for (size_t i = 0; i < b->descs.size(); ++i) {
    const groove_sample_loop l = i < b->loops.size() ? b->loops[i] : groove_sample_loop{0, 0};
    if (out && i < cap) out[i] = l;
    looped += l.end != 0;
  }
  return looped;
}
// Like the loops a property of the bank beside parameters and state, in a buffer of its own (d_env).  The kernels read a voice's
// record by its index, so the samples' envelopes are spread over the voices (sampler_upload_envelopes).
int groove_bank_set_sample_envelopes(groove_bank* b, const groove_envelope_params* env, const uint32_t* enabled, uint32_t n_samples) {
  if (!b) return fail(nullptr, "groove_bank_set_sample_envelopes: bank is NULL");
  groove_ctx* ctx = b->ctx;
  if (b->kind != BANK_SAMPLER) return fail(ctx, "groove_bank_set_sample_envelopes: only sampler and drumkit banks play samples");
  bool any = false;
  if (env) {
    if (n_samples != b->descs.size()) return fail(ctx, "groove_bank_set_sample_envelopes: n_samples is not the bank's sample count (" + std::to_string(b->descs.size()) + ")");
    for (uint32_t i = 0; i < n_samples; ++i) {
      if (enabled && !enabled[i]) continue;
      const groove_envelope_params& e = env[i];
      if (!(e.attack >= 0.0) || !(e.decay >= 0.0) || !(e.release >= 0.0) || !std::isfinite(e.attack) || !std::isfinite(e.decay) || !std::isfinite(e.release))
        return fail(ctx, "groove_bank_set_sample_envelopes: a negative or non-finite time (sample " + std::to_string(i) + ")");
      if (!(e.sustain >= 0.0 && e.sustain <= 1.0)) return fail(ctx, "groove_bank_set_sample_envelopes: sustain outside [0, 1] (sample " + std::to_string(i) + ")");
      any = true;
    }
  }
  if (flush_events(b)) return 1; // (queued notes come first: they see the envelopes they were sent under)
  if (ctx_join(ctx)) return 1;
  b->ctx_touched = true;
  if (!any && !b->enveloped) { b->envs.clear(); b->env_enabled.clear(); return 0; }
  GHIP(ctx, hipSetDevice(ctx->device));
  GHIP(ctx, ctx_wait(ctx)); // (the last launch that read d_env has finished)
  const uint32_t n = b->n;
  if (any) {
    if (!b->d_env && hipMalloc(&b->d_env, (size_t)kSampleEnvWords * n * 4) != hipSuccess) { b->d_env = nullptr; return fail(ctx, "groove_bank_set_sample_envelopes: hipMalloc failed"); }
    if (!b->d_loops) { // the ENV kernels are the LOOP text: a loop table of zeros for a bank that never had a loop
      if (hipMalloc(&b->d_loops, (size_t)2 * n * 4) != hipSuccess) { b->d_loops = nullptr; return fail(ctx, "groove_bank_set_sample_envelopes: hipMalloc failed"); }
      GHIP(ctx, hipMemsetAsync(b->d_loops, 0, (size_t)2 * n * 4, ctx->stream));
    }
    b->envs.assign(env, env + n_samples);
    b->env_enabled.assign(n_samples, 1u);
    if (enabled) b->env_enabled.assign(enabled, enabled + n_samples);
    if (sampler_upload_envelopes(b)) return 1;
  }
  hipLaunchKernelGGL(sampler_env_setup_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, ctx->stream, b->d_params, b->d_state, b->d_env, n, any ? 0 : 1);
  GHIP(ctx, hipGetLastError());
  if (!any) { b->envs.clear(); b->env_enabled.clear(); }
  b->enveloped = any;
  return 0;
}
uint32_t groove_bank_sample_envelopes(groove_bank* b, groove_envelope_params* out, uint32_t* enabled_out, uint32_t cap) {
  if (!b || b->kind != BANK_SAMPLER) return 0;
  uint32_t count = 0;
  for (size_t i = 0; i < b->descs.size(); ++i) {
    const bool on = i < b->envs.size() && b->env_enabled[i];
    if (out && i < cap) out[i] = on ? b->envs[i] : groove_envelope_params{};
    if (enabled_out && i < cap) enabled_out[i] = on ? 1u : 0u;
    count += on;
  }
  return count;
}
int groove_bank_download_sample_envelope_state(groove_bank* b, uint32_t* words) {
  if (!b || !words) return fail(b ? b->ctx : nullptr, "groove_bank_download_sample_envelope_state: NULL argument");
  groove_ctx* ctx = b->ctx;
  if (b->kind != BANK_SAMPLER || !b->enveloped) return fail(ctx, "groove_bank_download_sample_envelope_state: the bank has no sample envelopes");
  if (flush_events(b)) return 1;
  if (ctx_join(ctx)) return 1;
  GHIP(ctx, ctx_wait(ctx));
  GHIP(ctx, ctx_memcpy(ctx, words, b->d_env + (size_t)kSampleEnvParamWords * b->n, (size_t)kSampleEnvStateWords * b->n * 4, hipMemcpyDeviceToHost));
  return 0;
}
int groove_bank_destroy(groove_bank* b) {
  if (!b) return 0;
  groove_ctx* ctx = b->ctx;
  (void)paced_reduce(b, false);
  (void)ctx_join(ctx);
  (void)hipStreamSynchronize(ctx->stream);
  for (int slot = 0; slot < 2; ++slot) {
    (void)hipFree(b->d_pipe_part[slot]); (void)hipFree(b->d_pipe_seg[slot]);
    if (b->ev_reduce_done[slot]) (void)hipEventDestroy(b->ev_reduce_done[slot]);
    for (int k = 0; k < kBaseKinds + 4; ++k) if (b->ev_render_done[k][slot]) (void)hipEventDestroy(b->ev_render_done[k][slot]);
  }
  auto it = std::find(ctx->banks.begin(), ctx->banks.end(), b);
  if (it != ctx->banks.end()) ctx->banks.erase(it);
  for (groove_ctl_link* l : ctx->links) // a link onto this bank has no target any more: its next apply is an error, not a write
    if (l->bank == b) l->bank = nullptr;
  (void)hipFree(b->d_dca);
  for (int k = 0; k < 2; ++k) { if (b->h_ev[k]) (void)hipHostFree(b->h_ev[k]); if (b->ev_staged[k]) (void)hipEventDestroy(b->ev_staged[k]); }
  (void)hipFree(b->d_params); (void)hipFree(b->d_state); (void)hipFree(b->d_cold); (void)hipFree(b->d_pcm); (void)hipFree(b->d_loops); (void)hipFree(b->d_env); (void)hipFree(b->d_ev[0]); (void)hipFree(b->d_ev[1]); (void)hipFree(b->d_waves); (void)hipFree(b->d_wg_list); (void)hipFree(b->d_wg_cls); (void)hipFree(b->d_wg_base); (void)hipFree(b->d_wg_f32);
  delete b;
  return 0;
}
uint32_t groove_bank_voices(groove_bank* b) { return b ? b->n : 0; }
int groove_bank_note_events(groove_bank* b, const groove_note_event* ev, uint32_t n_ev) {
  if (!b) return fail(nullptr, "groove_bank_note_events: bank is NULL");
  if (n_ev && !ev) return fail(b->ctx, "groove_bank_note_events: ev is NULL");
  for (uint32_t i = 0; i < n_ev; ++i)
    if (ev[i].voice != GROOVE_ALL_VOICES && ev[i].voice >= b->n)
      return fail(b->ctx, "groove_bank_note_events: voice index out of range");
  b->pending.insert(b->pending.end(), ev, ev + n_ev);
  return 0;
}
int groove_bank_set_param(groove_bank* b, uint32_t voice, uint32_t control_index, double value01) {
  if (!b) return fail(nullptr, "groove_bank_set_param: bank is NULL");
  groove_ctx* ctx = b->ctx;
  if (voice != GROOVE_ALL_VOICES && voice >= b->n) return fail(ctx, "groove_bank_set_param: voice out of range");
  const uint32_t lo = voice == GROOVE_ALL_VOICES ? 0 : voice, hi = voice == GROOVE_ALL_VOICES ? b->n : voice + 1;
  if (b->kind != BANK_WELSH) {
    // an FM bank's four controls, a sampler (drumkit) bank's gain: the laws of ctl_core.h, the ones a bank link's kernel runs
    if (ctl_bank_target_ok(control_index)) return fail(ctx, "groove_bank_set_param: only Welsh banks expose controls 32 - 34 (dca-gain, dca-pan, filter-cutoff)");
    const bool fm = b->kind == BANK_FM;
    if (fm && !ctl_fm_target_ok(control_index))
      return fail(ctx, ctl_sampler_target_ok(control_index) ? "groove_bank_set_param: an FM bank's controls are 48 - 51 (dca-gain, dca-pan, depth, beta); 64 is a sampler bank's gain"
                                                            : "groove_bank_set_param: unknown control index");
    if (!fm && !ctl_sampler_target_ok(control_index))
      return fail(ctx, ctl_fm_target_ok(control_index) ? "groove_bank_set_param: a sampler bank's control is 64 (gain); 48 - 51 are an FM bank's"
                                                       : "groove_bank_set_param: unknown control index");
    for (uint32_t v = lo; v < hi; ++v) {
      if (!fm) { b->sampler[v].gain = ctl_sampler_gain_f64(value01); continue; }
      groove_fm_params& p = b->fm[v];
      const float x = ctl_fm_param_f64(control_index, value01);
      switch (control_index) {
        case GROOVE_CTL_FM_DCA_GAIN: p.dca_gain = x; break;
        case GROOVE_CTL_FM_DCA_PAN: p.dca_pan = x; break;
        case GROOVE_CTL_FM_DEPTH: p.depth = x; break;
        default: p.beta = x; break;
      }
    }
    // control-plane path like the Welsh one below: the parameter SoA only — the voices' state and d_cold stay where they are
    if (ctx_join(ctx)) return 1;
    GHIP(ctx, ctx_wait(ctx));
    return fm ? fm_upload_params(b) : sampler_upload_params(b);
  }
  const double v01 = value01 < 0.0 ? 0.0 : (value01 > 1.0 ? 1.0 : value01);
  for (uint32_t v = lo; v < hi; ++v) {
    groove_welsh_params& p = b->welsh[v];
    switch (control_index) {
      case GROOVE_CTL_WELSH_DCA_GAIN: p.dca_gain = (float)v01; break;
      case GROOVE_CTL_WELSH_DCA_PAN: p.dca_pan = (float)(v01 * 2.0 - 1.0); break; // ControlValue 0..1 → BipolarNormal
      case GROOVE_CTL_WELSH_CUTOFF: p.filter_cutoff_hz = (float)percent_to_frequency_h(v01); break;
      default: return fail(ctx, "groove_bank_set_param: unknown control index");
    }
  }
  // control-plane path: re-derive and re-upload the parameter tables (state is untouched)
  if (ctx_join(ctx)) return 1;
  GHIP(ctx, ctx_wait(ctx));
  return welsh_upload_params(b, false); // the state stays where it is: keep the lane order
}
// The block's row-sum buffer for a render of `rows` partial rows (reallocated when it grows).
static float* block_sums(groove_block* blk, uint32_t rows, uint32_t frames) {
  const size_t need = (size_t)rows * 2 * frames;
  if (blk->sums_cap < need) {
    if (blk->d_sums) { (void)hipStreamSynchronize(blk->ctx->stream); (void)hipFree(blk->d_sums); blk->d_sums = nullptr; blk->sums_cap = 0; }
    const size_t cap = std::max(need, (size_t)rows * 2 * std::min<uint32_t>(blk->cap, 4096));
    if (hipMalloc(&blk->d_sums, cap * 4) != hipSuccess) { fail(blk->ctx, "block row sums: hipMalloc failed"); return nullptr; }
    blk->sums_cap = cap;
  }
  blk->sums_valid = false;
  blk->sums_on_ap = false;
  return blk->d_sums;
}
// Small Welsh banks and blocks of up to 256 frames: one wavefront per voice, lanes = time (welsh_tp.h).
static bool use_tp(const groove_bank* b, uint32_t frames) {
  if (frames > kTpMaxFrames || b->ctx->tp_max_voices == 0) return false;
  if (b->kind == BANK_WELSH) {
    // two voices per wavefront move the crossover with the role-split kernel up by three eighths (measured, round 3: 18,432
    // voices 0.069 ms per block against 0.083, 22,528 0.080 against 0.084, 24,576 0.084 against 0.083)
    const uint32_t tmax = b->ctx->tp_max_voices;
    const bool pairs = b->plan.tp_pairs && b->ctx->tp_vpw2_min_voices && b->n >= b->ctx->tp_vpw2_min_voices;
    return b->n <= (pairs ? tmax + (uint32_t)std::min<uint64_t>((uint64_t)tmax * 3 / 8, 0x40000000u) : tmax);
  }
  if (b->kind == BANK_FM) return b->n <= b->ctx->fm_tp_max_voices; // no filter scan: far cheaper per voice than a Welsh voice
  if (b->kind == BANK_SAMPLER) return b->n <= kSamplerTpMaxVoices; // a pure gather
  return false;
}
static uint32_t tp_vpw(const groove_bank* b) { // voices per wavefront of the time-parallel Welsh / FM kernels
  if (b->kind == BANK_FM) { // (parameters per lane: no condition on the patches) four once the one-voice form is past ~3 wavefronts per SIMD
    const uint32_t m = b->ctx->fm_tp_vpw4_min_voices;
    return (m && b->n >= m) ? 4u : 1u;
  }
  return (b->kind == BANK_WELSH && b->plan.tp_pairs && b->ctx->tp_vpw2_min_voices && b->n >= b->ctx->tp_vpw2_min_voices) ? 2u : 1u;
}
// ---- which kernel form a bank takes for a block, and the launches of each form
// THE form decision: the entry points below, fused_rows, use_split and groove_bank_kernel_form all ask here.
enum class Form {
  TimeParallel,      // use_tp: one launch (welsh_tp.h), all three bank kinds
  WelshPerLane,      // n_vwaves == 0 (every voice its own patch): the per-lane kernel over the physical lanes
  WelshSmallUniform, // below the per-kind pipeline's threshold: all base kinds in one launch (launch_small_uniform)
  WelshBigUniform,   // at or above it: the mix kernel's three sections and a kernel per exact-f64 kind (big_pieces), or one kernel per base kind (launch_render) — several launches on several streams
  FmSerial,          // one voice per lane
  SamplerSerial,
};
static Form form_of(const groove_bank* b, uint32_t frames) {
  if (use_tp(b, frames)) return Form::TimeParallel;
  if (b->kind == BANK_FM) return Form::FmSerial;
  if (b->kind == BANK_SAMPLER) return Form::SamplerSerial;
  if (b->plan.n_vwaves == 0) return Form::WelshPerLane;
  return b->plan.n_vwaves < b->ctx->pipeline_min_waves ? Form::WelshSmallUniform : Form::WelshBigUniform;
}
// rows of partial[][2][frames] a bank's fused render writes: one per workgroup of the form's launch(es)
static uint32_t fused_rows(const groove_bank* b, Form form) {
  switch (form) {
    case Form::TimeParallel: return b->kind == BANK_SAMPLER ? sampler_tp_workgroups(b->n) : b->kind == BANK_WELSH ? welsh_tp_grid(b->n, tp_vpw(b)) : welsh_tp_workgroups(b->n, tp_vpw(b));
    case Form::WelshSmallUniform: case Form::WelshBigUniform: return (b->plan.n_vwaves + kWaves - 1) / kWaves;
    default: return blocks_for(b->n);
  }
}
// A small-uniform bank's launch is role-split (welsh_split.h) when the bank is mid-size and the block long enough.
static bool use_split(const groove_bank* b, Form form, uint32_t frames) {
  return form == Form::WelshSmallUniform && b->plan.n_vwaves <= b->ctx->split_max_waves && frames >= 2 * kSplitChunk;
}
// The one argument block of the wave-uniform Welsh kernels: entries [wg_off, wg_off + n_wgs) of the bank's workgroup lists.
static UniformArgs uniform_args(const groove_bank* b, float* out, float* rows, size_t wg_off, size_t chs, uint32_t frames, uint32_t n_wgs) {
  UniformArgs a{b->d_waves, b->d_state, out, rows, b->d_wg_list + wg_off, b->d_wg_cls + wg_off, b->d_wg_f32 + wg_off, chs, render_consts_of(b->ctx), b->plan.n_vwaves, b->n, frames, n_wgs, TpPrev{}};
  a.diag = b->ctx->d_diag;
#ifdef GROOVE_HEARTBEAT
  a.heartbeat = b->ctx->hb;
#endif
  return a;
}
// The per-base-kind slices of a wave-uniform bank's kind-sorted workgroup list (welsh_plan.h KindSlices).
static KindSlices kind_slices(const groove_bank* b) { return kind_slices(b->plan.wgs_of_kind); }
// One base kind's own kernel over `a`'s workgroups on stream `st`, one translation unit each (csrc/welsh_class.hip).  Fused: the
// exact-f64 kinds 4 and 5 only — the four others have no fused kernel of their own: the all-kinds, role-split and mix kernels carry them.
static void launch_welsh_kind(int k, const UniformArgs& a, hipStream_t st, bool fused, hipEvent_t done = nullptr) {
  typedef void (*Launcher)(const UniformArgs&, hipStream_t, bool, hipEvent_t);
  static constexpr Launcher of_kind[kBaseKinds] = {launch_welsh_uniform_specialised<0>, launch_welsh_uniform_specialised<1>, launch_welsh_uniform_specialised<2>,
                                                   launch_welsh_uniform_specialised<3>, launch_welsh_uniform_specialised<4>, launch_welsh_uniform_specialised<5>};
  of_kind[k](a, st, fused, done);
}
// ... over the kind's slice of the bank's kind-sorted workgroup list
static void launch_kind_slice(const groove_bank* b, int k, bool fused, size_t chs, float* out, float* rows, uint32_t frames, hipStream_t st, hipEvent_t done = nullptr) {
  const KindSlices p = kind_slices(b);
  launch_welsh_kind(k, uniform_args(b, out, rows, p.offset[k], chs, frames, p.count[k]), st, fused, done);
}
// The pieces of a BIG wave-uniform bank (Form::WelshBigUniform) in the pipelined fused and the asynchronous block-writing walks
// (the synchronous one has its own: launch_render), in launch order, longest walk first: the exact-f64 kinds 5 and 4, a
// kernel each over the kind's slice of the sorted list, then sections 2, 1, 0 of the MIX kernel (kernels.h; round 6) — the
// class-specialised workgroups in three launches, each over a third of them: the section's entries of the striped copies of all four
// lists (welsh_plan.h).  A piece is named by the side stream the pipelined and asynchronous walks give it: kind k -> k, section s -> s.
// Empty pieces are left out.
struct BigPieces {
  int k[5]; int n = 0;
  const int* begin() const { return k; }
  const int* end() const { return k + n; }
};
static BigPieces big_pieces(const groove_bank* b) {
  BigPieces l;
  const KindSlices p = kind_slices(b);
  for (int k = kBaseKinds - 1; k >= 4; --k) if (p.count[k]) l.k[l.n++] = k;
  for (int sec = 2; sec >= 0; --sec) if (b->plan.mix_cnt[sec]) l.k[l.n++] = sec;
  return l;
}
static void launch_piece(const groove_bank* b, int piece, bool fused, size_t chs, float* out, float* rows, uint32_t frames, hipStream_t st, hipEvent_t done = nullptr) {
  if (piece >= 4) { launch_kind_slice(b, piece, fused, chs, out, rows, frames, st, done); return; }
  const size_t o = b->wg_list_cap + b->plan.mix_off[piece];
  const UniformArgs a = uniform_args(b, out, rows, o, chs, frames, b->plan.mix_cnt[piece]);
  if (fused) launch_welsh_uniform_mix(a, b->d_wg_base + o, st, done);
  else launch_welsh_uniform_mix_unfused(a, b->d_wg_base + o, st, done);
}
// A Welsh bank below the per-kind pipeline's threshold: ONE launch for the workgroups of the four class-specialised base kinds —
// role-split when `split`, the all-kinds kernel otherwise.  `done` is bound to the last launch.
static void launch_small_uniform(const groove_bank* b, const UniformArgs& a, hipStream_t st, bool fused, bool split, hipEvent_t done) {
  const KindSlices p = kind_slices(b);
  if (p.n_spec) {
    UniformArgs s = a;
    s.n_wgs = p.n_spec;
    const hipEvent_t d = (p.count[4] || p.count[5]) ? nullptr : done;
    if (split) launch_welsh_split4(s, b->d_wg_base, st, fused, d);
    else if (fused) launch_welsh_uniform_any(s, b->d_wg_base, st, d);
    else launch_welsh_uniform_any_unfused(s, b->d_wg_base, st, d);
  }
  // exact-f64 LFO kinds (rare; their bodies need 133 VGPRs): the per-kind kernels, budgeted for them, behind it on the same stream
  for (int k = 4; k < kBaseKinds; ++k) {
    if (!p.count[k]) continue;
    UniformArgs r = a;
    r.prev = TpPrev{}; // (the launch above carried the previous block's rows)
    r.wg_list = a.wg_list + p.offset[k]; r.wg_cls = a.wg_cls + p.offset[k]; r.n_wgs = p.count[k];
    launch_welsh_kind(k, r, st, fused, (k == 5 || !p.count[5]) ? done : nullptr);
  }
}
// The serial sampler kernel: one mode, with or without looped samples (LOOP: b->d_loops, the voices' loop words), with or without
// enveloped ones (ENV, on the LOOP text: b->d_env, the voices' envelope records).
extern "C++" template <int MODE, bool LOOP, bool ENV = false>
static void launch_sampler_serial_form(groove_bank* b, uint32_t frames, bool fused, size_t chs, float* out, float* rows, dim3 grid, dim3 blk, hipStream_t st, hipEvent_t done) {
  const uint32_t* loops = LOOP ? b->d_loops : nullptr;
  uint32_t* envs = ENV ? b->d_env : nullptr;
  if (b->pcm_stereo) {
    if (fused) launch_bound(sampler_render_kernel<true, true, MODE, LOOP, ENV>, grid, blk, st, done, b->d_params, b->d_state, b->n, frames, chs, out, rows, (const float*)b->d_pcm, loops, envs);
    else launch_bound(sampler_render_kernel<false, true, MODE, LOOP, ENV>, grid, blk, st, done, b->d_params, b->d_state, b->n, frames, chs, out, rows, (const float*)b->d_pcm, loops, envs);
  } else if (fused) launch_bound(sampler_render_kernel<true, false, MODE, LOOP, ENV>, grid, blk, st, done, b->d_params, b->d_state, b->n, frames, chs, out, rows, (const float*)b->d_pcm, loops, envs);
  else launch_bound(sampler_render_kernel<false, false, MODE, LOOP, ENV>, grid, blk, st, done, b->d_params, b->d_state, b->n, frames, chs, out, rows, (const float*)b->d_pcm, loops, envs);
}
extern "C++" template <int MODE>
static void launch_sampler_serial_mode(groove_bank* b, uint32_t frames, bool fused, size_t chs, float* out, float* rows, dim3 grid, dim3 blk, hipStream_t st, hipEvent_t done) {
  if (b->enveloped) launch_sampler_serial_form<MODE, true, true>(b, frames, fused, chs, out, rows, grid, blk, st, done);
  else if (b->looped) launch_sampler_serial_form<MODE, true>(b, frames, fused, chs, out, rows, grid, blk, st, done);
  else launch_sampler_serial_form<MODE, false>(b, frames, fused, chs, out, rows, grid, blk, st, done);
}
// Every form but the big uniform one is ONE launch sequence on ONE stream, and this is where it is launched.  fused: `rows` =
// partial rows only; otherwise `out` = the planar block and `rows` = its row sums (kernels.h run_frames), null for none.
// `done` (optional) completes with the (last) kernel: bound to the dispatch (kernels.h launch_bound).  `prev`: the previous
// deferred block's rows, for this launch to put on their bus (time-parallel and small uniform forms); `head`: a BiQuad effect
// bank fused into the block-writing time-parallel Welsh kernel (welsh_tp.h); `sampler_vpw`: time-parallel sampler, voices per
// wavefront (0: the default rule).
static void launch_single(groove_bank* b, Form form, uint32_t frames, bool fused, size_t chs, float* out, float* rows, hipStream_t st, hipEvent_t done = nullptr,
                          const TpPrev* prev = nullptr, const groove_fx* head = nullptr, uint32_t sampler_vpw = 0) {
  const dim3 grid(form == Form::TimeParallel ? 0 : fused_rows(b, form)), blk(kThreads);
  switch (form) {
    case Form::TimeParallel: {
      TpArgs a{b->d_params, b->d_state, out, rows, chs, render_consts_of(b->ctx), b->n, frames, TpPrev{}};
      if (prev) a.prev = *prev;
      if (head) { a.bq_coef = head->d_coef; a.bq_st = head->d_st; a.bq_wet = head->d_wet; }
      if (b->kind == BANK_FM) { a.vpw = tp_vpw(b); launch_fm_tp(a, st, fused, done); }
      else if (b->kind == BANK_SAMPLER) { a.vpw = sampler_vpw; launch_sampler_tp(a, b->d_pcm, b->pcm_stereo, b->pcm_interp, b->looped || b->enveloped ? b->d_loops : nullptr, b->enveloped ? b->d_env : nullptr, b->inline_ev, st, fused, done); b->inline_ev.n = 0; }
      else { a.full_coef = b->plan.tp_full_coef; a.vpw = tp_vpw(b); launch_welsh_tp(a, st, fused, done); }
      break;
    }
    case Form::WelshSmallUniform: {
      UniformArgs a = uniform_args(b, out, rows, 0, chs, frames, grid.x);
      if (prev) a.prev = *prev;
      launch_small_uniform(b, a, st, fused, use_split(b, form, frames), done);
      break;
    }
    case Form::WelshPerLane:
      if (fused) launch_bound(welsh_render_kernel<true>, grid, blk, st, done, b->d_params, b->d_state, b->n, frames, chs, out, rows, render_consts_of(b->ctx));
      else launch_bound(welsh_render_kernel<false>, grid, blk, st, done, b->d_params, b->d_state, b->n, frames, chs, out, rows, render_consts_of(b->ctx));
      break;
    case Form::FmSerial:
      if (fused) launch_bound(fm_render_kernel<true>, grid, blk, st, done, b->d_params, b->d_state, b->n, frames, chs, out, rows);
      else launch_bound(fm_render_kernel<false>, grid, blk, st, done, b->d_params, b->d_state, b->n, frames, chs, out, rows);
      break;
    case Form::SamplerSerial:
      if (b->pcm_interp == GROOVE_SAMPLE_LINEAR) launch_sampler_serial_mode<GROOVE_SAMPLE_LINEAR>(b, frames, fused, chs, out, rows, grid, blk, st, done);
      else if (b->pcm_interp == GROOVE_SAMPLE_CUBIC) launch_sampler_serial_mode<GROOVE_SAMPLE_CUBIC>(b, frames, fused, chs, out, rows, grid, blk, st, done);
      else launch_sampler_serial_mode<GROOVE_SAMPLE_NEAREST>(b, frames, fused, chs, out, rows, grid, blk, st, done);
      break;
    case Form::WelshBigUniform: break; // (the callers' own walks over big_pieces / the base kinds: their stream policies differ on purpose)
  }
}
// groove_bank_render and the non-pipelined groove_bank_render_mix: everything on the ctx stream, but for the big uniform form.
static int launch_render(groove_bank* b, uint32_t frames, bool fused, size_t chs, float* out, float* rows) {
  groove_ctx* ctx = b->ctx;
  b->ctx_touched = true;
  const Form form = form_of(b, frames);
  if (form == Form::WelshBigUniform) {
    // One block-writing kernel per base kind present, all running concurrently: the most expensive kind goes out first on the ctx
    // stream (list scheduling, longest first), the others on side streams forked from it, and the ctx stream joins them before
    // whatever reads the block.  (Not big_pieces: at 1,000,000 voices the mix kernel's three launches take 0.912 ms per block here
    // where these take 0.857 — docs/HISTORY.md section 17; the bits are the same.)
    if (fused) return fail(ctx, "launch_render: the fused render of a big uniform bank is render_mix_pipelined's"); // (groove_bank_render_mix sends it there)
    const KindSlices p = kind_slices(b);
    int present = 0;
    for (uint32_t c : p.count) present += c ? 1 : 0;
    if (present > 1) GHIP(ctx, hipEventRecord(ctx->ev_fork, ctx->stream));
    int side = -1; // the first kind: the ctx stream
    for (int k = kBaseKinds - 1; k >= 0; --k) {
      if (!p.count[k]) continue;
      hipStream_t st = side < 0 ? ctx->stream : side_stream_of(ctx, side);
      if (side >= 0) GHIP(ctx, hipStreamWaitEvent(st, ctx->ev_fork, 0));
      launch_kind_slice(b, k, false, chs, out, rows, frames, st);
      if (side >= 0) {
        GHIP(ctx, hipEventRecord(ctx->ev_join[side], st));
        GHIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_join[side], 0));
      }
      ++side;
    }
    ctx->need_fork = true; // ctx-stream work the pipelined path's side streams must see
  } else {
    launch_single(b, form, frames, fused, chs, out, rows, ctx->stream);
  }
  GHIP(ctx, hipGetLastError());
  return 0;
}
int groove_bank_render(groove_bank* b, uint32_t frames, groove_block* out) {
  if (!b || !out) return fail(nullptr, "groove_bank_render: NULL argument");
  groove_ctx* ctx = b->ctx;
  if (out->n != b->n) return fail(ctx, "groove_bank_render: block lanes != bank voices");
  if (frames > out->cap) return fail(ctx, "groove_bank_render: frames > block capacity");
  if (frames == 0) return 0;
  GHIP(ctx, hipSetDevice(ctx->device));
  if (flush_events(b, use_tp(b, frames))) return 1;
  if (ctx_join(ctx)) return 1; // the bank's state may still be in flight on the side streams (pipelined fused renders)
  b->side_mode = 0;
  out->ready_mask = 0; // joined above
  const uint32_t rows_n = fused_rows(b, form_of(b, frames));
  float* rows = block_sums(out, rows_n, frames);
  if (!rows) return 1;
  auto rendered = [&]() { out->sum_rows = rows_n; out->sum_frames = frames; out->sums_valid = true; return 0; };
  // a regrouped bank renders in ITS lane order (coalesced rows) into the block's second buffer; the caller's order is
  // produced when — and if — something asks for it (groove_block: lazy lane order)
  float* dst = nullptr;
  if (block_render_target(out, b->order, frames, &dst)) return 1;
  return launch_render(b, frames, false, (size_t)out->cap * out->n, dst, rows) || rendered();
}
// groove_bank_render on the side streams: the render kernels start once everything submitted to the
// ctx stream so far has finished (that covers the previous users of `out` and of the bank), and run
// beside whatever the ctx stream is given next; the ctx-stream operations that take `out` wait for
// them (block_acquire).  A host that keeps two blocks per instrument and submits the render of block
// b+1 before the effect chain of block b overlaps the two (bench.py, workload chain-4096: the Welsh
// render of a 4,096-voice bank is one wavefront's serial walk, 0.2 ms whatever else runs).
static bool fx_is_biquad12(uint32_t kind) {
  switch (kind) {
    case GROOVE_FX_BIQUAD_LP12: case GROOVE_FX_BIQUAD_HP12: case GROOVE_FX_BIQUAD_BP12: case GROOVE_FX_BIQUAD_BS12:
    case GROOVE_FX_BIQUAD_AP12: case GROOVE_FX_BIQUAD_PEAK12: case GROOVE_FX_BIQUAD_LSHELF12: case GROOVE_FX_BIQUAD_HSHELF12: return true;
    default: return false;
  }
}
// A block's ev_free and ev_ready[], created on its first asynchronous use.
static int block_events(groove_block* blk) {
  if (blk->ev_free) return 0;
  GHIP(blk->ctx, hipEventCreateWithFlags(&blk->ev_free, kSyncEventFlags));
  for (int k = 0; k < kSideStreams; ++k) GHIP(blk->ctx, hipEventCreateWithFlags(&blk->ev_ready[k], kSyncEventFlags));
  return 0;
}
// `head` (may be null): a 12 dB BiQuad effect bank to be applied to the block inside the render kernel — only honoured
// (*head_fused = true) when the bank renders time-parallel and its lanes are in the caller's order.
// `chained`: an effect chain follows on this block (groove_bank_render_chain_async), so the lane sums the render would leave are
// never read — a time-parallel Welsh render then does not write them (2 MB per block for config #3's 4,096 voices).
static int render_async_impl(groove_bank* b, uint32_t frames, groove_block* out, groove_fx* head, bool* head_fused, bool chained = false) {
  if (head_fused) *head_fused = false;
  if (!b || !out) return fail(nullptr, "groove_bank_render_async: NULL argument");
  groove_ctx* ctx = b->ctx;
  if (out->n != b->n) return fail(ctx, "groove_bank_render_async: block lanes != bank voices");
  if (frames > out->cap) return fail(ctx, "groove_bank_render_async: frames > block capacity");
  if (frames == 0) return 0;
  GHIP(ctx, hipSetDevice(ctx->device));
  if (flush_events(b, use_tp(b, frames))) return 1;
  const bool was_released = out->released;
  if (block_acquire(out)) return 1; // an earlier asynchronous render into the same block comes first
  const Form form = form_of(b, frames);
  const bool tp = form == Form::TimeParallel, uniform = form == Form::WelshBigUniform;
  if (bank_side_mode(b, uniform ? 1 : 2)) return 1;
  if (block_events(out)) return 1;
  const size_t chs = (size_t)out->cap * out->n;
  const uint32_t rows_n = fused_rows(b, form);
  const bool no_sums = chained && tp && b->kind == BANK_WELSH;
  float* rows = no_sums ? nullptr : block_sums(out, rows_n, frames);
  if (!rows && !no_sums) return 1;
  if (no_sums) out->sums_valid = false;
  float* dst = nullptr; // a regrouped bank: the block's library-order buffer (lazy lane order)
  if (block_render_target(out, b->order, frames, &dst)) return 1;
  // What the render has to wait for on the ctx stream: the block's consumers, and the bank's state if
  // the ctx stream has worked on it.  A block the host has released (groove_block_release) carries the
  // event of that moment, typically long past, so the render follows the previous one on its stream
  // without a cross-queue wait; otherwise everything submitted so far is waited for.
  const bool free_recorded_now = !(was_released && !b->ctx_touched);
  if (free_recorded_now) GHIP(ctx, hipEventRecord(out->ev_free, ctx->stream));
  b->ctx_touched = false;
  uint32_t used = 0;
  auto begin = [&](int k) -> hipStream_t {
    hipStream_t st = side_stream_of(ctx, k);
    (void)hipStreamWaitEvent(st, out->ev_free, 0);
    // An ev_free recorded in this call is later than any ev_fork; the event of an earlier release may
    // predate one, and then this (shared) side stream still owes the wait for the fork.
    if (ctx->fork_pending[k] && !free_recorded_now) (void)hipStreamWaitEvent(st, ctx->ev_fork, 0);
    ctx->fork_pending[k] = false;
    return st;
  };
  bool ready_bound = false; // the launch itself carries out->ev_ready[k]
  auto end = [&](int k) {
    if (!ready_bound) (void)hipEventRecord(out->ev_ready[k], side_stream_of(ctx, k));
    used |= 1u << k;
    ctx->side_busy[k] = true;
  };
  if (uniform) {
    // the exact-f64 kinds' own kernels and the MIX kernel's sections in its block-writing form, each on its own side stream
    for (int k : big_pieces(b)) {
      hipStream_t st = begin(k);
      launch_piece(b, k, false, chs, dst, rows, frames, st);
      end(k);
    }
  } else {
    const int k = b->stream_slot;
    hipStream_t st = begin(k);
    if (tp) {
      const bool fuse = head && b->kind == BANK_WELSH && !b->order && fx_is_biquad12(head->kind) && head->n == b->n && head->ctx == ctx;
      if (fuse) { // the effect's state moves to this side stream (fx_acquire_ctx)
        if (head->last_side != k) {
          if (!head->ev_done) GHIP(ctx, hipEventCreateWithFlags(&head->ev_done, kSyncEventFlags));
          if (head->last_side < 0) GHIP(ctx, hipEventRecord(head->ev_done, ctx->stream));
          else if (fx_done_event(head)) return 1;
          GHIP(ctx, hipStreamWaitEvent(st, head->ev_done, 0));
        }
      }
      // the block's "ready" event completes with the render kernel itself (no record behind it)
      const bool bind = ctx->bind_events && b->kind == BANK_WELSH;
      launch_single(b, form, frames, false, chs, dst, rows, st, bind ? out->ev_ready[k] : nullptr, nullptr, fuse ? head : nullptr);
      if (fuse) { // the effect's last use ends with that kernel too: its own event is recorded when somebody asks (fx_done_event)
        if (bind) head->done_recorded = false;
        else { GHIP(ctx, hipEventRecord(head->ev_done, st)); head->done_recorded = true; }
        head->last_side = k;
        *head_fused = true;
      }
      ready_bound = bind;
    } else {
      launch_single(b, form, frames, false, chs, dst, rows, st);
    }
    end(k);
  }
  out->ready_mask = used;
  if (!no_sums) { out->sum_rows = rows_n; out->sum_frames = frames; out->sums_valid = true; }
  GHIP(ctx, hipGetLastError());
  return 0;
}
int groove_bank_render_async(groove_bank* b, uint32_t frames, groove_block* out) { return render_async_impl(b, frames, out, nullptr, nullptr); }
int groove_block_release(groove_block* b) {
  if (!b) return fail(nullptr, "groove_block_release: block is NULL");
  groove_ctx* ctx = b->ctx;
  const bool marked = b->free_marked; // nothing has taken the block since the mix that bound ev_free to its last kernel
  if (ctx->fx_ap_stream >= 0 && b->ev_free && b->ready_mask == (1u << ctx->fx_ap_stream)) {
    // the block's last kernel is on the all-pass stream and nothing of the ctx stream's is behind it: the release is recorded there
    // (the ctx stream does not wait for the block); the block stays "pending" for the ctx stream until somebody has waited
    GHIP(ctx, hipEventRecord(b->ev_free, ap_stream(ctx)));
    b->released = true; b->free_marked = false;
    return 0;
  }
  if (block_acquire(b)) return 1;
  if (block_events(b)) return 1;
  if (!marked) GHIP(ctx, hipEventRecord(b->ev_free, ctx->stream));
  b->released = true;
  return 0;
}
int groove_block_acquire(groove_block* b) {
  if (!b) return fail(nullptr, "groove_block_acquire: block is NULL");
  b->sums_valid = false; // the caller is about to run its own kernels on the block (include/groove_hip.h)
  return block_acquire(b);
}
// Fused render + mix of a wave-uniform Welsh bank, pipelined over blocks.  Every base kind has its
// own stream that carries that kind's kernels block after block (a workgroup's state only depends
// on the same workgroup's previous block); the ctx stream carries the bus reductions, each waiting
// for its block's kernels.  Nothing makes block b+1's kernels wait for block b's reduction, so the
// thinly occupied tail of one block (the last, partly filled round of waves) overlaps the head of
// the next: ≈ 15 % at 1,000,000 voices, more for smaller banks.  Two slots of partial rows; a kind's
// render of block b+2 waits for the reduction of block b.
static int render_mix_pipelined(groove_bank* b, uint32_t frames, float* bus_dev, int accumulate, bool paced = false) {
  groove_ctx* ctx = b->ctx;
  const Form form = form_of(b, frames);
  const bool uniform = form == Form::WelshBigUniform;
  const uint32_t rows = fused_rows(b, form);
  const size_t part_floats = (size_t)rows * 2 * frames, seg_floats = reduce_seg_floats(rows, frames);
  if (bank_side_mode(b, uniform ? 1 : 2)) return 1;
  const int slot = b->pipe_slot;
  b->pipe_slot ^= 1;
  if (b->paced.active && (!paced || b->paced.slot == slot)) // (an unpaced call, or the slot's rows still owed)
    if (const int rc = paced_reduce(b, false)) return rc;
  if (b->pipe_part_cap[slot] < part_floats || b->pipe_seg_cap[slot] < seg_floats) {
    if (b->paced.active) if (const int rc = paced_reduce(b, false)) return rc;
    if (ctx_join(ctx)) return 1;
    GHIP(ctx, ctx_wait(ctx));
    if (b->d_pipe_part[slot]) GHIP(ctx, hipFree(b->d_pipe_part[slot]));
    GHIP(ctx, hipMalloc(&b->d_pipe_part[slot], part_floats * 4));
    b->pipe_part_cap[slot] = part_floats;
    if (ensure_seg_buffer(ctx, &b->d_pipe_seg[slot], &b->pipe_seg_cap[slot], seg_floats)) return 1;
    b->reduce_recorded[slot] = false;
  }
  if (!b->ev_reduce_done[slot]) {
    GHIP(ctx, hipEventCreateWithFlags(&b->ev_reduce_done[slot], kSyncEventFlags));
    for (int k = 0; k < kSideStreams; ++k) GHIP(ctx, hipEventCreateWithFlags(&b->ev_render_done[k][slot], kSyncEventFlags));
  }
  // Which side streams carry a launch, in launch order: a big uniform bank's pieces (big_pieces: streams 5, 4 the exact-f64 kinds, 2 - 0
  // the mix launches, 3 nothing); every other form is one kernel on the bank's own side stream.
  int on[kSideStreams], n_on = 0;
  if (uniform) for (int piece : big_pieces(b)) on[n_on++] = piece; // (a piece's name IS its side stream)
  else if (rows) on[n_on++] = b->stream_slot;
  if (ctx->need_fork) { // side streams must see what the ctx stream did since the last join (note events, uploads)
    GHIP(ctx, hipEventRecord(ctx->ev_fork, ctx->stream));
    for (bool& f : ctx->fork_pending) f = true;
    ctx->need_fork = false;
  }
  // paced: the HOST waits for the reduction that frees this slot's rows (two blocks back: long done), so that the waits below are
  // dropped when they are made and the render streams carry no wait packet (docs/STREAMS.md item 13)
  // (A deadline that passes here loses nothing either: the streams wait for that reduction themselves below — with a wait packet this
  // once — the block is rendered and registered, and the call reports the deadline when it returns.  Found under GROOVE_SAFE_STREAMS=1,
  // where the bank streams are the kind streams and a blocked stream holds back more: the call used to return BEFORE its render, and a
  // caller that carried on had skipped a block of that bank.)
  int late = 0;
  if (paced && b->reduce_recorded[slot]) {
    const hipError_t e = wait_deadline(ctx, nullptr, b->ev_reduce_done[slot], "groove_bank_render_mix_paced: the slot's previous reduction");
    if (e == hipErrorNotReady) late = 2;
    else GHIP(ctx, e);
  }
  uint32_t used = 0;
  for (int i = 0; i < n_on; ++i) {
    const int k = on[i];
    hipStream_t st = side_stream_of(ctx, k);
    used |= 1u << k;
    if (ctx->fork_pending[k]) { GHIP(ctx, hipStreamWaitEvent(st, ctx->ev_fork, 0)); ctx->fork_pending[k] = false; }
    if (b->reduce_recorded[slot]) GHIP(ctx, hipStreamWaitEvent(st, b->ev_reduce_done[slot], 0));
    // the block's "render done" event completes with the render kernel itself (kernels.h launch_bound): no record packet between
    // this block's kernel and the next block's on the stream
    const hipEvent_t done = ctx->bind_events ? b->ev_render_done[k][slot] : nullptr;
    float* part = b->d_pipe_part[slot];
    if (uniform) launch_piece(b, k, true, 0, part, part, frames, st, done);
    else launch_single(b, form, frames, true, 0, part, part, st, done);
    if (!done) GHIP(ctx, hipEventRecord(b->ev_render_done[k][slot], st));
    if (!paced) GHIP(ctx, hipStreamWaitEvent(ctx->stream, b->ev_render_done[k][slot], 0));
    ctx->side_busy[k] = true;
  }
  b->ctx_touched = false; // the bank's stream(s) have waited for whatever the ctx stream did to its state (ev_fork above)
  if (paced) {
    // this block's reduction is launched by the bank's NEXT paced call (or a flush point); the previous block's is launched now: its
    // renders were submitted a whole call ago, the host waits for them (this block's are already queued behind them)
    if (b->paced.active) {
      int rc = paced_reduce(b, true);
      if (rc == 2) {
        // The host's wait for the previous block's renders passed its deadline.  This block's kernels are already queued and a
        // bank has ONE pending record: the previous block's reduction is queued behind device-side waits instead (it completes
        // when the renders do), this block is registered below, and the call still reports the deadline (2, unchanged).
        late = 2;
        rc = paced_reduce(b, false);
      }
      if (rc) return rc;
    }
    b->paced.active = true; b->paced.slot = slot; b->paced.rows = rows; b->paced.frames = frames; b->paced.used = used; b->paced.bus = bus_dev; b->paced.accumulate = accumulate;
    b->reduce_recorded[slot] = false; // (recorded when the reduction is launched)
    ctx->paced_order.push_back(b);
    GHIP(ctx, hipGetLastError());
    return late;
  }
  launch_reduce(ctx, b->d_pipe_part[slot], rows, frames, b->d_pipe_seg[slot], bus_dev, accumulate);
  GHIP(ctx, hipEventRecord(b->ev_reduce_done[slot], ctx->stream));
  b->reduce_recorded[slot] = true;
  GHIP(ctx, hipGetLastError());
  return 0;
}
// groove_bank_render_mix for a project whose banks render side by side, PACED by the host (include/groove_hip.h).
int groove_bank_render_mix_paced(groove_bank* b, uint32_t frames, float* bus_dev, int accumulate) {
  if (!b || !bus_dev) return fail(nullptr, "groove_bank_render_mix_paced: NULL argument");
  groove_ctx* ctx = b->ctx;
  if (frames == 0) return 0;
  if (frames > 4096) return fail(ctx, "groove_bank_render_mix_paced: frames > 4096");
  GHIP(ctx, hipSetDevice(ctx->device));
  if (bus_flush_deferred(ctx) || bus_flush_ap(ctx)) return 1; // (the other deferrals' pending rows come first; paced reductions of other banks stay pending)
  if (flush_events(b, use_tp(b, frames))) return 1;
  return render_mix_pipelined(b, frames, bus_dev, accumulate, true);
}
// How many partial rows a bank's deferred render writes (0: the bank does not take a deferred form and goes through
// groove_bank_render_mix), and for a sampler bank the voices-per-workgroup spread of that form.
static uint32_t deferred_rows_of(groove_bank* b, uint32_t frames, uint32_t* svpw_out = nullptr, Form* form_out = nullptr) {
  groove_ctx* ctx = b->ctx;
  if (svpw_out) *svpw_out = 0;
  if (ctx->pipeline_min_waves <= 1 || frames == 0 || frames > 4096) return 0;
  const Form form = form_of(b, frames);
  if (form_out) *form_out = form;
  if (form != Form::TimeParallel) { // the all-kinds / role-split kernel of a mid-size Welsh bank, its rows summed by the next block's launch
    if (form != Form::WelshSmallUniform) return 0;
    const uint32_t urows = fused_rows(b, form);
    return kind_slices(b).n_spec && urows <= 2048 ? urows : 0;
  }
  uint32_t svpw = 0; // sampler: spread over more workgroups than the form with a reduction launch would (welsh_tp.h)
  if (b->kind == BANK_SAMPLER) { svpw = sampler_tp_vpw_deferred(b->n); if (sampler_tp_workgroups(b->n, svpw) > 512) svpw = 0; }
  // (up to 2,048 rows: the 512 columns' workgroups then take two to four batches of rows, a few us of a render that is long by then)
  const uint32_t rows = svpw ? sampler_tp_workgroups(b->n, svpw) : fused_rows(b, form);
  if (rows == 0 || rows > 2048 || frames > kTpMaxFrames) return 0;
  if (svpw_out) *svpw_out = svpw;
  return rows;
}
// The two row buffers of the deferred renders, BOTH sized at once and for the LARGEST need among the ctx's banks: growing one of
// them later would have to flush the pending block through the reduction kernels — whose order of additions differs from the
// carried reduction's — and a project's first run would then round one block differently from every later run (seen by
// tools/soak.py: 1 CRC in 138,107 repeats of config #4; with banks of different row counts taking turns — config #5's per-GPU
// share — the later banks of the first block would still have grown the buffers had they been sized for the first caller only).
static int ensure_dpart(groove_ctx* ctx, size_t need, uint32_t frames) {
  if (ctx->dpart_cap[0] >= need && ctx->dpart_cap[1] >= need) return 0;
  for (groove_bank* o : ctx->banks) need = std::max(need, (size_t)deferred_rows_of(o, frames) * 2 * frames);
  if (bus_flush(ctx)) return 1;                      // (the pending rows may live in a buffer that is about to go)
  GHIP(ctx, wait_deadline(ctx, ctx->stream, nullptr, "deferred partial rows"));
  for (int slot = 0; slot < 2; ++slot) {
    if (ctx->dpart_cap[slot] >= need) continue;
    if (ctx->d_dpart[slot]) GHIP(ctx, hipFree(ctx->d_dpart[slot]));
    ctx->d_dpart[slot] = nullptr; ctx->dpart_cap[slot] = 0;
    GHIP(ctx, hipMalloc(&ctx->d_dpart[slot], need * 4));
    ctx->dpart_cap[slot] = need;
  }
  return 0;
}
// Fused render + mix whose bus reduction is left to the bank's NEXT deferred render (welsh_tp.h, tp_reduce_prev) — or to
// whatever waits for the ctx stream, records an event on it or touches a bus (bus_flush).  For banks that render time-parallel
// on the ctx stream with at most 2,048 partial rows; anything else is groove_bank_render_mix.
int groove_bank_render_mix_deferred(groove_bank* b, uint32_t frames, float* bus_dev, int accumulate) {
  if (!b || !bus_dev) return fail(nullptr, "groove_bank_render_mix_deferred: NULL argument");
  groove_ctx* ctx = b->ctx;
  if (frames == 0) return 0;
  // (several banks of a small project may take turns on the ctx stream this way — each render carries the reduction of the one
  // before it, in submission order — instead of side by side on side streams with their cross-queue waits: the caller's choice)
  // A Welsh bank too big for the time-parallel form and too small for the per-kind pipeline (the all-kinds or the role-split
  // kernel on the ctx stream, then two reduction launches in line behind it: ~18 us of a 125,000-voice shard's 130) takes the same
  // deferral, the next block's kernel summing the rows — when the launch that would carry them exists (some workgroup of the four
  // class-specialised kinds) and the rows are few enough (deferred_rows_of).
  uint32_t svpw = 0;
  Form form = Form::TimeParallel;
  const uint32_t rows = deferred_rows_of(b, frames, &svpw, &form);
  if (rows == 0) return groove_bank_render_mix(b, frames, bus_dev, accumulate);
  GHIP(ctx, hipSetDevice(ctx->device));
  if (const int rc = flush_paced(ctx)) return rc;
  if (flush_events(b, form == Form::TimeParallel)) return 1;
  if (ctx_join(ctx)) return 1;
  const size_t need = (size_t)rows * 2 * frames;
  if (ensure_dpart(ctx, need, frames)) return 1;
  const int slot = ctx->dpart_next;
  ctx->dpart_next ^= 1;
  const TpPrev prev = ctx->deferred;
  deferred_taken(ctx);
  b->ctx_touched = true;
  launch_single(b, form, frames, true, 0, ctx->d_dpart[slot], ctx->d_dpart[slot], ctx->stream, nullptr, prev.rows ? &prev : nullptr, nullptr, svpw);
  GHIP(ctx, hipGetLastError());
  ctx->deferred = TpPrev{ctx->d_dpart[slot], bus_dev, rows, frames, accumulate};
  return 0;
}
// groove_bank_render_mix_deferred for SEVERAL small banks of different kinds at once: ONE launch for the whole block (welsh_tp.h
// tp_mixed_kernel: a grid whose workgroups dispatch on their index into the Welsh / FM / sampler time-parallel bodies), one row
// buffer, one carried reduction — Orchestrator::gather_audio's one sum over all instruments (orchestrator.rs:397-410).  Takes
// projects with at most one time-parallel bank of each kind, no stereo, interpolated, looped or enveloped sampler bank, and at most 2,048 rows in all; anything else goes bank by bank
// through groove_bank_render_mix_deferred, in the order given.
int groove_banks_render_mix_deferred(groove_ctx* ctx, groove_bank* const* banks, uint32_t n_banks, uint32_t frames, float* bus_dev, int accumulate) {
  if (!ctx || !bus_dev || (n_banks && !banks)) return fail(ctx, "groove_banks_render_mix_deferred: NULL argument");
  if (frames == 0) return 0;
  if (n_banks == 0) { // nothing patched: silence (orchestrator.rs:1452-1455)
    if (bus_flush(ctx)) return 1;
    if (!accumulate) GHIP(ctx, hipMemsetAsync(bus_dev, 0, (size_t)frames * 8, ctx->stream));
    return 0;
  }
  groove_bank* of_kind[3] = {nullptr, nullptr, nullptr}; // BANK_WELSH, BANK_FM, BANK_SAMPLER
  bool ok = n_banks >= 2 && n_banks <= 3 && ctx->pipeline_min_waves > 1 && frames <= kTpMaxFrames;
  for (uint32_t i = 0; i < n_banks; ++i) {
    groove_bank* b = banks[i];
    if (!b) return fail(ctx, "groove_banks_render_mix_deferred: NULL bank");
    if (b->ctx != ctx) return fail(ctx, "groove_banks_render_mix_deferred: a bank of another ctx");
    const int k = b->kind == BANK_WELSH ? 0 : b->kind == BANK_FM ? 1 : 2;
    if (of_kind[k] || !use_tp(b, frames) || (k == 0 && b->plan.tp_full_coef) || b->pcm_stereo || b->pcm_interp != GROOVE_SAMPLE_NEAREST || b->looped || b->enveloped) ok = false; // (tp_mixed_kernel's sampler body is the mono, nearest, loop-free one without envelopes)
    of_kind[k] = b;
  }
  TpMixedArgs m{};
  uint32_t grid = 0;
  if (ok) {
    // the kinds' workgroup ranges in dispatch order, the most expensive kind first (measured, profiles/r05_mixed_ab.log: Welsh | FM |
    // sampler 0.0408 ms per block for config #5's share, sampler-first orders 0.0414 - 0.0423; 8 sampler voices per wavefront: 2 / 4 /
    // 8 / 16 -> 0.0426 / 0.0413 / 0.0408 / 0.0407, and 16 costs the 4,096-voice project 0.0199 against 0.0183)
    if (groove_bank* b = of_kind[0]) { const uint32_t v = tp_vpw(b); m.welsh = TpMixedBank{b->d_params, b->d_state, b->n, v, grid, welsh_tp_grid(b->n, v)}; grid += m.welsh.n_wg; }
    if (groove_bank* b = of_kind[1]) { const uint32_t v = tp_vpw(b); m.fm = TpMixedBank{b->d_params, b->d_state, b->n, v, grid, welsh_tp_workgroups(b->n, v)}; grid += m.fm.n_wg; }
    if (groove_bank* b = of_kind[2]) {
      m.sampler = TpMixedBank{b->d_params, b->d_state, b->n, kMixedSamplerVpw, grid, mixed_sampler_workgroups(b->n, kMixedSamplerVpw)}; grid += m.sampler.n_wg;
      m.pcm = b->d_pcm;
    }
    if (grid == 0 || grid > 2048) ok = false;
  }
  if (!ok) {
    for (uint32_t i = 0; i < n_banks; ++i)
      if (const int rc = groove_bank_render_mix_deferred(banks[i], frames, bus_dev, accumulate || i > 0)) return rc;
    return 0;
  }
  GHIP(ctx, hipSetDevice(ctx->device));
  if (const int rc = flush_paced(ctx)) return rc;
  for (uint32_t i = 0; i < n_banks; ++i)
    if (flush_events(banks[i], true)) return 1;
  if (ctx_join(ctx)) return 1;
  if (ensure_dpart(ctx, (size_t)grid * 2 * frames, frames)) return 1;
  const int slot = ctx->dpart_next;
  ctx->dpart_next ^= 1;
  m.prev = ctx->deferred;
  deferred_taken(ctx);
  m.rows = ctx->d_dpart[slot]; m.rc = render_consts_of(ctx); m.frames = frames;
  static const InlineEvents no_events{};
  launch_tp_mixed(m, of_kind[2] ? of_kind[2]->inline_ev : no_events, grid, ctx->stream);
  for (uint32_t i = 0; i < n_banks; ++i) banks[i]->ctx_touched = true;
  if (of_kind[2]) of_kind[2]->inline_ev.n = 0;
  GHIP(ctx, hipGetLastError());
  ctx->deferred = TpPrev{ctx->d_dpart[slot], bus_dev, grid, frames, accumulate};
  return 0;
}
int groove_bus_flush(groove_ctx* ctx) {
  if (!ctx) return fail(nullptr, "groove_bus_flush: ctx is NULL");
  GHIP(ctx, hipSetDevice(ctx->device));
  return bus_flush(ctx);
}
int groove_bank_render_mix(groove_bank* b, uint32_t frames, float* bus_dev, int accumulate) {
  if (!b || !bus_dev) return fail(nullptr, "groove_bank_render_mix: NULL argument");
  groove_ctx* ctx = b->ctx;
  if (frames == 0) return 0;
  if (bus_flush(ctx)) return 1;
  if (frames > 4096) return fail(ctx, "groove_bank_render_mix: frames > 4096");
  GHIP(ctx, hipSetDevice(ctx->device));
  if (flush_events(b, use_tp(b, frames))) return 1;
  // Asynchronous form (kernels on side streams, only the bus reductions on the ctx stream):
  //  - a large Welsh bank (>= ~550,000 voices) runs one kernel per base kind and pipelines its own blocks
  //    (+11 % at 1,000,000 voices, +7 % at 600,000); below that the all-kinds kernel wins, run block after block on the
  //    ctx stream (500,000 voices: 0.342 ms against 0.357; 300,000: 0.250 against 0.275; through the block pipeline
  //    it is no faster: 250,000 voices 0.222 against 0.215);
  //  - in a project of several banks (synths, samplers) every bank takes it, so that the banks of one block
  //    run beside each other instead of one after the other (mixed-131072: 0.46 -> 0.2x ms per block).
  const bool force = ctx->pipeline_min_waves <= 1;
  const Form form = form_of(b, frames);
  // (a Welsh bank past the threshold that still renders time-parallel — the knobs can make one — has always walked this way too)
  const bool big = form == Form::WelshBigUniform || (form == Form::TimeParallel && b->kind == BANK_WELSH && b->plan.n_vwaves >= ctx->pipeline_min_waves);
  if (big || force || ctx->banks.size() > 1) return render_mix_pipelined(b, frames, bus_dev, accumulate);
  if (ctx_join(ctx)) return 1; // earlier pipelined blocks of this bank may still be running on the side streams
  const uint32_t rows = fused_rows(b, form);
  const size_t part_floats = (size_t)rows * 2 * frames;
  if (ctx->fpart_cap < part_floats) {
    if (ctx->d_fpart) GHIP(ctx, hipFree(ctx->d_fpart));
    GHIP(ctx, hipMalloc(&ctx->d_fpart, part_floats * 4));
    ctx->fpart_cap = part_floats;
  }
  if (ensure_seg_buffer(ctx, &ctx->d_fseg, &ctx->fseg_cap, reduce_seg_floats(rows, frames))) return 1;
  if (launch_render(b, frames, true, 0, ctx->d_fpart, ctx->d_fpart)) return 1;
  launch_reduce(ctx, ctx->d_fpart, rows, frames, ctx->d_fseg, bus_dev, accumulate);
  GHIP(ctx, hipGetLastError());
  return 0;
}
static const char* kernel_form_text(groove_bank* b, uint32_t frames, int fused);
const char* groove_bank_kernel_form(groove_bank* b, uint32_t frames, int fused) {
  const char* text = kernel_form_text(b, frames, fused);
  if (!b || b->kind != BANK_SAMPLER || !b->enveloped) return text;
  b->form_text = text; // "... (a, b)" -> "... (a, b, enveloped)"
  if (!b->form_text.empty() && b->form_text.back() == ')') b->form_text.pop_back();
  b->form_text += ", enveloped)";
  return b->form_text.c_str();
}
static const char* kernel_form_text(groove_bank* b, uint32_t frames, int fused) {
  if (!b) return "";
  const Form form = form_of(b, frames);
  switch (form) {
    case Form::TimeParallel:
      if (b->kind == BANK_WELSH) return tp_vpw(b) == 2 ? "welsh_tp_kernel (time-parallel, two voices per wavefront)" : "welsh_tp_kernel (time-parallel, one wavefront per voice)";
      if (b->kind == BANK_FM) return tp_vpw(b) == 4 ? "fm_tp_kernel (time-parallel, four voices per wavefront)" : "fm_tp_kernel (time-parallel)";
      if (b->looped)
        return b->pcm_interp == GROOVE_SAMPLE_LINEAR ? "sampler_tp_kernel (time-parallel, linear interpolation, looped)"
             : b->pcm_interp == GROOVE_SAMPLE_CUBIC ? "sampler_tp_kernel (time-parallel, cubic interpolation, looped)" : "sampler_tp_kernel (time-parallel, looped)";
      return b->pcm_interp == GROOVE_SAMPLE_LINEAR ? "sampler_tp_kernel (time-parallel, linear interpolation)"
           : b->pcm_interp == GROOVE_SAMPLE_CUBIC ? "sampler_tp_kernel (time-parallel, cubic interpolation)" : "sampler_tp_kernel (time-parallel)";
    case Form::FmSerial: return "fm_render_kernel (serial, one voice per lane)";
    case Form::SamplerSerial:
      if (b->looped)
        return b->pcm_interp == GROOVE_SAMPLE_LINEAR ? "sampler_render_kernel (serial, one voice per lane, linear interpolation, looped)"
             : b->pcm_interp == GROOVE_SAMPLE_CUBIC ? "sampler_render_kernel (serial, one voice per lane, cubic interpolation, looped)" : "sampler_render_kernel (serial, one voice per lane, looped)";
      return b->pcm_interp == GROOVE_SAMPLE_LINEAR ? "sampler_render_kernel (serial, one voice per lane, linear interpolation)"
           : b->pcm_interp == GROOVE_SAMPLE_CUBIC ? "sampler_render_kernel (serial, one voice per lane, cubic interpolation)" : "sampler_render_kernel (serial, one voice per lane)";
    case Form::WelshPerLane: return "welsh_render_kernel (per-lane parameters)";
    case Form::WelshBigUniform: // fused: groove_bank_render_mix takes render_mix_pipelined; otherwise groove_bank_render's walk (launch_render)
      return fused ? "welsh_render_uniform_mix_kernel (big-bank form: three launches per block over thirds of the kind-sorted workgroups, one launch per base kind for the exact-f64 kinds only; class-specialised bodies, blocks pipelined)"
                   : "welsh_render_uniform_kernel (one launch per base kind, class-specialised bodies)";
    case Form::WelshSmallUniform: break;
  }
  if (use_split(b, form, frames)) return "welsh_render_split4_kernel (role-split: four wavefronts per 64 voices, pipelined over the frames)";
  return "welsh_render_uniform_any_kernel (all base kinds in one launch, class-specialised bodies)";
}
int groove_bank_reset(groove_bank* b) {
  if (!b) return fail(nullptr, "groove_bank_reset: bank is NULL");
  groove_ctx* ctx = b->ctx;
  GHIP(ctx, hipSetDevice(ctx->device));
  if (ctx_join(ctx)) return 1;
  b->side_mode = 0;
  b->ctx_touched = true;
  b->pending.clear();
  b->inline_ev.n = 0;
  StateWords w{};
  if (b->kind == BANK_WELSH) { const WelshState s = initial_welsh_state(); std::memcpy(w.w, &s, sizeof(s)); }
  else if (b->kind == BANK_FM) { const FmState s = initial_fm_state(); std::memcpy(w.w, &s, sizeof(s)); }
  else { const SamplerState s{0, 0, 0, 0}; std::memcpy(w.w, &s, sizeof(s)); }
  hipLaunchKernelGGL(state_fill_kernel, dim3(blocks_for(b->n)), dim3(kThreads), 0, ctx->stream, b->d_state, b->n, b->sw, w);
  GHIP(ctx, hipGetLastError());
  if (b->kind == BANK_SAMPLER && b->enveloped) { // the envelopes stay, every record idle
    GHIP(ctx, ctx_wait(ctx));
    if (sampler_upload_envelopes(b)) return 1;
  }
  // An FM bank with links: its shadow goes back to the host's copy, and the records with it — gl, gr and depth_beta each come from TWO
  // shadow words, so a shadow refreshed alone would pair the host's gain with a pan that the records no longer hold.
  if (b->kind == BANK_FM && b->d_dca) return fm_upload_params(b);
  return 0;
}
uint32_t groove_bank_state_words(groove_bank* b) { return b ? b->sw : 0; }
int groove_bank_download_state(groove_bank* b, uint32_t* host_words) {
  if (!b || !host_words) return fail(nullptr, "groove_bank_download_state: NULL argument");
  groove_ctx* ctx = b->ctx;
  if (flush_events(b)) return 1;
  if (ctx_join(ctx)) return 1;
  GHIP(ctx, ctx_wait(ctx));
  if (b->plan.perm.empty()) {
    GHIP(ctx, ctx_memcpy(ctx, host_words, b->d_state, (size_t)b->sw * b->n * 4, hipMemcpyDeviceToHost));
  } else { // internal lane order -> caller's voice order
    std::vector<uint32_t> tmp((size_t)b->sw * b->n);
    GHIP(ctx, ctx_memcpy(ctx, tmp.data(), b->d_state, tmp.size() * 4, hipMemcpyDeviceToHost));
    for (uint32_t w = 0; w < b->sw; ++w)
      for (uint32_t i = 0; i < b->n; ++i) host_words[(size_t)w * b->n + b->plan.perm[i]] = tmp[(size_t)w * b->n + i];
  }
  return 0;
}

// ============================================================================ effects
int groove_fx_create(groove_ctx* ctx, uint32_t kind, const groove_fx_params* p, uint32_t n, groove_fx** out) {
  if (!ctx || !p || !out) return fail(ctx, "groove_fx_create: NULL argument");
  if (n == 0) return fail(ctx, "groove_fx_create: n == 0");
  if (kind >= GROOVE_FX_KIND_COUNT) return fail(ctx, "groove_fx_create: unknown effect kind");
  GHIP(ctx, hipSetDevice(ctx->device));
  groove_fx* fx = new groove_fx();
  fx->ctx = ctx; fx->kind = kind; fx->n = n;
  fx->p.assign(p, p + n);
  if (fx_check_uniform(fx)) { delete fx; return 1; }
  if (hipMalloc(&fx->d_fa, n * 4) != hipSuccess || hipMalloc(&fx->d_fb, n * 4) != hipSuccess ||
      hipMalloc(&fx->d_ua, n * 4) != hipSuccess || hipMalloc(&fx->d_wet, n * 4) != hipSuccess ||
      hipMalloc(&fx->d_coef, (size_t)6 * n * 8) != hipSuccess) {
    groove_fx_destroy(fx);
    return fail(ctx, "groove_fx_create: hipMalloc failed");
  }
  if (fx_setup_state(fx) || fx_upload_params(fx)) { groove_fx_destroy(fx); return 1; }
  ctx->fxs.push_back(fx);
  *out = fx;
  return 0;
}
// A reverb whose all-passes went to the all-pass stream last: the ctx stream waits for them before it touches the lines itself.
static int fx_ap_settle(groove_fx* fx) {
  if (!fx->ap_busy) return 0;
  fx->ap_busy = false;
  return ap_join(fx->ctx);
}
int groove_fx_destroy(groove_fx* fx) {
  if (!fx) return 0;
  groove_ctx* ctx = fx->ctx;
  (void)fx_acquire_ctx(fx);
  (void)fx_ap_settle(fx);
  (void)hipStreamSynchronize(ctx->stream);
  if (fx->ev_done) (void)hipEventDestroy(fx->ev_done);
  auto it = std::find(ctx->fxs.begin(), ctx->fxs.end(), fx);
  if (it != ctx->fxs.end()) ctx->fxs.erase(it);
  for (groove_ctl_link* l : ctx->links) // a link onto this effect has no target any more: its next apply is an error, not a write
    if (l->target == fx) l->target = nullptr;
  (void)hipFree(fx->d_fa); (void)hipFree(fx->d_fb); (void)hipFree(fx->d_ua); (void)hipFree(fx->d_wet);
  (void)hipFree(fx->d_coef); (void)hipFree(fx->d_shadow); (void)hipFree(fx->d_st); (void)hipFree(fx->d_ring); (void)hipFree(fx->d_tmp);
  delete fx;
  return 0;
}
int groove_fx_reset(groove_fx* fx) {
  if (!fx) return fail(nullptr, "groove_fx_reset: fx is NULL");
  groove_ctx* ctx = fx->ctx;
  GHIP(ctx, hipSetDevice(ctx->device));
  if (fx_acquire_ctx(fx) || fx_ap_settle(fx)) return 1;
  const size_t ln = 2 * (size_t)fx->n;
  if (fx->d_st) GHIP(ctx, hipMemsetAsync(fx->d_st, 0, 4 * ln * 8, ctx->stream));
  if (fx->d_ring) GHIP(ctx, hipMemsetAsync(fx->d_ring, 0, fx->ring_rows * ln * 4, ctx->stream));
  fx->w = 0;
  for (uint32_t& w : fx->geo.w) w = 0;
  return 0;
}
// ---- effect stages ---------------------------------------------------------------------
// THE effect form decision: groove_fx_chain_process (which stages join a fused run), fx_launch_run (what follows a reverb's
// combs), fx_launch_serial (which kernel walks the frames) and groove_fx_kernel_form all ask here.  kFxFormNames holds one
// string per form, in the enum's order: the only list of them (groove_fx_kernel_form_name hands it out).
enum class FxForm : uint32_t {
  Identity, RunStage,
  RunDirectAp, RunDirect, RunChunked, RunSeq,
  BiquadTp, BiquadSeg, BiquadSerial, Lp24Tp, Lp24Serial,
  Delay16, Delay1, Chorus16, Chorus1, Reverb8, Reverb1,
  Count
};
static const char* const kFxFormNames[(size_t)FxForm::Count] = {
  "identity (Mixer: no launch)",
  "fx_run_kernel (a stage of the fused run)",
  "fx_run_kernel + fx_reverb_allpass_direct_kernel (combs in the fused run, direct all-pass on the all-pass stream)",
  "fx_run_kernel + fx_reverb_allpass_direct_kernel (combs in the fused run, direct all-pass behind it)",
  "fx_run_kernel + fx_reverb_allpass_chunked_kernel (combs in the fused run, chunked all-pass)",
  "fx_run_kernel + fx_reverb_allpass_kernel<32> (combs in the fused run, sequential all-pass)",
  "fx_biquad_tp_kernel (IIR time-parallel)",
  "fx_biquad_seg_kernel (IIR four-segment)",
  "fx_biquad_kernel<16> (IIR serial)",
  "fx_lp24_tp_kernel (IIR time-parallel)",
  "fx_lp24_kernel<16> (IIR serial)",
  "fx_delay_kernel<16> (delay serial, chunk 16)",
  "fx_delay_kernel<1> (delay serial, chunk 1)",
  "fx_chorus_kernel<16> (chorus serial, chunk 16)",
  "fx_chorus_kernel<1> (chorus serial, chunk 1)",
  "fx_reverb_kernel<8> (reverb serial, chunk 8)",
  "fx_reverb_kernel<1> (reverb serial, chunk 1)",
};
// `last_on_ctx`: the launch is the last of its chain and goes to the ctx stream (only such a launch may leave for the all-pass
// stream).  The element-wise kinds are always stages of a fused run (kernels.h, fx_run_kernel); a delay line is one when it is
// at least a block long (no feedback inside the block).
// A reverb whose output needs its input again: a lane of the host's copy is below wet 1, or a wet link is alive (the device's values
// are then the link's, whatever the host's copy says).  Such a reverb walks the frames serially (fx_reverb_kernel) unless
// groove_set_fx_wet_reverb_run is on; then it takes the run's forms with the DRY instantiations of their kernels (kernels.h).
static bool fx_needs_dry(const groove_fx* fx) { return !fx->all_wet || fx->wet_links > 0; }
static FxForm fx_form_of(const groove_fx* fx, const groove_block* io, uint32_t frames, bool last_on_ctx) {
  const groove_ctx* ctx = fx->ctx;
  const size_t n = fx->n;
  switch (fx->kind) {
    case GROOVE_FX_MIXER: return FxForm::Identity;
    case GROOVE_FX_GAIN: case GROOVE_FX_BITCRUSHER: case GROOVE_FX_LIMITER: case GROOVE_FX_COMPRESSOR: return FxForm::RunStage;
    case GROOVE_FX_BIQUAD_LP12: case GROOVE_FX_BIQUAD_HP12: case GROOVE_FX_BIQUAD_BP12: case GROOVE_FX_BIQUAD_BS12:
    case GROOVE_FX_BIQUAD_AP12: case GROOVE_FX_BIQUAD_PEAK12: case GROOVE_FX_BIQUAD_LSHELF12: case GROOVE_FX_BIQUAD_HSHELF12:
      // few lane-channels: one wavefront each, frames over its lanes (fx_tp.h); many: one thread each, frames serial
      if (frames <= kTpMaxFrames && 2 * n <= ctx->fx_tp_max_lanes && ctx->tp_max_voices) return FxForm::BiquadTp;
      if (frames <= (uint32_t)(kBqSegs * kBqSegMax) && frames >= 16 && 2 * n <= ctx->fx_seg_max_lanes) return FxForm::BiquadSeg; // four time segments per lane-channel
      return FxForm::BiquadSerial;
    case GROOVE_FX_BIQUAD_LP24:
      if (frames <= kTpMaxFrames && 4 * n <= ctx->fx_tp_max_lanes && ctx->tp_max_voices) return FxForm::Lp24Tp;
      return FxForm::Lp24Serial;
    case GROOVE_FX_DELAY:
      if (fx->N >= frames) return FxForm::RunStage;
      return fx->N >= 16 ? FxForm::Delay16 : FxForm::Delay1; // chunked loads need every read of a chunk to precede its writes: N >= chunk
    case GROOVE_FX_CHORUS: {
      const uint32_t nearest = fx->N - (fx->voices - 1) * fx->spacing; // newest tap: pushed this many frames ago
      if (nearest >= frames && (fx->voices == 1 || fx->spacing >= frames)) return FxForm::RunStage;
      return nearest >= 16 && (fx->voices == 1 || fx->spacing >= 16) ? FxForm::Chorus16 : FxForm::Chorus1;
    }
    case GROOVE_FX_REVERB: { // combs in the run, the two all-passes behind it
      uint32_t shortest_comb = fx->geo.N[0];
      for (int i = 1; i < 4; ++i) shortest_comb = std::min(shortest_comb, fx->geo.N[i]);
      const uint32_t shortest_ap = std::min(fx->geo.N[4], fx->geo.N[5]);
      if (!((!fx_needs_dry(fx) || ctx->fx_wet_reverb_run) && shortest_comb >= frames && shortest_ap >= 32)) return std::min(shortest_comb, shortest_ap) >= 8 ? FxForm::Reverb8 : FxForm::Reverb1;
      // the direct all-pass form unrolls at most 8 hops per frame, and wants the comb sum in a staging block of the block's capacity
      const bool direct = !ctx->seq_allpass && !ctx->chunked_allpass && frames <= 8 * shortest_ap && (size_t)2 * io->cap * n * 4 <= ((size_t)1 << 30);
      // (the other forms keep the dry signal in a staging block of the same size)
      if (!direct && fx_needs_dry(fx) && (size_t)2 * io->cap * n * 4 > ((size_t)1 << 30)) return std::min(shortest_comb, shortest_ap) >= 8 ? FxForm::Reverb8 : FxForm::Reverb1;
      if (direct) return last_on_ctx && ctx->fx_ap_stream >= 0 && io->ev_free ? FxForm::RunDirectAp : FxForm::RunDirect;
      return ctx->seq_allpass ? FxForm::RunSeq : FxForm::RunChunked;
    }
    default: return FxForm::Count; // (groove_fx_create refuses unknown kinds)
  }
}
static bool fx_form_is_run(FxForm f) { return f >= FxForm::RunStage && f <= FxForm::RunSeq; }
static bool fx_is_iir(uint32_t kind) {
  switch (kind) {
    case GROOVE_FX_BIQUAD_LP12: case GROOVE_FX_BIQUAD_HP12: case GROOVE_FX_BIQUAD_BP12: case GROOVE_FX_BIQUAD_BS12:
    case GROOVE_FX_BIQUAD_AP12: case GROOVE_FX_BIQUAD_PEAK12: case GROOVE_FX_BIQUAD_LSHELF12: case GROOVE_FX_BIQUAD_HSHELF12:
    case GROOVE_FX_BIQUAD_LP24: return true;
    default: return false;
  }
}
static void fx_advance(groove_fx* fx, uint32_t frames) { // the delay lines' write positions after a block
  if (fx->kind == GROOVE_FX_DELAY || fx->kind == GROOVE_FX_CHORUS) fx->w = (uint32_t)(((uint64_t)fx->w + frames) % fx->N);
  if (fx->kind == GROOVE_FX_REVERB)
    for (int i = 0; i < 6; ++i) fx->geo.w[i] = (uint32_t)(((uint64_t)fx->geo.w[i] + frames) % fx->geo.N[i]);
}
// One launch for `count` (<= kRunMaxStages) run-capable stages in chain order; a reverb, if there is one, is the last,
// and its all-passes follow.
static int fx_launch_run(groove_ctx* ctx, groove_fx* const* run, uint32_t count, groove_block* io, uint32_t frames, hipStream_t st, bool last) {
  const uint32_t n = io->n;
  const size_t chs = (size_t)io->cap * n;
  FxRunArgs a{};
  for (uint32_t s = 0; s < count; ++s) {
    const groove_fx* fx = run[s];
    a.st[s] = FxRunStage{fx->kind, fx->N, fx->w, fx->voices, fx->spacing, 0, fx->d_ring, fx->d_fa, fx->d_fb, fx->d_ua, fx->d_wet};
  }
  a.n_stages = count; a.n = n;
  a.src = io->d; a.src_chs = chs;
  a.dst = io->d; a.dst_chs = chs;
  groove_fx* rv = run[count - 1]->kind == GROOVE_FX_REVERB ? run[count - 1] : nullptr;
  bool direct = false, on_ap = false, seq = false, dry = false;
  auto tmp_block = [&]() -> int { // the reverb's staging block, of the block's capacity
    if (rv->tmp_cap >= io->cap) return 0;
    GHIP(ctx, wait_deadline(ctx, st, nullptr, "effect staging block"));
    if (rv->d_tmp) { GHIP(ctx, hipFree(rv->d_tmp)); rv->d_tmp = nullptr; rv->tmp_cap = 0; }
    GHIP(ctx, hipMalloc(&rv->d_tmp, (size_t)2 * io->cap * n * 4));
    rv->tmp_cap = io->cap;
    return 0;
  };
  if (rv) {
    a.geo = rv->geo;
    // the direct all-pass form wants the comb sum in a staging block (it reads other frames than the one it writes)
    // The all-pass stream: the chain's LAST launch (nothing on the ctx stream reads the block behind it; its lane sums go to the
    // bus through groove_mix / groove_mix_deferred) leaves the ctx stream, so the next block's run follows this one directly.
    const FxForm form = fx_form_of(rv, io, frames, last && st == ctx->stream);
    on_ap = form == FxForm::RunDirectAp;
    direct = on_ap || form == FxForm::RunDirect;
    seq = form == FxForm::RunSeq;
    if (!on_ap && rv->ap_busy) { if (ap_join(ctx)) return 1; rv->ap_busy = false; }
    if (direct && on_ap) {
      if (io->stage_cap < io->cap) { // (first use of the block on this path: nothing of the block's is in flight on that stream yet)
        if (io->d_stage) { if (ap_join(ctx)) return 1; GHIP(ctx, wait_deadline(ctx, st, nullptr, "effect staging block")); GHIP(ctx, hipFree(io->d_stage)); io->d_stage = nullptr; io->stage_cap = 0; }
        GHIP(ctx, hipMalloc(&io->d_stage, (size_t)2 * io->cap * n * 4));
        io->stage_cap = io->cap;
      }
      a.dst = io->d_stage; a.dst_chs = (size_t)io->stage_cap * n;
    } else if (direct) {
      if (tmp_block()) return 1;
      a.dst = rv->d_tmp; a.dst_chs = (size_t)rv->tmp_cap * n;
    }
    // the reverb's input, for the wet-dry mix behind the all-passes (kernels.h, fx_wet_mix): in the block itself under the direct
    // forms, in the reverb's staging block otherwise (the comb sum is in the block then)
    dry = fx_needs_dry(rv);
    if (dry && direct) { a.dry = io->d; a.dry_chs = chs; }
    else if (dry) {
      if (tmp_block()) return 1;
      a.dry = rv->d_tmp; a.dry_chs = (size_t)rv->tmp_cap * n;
    }
  }
  const dim3 blk(kThreads);
  const uint32_t V = n % 4 == 0 ? 4 : 1, wg_per_ch = fx_wg_per_ch(n, V);
  // the chain's last launch leaves the block's lane sums for groove_mix (kernels.h, fx_row_sum)
  float* rows = nullptr;
  if (on_ap) { // one of the block's two buffers that only that stream's kernels write
    const int f = io->ap_flip;
    const size_t need = (size_t)wg_per_ch * 2 * frames;
    if (io->sums_ap_cap[f] < need) {
      if (io->d_sums_ap[f]) { if (bus_flush_ap(ctx) || ap_join(ctx)) return 1; GHIP(ctx, wait_deadline(ctx, st, nullptr, "block row sums")); GHIP(ctx, hipFree(io->d_sums_ap[f])); io->d_sums_ap[f] = nullptr; io->sums_ap_cap[f] = 0; }
      const size_t cap = std::max(need, (size_t)wg_per_ch * 2 * std::min<uint32_t>(io->cap, 4096));
      GHIP(ctx, hipMalloc(&io->d_sums_ap[f], cap * 4));
      io->sums_ap_cap[f] = cap;
    }
    io->sums_valid = false;
    rows = io->d_sums_ap[f];
  } else if (last) {
    rows = block_sums(io, wg_per_ch, frames);
    if (!rows) return 1;
  }
  a.frames = frames; a.wg_per_ch = wg_per_ch;
  if (ctx->deferred.rows && st == ctx->stream) { // groove_mix_deferred: this launch sums the pending block's rows onto its bus
    a.prev = ctx->deferred;
    deferred_taken(ctx);
  }
  a.rows = (rv && direct) ? nullptr : rows;
  if (rv && !direct) rows = nullptr; // the sequential / chunked all-pass kernels run last and leave none
  const dim3 run_grid(2 * wg_per_ch, frames);
  if (dry) { // (the all-wet launches keep the instantiations without the dry store)
    if (V == 4) hipLaunchKernelGGL((fx_run_kernel<4, true>), run_grid, blk, 0, st, a);
    else hipLaunchKernelGGL((fx_run_kernel<1, true>), run_grid, blk, 0, st, a);
  } else if (V == 4) hipLaunchKernelGGL((fx_run_kernel<4, false>), run_grid, blk, 0, st, a);
  else hipLaunchKernelGGL((fx_run_kernel<1, false>), run_grid, blk, 0, st, a);
  if (rv) {
    const ReverbGeom& g = rv->geo;
    if (direct) {
      AllpassDirectArgs d{};
      d.src = a.dst; d.src_chs = a.dst_chs;
      d.dst = io->d; d.dst_chs = chs;
      d.ring = rv->d_ring;
      for (int i = 0; i < 2; ++i) {
        d.old_base[i] = g.base[4 + i]; d.new_base[i] = rv->ap_alt[i];
        d.N[i] = g.N[4 + i]; d.w[i] = g.w[4 + i]; d.g[i] = g.g[4 + i];
      }
      d.n = n; d.frames = frames;
      d.rows = rows; d.wg_per_ch = wg_per_ch;
      d.wet = rv->d_wet;
      const dim3 ap_grid(2 * wg_per_ch, std::max(frames, std::max(g.N[4], g.N[5])));
      auto launch_direct = [&](hipStream_t on) {
        if (dry) {
          if (V == 4) hipLaunchKernelGGL((fx_reverb_allpass_direct_kernel<4, true>), ap_grid, blk, 0, on, d);
          else hipLaunchKernelGGL((fx_reverb_allpass_direct_kernel<1, true>), ap_grid, blk, 0, on, d);
        } else if (V == 4) hipLaunchKernelGGL((fx_reverb_allpass_direct_kernel<4, false>), ap_grid, blk, 0, on, d);
        else hipLaunchKernelGGL((fx_reverb_allpass_direct_kernel<1, false>), ap_grid, blk, 0, on, d);
      };
      hipStream_t ast = st;
      if (on_ap) {
        const int k = ctx->fx_ap_stream;
        ast = ap_stream(ctx);
        if (ap_events(ctx)) return 1;
        GHIP(ctx, hipEventRecord(ctx->ev_ap_run, st));
        GHIP(ctx, hipStreamWaitEvent(ast, ctx->ev_ap_run, 0));
        if (ctx->deferred_ap.rows) { // the previous block's lane sums: written by that stream's last kernel, summed by this one
          d.prev = ctx->deferred_ap;
          ctx->deferred_ap = TpPrev{};
        }
        launch_direct(ast);
        GHIP(ctx, hipEventRecord(io->ev_ready[k], ast)); // the block is ready when that kernel is
        io->ready_mask |= 1u << k;
        ctx->side_busy[k] = true;
        rv->ap_busy = true;
      } else {
        launch_direct(ast);
      }
      for (int i = 0; i < 2; ++i) std::swap(rv->geo.base[4 + i], rv->ap_alt[i]);
    } else if (seq) {
      if (dry) hipLaunchKernelGGL((fx_reverb_allpass_kernel<32, true>), dim3(blocks_for(2 * (size_t)n)), blk, 0, st, io->d, n, frames, chs, rv->d_ring, g, a.dry, a.dry_chs, rv->d_wet);
      else hipLaunchKernelGGL((fx_reverb_allpass_kernel<32, false>), dim3(blocks_for(2 * (size_t)n)), blk, 0, st, io->d, n, frames, chs, rv->d_ring, g, (const float*)nullptr, (size_t)0, (const float*)nullptr);
    } else { // chunks of one line length, parallel inside (kernels.h)
      const uint32_t T = std::max<uint32_t>(1, std::min<uint32_t>(64, 2 * n / 512));
      if (dry) hipLaunchKernelGGL(fx_reverb_allpass_chunked_kernel<true>, dim3((2 * n + T - 1) / T), dim3(kAllpassThreads), 0, st, io->d, n, frames, chs, rv->d_ring, g, T, a.dry, a.dry_chs, rv->d_wet);
      else hipLaunchKernelGGL(fx_reverb_allpass_chunked_kernel<false>, dim3((2 * n + T - 1) / T), dim3(kAllpassThreads), 0, st, io->d, n, frames, chs, rv->d_ring, g, T, (const float*)nullptr, (size_t)0, (const float*)nullptr);
    }
  }
  for (uint32_t s = 0; s < count; ++s) fx_advance(run[s], frames);
  GHIP(ctx, hipGetLastError());
  if (rows) { io->sum_rows = wg_per_ch; io->sum_frames = frames; io->sums_valid = true; io->sums_on_ap = on_ap; }
  return 0;
}
// The kinds with feedback inside a block: the IIR filters, and delay lines shorter than the block.
static int fx_launch_serial(groove_fx* fx, FxForm form, groove_block* io, uint32_t frames, hipStream_t st) {
  groove_ctx* ctx = fx->ctx;
  const uint32_t n = fx->n;
  const size_t chs = (size_t)io->cap * n;
  const dim3 blk(kThreads), lanes_grid(blocks_for(2 * (size_t)n));
  // (64-frame chunks instead of 16 were measured for the serial IIR kernels: no change at any bank size — the walk is
  // bound by its dependent f64 chain, not by the chunk loads.)
  switch (form) {
    case FxForm::BiquadTp:
      hipLaunchKernelGGL(fx_biquad_tp_kernel, dim3((n + kFxTile - 1) / kFxTile, 2), dim3(kFxTpThreads), 0, st, io->d, n, frames, chs, fx->d_coef, fx->d_st, fx->d_wet);
      break;
    case FxForm::BiquadSeg:
      hipLaunchKernelGGL(fx_biquad_seg_kernel, dim3((2 * n + 63) / 64), blk, 0, st, io->d, n, frames, chs, fx->d_coef, fx->d_st, fx->d_wet);
      break;
    case FxForm::BiquadSerial:
      hipLaunchKernelGGL(fx_biquad_kernel<16>, lanes_grid, blk, 0, st, io->d, n, frames, chs, fx->d_coef, fx->d_st, fx->d_wet);
      break;
    case FxForm::Lp24Tp:
      hipLaunchKernelGGL(fx_lp24_tp_kernel, dim3((n + kFxTile - 1) / kFxTile, 2), dim3(kFxTpThreads), 0, st, io->d, n, frames, chs, fx->d_coef, fx->d_st, fx->d_wet);
      break;
    case FxForm::Lp24Serial:
      hipLaunchKernelGGL(fx_lp24_kernel<16>, lanes_grid, blk, 0, st, io->d, n, frames, chs, fx->d_coef, fx->d_st, fx->d_wet);
      break;
    case FxForm::Delay16:
      hipLaunchKernelGGL(fx_delay_kernel<16>, lanes_grid, blk, 0, st, io->d, n, frames, chs, fx->d_ring, fx->N, fx->w, fx->d_wet);
      break;
    case FxForm::Delay1:
      hipLaunchKernelGGL(fx_delay_kernel<1>, lanes_grid, blk, 0, st, io->d, n, frames, chs, fx->d_ring, fx->N, fx->w, fx->d_wet);
      break;
    case FxForm::Chorus16:
      hipLaunchKernelGGL(fx_chorus_kernel<16>, lanes_grid, blk, 0, st, io->d, n, frames, chs, fx->d_ring, fx->N, fx->w, fx->voices, fx->spacing, fx->d_wet);
      break;
    case FxForm::Chorus1:
      hipLaunchKernelGGL(fx_chorus_kernel<1>, lanes_grid, blk, 0, st, io->d, n, frames, chs, fx->d_ring, fx->N, fx->w, fx->voices, fx->spacing, fx->d_wet);
      break;
    case FxForm::Reverb8:
    case FxForm::Reverb1:
      if (fx_ap_settle(fx)) return 1;
      if (form == FxForm::Reverb8) hipLaunchKernelGGL(fx_reverb_kernel<8>, lanes_grid, blk, 0, st, io->d, n, frames, chs, fx->d_ring, fx->geo, fx->d_fa, fx->d_wet);
      else hipLaunchKernelGGL(fx_reverb_kernel<1>, lanes_grid, blk, 0, st, io->d, n, frames, chs, fx->d_ring, fx->geo, fx->d_fa, fx->d_wet);
      break;
    default: return fail(ctx, "groove_fx_process: unknown kind");
  }
  fx_advance(fx, frames);
  GHIP(ctx, hipGetLastError());
  return 0;
}
static int fx_chain_check(groove_fx* const* chain, uint32_t n_fx, groove_block* io, uint32_t frames, const char* who) {
  if (!io || (n_fx && !chain)) return fail(nullptr, std::string(who) + ": NULL argument");
  groove_ctx* ctx = io->ctx;
  for (uint32_t i = 0; i < n_fx; ++i) {
    if (!chain[i]) return fail(ctx, std::string(who) + ": NULL effect");
    if (chain[i]->ctx != ctx) return fail(ctx, std::string(who) + ": effect and block belong to different contexts");
    if (chain[i]->n != io->n) return fail(ctx, std::string(who) + ": block lanes != effect lanes");
    for (uint32_t j = 0; j < i; ++j)
      if (chain[j] == chain[i]) return fail(ctx, std::string(who) + ": the same effect twice in one chain");
  }
  if (frames > io->cap) return fail(ctx, std::string(who) + ": frames > block capacity");
  return 0;
}
int groove_fx_chain_process(groove_fx* const* chain, uint32_t n_fx, groove_block* io, uint32_t frames) {
  if (fx_chain_check(chain, n_fx, io, frames, "groove_fx_chain_process")) return 1;
  groove_ctx* ctx = io->ctx;
  if (frames == 0 || n_fx == 0) return 0;
  GHIP(ctx, hipSetDevice(ctx->device));
  if (block_acquire(io) || block_normalise(io)) return 1; // effects carry per-lane parameters in the caller's order
  uint32_t last_stage = n_fx; // the last stage that launches anything (the Mixer is the identity)
  for (uint32_t i = 0; i < n_fx; ++i) if (chain[i]->kind != GROOVE_FX_MIXER) last_stage = i;
  groove_fx* run[kRunMaxStages];
  uint32_t count = 0;
  auto flush = [&](bool last) -> int {
    if (!count) return 0;
    const int rc = fx_launch_run(ctx, run, count, io, frames, ctx->stream, last);
    count = 0;
    return rc;
  };
  for (uint32_t i = 0; i < n_fx; ++i) {
    groove_fx* fx = chain[i];
    if (fx->kind == GROOVE_FX_MIXER) continue; // identity
    if (fx_acquire_ctx(fx)) return 1;
    io->sums_valid = false; // the block is transformed in place
    const FxForm form = fx_form_of(fx, io, frames, i == last_stage);
    if (fx_form_is_run(form)) {
      run[count++] = fx;
      if (count == kRunMaxStages || fx->kind == GROOVE_FX_REVERB) { if (flush(i == last_stage)) return 1; }
    } else {
      if (flush(false)) return 1;
      if (fx_launch_serial(fx, form, io, frames, ctx->stream)) return 1;
    }
  }
  return flush(true);
}
// The LEADING stages of a chain that walk the block's frames one lane-channel per thread (the IIR filters, delay lines
// shorter than the block) on the side stream that carries `io`'s pending asynchronous render, right behind it: these
// are latency-bound kernels of a few hundred wavefronts, and behind the render of block b+1 they run beside the wide,
// HBM-bound stages of block b on the ctx stream instead of in front of them (config #3: the BiQuad took 29 us of the
// ctx stream's 82 us per block).  *n_done = how many stages were taken; the caller passes the rest of the chain to
// groove_fx_chain_process when it gets to the block.  Nothing is taken (and 0 returned) when the block has no pending
// render on exactly one side stream, or when the chain does not start with such a stage.
int groove_fx_chain_process_async(groove_fx* const* chain, uint32_t n_fx, groove_block* io, uint32_t frames, uint32_t* n_done) {
  if (!n_done) return fail(nullptr, "groove_fx_chain_process_async: n_done is NULL");
  *n_done = 0;
  if (fx_chain_check(chain, n_fx, io, frames, "groove_fx_chain_process_async")) return 1;
  groove_ctx* ctx = io->ctx;
  if (frames == 0 || n_fx == 0) return 0;
  int k = -1;
  for (int j = 0; j < kSideStreams; ++j)
    if (io->ready_mask & (1u << j)) k = (k == -1) ? j : -2;
  if (k < 0) return 0; // no pending render, or one spread over several kind streams
  if (io->order) return 0; // the block is in the library's lane order: the ctx stream produces the caller's first
  GHIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = side_stream_of(ctx, k);
  uint32_t done = 0;
  for (uint32_t i = 0; i < n_fx; ++i) {
    groove_fx* fx = chain[i];
    if (fx->kind == GROOVE_FX_MIXER) { ++done; continue; }
    // Only the IIR filters: they walk the frames serially whatever the block length, so an effect is EITHER always ahead
    // of the ctx stream's walk OR never.  (A delay line is a serial kernel for blocks longer than the line and a stage of the
    // fused run otherwise: taken here for some blocks and left to the ctx stream for others, its blocks would be
    // submitted out of order — found by the ragged-block test.)
    if (!fx_is_iir(fx->kind)) break;
    if (fx->last_side != k) { // the stream that used the effect last: the ctx stream (or another side stream)
      if (!fx->ev_done) GHIP(ctx, hipEventCreateWithFlags(&fx->ev_done, kSyncEventFlags));
      if (fx->last_side < 0) GHIP(ctx, hipEventRecord(fx->ev_done, ctx->stream));
      else if (fx_done_event(fx)) return 1;
      GHIP(ctx, hipStreamWaitEvent(st, fx->ev_done, 0));
    }
    io->sums_valid = false;
    if (fx_launch_serial(fx, fx_form_of(fx, io, frames, false), io, frames, st)) return 1;
    GHIP(ctx, hipEventRecord(fx->ev_done, st));
    fx->done_recorded = true;
    fx->last_side = k;
    ++done;
  }
  if (done) {
    GHIP(ctx, hipEventRecord(io->ev_ready[k], st)); // the block is ready when these stages are
    ctx->side_busy[k] = true;
  }
  *n_done = done;
  return 0;
}
// groove_bank_render_async + groove_fx_chain_process_async in one call, which lets the library FUSE the chain's first
// stage into the render kernel when it can (a 12 dB BiQuad behind a bank that renders time-parallel: welsh_tp.h HEAD_BQ).
int groove_bank_render_chain_async(groove_bank* b, uint32_t frames, groove_block* out, groove_fx* const* chain, uint32_t n_fx, uint32_t* n_done) {
  if (!n_done) return fail(nullptr, "groove_bank_render_chain_async: n_done is NULL");
  *n_done = 0;
  if (!b || !out) return fail(nullptr, "groove_bank_render_chain_async: NULL argument");
  if (fx_chain_check(chain, n_fx, out, frames, "groove_bank_render_chain_async")) return 1;
  uint32_t first = 0; // the first stage that does anything (the Mixer is the identity)
  while (first < n_fx && chain[first]->kind == GROOVE_FX_MIXER) ++first;
  groove_fx* head = first < n_fx ? chain[first] : nullptr;
  bool fused = false;
  if (render_async_impl(b, frames, out, head, &fused, head != nullptr)) return 1;
  if (frames == 0) return 0;
  uint32_t taken = 0;
  if (fused) taken = first + 1;
  uint32_t more = 0;
  if (taken < n_fx && groove_fx_chain_process_async(chain + taken, n_fx - taken, out, frames, &more)) return 1;
  *n_done = taken + more;
  return 0;
}
const char* groove_fx_kernel_form(groove_fx* fx, groove_block* block, uint32_t frames) {
  if (!fx || !block) return "";
  const FxForm form = fx_form_of(fx, block, frames, true);
  return form < FxForm::Count ? kFxFormNames[(size_t)form] : "";
}
const char* groove_fx_kernel_form_name(uint32_t index) { return index < (uint32_t)FxForm::Count ? kFxFormNames[index] : nullptr; }
int groove_fx_process(groove_fx* fx, groove_block* io, uint32_t frames) {
  if (!fx || !io) return fail(nullptr, "groove_fx_process: NULL argument");
  return groove_fx_chain_process(&fx, 1, io, frames);
}
int groove_fx_set_params(groove_fx* fx, const groove_fx_params* p, uint32_t n) {
  if (!fx || !p) return fail(nullptr, "groove_fx_set_params: NULL argument");
  groove_ctx* ctx = fx->ctx;
  if (n != fx->n) return fail(ctx, "groove_fx_set_params: n != lanes");
  std::vector<groove_fx_params> old = fx->p;
  fx->p.assign(p, p + n);
  const groove_fx_params &a = old[0], &b = fx->p[0];
  if (fx_check_uniform(fx) ||
      ((fx->kind == GROOVE_FX_CHORUS || fx->kind == GROOVE_FX_DELAY) && (a.delay_seconds != b.delay_seconds || (fx->kind == GROOVE_FX_CHORUS && a.voices != b.voices))) ||
      (fx->kind == GROOVE_FX_REVERB && a.reverb_seconds != b.reverb_seconds)) {
    fx->p = old;
    return fail(ctx, "groove_fx_set_params: delay-line geometry cannot change after creation");
  }
  if (fx_acquire_ctx(fx) || fx_ap_settle(fx)) return 1;
  GHIP(ctx, ctx_wait(ctx));
  return fx_upload_params(fx);
}
int groove_fx_set_param(groove_fx* fx, uint32_t lane, uint32_t control_index, double value01) {
  if (!fx) return fail(nullptr, "groove_fx_set_param: fx is NULL");
  groove_ctx* ctx = fx->ctx;
  if (lane != GROOVE_ALL_VOICES && lane >= fx->n) return fail(ctx, "groove_fx_set_param: lane out of range");
  const double v = value01 < 0.0 ? 0.0 : (value01 > 1.0 ? 1.0 : value01);
  const uint32_t lo = lane == GROOVE_ALL_VOICES ? 0 : lane, hi = lane == GROOVE_ALL_VOICES ? fx->n : lane + 1;
  for (uint32_t i = lo; i < hi; ++i) {
    groove_fx_params& p = fx->p[i];
    switch (control_index) {
      case GROOVE_CTL_FX_CEILING: p.ceiling = (float)v; break;
      case GROOVE_CTL_FX_BITS: p.bits = (uint32_t)(v * 16.0); break;
      case GROOVE_CTL_FX_CUTOFF: p.cutoff_hz = (float)percent_to_frequency_h(v); break;
      case GROOVE_CTL_FX_Q: p.q = (float)(v * v * 10.0 + 0.707); break; /* denormalize_q */
      case GROOVE_CTL_FX_PASSBAND_RIPPLE: p.passband_ripple = (float)(v * v * 10.0 + 0.707); break;
      case GROOVE_CTL_FX_ATTENUATION: p.attenuation = (float)v; break;
      case GROOVE_CTL_FX_WET: p.wet = (float)v; break;
      case GROOVE_CTL_FX_THRESHOLD: p.limit_min = (float)v; break; /* Compressor threshold (limit_min doubles as it: groove_types.h) */
      default: return fail(ctx, "groove_fx_set_param: unknown control index");
    }
  }
  if (fx_acquire_ctx(fx) || fx_ap_settle(fx)) return 1;
  GHIP(ctx, ctx_wait(ctx));
  return fx_upload_params(fx);
}

// ============================================================================ control links
// Six creates, two sources times the effect / wet / bank entry points, are thin: each owns its `who` and the sentences it refuses with;
// what they share is below, in the order a create uses it.  The route table (ctl_core.h: ctl_fx_class, ctl_fx_route, ctl_bank_route)
// says which class a parameter is in.
// What every create onto an effect asks of its arguments (have_source: the source's own pointers are there) and its target.
static int fx_link_check(groove_ctx* ctx, const char* who, bool have_source, uint32_t n_src, groove_fx* target, groove_ctl_link** out) {
  const std::string w = std::string(who) + ": ";
  if (!ctx || !have_source || !target || !out) return fail(ctx, w + "NULL argument");
  if (std::find(ctx->fxs.begin(), ctx->fxs.end(), target) == ctx->fxs.end()) return fail(ctx, w + "the target is not a live effect of this context");
  if (n_src != 1 && n_src != target->n) return fail(ctx, w + "n_src must be the target's lane count, or 1 (broadcast)");
  return 0;
}
// Every effect kernel reads d_wet[lane] at launch and takes `wm < 1` per lane; the one HOST decision that hangs on the value is a
// reverb's form, and a reverb counts its live wet links for that (fx_needs_dry).  The law is groove_fx_set_param's (float)clamp01(v):
// ctl_target_float / ctl_target_float_f64, stored into d_wet instead of d_fa.  The applies' fx_ap_settle orders the store behind a
// direct all-pass kernel that is still reading d_wet on the all-pass stream (events between streams: no host wait).
static int wet_link_check_target(groove_ctx* ctx, const char* who, groove_fx* target) {
  if (!ctl_fx_route(target->kind, GROOVE_CTL_FX_WET)) return fail(ctx, std::string(who) + ": a Mixer is the identity and launches nothing: it reads no wet-dry-mix");
  return 0;
}
// The first filter link onto this effect: from here on fx_upload_params keeps the parameter shadow beside the coefficients.
static int fx_ensure_shadow(groove_fx* target, const char* who) {
  groove_ctx* ctx = target->ctx;
  GHIP(ctx, hipSetDevice(ctx->device));
  if (target->d_shadow) return 0;
  if (hipMalloc(&target->d_shadow, (size_t)CTL_SHADOW_WORDS * target->n * 4) != hipSuccess) {
    target->d_shadow = nullptr;
    return fail(ctx, std::string(who) + ": hipMalloc failed");
  }
  return fx_acquire_ctx(target) || fx_upload_shadow(target);
}
// ---- links onto a bank: a Welsh bank's dca-gain, dca-pan, filter-cutoff; an FM bank's dca-gain, dca-pan, depth, beta; a sampler bank's gain
// What both bank creates ask of their target, and of n_src for it.
static int bank_link_check(groove_ctx* ctx, const char* who, groove_bank* b, uint32_t n_src, uint32_t control_index) {
  const std::string w = std::string(who) + ": ";
  if (std::find(ctx->banks.begin(), ctx->banks.end(), b) == ctx->banks.end()) return fail(ctx, w + "the target is not a live bank of this context");
  if (b->kind != BANK_WELSH) { // an FM bank's four controls, a sampler (drumkit) bank's gain; one source lane for all voices or one per voice
    if (ctl_bank_route(BANK_WELSH, control_index)) return fail(ctx, w + "only Welsh banks expose controls 32 - 34 (dca-gain, dca-pan, filter-cutoff)");
    const bool fm = b->kind == BANK_FM;
    if (!ctl_bank_route(b->kind, control_index)) {
      if (ctl_bank_route(fm ? BANK_SAMPLER : BANK_FM, control_index))
        return fail(ctx, w + (fm ? "an FM bank's controls are 48 - 51 (dca-gain, dca-pan, depth, beta); 64 is a sampler bank's gain"
                                 : "a sampler bank's control is 64 (gain); 48 - 51 are an FM bank's"));
      return fail(ctx, w + (fm ? "unknown control index (a link onto an FM bank reaches dca-gain, dca-pan, depth or beta)"
                               : "unknown control index (a link onto a sampler bank reaches gain)"));
    }
    if (n_src != 1 && n_src != b->n) return fail(ctx, w + "n_src must be the bank's voice count, or 1 (broadcast)");
    return 0;
  }
  if (!ctl_bank_route(BANK_WELSH, control_index)) return fail(ctx, w + "unknown control index (a bank link reaches dca-gain, dca-pan or filter-cutoff)");
  if (n_src != 1)
    return fail(ctx, w + "n_src must be 1: the value is broadcast to every voice (a per-voice source would break the wave-uniform parameter records; per-voice changes keep groove_bank_set_param)");
  return 0;
}
// The bank's side of a new link, before the link exists: the (gain, pan) shadow with the first gain or pan link.
static int bank_link_prepare(groove_bank* b, const char* who, uint32_t control_index) {
  groove_ctx* ctx = b->ctx;
  GHIP(ctx, hipSetDevice(ctx->device));
  if (control_index == GROOVE_CTL_WELSH_CUTOFF || b->kind == BANK_SAMPLER || b->d_dca) return 0; // (a sampler's gain is one word: no shadow)
  if (hipMalloc(&b->d_dca, (size_t)(b->kind == BANK_FM ? CTL_FM_WORDS : CTL_DCA_WORDS) * b->n * 4) != hipSuccess) {
    b->d_dca = nullptr;
    return fail(ctx, std::string(who) + ": hipMalloc failed");
  }
  return b->kind == BANK_FM ? fm_upload_shadow(b) : welsh_upload_dca(b); // from here on welsh_upload_params / fm_upload_params keeps it beside the records
}
// The bank re-planned for its count of cutoff links (welsh_plan.h welsh_flag_filter_f32): a control-plane step like groove_bank_set_param's,
// which it repeats — the host's copy goes up again, the voices' state stays where it is.
static int bank_replan(groove_bank* b) {
  groove_ctx* ctx = b->ctx;
  if (ctx_join(ctx)) return 1;
  GHIP(ctx, ctx_wait(ctx));
  b->ctx_touched = true;
  return welsh_upload_params(b, false);
}
// The source half of a link, with no target yet (link_attach gives it one and lists it): an LFO's or a signal's lanes ...
static int ctl_link_check_sources(groove_ctx* ctx, const char* who, const groove_ctl_source* src, uint32_t n_src) {
  const std::string w = std::string(who) + ": ";
  for (uint32_t i = 0; i < n_src; ++i) {
    if (src[i].source != GROOVE_CTL_SRC_LFO && src[i].source != GROOVE_CTL_SRC_SIGNAL) return fail(ctx, w + "unknown source kind");
    if (src[i].source != src[0].source) return fail(ctx, w + "the lanes of one link share one source kind");
    if (src[i].source == GROOVE_CTL_SRC_LFO) {
      if (!ctl_lfo_waveform_ok(src[i].waveform))
        return fail(ctx, w + "an LFO source is sine, triangle, square, sawtooth, pulse-width or triangle-sine (a noise generator's state at a block start has no closed form)");
      if (!(src[i].frequency_hz >= 0.0) || !(src[i].frequency_hz < (double)ctx->sr)) return fail(ctx, w + "LFO frequency outside [0, sample rate)");
    } else if (!ctl_signal_law_ok(src[i].law)) {
      return fail(ctx, w + "unknown signal law");
    }
  }
  return 0;
}
static int ctl_link_make(groove_ctx* ctx, const char* who, const groove_ctl_source* src, uint32_t n_src, uint32_t control_index, groove_ctl_link** out) {
  const std::string w = std::string(who) + ": ";
  GHIP(ctx, hipSetDevice(ctx->device));
  groove_ctl_link* l = new groove_ctl_link();
  l->ctx = ctx; l->source = src[0].source; l->n_src = n_src; l->control_index = control_index; l->target = nullptr;
  l->src.assign(src, src + n_src);
  if (hipMalloc(&l->d_lanes, ctl_lanes_layout(n_src).bytes) != hipSuccess || hipMalloc(&l->d_value, (size_t)n_src * 4) != hipSuccess ||
      hipMalloc(&l->d_captured, 4) != hipSuccess) {
    groove_ctl_link_destroy(l);
    return fail(ctx, w + "hipMalloc failed");
  }
  if (hipMemsetAsync(l->d_value, 0, (size_t)n_src * 4, ctx->stream) != hipSuccess || hipMemsetAsync(l->d_captured, 0, 4, ctx->stream) != hipSuccess) {
    groove_ctl_link_destroy(l);
    return fail(ctx, w + "hipMemsetAsync failed");
  }
  if (ctl_upload_lanes(l)) { groove_ctl_link_destroy(l); return 1; } // (its message stands)
  *out = l;
  return 0;
}
// ... or a trip's step table (the effect and the bank form alike).
static int ctl_trip_check_steps(groove_ctx* ctx, const char* who, const groove_ctl_step* steps, uint32_t n_steps, const double* start_beat, uint32_t n_src) {
  const std::string w = std::string(who) + ": ";
  if (n_steps == 0) return fail(ctx, w + "a trip has at least one step");
  if (n_steps > 65536u) return fail(ctx, w + "more than 65,536 steps");
  for (uint32_t s = 0; s < n_src; ++s) {
    if (!std::isfinite(start_beat[s])) return fail(ctx, w + "start_beat is not finite");
    for (uint32_t i = 0; i < n_steps; ++i) {
      const groove_ctl_step& st = steps[(size_t)s * n_steps + i];
      if (!ctl_trip_kind_ok(st.kind)) return fail(ctx, w + "unknown step kind (flat, slope, logarithmic, exponential; `Triggered` has no behaviour)");
      if (!std::isfinite(st.beats) || !std::isfinite(st.start) || !std::isfinite(st.end)) return fail(ctx, w + "a step's beats, start or end is not finite");
      if (!(st.beats > 0.0)) return fail(ctx, w + "a step's beats must be > 0");
    }
  }
  return 0;
}
static int ctl_trip_make(groove_ctx* ctx, const char* who, const groove_ctl_step* steps, uint32_t n_steps, const double* start_beat, uint32_t n_src,
                         uint32_t control_index, groove_ctl_link** out) {
  const std::string who_s = std::string(who) + ": ";
  GHIP(ctx, hipSetDevice(ctx->device));
  const CtlTripLayout lay = ctl_trip_layout(n_src, n_steps);
  std::vector<double> w(lay.bytes / 8);
  double *begin = ctl_section<double>(w.data(), lay.begin), *start = ctl_section<double>(w.data(), lay.start), *end = ctl_section<double>(w.data(), lay.end),
         *beats = ctl_section<double>(w.data(), lay.beats);
  uint32_t* kind = ctl_section<uint32_t>(w.data(), lay.kind);
  for (uint32_t s = 0; s < n_src; ++s) {
    const groove_ctl_step* st = steps + (size_t)s * n_steps;
    for (uint32_t i = 0; i < n_steps; ++i) {
      const size_t at = (size_t)i * n_src + s;
      start[at] = st[i].start; end[at] = st[i].end; beats[at] = st[i].beats; kind[at] = st[i].kind;
    }
    ctl_trip_begins(start_beat[s], beats + s, n_src, n_steps, begin + s, n_src);
  }
  groove_ctl_link* l = new groove_ctl_link();
  l->ctx = ctx; l->source = GROOVE_CTL_SRC_TRIP; l->n_src = n_src; l->control_index = control_index; l->target = nullptr;
  l->n_steps = n_steps;
  if (hipMalloc(&l->d_trip, lay.bytes) != hipSuccess) {
    l->d_trip = nullptr;
    groove_ctl_link_destroy(l);
    return fail(ctx, who_s + "hipMalloc failed");
  }
  if (ctx_memcpy(ctx, l->d_trip, w.data(), lay.bytes, hipMemcpyHostToDevice) != hipSuccess) {
    groove_ctl_link_destroy(l);
    return fail(ctx, who_s + "the upload of the step table failed");
  }
  *out = l;
  return 0;
}
// The finished source half `l` gets its target — an effect or a bank — and is listed with the context.  A reverb counts its wet links
// (fx_needs_dry); the first cutoff link takes WF_FILTER_F32 off a Welsh bank's records.  groove_ctl_link_destroy unwinds all of it.
static int link_attach(groove_ctl_link* l, groove_fx* fx, groove_bank* b, groove_ctl_link** out) {
  groove_ctx* ctx = l->ctx;
  l->target = fx; l->bank = b; l->on_bank = b != nullptr;
  ctx->links.push_back(l);
  if (fx && l->control_index == GROOVE_CTL_FX_WET) ++fx->wet_links;
  if (b && l->control_index == GROOVE_CTL_WELSH_CUTOFF && b->cutoff_links++ == 0 && ctx->f32_filter && bank_replan(b)) {
    groove_ctl_link_destroy(l);
    return 1;
  }
  *out = l;
  return 0;
}

int groove_ctl_link_create(groove_ctx* ctx, const groove_ctl_source* src, uint32_t n_src, groove_fx* target, uint32_t control_index,
                           groove_ctl_link** out) {
  const char* who = "groove_ctl_link_create";
  if (fx_link_check(ctx, who, src != nullptr, n_src, target, out)) return 1;
  switch (ctl_fx_class(control_index)) {
    case CTL_ROUTE_DERIVED:
      return fail(ctx, "groove_ctl_link_create: cutoff, q and passband-ripple become filter coefficients on the host (f64): not linkable on the device; use groove_fx_set_param");
    case CTL_ROUTE_WET:
      return fail(ctx, "groove_ctl_link_create: wet-dry-mix chooses a kernel path on the host: not linkable on the device; use groove_fx_set_param");
    case CTL_ROUTE_FLOAT: case CTL_ROUTE_UINT: break;
    default: return fail(ctx, "groove_ctl_link_create: unknown control index");
  }
  if (!ctl_fx_route(target->kind, control_index))
    return fail(ctx, "groove_ctl_link_create: the target's kind has no such parameter (ceiling: Gain; bits: Bitcrusher; attenuation: Reverb; threshold: Compressor / Limiter)");
  groove_ctl_link* l = nullptr;
  if (ctl_link_check_sources(ctx, who, src, n_src) || ctl_link_make(ctx, who, src, n_src, control_index, &l)) return 1;
  return link_attach(l, target, nullptr, out);
}
int groove_ctl_filter_link_create(groove_ctx* ctx, const groove_ctl_source* src, uint32_t n_src, groove_fx* target, uint32_t control_index,
                                  groove_ctl_link** out) {
  const char* who = "groove_ctl_filter_link_create";
  if (fx_link_check(ctx, who, src != nullptr, n_src, target, out)) return 1;
  switch (ctl_fx_class(control_index)) {
    case CTL_ROUTE_DERIVED: break;
    case CTL_ROUTE_WET:
      return fail(ctx, "groove_ctl_filter_link_create: wet-dry-mix chooses a kernel path on the host: not linkable on the device; use groove_fx_set_param");
    case CTL_ROUTE_FLOAT: case CTL_ROUTE_UINT:
      return fail(ctx, "groove_ctl_filter_link_create: a filter link reaches cutoff, q or passband-ripple; this parameter's device form is the value itself: use groove_ctl_link_create");
    default:
      return fail(ctx, "groove_ctl_filter_link_create: unknown control index (a filter link reaches cutoff, q or passband-ripple)");
  }
  if (!ctl_fx_route(target->kind, control_index))
    return fail(ctx, "groove_ctl_filter_link_create: the target's kind does not derive its coefficients from that parameter (cutoff: the nine filter kinds; q: low-pass, high-pass and all-pass 12 dB; passband-ripple: low-pass 24 dB)");
  groove_ctl_link* l = nullptr;
  if (ctl_link_check_sources(ctx, who, src, n_src) || fx_ensure_shadow(target, who) || ctl_link_make(ctx, who, src, n_src, control_index, &l)) return 1;
  return link_attach(l, target, nullptr, out);
}
int groove_ctl_wet_link_create(groove_ctx* ctx, const groove_ctl_source* src, uint32_t n_src, groove_fx* target, groove_ctl_link** out) {
  const char* who = "groove_ctl_wet_link_create";
  groove_ctl_link* l = nullptr;
  if (fx_link_check(ctx, who, src != nullptr, n_src, target, out) || wet_link_check_target(ctx, who, target) || ctl_link_check_sources(ctx, who, src, n_src) ||
      ctl_link_make(ctx, who, src, n_src, GROOVE_CTL_FX_WET, &l))
    return 1;
  return link_attach(l, target, nullptr, out);
}
// A trip link: ONE create for the plain and the filter form, by the parameter.
int groove_ctl_trip_create(groove_ctx* ctx, const groove_ctl_step* steps, uint32_t n_steps, const double* start_beat, uint32_t n_src,
                           groove_fx* target, uint32_t control_index, groove_ctl_link** out) {
  const char* who = "groove_ctl_trip_create";
  if (fx_link_check(ctx, who, steps && start_beat, n_src, target, out)) return 1;
  const CtlRoute cls = ctl_fx_class(control_index);
  if (cls == CTL_ROUTE_WET) return fail(ctx, "groove_ctl_trip_create: wet-dry-mix chooses a kernel path on the host: not linkable on the device; use groove_fx_set_param");
  if (cls == CTL_ROUTE_NONE) return fail(ctx, "groove_ctl_trip_create: unknown control index");
  if (!ctl_fx_route(target->kind, control_index))
    return fail(ctx, cls == CTL_ROUTE_DERIVED
                         ? "groove_ctl_trip_create: the target's kind has no such parameter (cutoff: the nine filter kinds; q: low-pass, high-pass and all-pass 12 dB; passband-ripple: low-pass 24 dB)"
                         : "groove_ctl_trip_create: the target's kind has no such parameter (ceiling: Gain; bits: Bitcrusher; attenuation: Reverb; threshold: Compressor / Limiter)");
  groove_ctl_link* l = nullptr;
  if (ctl_trip_check_steps(ctx, who, steps, n_steps, start_beat, n_src) || (cls == CTL_ROUTE_DERIVED && fx_ensure_shadow(target, who)) ||
      ctl_trip_make(ctx, who, steps, n_steps, start_beat, n_src, control_index, &l))
    return 1;
  return link_attach(l, target, nullptr, out);
}
int groove_ctl_wet_trip_create(groove_ctx* ctx, const groove_ctl_step* steps, uint32_t n_steps, const double* start_beat, uint32_t n_src, groove_fx* target,
                               groove_ctl_link** out) {
  const char* who = "groove_ctl_wet_trip_create";
  groove_ctl_link* l = nullptr;
  if (fx_link_check(ctx, who, steps && start_beat, n_src, target, out) || wet_link_check_target(ctx, who, target) ||
      ctl_trip_check_steps(ctx, who, steps, n_steps, start_beat, n_src) || ctl_trip_make(ctx, who, steps, n_steps, start_beat, n_src, GROOVE_CTL_FX_WET, &l))
    return 1;
  return link_attach(l, target, nullptr, out);
}
int groove_ctl_bank_link_create(groove_ctx* ctx, const groove_ctl_source* src, uint32_t n_src, groove_bank* target, uint32_t control_index,
                                groove_ctl_link** out) {
  const char* who = "groove_ctl_bank_link_create";
  if (!ctx || !src || !target || !out) return fail(ctx, std::string(who) + ": NULL argument");
  groove_ctl_link* l = nullptr;
  if (bank_link_check(ctx, who, target, n_src, control_index) || ctl_link_check_sources(ctx, who, src, n_src) || bank_link_prepare(target, who, control_index) ||
      ctl_link_make(ctx, who, src, n_src, control_index, &l))
    return 1;
  return link_attach(l, nullptr, target, out);
}
int groove_ctl_bank_trip_create(groove_ctx* ctx, const groove_ctl_step* steps, uint32_t n_steps, const double* start_beat, uint32_t n_src,
                                groove_bank* target, uint32_t control_index, groove_ctl_link** out) {
  const char* who = "groove_ctl_bank_trip_create";
  if (!ctx || !steps || !start_beat || !target || !out) return fail(ctx, std::string(who) + ": NULL argument");
  groove_ctl_link* l = nullptr;
  if (bank_link_check(ctx, who, target, n_src, control_index) || ctl_trip_check_steps(ctx, who, steps, n_steps, start_beat, n_src) ||
      bank_link_prepare(target, who, control_index) || ctl_trip_make(ctx, who, steps, n_steps, start_beat, n_src, control_index, &l))
    return 1;
  return link_attach(l, nullptr, target, out);
}
int groove_ctl_link_capture(groove_ctl_link* l, groove_block* blk, uint32_t frames) {
  if (!l || !blk) return fail(nullptr, "groove_ctl_link_capture: NULL argument");
  groove_ctx* ctx = l->ctx;
  if (blk->ctx != ctx) return fail(ctx, "groove_ctl_link_capture: link and block belong to different contexts");
  if (l->source == GROOVE_CTL_SRC_TRIP) return fail(ctx, "groove_ctl_link_capture: a trip link captures nothing (groove_ctl_trip_apply is its only call)");
  if (l->source != GROOVE_CTL_SRC_SIGNAL) return fail(ctx, "groove_ctl_link_capture: not a signal link");
  if (blk->n != l->n_src) return fail(ctx, "groove_ctl_link_capture: block lanes != source lanes");
  if (frames > blk->cap) return fail(ctx, "groove_ctl_link_capture: frames > block capacity");
  if (frames == 0) return 0; // nothing has been transformed
  GHIP(ctx, hipSetDevice(ctx->device));
  if (block_acquire(blk) || block_normalise(blk)) return 1; // the source lanes are in the caller's order, like an effect's
  hipLaunchKernelGGL(ctl_capture_kernel, dim3(blocks_for(blk->n)), dim3(kThreads), 0, ctx->stream, blk->d, (size_t)blk->cap * blk->n, blk->n, frames - 1,
                     l->d_value, l->d_captured);
  GHIP(ctx, hipGetLastError());
  return 0;
}
// groove_ctl_link_apply / groove_ctl_trip_apply: which target, order the ctx stream against its other users, one launch of the apply
// kernel by (source, target).  An effect: fx_acquire_ctx + fx_ap_settle.  A bank's renders run on side streams: the ctx stream joins them
// by events (no host wait), the kernel runs there, and every later render of the bank forks behind it (ctx_join: need_fork; ctx_touched
// for the asynchronous render's own choice of what to wait for) — no render of the bank overlaps the write of its records.
static int link_apply(groove_ctl_link* l, const char* who, uint64_t at) {
  groove_ctx* ctx = l->ctx;
  groove_fx* fx = l->target;
  groove_bank* b = l->bank;
  if (l->on_bank) {
    if (!b || std::find(ctx->banks.begin(), ctx->banks.end(), b) == ctx->banks.end()) return fail(ctx, std::string(who) + ": the target bank has been destroyed");
    GHIP(ctx, hipSetDevice(ctx->device));
    b->ctx_touched = true;
    if (ctx_join(ctx)) return 1;
  } else {
    if (!fx || std::find(ctx->fxs.begin(), ctx->fxs.end(), fx) == ctx->fxs.end()) return fail(ctx, std::string(who) + ": the target effect has been destroyed");
    GHIP(ctx, hipSetDevice(ctx->device));
    if (fx_acquire_ctx(fx) || fx_ap_settle(fx)) return 1;
  }
  auto launch = [&](const auto& source, const auto& target) {
    using Source = std::decay_t<decltype(source)>;
    using Target = std::decay_t<decltype(target)>;
    hipLaunchKernelGGL((ctl_apply_kernel<Source, Target>), dim3(blocks_for(target.threads())), dim3(kThreads), 0, ctx->stream, source, target);
  };
  auto from_source = [&](const auto& target) {
    if (l->source == GROOVE_CTL_SRC_TRIP) launch(CtlTripAt{ctl_trip_view(l), l->n_src, at}, target);
    else launch(CtlLive{l->source, l->n_src, ctl_lanes_view(l), at, l->d_value, l->d_captured}, target);
  };
  if (l->on_bank) { // a Welsh bank's records and per-wave copies; an FM or sampler bank's per-voice SoA, the one place its kernels read (ctl_link.h)
    if (b->kind == BANK_WELSH) from_source(CtlBank{b->d_params, b->plan.n_vwaves ? b->d_waves : nullptr, b->d_dca, b->n, b->plan.n_vwaves, l->control_index});
    else from_source(CtlVoices{b->d_params, b->kind == BANK_FM ? b->d_dca : nullptr, b->n, l->control_index});
  } else {
    switch (ctl_fx_route(fx->kind, l->control_index)) {
      case CTL_ROUTE_DERIVED: from_source(CtlFilter{fx->kind, l->control_index, (double)ctx->sr, fx->d_shadow, fx->d_coef, fx->n}); break;
      case CTL_ROUTE_UINT: from_source(CtlPlain{nullptr, fx->d_ua, fx->n}); break;
      case CTL_ROUTE_WET: from_source(CtlPlain{fx->d_wet, nullptr, fx->n}); break;
      default: from_source(CtlPlain{fx->d_fa, nullptr, fx->n}); break;
    }
  }
  GHIP(ctx, hipGetLastError());
  return 0;
}
int groove_ctl_link_apply(groove_ctl_link* l, uint64_t at_frame) {
  if (!l) return fail(nullptr, "groove_ctl_link_apply: link is NULL");
  if (l->source == GROOVE_CTL_SRC_TRIP) return fail(l->ctx, "groove_ctl_link_apply: a trip link is applied at a musical time: use groove_ctl_trip_apply");
  return link_apply(l, "groove_ctl_link_apply", at_frame);
}
int groove_ctl_trip_apply(groove_ctl_link* l, uint64_t at_units) {
  if (!l) return fail(nullptr, "groove_ctl_trip_apply: link is NULL");
  if (l->source != GROOVE_CTL_SRC_TRIP) return fail(l->ctx, "groove_ctl_trip_apply: not a trip link (an LFO or signal link is applied at a frame: groove_ctl_link_apply)");
  return link_apply(l, "groove_ctl_trip_apply", at_units);
}
int groove_ctl_link_reset(groove_ctl_link* l) {
  if (!l) return fail(nullptr, "groove_ctl_link_reset: link is NULL");
  groove_ctx* ctx = l->ctx;
  if (l->source == GROOVE_CTL_SRC_TRIP) return 0; // a closed form of musical time: nothing to forget
  GHIP(ctx, hipSetDevice(ctx->device));
  GHIP(ctx, hipMemsetAsync(l->d_captured, 0, 4, ctx->stream));
  return 0;
}
int groove_ctl_link_destroy(groove_ctl_link* l) {
  if (!l) return 0;
  groove_ctx* ctx = l->ctx;
  // the last cutoff link off a live bank: its records may carry WF_FILTER_F32 again (link_attach)
  if (l->bank && l->control_index == GROOVE_CTL_WELSH_CUTOFF && std::find(ctx->banks.begin(), ctx->banks.end(), l->bank) != ctx->banks.end() &&
      l->bank->cutoff_links && --l->bank->cutoff_links == 0 && ctx->f32_filter)
    (void)bank_replan(l->bank);
  // the last wet link off a live effect: a reverb is all wet again when the host's copy says so (fx_needs_dry); an effect that died
  // first cleared l->target (groove_fx_destroy)
  if (!l->on_bank && l->target && l->control_index == GROOVE_CTL_FX_WET && std::find(ctx->fxs.begin(), ctx->fxs.end(), l->target) != ctx->fxs.end() &&
      l->target->wet_links)
    --l->target->wet_links;
  (void)hipStreamSynchronize(ctx->stream); // the link's kernels run there
  auto it = std::find(ctx->links.begin(), ctx->links.end(), l);
  if (it != ctx->links.end()) ctx->links.erase(it);
  (void)hipFree(l->d_lanes); (void)hipFree(l->d_value); (void)hipFree(l->d_captured); (void)hipFree(l->d_trip);
  delete l;
  return 0;
}

// ============================================================================ mix bus
int groove_mix(groove_ctx* ctx, groove_block* const* blocks, uint32_t n_blocks, uint32_t frames,
               float* bus_dev, int accumulate) {
  if (!ctx || !bus_dev) return fail(ctx, "groove_mix: NULL argument");
  if (bus_flush(ctx)) return 1;
  if (n_blocks && !blocks) return fail(ctx, "groove_mix: blocks is NULL");
  if (frames == 0) return 0;
  GHIP(ctx, hipSetDevice(ctx->device));
  if (n_blocks == 0) { // nothing patched: silence (orchestrator.rs:1452-1455)
    if (!accumulate) GHIP(ctx, hipMemsetAsync(bus_dev, 0, (size_t)frames * 8, ctx->stream));
    return 0;
  }
  for (uint32_t i = 0; i < n_blocks; ++i) {
    if (!blocks[i]) return fail(ctx, "groove_mix: NULL block");
    if (frames > blocks[i]->cap) return fail(ctx, "groove_mix: frames > block capacity");
    if (block_acquire(blocks[i])) return 1;
    groove_block* blk = blocks[i];
    if (blk->sums_valid && blk->sum_frames == frames) { // the render left the block's lane sums: reduce those rows
      // a block of the render-ahead rotation (it has its events): this reduction is normally its last consumer before the host
      // releases it, so the block's "free" event is bound to the reduction's last kernel and the release records nothing
      const bool mark = blk->ev_free && ctx->bind_events;
      if (reduce_rows(ctx, blk->sums_on_ap ? blk->d_sums_ap[blk->ap_flip] : blk->d_sums, blk->sum_rows, frames, bus_dev, accumulate || i > 0, mark ? blk->ev_free : nullptr)) return 1;
      if (blk->sums_on_ap && ap_follow(ctx)) return 1; // (that stream's later all-passes rewrite the buffer)
      blk->free_marked = mark;
    } else if (mix_one(ctx, blocks[i], frames, bus_dev, accumulate || i > 0)) return 1;
  }
  return 0;
}
// groove_mix for ONE block whose lane sums are valid (a render or an effect chain has just left them), with the reduction of
// those few rows DEFERRED: the next fused effect-chain launch on the ctx stream (fx_run_kernel), the next deferred render, or
// bus_flush puts them on the bus.  Anything else: groove_mix.
int groove_mix_deferred(groove_ctx* ctx, groove_block* blk, uint32_t frames, float* bus_dev, int accumulate) {
  if (!ctx || !bus_dev || !blk) return fail(ctx, "groove_mix_deferred: NULL argument");
  if (frames == 0) return 0;
  if (blk->ctx != ctx) return fail(ctx, "groove_mix_deferred: the block belongs to another ctx");
  if (!(blk->sums_valid && blk->sum_frames == frames && blk->sum_rows <= 2048 && frames <= 4096)) return groove_mix(ctx, &blk, 1, frames, bus_dev, accumulate);
  GHIP(ctx, hipSetDevice(ctx->device));
  if (blk->sums_on_ap && ctx->fx_ap_stream >= 0 && blk->ready_mask == (1u << ctx->fx_ap_stream)) {
    // The rows are being written on the all-pass stream: that stream's NEXT all-pass launch sums them (ordered behind their
    // writer without a wait; the ctx stream is not held up for the block).  Pending rows of any other kind go first, and the
    // all-pass stream behind them: the order of a bus's sums is the order of the calls.
    if (ctx->deferred.rows || ctx->deferred_ap.rows || !ctx->paced_order.empty()) { if (bus_flush(ctx) || ap_follow(ctx)) return 1; }
    ctx->deferred_ap = TpPrev{blk->d_sums_ap[blk->ap_flip], bus_dev, blk->sum_rows, frames, accumulate};
    blk->ap_flip ^= 1; // the block's next chain writes the other buffer: this one is read one launch from now
    blk->sums_valid = false; blk->sums_on_ap = false;
    return 0;
  }
  if (bus_flush(ctx)) return 1; // an earlier pending block nobody carried: its own reduction launch, first (order of the bus's sums)
  if (block_acquire(blk)) return 1;
  if (blk->sums_on_ap) { const int rc = groove_mix(ctx, &blk, 1, frames, bus_dev, accumulate); return rc; } // (not this path's buffers)
  ctx->deferred = TpPrev{blk->d_sums, bus_dev, blk->sum_rows, frames, accumulate};
  // the rows leave the block: whatever writes the block's lane sums next (its next render may run on another stream) cannot touch them
  ctx->deferred_owned_cap = blk->sums_cap;
  blk->d_sums = nullptr; blk->sums_cap = 0; blk->sums_valid = false;
  // a spare at least as large as the buffer that left (a smaller one would make block_sums free and reallocate — device-wide
  // synchronisations inside the paced walk — until every buffer of the rotation had grown): the smallest that fits
  int pick = -1;
  for (int i = 0; i < (int)ctx->spare_sums.size(); ++i)
    if (ctx->spare_sums[i].second >= ctx->deferred_owned_cap && (pick < 0 || ctx->spare_sums[i].second < ctx->spare_sums[pick].second)) pick = i;
  if (pick >= 0) { blk->d_sums = ctx->spare_sums[pick].first; blk->sums_cap = ctx->spare_sums[pick].second; ctx->spare_sums.erase(ctx->spare_sums.begin() + pick); }
  return 0;
}
// HOST PACING.  A wait for another queue's event costs the waiting stream 7 - 9 us of its timeline whether or not the event has
// completed by the time the stream gets there (docs/STREAMS.md item 13), but the runtime drops a wait whose event is already
// complete when the call is made.  An offline host has nothing else to do: it can wait for the event itself, and the streams
// then carry no wait packets at all.
int groove_block_wait_ready(groove_block* b) {
  if (!b) return fail(nullptr, "groove_block_wait_ready: block is NULL");
  groove_ctx* ctx = b->ctx;
  for (int k = 0; k < kSideStreams; ++k)
    if (b->ready_mask & (1u << k)) GHIP(ctx, wait_deadline(ctx, nullptr, b->ev_ready[k], "groove_block_wait_ready"));
  b->ready_mask = 0; // complete: what the host submits from now on is ordered behind it without a device-side wait
  return 0;
}
int groove_block_wait_released(groove_block* b) {
  if (!b) return fail(nullptr, "groove_block_wait_released: block is NULL");
  if (b->released && b->ev_free) {
    GHIP(b->ctx, wait_deadline(b->ctx, nullptr, b->ev_free, "groove_block_wait_released"));
    // a release recorded on the all-pass stream sits behind the block's last kernel there: the host has seen that complete
    if (b->ctx->fx_ap_stream >= 0) b->ready_mask &= ~(1u << b->ctx->fx_ap_stream);
  }
  return 0;
}
int groove_block_accumulate(groove_block* dst, groove_block* src, uint32_t frames, int accumulate) {
  if (!dst || !src) return fail(nullptr, "groove_block_accumulate: NULL argument");
  groove_ctx* ctx = dst->ctx;
  if (frames > dst->cap || frames > src->cap) return fail(ctx, "groove_block_accumulate: frames > block capacity");
  if (frames == 0) return 0;
  GHIP(ctx, hipSetDevice(ctx->device));
  if (block_acquire(dst) || block_acquire(src)) return 1;
  dst->sums_valid = false;
  if (src->n == dst->n) {
    if (block_normalise(src)) return 1;                 // element-wise: both in the caller's lane order
    if (accumulate ? block_normalise(dst) : 0) return 1;
    if (!accumulate) dst->order.reset();
    const size_t total = (size_t)2 * frames * src->n;
    const uint32_t g = (uint32_t)std::min<size_t>(blocks_for(total), 256 * 16);
    hipLaunchKernelGGL(block_add_kernel, dim3(g), dim3(kThreads), 0, ctx->stream, dst->d, (size_t)dst->cap * dst->n,
                       src->d, (size_t)src->cap * src->n, src->n, frames, accumulate);
    GHIP(ctx, hipGetLastError());
    return 0;
  }
  if (dst->n == 1) { dst->order.reset(); return mix_one(ctx, src, frames, dst->d, accumulate, (size_t)dst->cap); } // a lane sum has no order
  return fail(ctx, "groove_block_accumulate: lane counts differ and the destination is not a 1-lane block");
}
int groove_block_zero(groove_block* b) {
  if (!b) return fail(nullptr, "groove_block_zero: NULL argument");
  if (block_acquire(b)) return 1;
  b->sums_valid = false;
  b->order.reset();
  GHIP(b->ctx, hipMemsetAsync(b->d, 0, (size_t)2 * b->cap * b->n * 4, b->ctx->stream));
  return 0;
}
int groove_bus_create(groove_ctx* ctx, size_t frames, float** out_dev) {
  if (!ctx || !out_dev) return fail(ctx, "groove_bus_create: NULL argument");
  GHIP(ctx, hipSetDevice(ctx->device));
  GHIP(ctx, hipMalloc(out_dev, std::max<size_t>(frames, 1) * 8));
  // zeroed ON THE CTX STREAM: hipMemset runs on the null stream, which the (non-blocking) ctx stream does
  // not wait for, and may land after the first kernels that write the bus
  GHIP(ctx, hipMemsetAsync(*out_dev, 0, std::max<size_t>(frames, 1) * 8, ctx->stream));
  return 0;
}
int groove_bus_destroy(groove_ctx* ctx, float* bus_dev) {
  if (!ctx) return fail(nullptr, "groove_bus_destroy: ctx is NULL");
  GHIP(ctx, ctx_wait(ctx));
  GHIP(ctx, hipFree(bus_dev));
  return 0;
}
int groove_bus_zero(groove_ctx* ctx, float* bus_dev, size_t frames) {
  if (!ctx || !bus_dev) return fail(ctx, "groove_bus_zero: NULL argument");
  if (bus_flush(ctx)) return 1;
  GHIP(ctx, hipMemsetAsync(bus_dev, 0, frames * 8, ctx->stream));
  return 0;
}
int groove_download(groove_ctx* ctx, const float* dev, float* host, size_t n_floats) {
  if (!ctx || !dev || !host) return fail(ctx, "groove_download: NULL argument");
  GHIP(ctx, ctx_wait(ctx, "copy on the ctx stream"));
  GHIP(ctx, hipMemcpyAsync(host, dev, n_floats * 4, hipMemcpyDeviceToHost, ctx->stream));
  GHIP(ctx, ctx_wait(ctx));
  return 0;
}
int groove_upload(groove_ctx* ctx, float* dev, const float* host, size_t n_floats) {
  if (!ctx || !dev || !host) return fail(ctx, "groove_upload: NULL argument");
  GHIP(ctx, ctx_wait(ctx, "copy on the ctx stream"));
  GHIP(ctx, hipMemcpyAsync(dev, host, n_floats * 4, hipMemcpyHostToDevice, ctx->stream));
  GHIP(ctx, ctx_wait(ctx));
  return 0;
}
int groove_bus_to_i16(groove_ctx* ctx, const float* bus_dev, size_t frames, int16_t* host_out) {
  if (!ctx || !bus_dev || !host_out) return fail(ctx, "groove_bus_to_i16: NULL argument");
  if (bus_flush(ctx)) return 1;
  const size_t count = frames * 2;
  if (count == 0) return 0;
  if (ctx->i16_cap < count) {
    if (ctx->d_i16) GHIP(ctx, hipFree(ctx->d_i16));
    GHIP(ctx, hipMalloc(&ctx->d_i16, count * 2));
    ctx->i16_cap = count;
  }
  hipLaunchKernelGGL(bus_to_i16_kernel, dim3(blocks_for(count)), dim3(kThreads), 0, ctx->stream, bus_dev, count, ctx->d_i16);
  GHIP(ctx, hipGetLastError());
  GHIP(ctx, ctx_wait(ctx, "copy on the ctx stream"));
  GHIP(ctx, hipMemcpyAsync(host_out, ctx->d_i16, count * 2, hipMemcpyDeviceToHost, ctx->stream));
  GHIP(ctx, ctx_wait(ctx));
  return 0;
}

// ============================================================================ multi-GPU
int groove_comm_unique_id(groove_ctx* ctx, uint8_t id_out[128]) { // ctx may be NULL (groove_init_comm wants the id before any ctx exists)
  if (!id_out) return fail(ctx, "groove_comm_unique_id: NULL argument");
  if (rccl_open(ctx)) return 1;
  auto f = (nccl_get_uid_fn)dlsym(g_rccl, "ncclGetUniqueId");
  if (!f) return fail(ctx, "ncclGetUniqueId not found");
  ncclUniqueId id;
  const ncclResult_t rc = f(&id);
  if (rc != ncclSuccess) return fail(ctx, "ncclGetUniqueId failed");
  std::memcpy(id_out, &id, sizeof(id));
  return 0;
}
static int comm_init_rank(groove_ctx* ctx, const uint8_t id[128], int rank, int world_size) {
  if (world_size < 1 || rank < 0 || rank >= world_size) return fail(ctx, "groove_comm_init: bad rank/world");
  if (ctx->comm) return fail(ctx, "groove_comm_init: this ctx already has a communicator");
  if (rccl_open(ctx)) return 1;
  GHIP(ctx, hipSetDevice(ctx->device));
  auto f = (nccl_init_rank_fn)dlsym(ctx->rccl, "ncclCommInitRank");
  if (!f) return fail(ctx, "ncclCommInitRank not found");
  ncclUniqueId uid;
  std::memcpy(&uid, id, sizeof(uid));
  ncclComm_t comm = nullptr;
  const ncclResult_t rc = f(&comm, world_size, uid, rank);
  if (rc != ncclSuccess) {
    auto es = (nccl_errstr_fn)dlsym(ctx->rccl, "ncclGetErrorString");
    return fail(ctx, std::string("ncclCommInitRank failed: ") + (es ? es(rc) : "?"));
  }
  ctx->comm = comm; ctx->rank = rank; ctx->world = world_size;
  return 0;
}
int groove_comm_init(groove_ctx* ctx, const uint8_t id[128], int rank, int world_size) {
  if (!ctx || !id) return fail(ctx, "groove_comm_init: NULL argument");
  return comm_init_rank(ctx, id, rank, world_size);
}
int groove_comm_ranks(groove_ctx* ctx, int* out_ranks) {
  if (!ctx || !out_ranks) return fail(ctx, "groove_comm_ranks: NULL argument");
  *out_ranks = 1;
  if (!ctx->comm) return 0; // no communicator: one rank
  auto f = (nccl_count_fn)dlsym(ctx->rccl, "ncclCommCount");
  if (!f) return fail(ctx, "ncclCommCount not found");
  int count = 0;
  const ncclResult_t rc = f((ncclComm_t)ctx->comm, &count);
  if (rc != ncclSuccess) return fail(ctx, "ncclCommCount failed");
  *out_ranks = count;
  return 0;
}
int groove_comm_destroy(groove_ctx* ctx) {
  if (!ctx || !ctx->comm) return 0;
  auto f = (nccl_destroy_fn)dlsym(ctx->rccl, "ncclCommDestroy");
  if (f) f((ncclComm_t)ctx->comm);
  ctx->comm = nullptr;
  return 0;
}
int groove_bus_reduce(groove_ctx* ctx, float* bus_dev, size_t frames_total, int root) {
  if (!ctx || !bus_dev) return fail(ctx, "groove_bus_reduce: NULL argument");
  if (bus_flush(ctx)) return 1;
  if (ctx->world == 1 && !ctx->comm) return 0; // single GPU: the bus is already complete
  if (!ctx->comm) return fail(ctx, "groove_bus_reduce: communicator not initialised");
  auto f = (nccl_reduce_fn)dlsym(ctx->rccl, "ncclReduce");
  if (!f) return fail(ctx, "ncclReduce not found");
  // in place on the root
  const ncclResult_t rc = f(bus_dev, bus_dev, frames_total * 2, ncclFloat32, ncclSum, root, (ncclComm_t)ctx->comm, ctx->stream);
  if (rc != ncclSuccess) {
    auto es = (nccl_errstr_fn)dlsym(ctx->rccl, "ncclGetErrorString");
    return fail(ctx, std::string("ncclReduce failed: ") + (es ? es(rc) : "?"));
  }
  return 0;
}

} // extern "C"
