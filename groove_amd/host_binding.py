"""ctypes binding of groove_amd/host/libgroove_host.so — the compiled (C++) host layer that
mirrors the reference's Orchestrator / entity surface above the C ABI."""
import ctypes as C
import os

import numpy as np

from . import abi_types as T

HERE = os.path.dirname(os.path.abspath(__file__))
HOST_LIB = os.path.join(HERE, "host", "libgroove_host.so")
_fp = C.POINTER(C.c_float)

STEP_FLAT, STEP_SLOPE, STEP_LOGARITHMIC, STEP_EXPONENTIAL, STEP_TRIGGERED = range(5)


def load():
    if not os.path.exists(HOST_LIB):
        raise RuntimeError(f"{HOST_LIB} not found: run __graft_entry__.build()")
    L = C.CDLL(HOST_LIB)
    vp, i, u32, d = C.c_void_p, C.c_int, C.c_uint32, C.c_double
    sig = {
        "gh_orchestrator_new": (vp, [i, u32, d]), "gh_orchestrator_free": (None, [vp]),
        "gh_last_error": (C.c_char_p, [vp]), "gh_add_toy_source": (i, [vp, d]),
        "gh_add_welsh": (i, [vp, C.POINTER(T.WelshParams), u32]), "gh_add_fm": (i, [vp, C.POINTER(T.FmParams), u32]),
        "gh_add_drumkit": (i, [vp, _fp, C.c_uint64, C.POINTER(T.SampleDesc), u32, C.POINTER(C.c_int)]),
        "gh_add_drumkit_stereo": (i, [vp, _fp, C.c_uint64, C.POINTER(T.SampleDesc), u32, C.POINTER(C.c_int)]),
        "gh_add_sampler": (i, [vp, _fp, C.c_uint64, d, u32]), "gh_add_sampler_stereo": (i, [vp, _fp, C.c_uint64, d, u32]),
        "gh_set_stereo_samples": (None, [vp, i]), "gh_stereo_samples": (i, [vp]),
        "gh_set_sample_interpolation": (i, [vp, u32]), "gh_sample_interpolation": (u32, [vp]),
        "gh_set_sample_envelope": (i, [vp, C.POINTER(T.EnvelopeParams)]), "gh_sample_envelope": (i, [vp, C.POINTER(T.EnvelopeParams)]),
        "gh_set_sample_loops": (None, [vp, i]), "gh_sample_loops": (i, [vp]), "gh_set_sample_loop": (i, [vp, i, u32, u32]),
        "gh_read_wav_loop": (i, [C.c_char_p, C.POINTER(u32), C.POINTER(u32)]),
        "gh_add_effect": (i, [vp, u32, C.POINTER(T.FxParams)]),
        "gh_patch": (i, [vp, i, i]), "gh_patch_chain_to_main_mixer": (i, [vp, C.POINTER(C.c_int), u32]),
        "gh_unpatch_all": (None, [vp]), "gh_set_render_ahead": (None, [vp, i]), "gh_set_fused_direct": (None, [vp, i]), "gh_set_filter_links_on_device": (None, [vp, i]),
        "gh_set_trips_on_device": (None, [vp, i]), "gh_control_trip_on_device": (i, [vp, i]),
        "gh_set_instrument_controls_on_device": (None, [vp, i]),
        "gh_set_wet_links_on_device": (None, [vp, i]), "gh_wet_links_on_device": (i, [vp]),
        "gh_set_wet_reverb_run": (i, [vp, i]), "gh_wet_reverb_run": (i, [vp]),
        "gh_debug_info": (i, [vp, C.c_char_p, C.c_size_t]), "gh_connect_midi_downstream": (i, [vp, i, i]),
        "gh_add_timer": (i, [vp, d]), "gh_add_sequencer": (i, [vp]),
        "gh_sequencer_insert": (i, [vp, i, i, i, d, d]), "gh_sequencer_set_end": (i, [vp, i, d]),
        "gh_add_control_trip": (i, [vp, i, C.c_char_p, d]), "gh_control_trip_add_step": (i, [vp, i, i, d, d, d]),
        "gh_add_lfo_controller": (i, [vp, u32, d, d]), "gh_add_signal_passthrough": (i, [vp]), "gh_link_control": (i, [vp, i, i, C.c_char_p]),
        "gh_control_step_value": (d, [i, d, d, d]), "gh_last_allocated_voice": (i, [vp, i]),
        "gh_gather_audio": (i, [vp, u32, _fp]), "gh_performance_frames": (C.c_uint64, [vp]),
        "gh_run": (C.c_int64, [vp, u32, _fp, C.c_uint64, i]), "gh_render_to_wav": (i, [vp, u32, C.c_char_p]),
        "gh_synthetic_kit": (i, [u32, _fp, C.c_uint64, C.POINTER(T.SampleDesc), u32, C.POINTER(C.c_int), C.POINTER(C.c_uint64), C.POINTER(u32)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    return L


def synthetic_kit(sample_rate=T.DEFAULT_SAMPLE_RATE):
    """The sample bank `groove-cli-hip --synthetic-kit` builds (data only, no GPU): (pcm, descs, key_to_sample)."""
    L = load()
    frames, nd = C.c_uint64(), C.c_uint32()
    assert L.gh_synthetic_kit(sample_rate, None, 0, None, 0, None, C.byref(frames), C.byref(nd)) == 0
    pcm = np.empty(frames.value, dtype=np.float32)
    descs = (T.SampleDesc * nd.value)()
    k2s = (C.c_int * 128)()
    assert L.gh_synthetic_kit(sample_rate, pcm.ctypes.data_as(_fp), pcm.size, descs, nd.value, k2s, None, None) == 0
    return pcm, descs, list(k2s)


class Orchestrator:
    MAIN_MIXER = 0

    def __init__(self, device=0, sample_rate=T.DEFAULT_SAMPLE_RATE, bpm=128.0):
        self.L = load()
        self.h = self.L.gh_orchestrator_new(device, sample_rate, bpm)
        if not self.h:
            raise RuntimeError("Orchestrator: no HIP device / context (there is no CPU path)")

    def _chk(self, rc):
        if rc != 0:
            raise RuntimeError(self.L.gh_last_error(self.h).decode())

    def add_toy_source(self, level): return self.L.gh_add_toy_source(self.h, level)
    def add_welsh(self, patch, voices=8): return self.L.gh_add_welsh(self.h, C.byref(patch), voices)
    def add_fm(self, patch, voices=8): return self.L.gh_add_fm(self.h, C.byref(patch), voices)

    def add_drumkit(self, pcm, descs, key_to_sample):
        pcm = np.ascontiguousarray(pcm, dtype=np.float32)
        k2s = (C.c_int * 128)(*key_to_sample)
        return self.L.gh_add_drumkit(self.h, pcm.ctypes.data_as(_fp), pcm.size, descs, len(descs), k2s)

    def add_drumkit_stereo(self, pcm_lr, descs, key_to_sample):
        """A drumkit over a stereo bank: pcm_lr is [frames, 2] (left, right per frame), descs in frames."""
        pcm = np.ascontiguousarray(pcm_lr, dtype=np.float32)
        assert pcm.ndim == 2 and pcm.shape[1] == 2, pcm.shape
        k2s = (C.c_int * 128)(*key_to_sample)
        return self.L.gh_add_drumkit_stereo(self.h, pcm.ctypes.data_as(_fp), pcm.shape[0], descs, len(descs), k2s)

    def add_sampler(self, pcm, root_hz, voices=8):
        """A sampler on one buffer: [frames] mono, or [frames, 2] stereo (gh_add_sampler_stereo)."""
        pcm = np.ascontiguousarray(pcm, dtype=np.float32)
        add = self.L.gh_add_sampler_stereo if pcm.ndim == 2 else self.L.gh_add_sampler
        return add(self.h, pcm.ctypes.data_as(_fp), pcm.shape[0], root_hz, voices)

    def set_stereo_samples(self, on):
        """Projects instantiated from here on keep the channels of two-channel sample files: a sampler on one is a stereo bank, a drumkit
        with one is a stereo bank whose mono files are on both channels.  Off by default (a stereo file is the mean of its channels)."""
        self.L.gh_set_stereo_samples(self.h, 1 if on else 0)

    def stereo_samples(self): return bool(self.L.gh_stereo_samples(self.h))

    def set_sample_interpolation(self, mode):
        """Sampler and drumkit banks added from here on (a project's among them) read their samples between frames by `mode`:
        abi_types.SAMPLE_NEAREST (the default, the reference's reading), SAMPLE_LINEAR or SAMPLE_CUBIC.  An unknown mode raises."""
        if self.L.gh_set_sample_interpolation(self.h, mode):
            raise RuntimeError(self.L.gh_last_error(self.h).decode())

    def sample_interpolation(self): return self.L.gh_sample_interpolation(self.h)

    def set_sample_loops(self, on):
        """A `sampler` a project creates from here on takes the forward sustain loop its WAV file carries (off by default)."""
        self.L.gh_set_sample_loops(self.h, int(bool(on)))

    def sample_loops(self): return bool(self.L.gh_sample_loops(self.h))

    def set_sample_envelope(self, envelope):
        """A `sampler` created from here on gets the amplitude envelope (attack, decay, sustain, release) — seconds, seconds, 0..1,
        seconds — on its sample and keeps a voice busy through its release tail; None: none (the default)."""
        env = None if envelope is None else C.byref(T.EnvelopeParams(*[float(x) for x in envelope]))
        if self.L.gh_set_sample_envelope(self.h, env):
            raise RuntimeError(self.L.gh_last_error(self.h).decode())

    def sample_envelope(self):
        out = T.EnvelopeParams()
        return (out.attack, out.decay, out.sustain, out.release) if self.L.gh_sample_envelope(self.h, C.byref(out)) else None

    def set_sample_loop(self, uid, start, end):
        """The forward loop [start, end), in frames, of the sampler `uid` (add_sampler's return); 0, 0 clears it."""
        if self.L.gh_set_sample_loop(self.h, uid, start, end):
            raise RuntimeError(self.L.gh_last_error(self.h).decode())

    def add_effect(self, kind, params): return self.L.gh_add_effect(self.h, kind, C.byref(params))
    def patch(self, source, sink): return self.L.gh_patch(self.h, source, sink)

    def patch_chain_to_main_mixer(self, uids):
        arr = (C.c_int * len(uids))(*uids)
        return self.L.gh_patch_chain_to_main_mixer(self.h, arr, len(uids))

    def unpatch_all(self): self.L.gh_unpatch_all(self.h)
    def set_fused_direct(self, on):
        """Instruments patched straight into the main mixer render fused onto the bus (default) or through their blocks."""
        self.L.gh_set_fused_direct(self.h, 1 if on else 0)

    def set_filter_links_on_device(self, on):
        """Links made from here on onto a filter's cutoff, q or passband-ripple derive the coefficients on the device (no host wait per
        block), from an LFO or a signal source; off (the default): an LFO goes through the host once per block, a signal source is dropped."""
        self.L.gh_set_filter_links_on_device(self.h, 1 if on else 0)

    def set_trips_on_device(self, on):
        """Control trips onto effect parameters the library can reach stay on the device (no host wait per automated block); decided for
        all trips when a run starts — control_trip_on_device(uid) says how it went.  Off by default."""
        self.L.gh_set_trips_on_device(self.h, 1 if on else 0)

    def set_instrument_controls_on_device(self, on):
        """Control trips and LFO `controls` links onto an instrument's controls — a Welsh synth's dca-gain, dca-pan or filter-cutoff, an
        FM synth's dca-gain, dca-pan, depth or beta, a sampler's or drumkit's gain — stay on the device (no re-upload of the instrument's
        bank, and no host wait, per automated block).  Trips are decided when a run starts — control_trip_on_device(uid)
        says how it went — LFO links when they are made, so set it before link_control.  Off by default; independent of
        set_trips_on_device."""
        self.L.gh_set_instrument_controls_on_device(self.h, 1 if on else 0)

    def set_wet_links_on_device(self, on):
        """Controls onto an effect's wet-dry-mix stay on the device: link_control links an LFO or a signal source onto it there (a signal
        source is dropped without), and — with set_trips_on_device — a trip onto it is device-resident and no longer keeps the effect's
        other trips on the host.  Off by default; set it before link_control."""
        self.L.gh_set_wet_links_on_device(self.h, 1 if on else 0)

    def wet_links_on_device(self): return bool(self.L.gh_wet_links_on_device(self.h))

    def set_wet_reverb_run(self, on):
        """The library's groove_set_fx_wet_reverb_run: a partly wet reverb keeps the fused run's kernel forms (same bits).  Off by default."""
        self._chk(self.L.gh_set_wet_reverb_run(self.h, 1 if on else 0))

    def wet_reverb_run(self): return bool(self.L.gh_wet_reverb_run(self.h))

    def control_trip_on_device(self, uid):
        """1: the trip has been device-resident since the last run started; 0: it goes through the host."""
        return self.L.gh_control_trip_on_device(self.h, uid)

    def debug_info(self):
        """groove_debug_info of the orchestrator's context, parsed (it waits for the ctx stream)."""
        import json
        buf = C.create_string_buffer(1 << 16)
        self._chk(self.L.gh_debug_info(self.h, buf, len(buf)))
        return json.loads(buf.value.decode())

    def set_render_ahead(self, on):
        """Offline runs: False = block by block, True = instruments one block ahead of the effects whenever the graph allows
        (the default, "auto", does so only for instruments whose render is long enough to be worth the hand-over)."""
        self.L.gh_set_render_ahead(self.h, 2 if on else 0)
    def connect_midi_downstream(self, uid, channel): self._chk(self.L.gh_connect_midi_downstream(self.h, uid, channel))
    def add_timer(self, beats): return self.L.gh_add_timer(self.h, beats)
    def add_sequencer(self): return self.L.gh_add_sequencer(self.h)

    def sequencer_insert(self, uid, channel, key, start_beat, duration_beats):
        self._chk(self.L.gh_sequencer_insert(self.h, uid, channel, key, start_beat, duration_beats))

    def sequencer_set_end(self, uid, beats): self._chk(self.L.gh_sequencer_set_end(self.h, uid, beats))

    def add_control_trip(self, target, param, start_beat=0.0):
        uid = self.L.gh_add_control_trip(self.h, target, param.encode(), start_beat)
        if uid < 0:
            raise RuntimeError(self.L.gh_last_error(self.h).decode())
        return uid

    def control_trip_add_step(self, uid, kind, start, end, beats):
        self._chk(self.L.gh_control_trip_add_step(self.h, uid, kind, start, end, beats))

    def add_lfo_controller(self, waveform, frequency_hz, duty=0.5):
        """LfoController{waveform, frequency}: a controller device whose links are worked once per block."""
        uid = self.L.gh_add_lfo_controller(self.h, waveform, duty, frequency_hz)
        if uid < 0:
            raise RuntimeError(self.L.gh_last_error(self.h).decode())
        return uid

    def add_signal_passthrough(self):
        """SignalPassthroughController: patchable like an effect (identity, one lane); the source of a sidechain link."""
        return self.L.gh_add_signal_passthrough(self.h)

    def link_control(self, source, target, param):
        """Orchestrator::link_control.  True: linked; False: dropped (a signal source onto a parameter only the host can derive —
        last_error() says why); raises on an error."""
        rc = self.L.gh_link_control(self.h, source, target, param.encode())
        if rc == 1:
            raise RuntimeError(self.L.gh_last_error(self.h).decode())
        return rc == 0

    def last_error(self): return self.L.gh_last_error(self.h).decode()

    def last_allocated_voice(self, uid): return self.L.gh_last_allocated_voice(self.h, uid)

    def gather_audio(self, frames):
        out = np.zeros((frames, 2), dtype=np.float32)
        self._chk(self.L.gh_gather_audio(self.h, frames, out.ctypes.data_as(_fp)))
        return out

    def performance_frames(self): return self.L.gh_performance_frames(self.h)

    def run(self, buffer_frames=64, performance=False):
        cap = self.performance_frames() + buffer_frames
        out = np.zeros((cap, 2), dtype=np.float32)
        n = self.L.gh_run(self.h, buffer_frames, out.ctypes.data_as(_fp), cap, 1 if performance else 0)
        if n < 0:
            raise RuntimeError(self.L.gh_last_error(self.h).decode())
        return out[:n]

    def render_to_wav(self, path, buffer_frames=256):
        self._chk(self.L.gh_render_to_wav(self.h, buffer_frames, path.encode()))

    def close(self):
        if self.h:
            self.L.gh_orchestrator_free(self.h)
            self.h = None
