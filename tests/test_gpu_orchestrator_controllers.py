"""GPU tier: controller devices through the compiled host layer (groove_amd/host/) — an LFO and a signal passthrough, linked to
parameters by a project's `controls` section or by Orchestrator::link_control.

The synthetic sidechain project below is this test's own text in the reference's schema: a sampler (from a WAV file the test writes)
through a passthrough into the main mixer, a raw Welsh synth through a compressor, and one `controls` entry that puts the passthrough's
value on the compressor's threshold."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from groove_amd import patches as P, abi_types as T
from tests.test_ctl_core_cpu import _closed_form, _delta64, signal_law_np
from tests.test_gpu_orchestrator import _wav_bytes, _mono_float, _quantise

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT_HZ = 261.6255653005986          # key 60: the sampler steps through its buffer one frame per frame

SIDECHAIN = """{
  title: "synthetic sidechain", clock: {bpm: 120, "time-signature": [4, 4]},
  devices: [
    {instrument: ["thump", {sampler: [{"midi-in": 0}, {filename: "thump.wav", root: 261.6255653005986}]}]},
    {instrument: ["pad", {"welsh-raw": [{"midi-in": 1}, {
        voice: {"oscillator-1": {waveform: {"pulse-width": 0.3}, "frequency-tune": 1.0},
                "oscillator-2": {waveform: "sawtooth", "frequency-tune": {osc: {octave: -1, semi: 0, cent: 4}}},
                "oscillator-2-sync": false, "oscillator-mix": 0.6,
                "amp-envelope": {attack: 0.01, decay: 0.2, sustain: 0.7, release: 0.3},
                lfo: {waveform: "square", frequency: 5.13}, "lfo-routing": "pitch", "lfo-depth": 0.05,
                filter: {cutoff: 900, "passband-ripple": 1.2}, "filter-cutoff-start": 0.4, "filter-cutoff-end": 0.5,
                "filter-envelope": {attack: 0.0, decay: 0.5, sustain: 0.3, release: 0.5}},
        dca: {gain: 0.8, pan: -0.25}}]}]},
    {effect: ["duck", {compressor: {threshold: 0.6, ratio: 0.25, attack: 0, release: 0}}]},
    {controller: ["tap", {"signal-passthrough-controller": [{"midi-in": 0, "midi-out": 0}]}]},
  ],
  "patch-cables": [["thump", "tap", "main-mixer"], ["pad", "duck", "main-mixer"]],
  %s
  patterns: [
    {id: "kick", "note-value": "eighth", notes: [[60, 0, 60, 60, 0, 60, 0, 60]]},
    {id: "chord", "note-value": "half", notes: [[50, 55], [62, 0]]},
  ],
  tracks: [{id: "t0", "midi-channel": 0, patterns: ["kick"]}, {id: "t1", "midi-channel": 1, patterns: ["chord"]}],
}"""
CONTROLS = 'controls: [{id: "duck-the-pad", source: "tap", target: {id: "duck", param: "threshold"}}],'
PATTERNS = {0: (0.5, [[60, 0, 60, 60, 0, 60, 0, 60]]), 1: (2.0, [[50, 55], [62, 0]])}
BPM, SR, UPB, BLOCK = 120.0, 44100, 65536, 256


def _thump():
    n = np.arange(5000)
    return (14000 * np.sin(2 * np.pi * n / 97.3) * np.exp(-n / 1500.0) + 9000 * np.exp(-n / 400.0)).astype(np.int64)


def _write_project(tmp_path, controls=CONTROLS):
    (tmp_path / "samples").mkdir(exist_ok=True)
    (tmp_path / "samples" / "thump.wav").write_bytes(_wav_bytes(_thump(), 1, 16))
    proj = tmp_path / ("sidechain.json5" if controls else "plain.json5")
    proj.write_text(SIDECHAIN % controls)
    return proj


def _render(proj, assets, render_ahead, fused_direct):
    from groove_amd import host_binding as H
    o = H.Orchestrator(0, SR, BPM)
    try:
        o.L.gh_load_project.restype, o.L.gh_load_project.argtypes = C.c_int, [C.c_void_p, C.c_char_p, C.c_char_p, C.c_int]
        assert o.L.gh_load_project(o.h, str(proj).encode(), str(assets).encode(), 0) == 0, o.last_error()
        o.set_render_ahead(render_ahead)
        o.set_fused_direct(fused_direct)
        return o.run(BLOCK)
    finally:
        o.close()


def test_sidechain_project_same_samples_from_every_walk(tmp_path):
    proj = _write_project(tmp_path)
    runs = {(ra, fd): _render(proj, tmp_path, ra, fd) for ra in (False, True) for fd in (True, False)}
    base = runs[(False, True)]
    assert len(base) == math.ceil(4.0 * 60 / BPM * SR) and np.abs(base).max() > 0.05
    for key, got in runs.items():
        assert np.array_equal(got.view(np.uint32), base.view(np.uint32)), key
    # ... and the link is heard: the same project without its `controls` section renders something else
    plain = _render(_write_project(tmp_path, ""), tmp_path, False, True)
    assert plain.shape == base.shape and np.max(np.abs(plain - base)) > 1e-3


class _Alloc:
    """VoiceBankInstrument::note_on / note_off restated (first idle voice, busy until note-off + release, steal the oldest)."""

    def __init__(self, voices, release_seconds):
        self.key, self.busy, self.started, self.rel = [-1] * voices, [0] * voices, [0] * voices, math.ceil(release_seconds * SR) + 1

    def on(self, key, now):
        m = len(self.key)
        v = next((i for i in range(m) if self.key[i] < 0 and self.busy[i] <= now), None)
        if v is None:
            v = min(range(m), key=lambda i: self.started[i])
        self.key[v], self.started[v], self.busy[v] = key, now, 1 << 62
        return [(v, key, True)]

    def off(self, key, now):
        out = []
        for i in range(len(self.key)):
            if self.key[i] == key:
                out.append((i, key, False)); self.key[i] = -1; self.busy[i] = now + self.rel
        return out


def _pad_patch():
    wp = T.WelshParams()
    wp.oscillator_1.waveform, wp.oscillator_1.duty, wp.oscillator_1.tune = T.WAVE_PULSE_WIDTH, 0.3, 1.0
    wp.oscillator_2.waveform, wp.oscillator_2.duty, wp.oscillator_2.tune = T.WAVE_SAWTOOTH, 0.5, P.semis_and_cents(-12, 4.0)
    wp.oscillator_2_sync, wp.oscillator_mix = 0, 0.6
    wp.amp_envelope, wp.filter_envelope = T.EnvelopeParams(0.01, 0.2, 0.7, 0.3), T.EnvelopeParams(0.0, 0.5, 0.3, 0.5)
    wp.lfo_waveform, wp.lfo_routing, wp.lfo_frequency, wp.lfo_depth = T.WAVE_SQUARE, T.LFO_PITCH, 5.13, 0.05
    wp.filter_cutoff_hz, wp.filter_passband_ripple, wp.filter_cutoff_start, wp.filter_cutoff_end = 900.0, 1.2, 0.4, 0.5
    wp.dca_gain, wp.dca_pan = 0.8, -0.25
    return wp


def test_cli_renders_the_sidechain_project_within_one_lsb_of_the_oracle_composition(tmp_path, oracle):
    """groove-cli-hip --wav against the oracle's pieces put together the way the project says: the sampler's bus is passed on as it is
    and its last frame of block b - 1 gives (numpy float32 law, bipolar) the threshold the oracle's compressor is given for block b."""
    proj = _write_project(tmp_path)
    cli = os.path.join(REPO, "groove_amd", "host", "groove-cli-hip")
    r = subprocess.run([cli, "--wav", "--assets", str(tmp_path), str(proj)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "Warning" not in r.stderr, r.stderr
    raw = (tmp_path / "sidechain.wav").read_bytes()
    pcm16 = np.frombuffer(raw[44:], dtype="<i2").reshape(-1, 2).astype(np.int32)
    total = math.ceil(4.0 * 60 / BPM * SR)
    total -= total % BLOCK                                # run_performance drops the partial block
    assert len(pcm16) == total and np.abs(pcm16).max() > 2000

    pcm = _mono_float(_thump(), 1, 16)
    sp = (T.SamplerParams * 8)()
    for k in range(8):
        sp[k].sample_index, sp[k].one_shot, sp[k].gain = 0, 0, 1.0
    banks = {0: (oracle.Bank.sampler(pcm, (T.SampleDesc * 1)(T.SampleDesc(0, len(pcm), ROOT_HZ)), sp, SR), _Alloc(8, 0.0)),
             1: (oracle.Bank.welsh((T.WelshParams * 8)(*[_pad_patch()] * 8)), _Alloc(8, 0.3))}
    comp = lambda thr: (T.FxParams * 1)(T.fx_params(limit_min=float(thr), limit_max=0.25))
    ofx = oracle.Fx(T.FX_COMPRESSOR, comp(0.6))
    events = []
    for ch, (beats, rows) in PATTERNS.items():
        for row in rows:
            for i, k in enumerate(row):
                if k:
                    events.append((int(i * beats * UPB + 0.5), len(events), ch, k, True))
                    events.append((int((i * beats + beats) * UPB + 0.5), len(events), ch, k, False))
    events.sort(key=lambda e: (e[0], e[1]))
    want, pos, thr, thresholds = [], 0, None, []
    while pos < total:
        t0, t1 = int(pos * BPM / 60.0 / SR * UPB), int((pos + BLOCK) * BPM / 60.0 / SR * UPB)
        for at, _, ch, key, on in events:
            if t0 <= at < t1:
                bank, al = banks[ch]
                for ev in (al.on(key, pos) if on else al.off(key, pos)):
                    bank.note_events(T.note_events([ev]))
        if thr is not None:                                # the control phase: what the passthrough captured from the block before
            ofx.set_params(comp(thr))
            thresholds.append(float(thr))
        drums = banks[0][0].render_bus(BLOCK)
        pad = banks[1][0].render(BLOCK).sum(axis=2, keepdims=True)
        want.append(drums + oracle.mix(ofx.process(np.ascontiguousarray(pad))))
        last = drums[BLOCK - 1].astype(np.float32)
        _, v = signal_law_np(T.CTL_LAW_BIPOLAR, last[0:1], last[1:2])
        thr = v[0]
        pos += BLOCK
    assert np.ptp(thresholds) > 0.2                        # the threshold really moves with the drums
    want = _quantise(oracle, np.concatenate(want, axis=0))
    assert want.shape == pcm16.shape
    assert np.max(np.abs(pcm16 - want)) <= 1, int(np.max(np.abs(pcm16 - want)))


def test_lfo_onto_a_welsh_synths_pan_follows_the_oracle_bank(oracle):
    """An LFO linked to an instrument's `pan` goes through Orchestrator::control_effect once per block with the law evaluated on the host
    in f64; the oracle's bank is given the closed form at the same block starts.  The bar is the one
    test_control_trip_onto_an_instrument_reaches_its_voices holds a trip onto `dca-pan` to."""
    from groove_amd import host_binding as H
    patch = P.welsh_patch(3)
    freq = 2.0
    o = H.Orchestrator(0, SR, BPM)
    try:
        w = o.add_welsh(patch, voices=4)
        assert o.patch(w, o.MAIN_MIXER) == 0
        o.connect_midi_downstream(w, 0)
        seq = o.add_sequencer()
        for k, s_, d in ((60, 0.0, 1.9), (64, 0.5, 1.0)):
            o.sequencer_insert(seq, 0, k, s_, d)
        o.sequencer_set_end(seq, 2.0)
        lfo = o.add_lfo_controller(T.WAVE_TRIANGLE, freq)
        assert o.link_control(lfo, w, "pan") is True
        with pytest.raises(RuntimeError, match="unknown control name"):
            o.link_control(lfo, w, "no-such-control")
        with pytest.raises(RuntimeError, match="not a controller device"):
            o.link_control(w, w, "pan")
        with pytest.raises(RuntimeError, match="LFO"):
            o.add_lfo_controller(T.WAVE_NOISE, 1.0)
        # a signal source onto a parameter only the host can derive is dropped, with the reason
        tap, lp = o.add_signal_passthrough(), o.add_effect(T.FX_BIQUAD_LP12, T.fx_params())
        assert o.link_control(tap, lp, "cutoff") is False and "download per block" in o.last_error()
        got = o.run(BLOCK).astype(np.float64)
    finally:
        o.close()
    total = math.ceil(2.0 * 60 / BPM * SR)
    assert len(got) == total
    ob = oracle.Bank.welsh((T.WelshParams * 4)(*[patch] * 4))
    evs = sorted([(int(0.0 * UPB + 0.5), 0, 0, 60, True), (int(1.9 * UPB + 0.5), 1, 0, 60, False), (int(0.5 * UPB + 0.5), 2, 1, 64, True), (int(1.5 * UPB + 0.5), 3, 1, 64, False)])
    want, pos, pans = [], 0, []
    while pos < total:
        fr = min(BLOCK, total - pos)
        t0, t1 = int(pos * BPM / 60.0 / SR * UPB), int((pos + fr) * BPM / 60.0 / SR * UPB)
        for at, _, v, key, on in evs:
            if t0 <= at < t1:
                ob.note_events(T.note_events([(v, key, on)]))
        val = (_closed_form("triangle", (_delta64(freq, SR) * pos) % 2 ** 64) + 1.0) * 0.5
        ob.set_param(T.CTL_WELSH_DCA_PAN, val)
        pans.append(val)
        want.append(ob.render_bus(fr)); pos += fr
    want = np.concatenate(want, axis=0)
    assert np.sqrt(np.mean(want ** 2)) > 1e-2 and np.ptp(pans) > 0.9
    assert np.sqrt(np.mean((got - want) ** 2)) <= 1e-5
