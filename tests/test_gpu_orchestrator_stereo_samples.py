"""GPU tier, through the host layer: `groove-cli-hip --stereo-samples` (Orchestrator::set_stereo_samples) keeps the channels of
two-channel sample files — a `sampler` on one is a stereo bank, a `drumkit` with one is a stereo bank whose mono files are on both
channels — and without the flag a stereo file is the mean of its channels, as before.

The oracle's sampler is mono.  THE CHANNEL TRICK: nothing in the project below crosses channels (two samplers, a gain, a Welsh synth, the
main mixer; no controller device, whose signal passthrough would read (L + R) / 2), so the LEFT channel of the stereo render is the left
channel of the oracle graph whose stereo sampler's bank is the file's LEFT channel as a mono file, and likewise on the right: +-1 LSB of
the 16-bit stream, tests/test_gpu_orchestrator.py's bar."""
import math
import os
import subprocess

import numpy as np
import pytest

from groove_amd import abi_types as T, patches as P
from tests.test_gpu_orchestrator import _mono_float, _quantise, _wav_bytes

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(REPO, "groove_amd", "host", "groove-cli-hip")
BPM, SR, UPB, BLOCK = 240.0, 44100, 65536, 256
ROOT_C4 = 261.6255653005986

PROJECT = """{
  title: "a stereo sampler, a mono sampler behind a gain, a Welsh synth", clock: {bpm: 240, "time-signature": [4, 4]},
  devices: [
    {instrument: ["s-stereo", {sampler: [{"midi-in": 0}, {filename: "st.wav", root: 261.6255653005986}]}]},
    {instrument: ["s-mono", {sampler: [{"midi-in": 1}, {filename: "mono.wav", root: 440.0}]}]},
    {instrument: ["raw-1", {"welsh-raw": [{"midi-in": 2}, {
        voice: {"oscillator-1": {waveform: {"pulse-width": 0.3}, "frequency-tune": 1.0},
                "oscillator-2": {waveform: "sawtooth", "frequency-tune": {osc: {octave: -1, semi: 0, cent: 4}}},
                "oscillator-2-sync": false, "oscillator-mix": 0.6,
                "amp-envelope": {attack: 0.01, decay: 0.2, sustain: 0.7, release: 0.3},
                lfo: {waveform: "square", frequency: 5.13}, "lfo-routing": "pitch", "lfo-depth": 0.05,
                filter: {cutoff: 900, "passband-ripple": 1.2}, "filter-cutoff-start": 0.4, "filter-cutoff-end": 0.5,
                "filter-envelope": {attack: 0.0, decay: 0.5, sustain: 0.3, release: 0.5}},
        dca: {gain: 0.8, pan: -0.25}}]}]},
    {effect: ["gain-1", {gain: {ceiling: 0.5}}]},
  ],
  "patch-cables": [["s-stereo", "main-mixer"], ["s-mono", "gain-1", "main-mixer"], ["raw-1", "main-mixer"]],
  patterns: [
    {id: "a0", "note-value": "quarter", notes: [[60, 64, 0, 67], [0, 72, 0, 0]]},
    {id: "a1", "note-value": "eighth", notes: [[55, 0, 60, 0, 62, 62, 0, 48]]},
    {id: "b0", "note-value": "eighth", notes: [[69, 71, 0, 0, 57, 0, 0, 0]]},
    {id: "b1", "note-value": "quarter", notes: [[0, 76, 69, 0]]},
    {id: "c0", "note-value": "quarter", notes: [[50, 62, 0, 55]]},
    {id: "c1", "note-value": "quarter", notes: [[57, 0, 45, 0]]},
  ],
  tracks: [{id: "t0", "midi-channel": 0, patterns: ["a0", "a1"]}, {id: "t1", "midi-channel": 1, patterns: ["b0", "b1"]},
           {id: "t2", "midi-channel": 2, patterns: ["c0", "c1"]}],
}"""
# channel: its track's patterns, one measure each: (beats per note, rows)
PATTERNS = {0: [(1.0, [[60, 64, 0, 67], [0, 72, 0, 0]]), (0.5, [[55, 0, 60, 0, 62, 62, 0, 48]])],
            1: [(0.5, [[69, 71, 0, 0, 57, 0, 0, 0]]), (1.0, [[0, 76, 69, 0]])],
            2: [(1.0, [[50, 62, 0, 55]]), (1.0, [[57, 0, 45, 0]])]}


def _files():
    """st.wav: 16-bit stereo, left a decaying sine, right the same an octave up; mono.wav: 16-bit mono."""
    n = np.arange(9000)
    env = np.exp(-n / 3000.0)
    left = (9000 * np.sin(2 * np.pi * n / 168.5) * env).astype(np.int64)
    right = (9000 * np.sin(2 * np.pi * n / 84.25) * env).astype(np.int64)
    mono = (8000 * np.sin(2 * np.pi * 3.0 * n[:7000] / 147.0) * np.exp(-n[:7000] / 2500.0)).astype(np.int64)
    return left, right, mono


def _events():
    """(units, insertion index, channel, key, on): the loader inserts track by track, pattern by pattern (a measure each), row by row; the
    sequencer keeps time order, equal times in insertion order."""
    events = []
    for ch, pats in PATTERNS.items():
        for measure, (beats, rows) in enumerate(pats):
            for row in rows:
                for i, k in enumerate(row):
                    if k:
                        events.append((int((4 * measure + i * beats) * UPB + 0.5), len(events), ch, k, True))
                        events.append((int((4 * measure + i * beats + beats) * UPB + 0.5), len(events), ch, k, False))
    events.sort(key=lambda e: (e[0], e[1]))
    return events


class _Alloc:   # VoiceBankInstrument::note_on / note_off restated (first idle voice, busy until note-off + release, steal the oldest)
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


def _oracle_render(oracle, stereo_file_as_mono, mono_pcm, total):
    """The project on the oracle graph, the stereo sampler's bank being the given MONO buffer; the quantised 16-bit stream [total][2]."""
    g = oracle.Graph(SR)
    g.set_bpm(BPM)

    def sampler(pcm, root_hz):
        descs = (T.SampleDesc * 1)(T.SampleDesc(0, len(pcm), root_hz))
        sp = (T.SamplerParams * 8)()
        for k in range(8):
            sp[k].sample_index, sp[k].one_shot, sp[k].gain = 0, 0, 1.0
        return g.add_instrument(oracle.Bank.sampler(pcm, descs, sp, SR))

    inst = {0: (sampler(stereo_file_as_mono, ROOT_C4), _Alloc(8, 0.0)), 1: (sampler(mono_pcm, 440.0), _Alloc(8, 0.0))}
    wp = T.WelshParams()
    wp.oscillator_1.waveform, wp.oscillator_1.duty, wp.oscillator_1.tune = T.WAVE_PULSE_WIDTH, 0.3, 1.0
    wp.oscillator_2.waveform, wp.oscillator_2.duty, wp.oscillator_2.tune = T.WAVE_SAWTOOTH, 0.5, P.semis_and_cents(-12, 4.0)
    wp.oscillator_2_sync, wp.oscillator_mix = 0, 0.6
    wp.amp_envelope, wp.filter_envelope = T.EnvelopeParams(0.01, 0.2, 0.7, 0.3), T.EnvelopeParams(0.0, 0.5, 0.3, 0.5)
    wp.lfo_waveform, wp.lfo_routing, wp.lfo_frequency, wp.lfo_depth = T.WAVE_SQUARE, T.LFO_PITCH, 5.13, 0.05
    wp.filter_cutoff_hz, wp.filter_passband_ripple, wp.filter_cutoff_start, wp.filter_cutoff_end = 900.0, 1.2, 0.4, 0.5
    wp.dca_gain, wp.dca_pan = 0.8, -0.25
    inst[2] = (g.add_instrument(oracle.Bank.welsh((T.WelshParams * 8)(*[wp] * 8))), _Alloc(8, 0.3))
    gain = g.add_effect(T.FX_GAIN, T.fx_params(ceiling=0.5))
    assert g.patch(inst[0][0], g.MAIN_MIXER) == 0 and g.patch(inst[1][0], gain) == 0 and g.patch(gain, g.MAIN_MIXER) == 0
    assert g.patch(inst[2][0], g.MAIN_MIXER) == 0
    events, want, pos = _events(), [], 0
    while pos < total:
        t0, t1 = int(pos * BPM / 60.0 / SR * UPB), int((pos + BLOCK) * BPM / 60.0 / SR * UPB)
        for at, _, ch, key, on in events:
            if t0 <= at < t1:
                u, al = inst[ch]
                for ev in (al.on(key, pos) if on else al.off(key, pos)):
                    g.note_events(u, T.note_events([ev]))
        want.append(g.tick(BLOCK)); pos += BLOCK
    return _quantise(oracle, np.concatenate(want, axis=0))


def _render(tmp_path, proj, flags):
    r = subprocess.run([CLI, "--wav", "--assets", str(tmp_path)] + flags + [str(proj)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    raw = (tmp_path / (proj.stem + ".wav")).read_bytes()
    return np.frombuffer(raw[44:], dtype="<i2").reshape(-1, 2).astype(np.int32)


def test_cli_renders_a_stereo_sampler_in_stereo_with_the_flag_and_averaged_without(tmp_path, oracle):
    left, right, mono = _files()
    (tmp_path / "samples").mkdir()
    (tmp_path / "samples" / "st.wav").write_bytes(_wav_bytes(np.stack([left, right], axis=1).ravel(), 2, 16))
    (tmp_path / "samples" / "mono.wav").write_bytes(_wav_bytes(mono, 1, 16))
    proj = tmp_path / "stereo.json5"
    proj.write_text(PROJECT)
    total = math.ceil(8.0 * 60 / BPM * SR)                # two measures
    total -= total % BLOCK                                # run_performance drops the partial block
    mono_pcm = _mono_float(mono, 1, 16)
    want_l = _oracle_render(oracle, _mono_float(left, 1, 16), mono_pcm, total)
    want_r = _oracle_render(oracle, _mono_float(right, 1, 16), mono_pcm, total)
    want_avg = _oracle_render(oracle, _mono_float(np.stack([left, right], axis=1).ravel(), 2, 16), mono_pcm, total)

    got = _render(tmp_path, proj, ["--stereo-samples"])
    assert got.shape == (total, 2) and np.abs(got).max() > 2000
    dl, dr = int(np.max(np.abs(got[:, 0] - want_l[:, 0]))), int(np.max(np.abs(got[:, 1] - want_r[:, 1])))
    print(f"--stereo-samples: max |got - oracle| = {dl} LSB (left), {dr} LSB (right)")
    assert dl <= 1 and dr <= 1, (dl, dr)
    assert np.max(np.abs(got[:, 0] - want_avg[:, 0])) > 100 and np.max(np.abs(got[:, 1] - want_avg[:, 1])) > 100   # not the averaged render

    plain = _render(tmp_path, proj, [])                   # the parent's behaviour, re-asserted
    d = int(np.max(np.abs(plain - want_avg)))
    print(f"without the flag: max |got - oracle on the averaged file| = {d} LSB")
    assert plain.shape == (total, 2) and d <= 1, d


# ---------------------------------------------------------------------------------------------------------------- drumkit
KIT = {35: "Kick 1 R1.wav", 36: "Kick 2 R1.wav", 37: "Rim R1.wav", 38: "Snare 1 R1.wav", 39: "Clap R1.wav", 40: "Snare 2 R1.wav", 41: "Tom 1 R1.wav",
       42: "Hat Closed R1.wav", 43: "Tom 1 R1.wav", 44: "Hat Closed R1.wav", 45: "Tom 2 R1.wav", 46: "Hat Open R1.wav", 47: "Tom 2 R1.wav",
       48: "Tom 3 R1.wav", 49: "Crash R1.wav", 50: "Tom 3 R1.wav", 51: "Ride R1.wav", 54: "Tambourine R1.wav", 56: "Cowbell R1.wav"}
STEREO_FILES = ("Snare 1 R1.wav", "Hat Open R1.wav", "Crash R1.wav")
KIT_ROWS = ([46, 0, 42, 38, 46, 0, 49, 44], [36, 0, 0, 36, 0, 0, 40, 0], [0, 0, 49, 0, 56, 45, 0, 38])   # eighth notes, one measure
KIT_PROJECT = """{
  title: "a 707 kit with three stereo files", clock: {bpm: 240, "time-signature": [4, 4]},
  devices: [{instrument: ["kit", {drumkit: [{"midi-in": 10}, {name: "707"}]}]}],
  "patch-cables": [["kit", "main-mixer"]],
  patterns: [{id: "p", "note-value": "eighth", notes: [[46, 0, 42, 38, 46, 0, 49, 44], [36, 0, 0, 36, 0, 0, 40, 0], [0, 0, 49, 0, 56, 45, 0, 38]]}],
  tracks: [{id: "t", "midi-channel": 10, patterns: ["p"]}],
}"""


def _kit_files():
    """name: (ints, channels): tiny 16-bit files, every one its own length and pitch; the stereo ones with different channels."""
    out = {}
    for j, name in enumerate(sorted(set(KIT.values()))):
        n = np.arange(700 + 130 * j)
        tone = lambda period: (9000 * np.sin(2 * np.pi * n / period) * np.exp(-n / 400.0)).astype(np.int64)
        if name in STEREO_FILES:
            out[name] = (np.stack([tone(23.0 + 3 * j), -tone(31.0 + 2 * j)], axis=1).ravel(), 2)
        else:
            out[name] = (tone(20.0 + 4 * j), 1)
    return out


def _kit_numpy(oracle, files, stereo, total):
    """Drum by drum: a note-on in a block restarts the drum's sample at the block's first frame (one-shot, step 1, gain 1); the f64 sum of
    the drums' fp32 values, quantised."""
    bus = np.zeros((total, 2))
    starts = {}                                            # key: block starts of its note-ons
    for row in KIT_ROWS:
        for i, k in enumerate(row):
            if k:
                at = int(i * 0.5 * UPB + 0.5)
                pos = 0
                while not (int(pos * BPM / 60.0 / SR * UPB) <= at < int((pos + BLOCK) * BPM / 60.0 / SR * UPB)):
                    pos += BLOCK
                starts.setdefault(k, set()).add(pos)
    for key, at in starts.items():
        ints, ch = files[KIT[key]]
        x = np.asarray(ints, dtype=np.int64).reshape(-1, ch) / 32768.0
        if stereo:
            pcm = x.astype(np.float32) if ch == 2 else np.repeat(x.astype(np.float32), 2, axis=1)
        else:
            pcm = np.repeat(_mono_float(ints, ch, 16)[:, None], 2, axis=1)
        at = sorted(p for p in at if p < total)
        for j, p in enumerate(at):                         # a re-trigger cuts the earlier hit off
            end = min(p + len(pcm), at[j + 1] if j + 1 < len(at) else total, total)
            bus[p:end] += pcm[:end - p].astype(np.float64)
    return _quantise(oracle, bus)


def test_cli_renders_a_kit_with_stereo_files_in_stereo_with_the_flag(tmp_path, oracle):
    files = _kit_files()
    kit_dir = tmp_path / "samples" / "elphnt.io" / "707"
    kit_dir.mkdir(parents=True)
    for name, (ints, ch) in files.items():
        (kit_dir / name).write_bytes(_wav_bytes(ints, ch, 16))
    proj = tmp_path / "kit.json5"
    proj.write_text(KIT_PROJECT)
    total = math.ceil(4.0 * 60 / BPM * SR)
    total -= total % BLOCK
    got = _render(tmp_path, proj, ["--stereo-samples"])
    want = _kit_numpy(oracle, files, True, total)
    assert got.shape == want.shape == (total, 2) and np.abs(got).max() > 2000
    assert np.max(np.abs(got[:, 0] - got[:, 1])) > 1000                                    # the channels differ ...
    d = int(np.max(np.abs(got - want)))
    print(f"kit, --stereo-samples: max |got - numpy| = {d} LSB")
    assert d <= 1, d
    plain = _render(tmp_path, proj, [])                                                    # ... and without the flag it is the mono render
    want_mono = _kit_numpy(oracle, files, False, total)
    assert np.array_equal(plain[:, 0], plain[:, 1])
    d = int(np.max(np.abs(plain - want_mono)))
    print(f"kit, without the flag: max |got - numpy| = {d} LSB")
    assert d <= 1, d
    synthetic = _render(tmp_path, proj, ["--stereo-samples", "--synthetic-kit"])           # --synthetic-kit stays mono
    assert np.array_equal(synthetic[:, 0], synthetic[:, 1]) and np.abs(synthetic).max() > 500
