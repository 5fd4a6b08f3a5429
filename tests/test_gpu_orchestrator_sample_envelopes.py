"""GPU tier, through the host layer: `groove-cli-hip --sample-envelope A,D,S,R` (Orchestrator::set_sample_envelope) gives a sampler an
amplitude envelope on its sample (groove_bank_set_sample_envelopes) and keeps a voice busy through its release, so the next note takes
another voice while the tail sounds; without the switch a project renders what it rendered before.

The project: one sampler on a WAV the test writes — 9,000 frames with a forward `smpl` loop [6000, 8000) — playing key 64 twice, two
eighth notes back to back at 120 bpm (11,025 frames each), run with `--sample-loops --sample-envelope 0.002,0.003,0.6,0.02`: the second
note starts in the block in which the first is released, 882 frames of release (529 from the sustain level) before the first is idle.
The reference is numpy and plain Python, docs/DSP_SPEC.md section 7 restated (tests/test_gpu_sampler_envelopes.py's envelope, an exact
integer cursor with the fold), the sequencer's block-granular events and VoiceBankInstrument's allocation rule restated as
tests/test_gpu_orchestrator.py's `Alloc` does: first idle voice, busy until note-off + ceil(release * SR) + 1 frames.  At most two
voices sound at once, each an fp32 value: the 16-bit stream is held to 1 LSB."""
import math
import os
import subprocess

import numpy as np
import pytest

from tests.test_gpu_orchestrator import _mono_float, _quantise, _wav_bytes
from tests.test_gpu_orchestrator_sample_loops import _smpl_chunk
from tests.test_gpu_sampler_envelopes import IDLE, _Env

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(REPO, "groove_amd", "host", "groove-cli-hip")
BPM, SR, UPB, BLOCK = 120.0, 44100, 65536, 256
FRAMES, LOOP, KEY, VOICES = 9000, (6000, 8000), 64, 8
ENV = (0.002, 0.003, 0.6, 0.02)
PROJECT = """{
  title: "a sampler playing one key twice", clock: {bpm: 120, "time-signature": [4, 4]},
  devices: [
    {instrument: ["s", {sampler: [{"midi-in": 0}, {filename: "pad.wav", root: 440.0}]}]},
  ],
  "patch-cables": [["s", "main-mixer"]],
  patterns: [
    {id: "a0", "note-value": "eighth", notes: [[64, 64, 0, 0, 0, 0, 0, 0]]},
  ],
  tracks: [{id: "t0", "midi-channel": 0, patterns: ["a0"]}],
}"""


class _Alloc:   # VoiceBankInstrument::note_on / note_off restated (first idle voice, busy until note-off + release, steal the oldest)
    def __init__(self, voices, release_seconds):
        self.key, self.busy, self.started, self.rel = [-1] * voices, [0] * voices, [0] * voices, math.ceil(release_seconds * SR) + 1

    def on(self, key, now):
        m = len(self.key)
        v = next((i for i in range(m) if self.key[i] < 0 and self.busy[i] <= now), None)
        if v is None:
            v = min(range(m), key=lambda i: self.started[i])
        self.key[v], self.started[v], self.busy[v] = key, now, 1 << 62
        return [(v, True)]

    def off(self, key, now):
        out = []
        for i in range(len(self.key)):
            if self.key[i] == key:
                out.append((i, False))
                self.key[i] = -1
                self.busy[i] = now + self.rel
        return out


def _numpy(pcm, total, env):
    """The two notes on the file's fp32 buffer: ([total] float64, the voices the two note-ons took, the first note-off's block start)."""
    step = int(440.0 * np.exp2((KEY - 69.0) / 12.0) / 440.0 * 17592186044416.0)
    big_s, big_e = LOOP[0] << 44, LOOP[1] << 44
    events = [(0, True), (int(0.5 * UPB + 0.5), False), (int(0.5 * UPB + 0.5), True), (int(1.0 * UPB + 0.5), False)]   # (units, on) in insertion order
    alloc = _Alloc(VOICES, env[3] if env else 0.0)
    voices = [{"idx": 0, "playing": False, "env": _Env(*env) if env else None} for _ in range(VOICES)]
    out, took, first_off = np.zeros(total), [], None
    for pos in range(0, total, BLOCK):
        t0, t1 = int(pos * BPM / 60.0 / SR * UPB), int((pos + BLOCK) * BPM / 60.0 / SR * UPB)
        for at, on in events:
            if not t0 <= at < t1:
                continue
            for v, is_on in (alloc.on(KEY, pos) if on else alloc.off(KEY, pos)):
                s = voices[v]
                if is_on:
                    s["idx"], s["playing"] = 0, True
                    took.append(v)
                    if env:
                        s["env"].attack()
                else:
                    first_off = pos if first_off is None else first_off
                    if env:
                        s["env"].release()
                    else:
                        s["playing"] = False
        for f in range(pos, pos + BLOCK):
            for s in voices:
                if not s["playing"]:
                    continue
                fac = 1.0
                if env:
                    s["env"].tick()
                    if s["env"].stage == IDLE:
                        s["playing"] = False
                        continue
                    fac = s["env"].value
                c = s["idx"]
                if c >= big_e:
                    c = big_s + (c - big_s) % (big_e - big_s)
                out[f] += float(pcm[c >> 44]) * fac                        # (a looping voice never meets the file's end)
                s["idx"] = c + step
    return out, took, first_off


def test_cli_gives_a_note_its_release_tail_and_the_next_note_another_voice(tmp_path, oracle):
    n = np.arange(FRAMES)
    ints = (9000 * np.cos(2 * np.pi * n / 168.5)).astype(np.int64)
    (tmp_path / "samples").mkdir(parents=True)
    (tmp_path / "samples" / "pad.wav").write_bytes(_wav_bytes(ints, 1, 16, extra=_smpl_chunk(LOOP[0], LOOP[1] - 1)))
    proj = tmp_path / "twice.json5"
    proj.write_text(PROJECT)
    pcm = _mono_float(ints, 1, 16)
    total = math.ceil(4.0 * 60 / BPM * SR)
    total -= total % BLOCK
    got = {}
    for name, flags, env in (("enveloped", ["--sample-loops", "--sample-envelope", ",".join(str(x) for x in ENV)], ENV), ("plain", ["--sample-loops"], None)):
        r = subprocess.run([CLI, "--wav", "--assets", str(tmp_path)] + flags + [str(proj)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        raw = (tmp_path / (proj.stem + ".wav")).read_bytes()
        got[name] = np.frombuffer(raw[44:], dtype="<i2").reshape(-1, 2).astype(np.int32)
        ref, took, first_off = _numpy(pcm, total, env)
        want = _quantise(oracle, np.stack([ref, ref], axis=1))
        assert got[name].shape == (total, 2) and np.array_equal(got[name][:, 0], got[name][:, 1])
        d = int(np.max(np.abs(got[name] - want)))
        print(f"{name}: max |got - numpy| = {d} LSB; the note-ons took voices {took}; first note-off in the block at frame {first_off}")
        assert d <= 1, (name, d)
        assert first_off == 11008 and took[0] == 0 and took[1] == 1                # the second note takes another voice (with the envelope: the first is in its tail)
        if env is None:                                                          # no tail: from the first note-off's block start on, the second note alone
            step = int(440.0 * np.exp2((KEY - 69.0) / 12.0) / 440.0 * 17592186044416.0)
            alone = np.array([float(pcm[(f * step) >> 44]) for f in range(BLOCK)])
            assert np.max(np.abs(got[name][first_off:first_off + BLOCK, 0] - _quantise(oracle, alone))) <= 1
    # the tail: with the envelope the first note sounds under the second for its release, and the second fades in
    a, b = got["enveloped"][:, 0], got["plain"][:, 0]
    assert np.abs(a[11008:11008 + 500] - b[11008:11008 + 500]).max() > 500       # the tail and the attack
    assert np.abs(a[11008 + 1024:22016] - 0.6 * b[11008 + 1024:22016]).max() <= 2.0                   # held: the sustain level times the plain render (two quantisations)
    assert not b[22016 + BLOCK:].any() and a[22016:22016 + 400].any() and not a[22016 + 1024:].any()   # the second note's own tail, then silence
