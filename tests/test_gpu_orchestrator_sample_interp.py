"""GPU tier, through the host layer: `groove-cli-hip --sample-interpolation nearest|linear|cubic` (Orchestrator::set_sample_interpolation)
sets the mode of every sampler and drumkit bank a project creates; without the flag a project renders what it rendered before.

The project: a sampler on a WAV the test writes (root 440 Hz; keys 69 on the root, 57 an octave below and 64, 72, 62 off it) and a 707
drumkit, both straight into the main mixer.  The reference is numpy (docs/DSP_SPEC.md section 7, as tests/test_gpu_sampler_interp.py
restates it): the sequencer's events fall on block starts, a voice's cursor is replayed in exact 64-bit integers, the taps are the file's
fp32 values and the formula is evaluated in float64.  Each track is one row of notes, so at most one sampler voice and one drum sound at
a time: every bus value is the sum of at most two non-zero fp32 values, which is the same fp32 number in whatever order it is taken —
that is why the NEAREST render can be held to 0 LSB of the 16-bit stream; LINEAR and CUBIC to +-1 LSB, tests/test_gpu_orchestrator.py's
bar."""
import math
import os
import subprocess

import numpy as np
import pytest

from tests.test_gpu_orchestrator import _mono_float, _quantise, _wav_bytes
from tests.test_gpu_orchestrator_stereo_samples import KIT, _Alloc, _kit_files

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(REPO, "groove_amd", "host", "groove-cli-hip")
BPM, SR, UPB, BLOCK = 240.0, 44100, 65536, 256
SAMPLER_ROWS = [(1.0, [69, 57, 64, 72]), (0.5, [62, 0, 57, 0, 72, 64, 0, 69])]      # a measure each: (beats per note, notes)
KIT_ROW = [46, 0, 42, 38, 36, 0, 49, 44]                                            # eighth notes, one measure
PROJECT = """{
  title: "a sampler off its root and a drumkit", clock: {bpm: 240, "time-signature": [4, 4]},
  devices: [
    {instrument: ["s", {sampler: [{"midi-in": 0}, {filename: "st.wav", root: 440.0}]}]},
    {instrument: ["kit", {drumkit: [{"midi-in": 10}, {name: "707"}]}]},
  ],
  "patch-cables": [["s", "main-mixer"], ["kit", "main-mixer"]],
  patterns: [
    {id: "a0", "note-value": "quarter", notes: [[69, 57, 64, 72]]},
    {id: "a1", "note-value": "eighth", notes: [[62, 0, 57, 0, 72, 64, 0, 69]]},
    {id: "p", "note-value": "eighth", notes: [[46, 0, 42, 38, 36, 0, 49, 44]]},
  ],
  tracks: [{id: "t0", "midi-channel": 0, patterns: ["a0", "a1"]}, {id: "t", "midi-channel": 10, patterns: ["p"]}],
}"""


def _sample_file():
    """st.wav: 16-bit stereo, 9,000 frames: two decaying tones that neither begin nor end at zero."""
    n = np.arange(9000)
    env = 0.3 + 0.7 * np.exp(-n / 3000.0)
    left = (9000 * np.cos(2 * np.pi * n / 168.5) * env).astype(np.int64)
    right = (9000 * np.cos(2 * np.pi * n / 61.25 + 0.4) * env).astype(np.int64)
    return left, right


def _block_of(units):
    pos = 0
    while not (int(pos * BPM / 60.0 / SR * UPB) <= units < int((pos + BLOCK) * BPM / 60.0 / SR * UPB)):
        pos += BLOCK
    return pos


def _taps(pcm, i, d, ok):
    j = i + d
    return np.where(ok & (j >= 0) & (j < len(pcm)), pcm[np.clip(j, 0, len(pcm) - 1)].astype(np.float64), 0.0)


def _sampler_numpy(pcm, mode, total):
    """The sampler track on one channel's fp32 buffer: [total] float64 (NEAREST: exactly the fp32 values)."""
    events = []
    for measure, (beats, row) in enumerate(SAMPLER_ROWS):
        for i, k in enumerate(row):
            if k:
                events.append((int((4 * measure + i * beats) * UPB + 0.5), len(events), k, True))
                events.append((int((4 * measure + i * beats + beats) * UPB + 0.5), len(events), k, False))
    events.sort(key=lambda e: (e[0], e[1]))
    at_block = {}
    for units, _, key, on in events:
        at_block.setdefault(_block_of(units), []).append((key, on))
    alloc, out = _Alloc(8, 0.0), np.zeros(total)
    idx, step, playing = np.zeros(8, dtype=np.uint64), np.zeros(8, dtype=np.uint64), np.zeros(8, dtype=bool)
    f = np.arange(BLOCK, dtype=np.uint64)
    for pos in range(0, total, BLOCK):
        for key, on in at_block.get(pos, []):
            for v, k, is_on in (alloc.on(key, pos) if on else alloc.off(key, pos)):
                if is_on:
                    idx[v], playing[v] = 0, True
                    step[v] = np.uint64(int(440.0 * np.exp2((k - 69.0) / 12.0) / 440.0 * 17592186044416.0))
                else:
                    playing[v] = False
        p = idx[None, :] + f[:, None] * step[None, :]
        i = (p >> np.uint64(44)).astype(np.int64)
        t = ((p >> np.uint64(20)) & np.uint64(0xFFFFFF)).astype(np.float64) * 2.0 ** -24
        ok = playing[None, :] & (i < len(pcm))
        if mode == "nearest":
            y = _taps(pcm, i, 0, ok)
        elif mode == "linear":
            p0, p1 = _taps(pcm, i, 0, ok), _taps(pcm, i, 1, ok)
            y = p0 + t * (p1 - p0)
        else:
            pm, p0, p1, p2 = (_taps(pcm, i, d, ok) for d in (-1, 0, 1, 2))
            y = ((((0.5 * (p2 - pm) + 1.5 * (p0 - p1)) * t + (pm - 2.5 * p0 + 2.0 * p1 - 0.5 * p2)) * t) + 0.5 * (p1 - pm)) * t + p0
        out[pos:pos + BLOCK] = y.sum(axis=1)
        valid = ok.sum(axis=0).astype(np.uint64)
        idx = idx + valid * step
        playing = playing & (valid == np.uint64(BLOCK))
    return out


def _kit_numpy(files, stereo, total):
    """The drum track: a note-on restarts the drum's sample at its block's first frame (one-shot, step 1, gain 1: the same in every mode)."""
    bus = np.zeros((total, 2))
    for i, key in enumerate(KIT_ROW):
        if not key:
            continue
        ints, ch = files[KIT[key]]
        x = np.asarray(ints, dtype=np.int64).reshape(-1, ch) / 32768.0
        if stereo:
            pcm = x.astype(np.float32) if ch == 2 else np.repeat(x.astype(np.float32), 2, axis=1)
        else:
            pcm = np.repeat(_mono_float(ints, ch, 16)[:, None], 2, axis=1)
        p = _block_of(int(i * 0.5 * UPB + 0.5))
        assert len(pcm) < 5000                                                     # (a hit is over before the next eighth note's)
        bus[p:p + len(pcm)] += pcm.astype(np.float64)
    return bus


def _render(tmp_path, proj, flags):
    r = subprocess.run([CLI, "--wav", "--assets", str(tmp_path)] + flags + [str(proj)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    raw = (tmp_path / (proj.stem + ".wav")).read_bytes()
    return np.frombuffer(raw[44:], dtype="<i2").reshape(-1, 2).astype(np.int32)


@pytest.mark.parametrize("stereo", [False, True], ids=["mono-banks", "stereo-samples"])
def test_cli_renders_by_the_mode_it_is_given_and_as_before_without_it(tmp_path, oracle, stereo):
    left, right = _sample_file()
    files = _kit_files()
    kit_dir = tmp_path / "samples" / "elphnt.io" / "707"
    kit_dir.mkdir(parents=True)
    for name, (ints, ch) in files.items():
        (kit_dir / name).write_bytes(_wav_bytes(ints, ch, 16))
    both = np.stack([left, right], axis=1).ravel()
    (tmp_path / "samples" / "st.wav").write_bytes(_wav_bytes(both, 2, 16))
    proj = tmp_path / "interp.json5"
    proj.write_text(PROJECT)
    total = math.ceil(8.0 * 60 / BPM * SR)                # two measures
    total -= total % BLOCK                                # run_performance drops the partial block
    if stereo:
        channels = [(np.asarray(c, dtype=np.int64) / 32768.0).astype(np.float32) for c in (left, right)]
    else:
        channels = [_mono_float(both, 2, 16)] * 2
    kit = _kit_numpy(files, stereo, total)
    want = {mode: _quantise(oracle, kit + np.stack([_sampler_numpy(c, mode, total) for c in channels], axis=1)) for mode in ("nearest", "linear", "cubic")}
    assert np.abs(want["linear"] - want["nearest"]).max() > 100 and np.abs(want["cubic"] - want["linear"]).max() > 2   # LSB: the modes are told apart
    extra = ["--stereo-samples"] if stereo else []
    for flags, mode, bar in (([], "nearest", 0), (["--sample-interpolation", "nearest"], "nearest", 0),
                             (["--sample-interpolation", "linear"], "linear", 1), (["--sample-interpolation", "cubic"], "cubic", 1)):
        got = _render(tmp_path, proj, extra + flags)
        assert got.shape == (total, 2) and np.abs(got).max() > 2000
        assert np.array_equal(got[:, 0], got[:, 1]) == (not stereo)
        d = [int(np.max(np.abs(got[:, ch] - want[mode][:, ch]))) for ch in range(2)]
        print(f"{'--stereo-samples ' if stereo else ''}{' '.join(flags) or '(no flag)'}: max |got - numpy| = {d[0]} LSB (left), {d[1]} LSB (right)")
        assert max(d) <= bar, (flags, d)
