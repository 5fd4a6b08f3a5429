"""GPU tier, through the host layer: `groove-cli-hip --sample-loops` (Orchestrator::set_sample_loops) gives a sampler the forward sustain
loop its WAV file's `smpl` chunk carries (project.hpp read_wav_loop); without the flag a project renders what it rendered before.

The project: one sampler on a WAV the test writes — 9,000 frames, a forward loop over frames 6,000 .. 7,999 (dwEnd inclusive: [6000,
8000)) — holding key 64 (off the root 440 Hz: a fractional step of ~0.749) for a whole note at 240 bpm, 44,100 frames, more than four
times the file's length.  The reference is numpy (docs/DSP_SPEC.md section 7, as tests/test_gpu_sampler_loops.py restates it): the
note-on falls on a block start, the cursor is replayed in exact integers with the fold, the taps are the file's fp32 values and the
formula is evaluated in float64.  One voice sounds, so every bus value is one fp32 value and the 16-bit stream can be held to 1 LSB
with the flag (tests/test_gpu_orchestrator.py's bar) and to 0 LSB without it, where the file ends after 12,017 frames into silence."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

from tests.test_gpu_orchestrator import _mono_float, _quantise, _wav_bytes

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(REPO, "groove_amd", "host", "groove-cli-hip")
BPM, SR, BLOCK = 240.0, 44100, 256
FRAMES, LOOP = 9000, (6000, 8000)
KEY = 64
PROJECT = """{
  title: "a sampler holding one note", clock: {bpm: 240, "time-signature": [4, 4]},
  devices: [
    {instrument: ["s", {sampler: [{"midi-in": 0}, {filename: "pad.wav", root: 440.0}]}]},
  ],
  "patch-cables": [["s", "main-mixer"]],
  patterns: [
    {id: "a0", "note-value": "whole", notes: [[64]]},
  ],
  tracks: [{id: "t0", "midi-channel": 0, patterns: ["a0"]}],
}"""


def _sample_file():
    """Two tones whose periods do not divide the loop's 2,000 frames: the seam is a step, and a tap read past it into the file shows."""
    n = np.arange(FRAMES)
    left = (9000 * np.cos(2 * np.pi * n / 168.5)).astype(np.int64)
    right = (9000 * np.cos(2 * np.pi * n / 61.25 + 0.4)).astype(np.int64)
    return left, right


def _smpl_chunk(first, last, loop_type=0):
    """A `smpl` chunk with one loop record; dwEnd is the last frame played."""
    body = struct.pack("<9I", 0, 0, 22675, 60, 0, 0, 0, 1, 0) + struct.pack("<6I", 0, loop_type, first, last, 0, 0)
    return b"smpl" + struct.pack("<I", len(body)) + body


def _numpy(pcm, mode, looped, total):
    """The held note on one channel's fp32 buffer: [total] float64.  Note-on at frame 0; the note-off lies past the render."""
    step = int(440.0 * np.exp2((KEY - 69.0) / 12.0) / 440.0 * 17592186044416.0)
    start, end = LOOP
    big_s, big_e = start << 44, end << 44
    out = np.zeros(total)
    for f in range(total):
        x = f * step                                                     # (Python integers: exact)
        if looped and x >= big_e:
            x = big_s + (x - big_s) % (big_e - big_s)
        i, t = x >> 44, ((x >> 20) & 0xFFFFFF) * 2.0 ** -24
        if i >= len(pcm):
            break

        def tap(d):
            j = i + d
            if looped and j >= end:
                j = start + (j - start) % (end - start)
            return float(pcm[j]) if 0 <= j < len(pcm) else 0.0
        if mode == "nearest":
            out[f] = tap(0)
        else:
            p0, p1 = tap(0), tap(1)
            out[f] = p0 + t * (p1 - p0)
    return out


def _render(tmp_path, proj, flags):
    r = subprocess.run([CLI, "--wav", "--assets", str(tmp_path)] + flags + [str(proj)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    raw = (tmp_path / (proj.stem + ".wav")).read_bytes()
    return np.frombuffer(raw[44:], dtype="<i2").reshape(-1, 2).astype(np.int32), r.stderr


@pytest.mark.parametrize("stereo", [False, True], ids=["mono-file", "stereo-file"])
def test_cli_holds_a_note_through_the_files_loop_and_plays_it_once_without_the_flag(tmp_path, oracle, stereo):
    left, right = _sample_file()
    (tmp_path / "samples").mkdir(parents=True)
    if stereo:
        ints, ch = np.stack([left, right], axis=1).ravel(), 2
        channels = [(np.asarray(c, dtype=np.int64) / 32768.0).astype(np.float32) for c in (left, right)]
    else:
        ints, ch = left, 1
        channels = [_mono_float(left, 1, 16)] * 2
    (tmp_path / "samples" / "pad.wav").write_bytes(_wav_bytes(ints, ch, 16, extra=_smpl_chunk(LOOP[0], LOOP[1] - 1)))
    proj = tmp_path / "held.json5"
    proj.write_text(PROJECT)
    total = math.ceil(4.0 * 60 / BPM * SR)                # one measure: the whole note
    total -= total % BLOCK                                # run_performance drops the partial block
    assert total >= 4 * FRAMES
    extra = ["--stereo-samples"] if stereo else []
    want = {(mode, looped): _quantise(oracle, np.stack([_numpy(c, mode, looped, total) for c in channels], axis=1))
            for mode in ("nearest", "linear") for looped in (False, True)}
    file_end = int(np.flatnonzero(np.abs(want[("nearest", False)]).max(axis=1))[-1]) + 1
    assert 12000 < file_end < 12100 and np.abs(want[("nearest", True)][-BLOCK:]).max() > 2000      # the file's end; a sounding tail
    for flags, key, bar in (([], ("nearest", False), 0), (["--sample-interpolation", "linear"], ("linear", False), 1),
                            (["--sample-loops"], ("nearest", True), 1), (["--sample-loops", "--sample-interpolation", "linear"], ("linear", True), 1)):
        got, stderr = _render(tmp_path, proj, extra + flags)
        assert got.shape == (total, 2) and "smpl" not in stderr, stderr
        assert np.array_equal(got[:, 0], got[:, 1]) == (not stereo)
        d = [int(np.max(np.abs(got[:, c] - want[key][:, c]))) for c in range(2)]
        print(f"{'--stereo-samples ' if stereo else ''}{' '.join(flags) or '(no flag)'}: max |got - numpy| = {d[0]} LSB (left), {d[1]} LSB (right)")
        assert max(d) <= bar, (flags, d)
        if key[1]:
            assert np.abs(got[-BLOCK:]).max() > 2000                              # the tail is not silent
        else:
            assert not got[file_end:].any() and got[file_end - 50:file_end].any()          # silence after the file's end, as before
    # a ping-pong loop is not played: a warning, and the render without loops
    (tmp_path / "samples" / "pad.wav").write_bytes(_wav_bytes(ints, ch, 16, extra=_smpl_chunk(LOOP[0], LOOP[1] - 1, loop_type=1)))
    got, stderr = _render(tmp_path, proj, extra + ["--sample-loops"])
    assert "Warning" in stderr and "type 1" in stderr, stderr
    assert np.array_equal(got, _render(tmp_path, proj, extra)[0])
