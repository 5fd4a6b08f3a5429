"""GPU tier: device-resident controls onto a Welsh synth through the compiled host layer (groove_amd/host/) —
Orchestrator::set_instrument_controls_on_device and `groove-cli-hip --device-instrument-controls`.  With the switch on, a ControlTrip or
an LFO `controls` link onto a synth's dca-gain, dca-pan or filter-cutoff lives in the library (groove_ctl_bank_trip_create /
groove_ctl_bank_link_create) and costs no groove_bank_set_param — no re-derivation, re-plan and re-upload of the bank, and no host wait —
per automated block.  The switch is independent of set_trips_on_device, off by default, and an instrument that ANY control reaches
through the host keeps all its trips there.

The project is the one tests/test_gpu_orchestrator_trips.py builds with pan_trip=True: its sweep project plus a four-voice Welsh synth
whose dca-pan a slope sweeps over the four beats.  A slope is evaluated without a logarithm, so the renders on the two sides of the
switch must be the same sample for sample."""
import math
import os
import subprocess

import numpy as np
import pytest

from groove_amd import patches as P, abi_types as T
from tests import ctl_trip_law as LAW
from tests.test_ctl_core_cpu import _closed_form, _delta64
from tests.test_gpu_orchestrator import _quantise
from tests.test_gpu_orchestrator_controllers import _Alloc, _pad_patch
from tests.test_gpu_orchestrator_trips import BLOCK, BPM, SR, STRAIGHT, TOTAL, _build, _units

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(REPO, "groove_amd", "host", "groove-cli-hip")
UPB = 65536
PAN_STEPS = [(LAW.SLOPE, 0.1, 0.9, 4.0)]           # what _build(..., pan_trip=True) gives the synth's dca-pan


def _render(on, ahead, extra=None, trips_switch=False):
    """(bus, host waits of the run, {trip: on the device?}); extra(o, trips): more of a project, after _build's."""
    from groove_amd.host_binding import Orchestrator
    o = Orchestrator(0, SR, BPM)
    try:
        o.set_render_ahead(ahead)
        o.set_trips_on_device(trips_switch)
        o.set_instrument_controls_on_device(on)
        trips = _build(o, STRAIGHT, pan_trip=True)
        if extra:
            extra(o, trips)
        assert all(o.control_trip_on_device(u) == 0 for u in trips.values())          # decided when a run starts, not before
        before = o.debug_info()["host_waits"]
        got = o.run(BLOCK)
        waits = o.debug_info()["host_waits"] - before
        info = o.debug_info()
        assert info["zero_segments"] == 0 and info["fast_table_misses"] == 0
        return got, waits, {name: o.control_trip_on_device(u) for name, u in trips.items()}
    finally:
        o.close()


@pytest.mark.parametrize("ahead", [0, 1, 2])
def test_pan_trip_switch_off_and_on(ahead):
    off, waits_off, dev_off = _render(False, ahead)
    on, waits_on, dev_on = _render(True, ahead)
    assert dev_off == {"cutoff": 0, "pan": 0} and dev_on == {"cutoff": 0, "pan": 1}     # (the effects' switch is off: the cutoff trip stays)
    assert off.shape == on.shape == (TOTAL, 2) and np.sqrt(np.mean(off.astype(np.float64) ** 2)) > 1e-2
    assert np.array_equal(off.view(np.uint32), on.view(np.uint32))
    assert np.abs(on[:, 0] - on[:, 1]).max() > 1e-3                                      # the image moves
    moved, last = 0, None
    for pos in range(0, TOTAL, BLOCK):
        v = LAW.trip_value(0.0, PAN_STEPS, _units(pos))
        if v is not None and v != last:                                                  # the host trip sends a value when it changes
            moved, last = moved + 1, v
    print(f"render-ahead {ahead}: host waits off {waits_off}, on {waits_on}; the pan value moved in {moved} blocks")
    assert moved > 300
    assert waits_off - waits_on >= moved, (waits_off, waits_on, moved)


def test_both_switches_are_independent():
    """The effects' switch alone leaves the pan trip on the host (tests/test_gpu_orchestrator_trips.py asserts the same); both on: both
    trips on the device, the same samples."""
    _, _, only_fx = _render(False, 1, trips_switch=True)
    both, _, dev_both = _render(True, 1, trips_switch=True)
    off, _, _ = _render(False, 1)
    assert only_fx == {"cutoff": 1, "pan": 0} and dev_both == {"cutoff": 1, "pan": 1}
    assert np.array_equal(off.view(np.uint32), both.view(np.uint32))


def test_control_trip_onto_an_instrument_on_the_device_follows_the_oracle_bank(oracle):
    """tests/test_gpu_orchestrator.py test_control_trip_onto_an_instrument_reaches_its_voices with the switch on: the same project, the
    same oracle walk, the same bar."""
    from groove_amd import host_binding as H
    bpm, sr, block = 120.0, 44100, 256
    patch = P.welsh_patch(3)
    o = H.Orchestrator(0, sr, bpm)
    try:
        o.set_instrument_controls_on_device(True)
        w = o.add_welsh(patch, voices=4)
        assert o.patch(w, o.MAIN_MIXER) == 0
        o.connect_midi_downstream(w, 0)
        seq = o.add_sequencer()
        for k, s_, d in ((60, 0.0, 1.9), (64, 0.5, 1.0)):
            o.sequencer_insert(seq, 0, k, s_, d)
        o.sequencer_set_end(seq, 2.0)
        trip = o.add_control_trip(w, "dca-pan", 0.0)
        o.control_trip_add_step(trip, H.STEP_SLOPE, 0.0, 1.0, 2.0)
        got = o.run(block).astype(np.float64)
        assert o.control_trip_on_device(trip) == 1
    finally:
        o.close()
    total = math.ceil(2.0 * 60 / bpm * sr)
    assert len(got) == total
    ob = oracle.Bank.welsh((T.WelshParams * 4)(*[patch] * 4))
    evs = sorted([(int(0.0 * UPB + 0.5), 0, 0, 60, True), (int(1.9 * UPB + 0.5), 1, 0, 60, False), (int(0.5 * UPB + 0.5), 2, 1, 64, True), (int(1.5 * UPB + 0.5), 3, 1, 64, False)])
    want, pos, last = [], 0, None
    while pos < total:
        fr = min(block, total - pos)
        t0, t1 = int(pos * bpm / 60.0 / sr * UPB), int((pos + fr) * bpm / 60.0 / sr * UPB)
        for at, _, v, key, on in evs:
            if t0 <= at < t1:
                ob.note_events(T.note_events([(v, key, on)]))
        val = min(1.0, max(0.0, (t0 / UPB) / 2.0))        # ControlTrip::work: the value at the block's start
        if val != last:
            ob.set_param(T.CTL_WELSH_DCA_PAN, val); last = val
        want.append(ob.render_bus(fr)); pos += fr
    want = np.concatenate(want, axis=0)
    assert np.sqrt(np.mean(want ** 2)) > 1e-2
    err = float(np.sqrt(np.mean((got - want) ** 2)))
    print(f"dca-pan trip on the device: bus RMS against the oracle {err:.3e}")
    assert err <= 1e-5
    q = total // 4
    assert np.abs(got[:q, 0]).mean() > 3 * np.abs(got[:q, 1]).mean() and np.abs(got[-q:, 1]).mean() > 3 * np.abs(got[-q:, 0]).mean()


@pytest.mark.parametrize("ahead", [0, 2])
def test_a_trip_the_library_refuses_keeps_all_the_synths_trips_on_the_host(ahead):
    """A second trip onto the same synth with a `Triggered` step, which groove_ctl_bank_trip_create refuses: its values would go through
    groove_bank_set_param, which re-uploads the host's stale pan over the one a device trip owns.  So both stay on the host — the pan trip,
    placed first, is taken back — and the render is the switch-off render bit for bit."""
    def second(o, trips):
        trips["gain"] = o.add_control_trip(_synth_of(trips), "dca-gain", 1.0)
        o.control_trip_add_step(trips["gain"], 4, 0.4, 0.4, 1.0)                          # ControlStep::TRIGGERED: the host hands on `start`

    off, _, dev_off = _render(False, ahead, second)
    on, _, dev_on = _render(True, ahead, second)
    assert dev_off == {"cutoff": 0, "pan": 0, "gain": 0} and dev_on == {"cutoff": 0, "pan": 0, "gain": 0}
    assert np.array_equal(off.view(np.uint32), on.view(np.uint32))
    plain, _, _ = _render(False, ahead)
    assert np.abs(off - plain).max() > 1e-3                                              # the gain trip does something


def _synth_of(trips):
    """The uid of the synth _build(..., pan_trip=True) added: the entity added just before its pan trip (uids count up)."""
    return trips["pan"] - 1


def _lfo_project(on):
    """(bus, host waits, blocks): a four-voice synth whose dca-gain a 2 Hz triangle LFO drives."""
    from groove_amd import host_binding as H
    o = H.Orchestrator(0, SR, BPM)
    try:
        o.set_instrument_controls_on_device(on)                      # before link_control: the link is made there
        w = o.add_welsh(P.welsh_patch(3), voices=4)
        assert o.patch(w, o.MAIN_MIXER) == 0
        o.connect_midi_downstream(w, 0)
        seq = o.add_sequencer()
        for k, s_, d in ((60, 0.0, 1.9), (64, 0.5, 1.0)):
            o.sequencer_insert(seq, 0, k, s_, d)
        o.sequencer_set_end(seq, 2.0)
        lfo = o.add_lfo_controller(T.WAVE_TRIANGLE, 2.0)
        assert o.link_control(lfo, w, "dca-gain") is True
        # a signal source onto an instrument stays dropped, whatever the switch says
        tap = o.add_signal_passthrough()
        assert o.link_control(tap, w, "dca-gain") is False
        before = o.debug_info()["host_waits"]
        got = o.run(BLOCK).astype(np.float64)
        waits = o.debug_info()["host_waits"] - before
        info = o.debug_info()
        assert info["zero_segments"] == 0 and info["fast_table_misses"] == 0
        return got, waits
    finally:
        o.close()


def test_lfo_link_onto_a_synths_gain_on_the_device(oracle):
    """The bar is the one tests/test_gpu_orchestrator_controllers.py holds the host path's LFO link to, for both sides of the switch: the
    device evaluates the law in fp32 (2e-7 of the closed form), the host in f64."""
    off, waits_off = _lfo_project(False)
    on, waits_on = _lfo_project(True)
    total = math.ceil(2.0 * 60 / BPM * SR)
    assert len(off) == len(on) == total
    patch = P.welsh_patch(3)
    ob = oracle.Bank.welsh((T.WelshParams * 4)(*[patch] * 4))
    evs = sorted([(int(0.0 * UPB + 0.5), 0, 0, 60, True), (int(1.9 * UPB + 0.5), 1, 0, 60, False), (int(0.5 * UPB + 0.5), 2, 1, 64, True), (int(1.5 * UPB + 0.5), 3, 1, 64, False)])
    want, pos, gains = [], 0, []
    while pos < total:
        fr = min(BLOCK, total - pos)
        t0, t1 = int(pos * BPM / 60.0 / SR * UPB), int((pos + fr) * BPM / 60.0 / SR * UPB)
        for at, _, v, key, on_ in evs:
            if t0 <= at < t1:
                ob.note_events(T.note_events([(v, key, on_)]))
        val = (_closed_form("triangle", (_delta64(2.0, SR) * pos) % 2 ** 64) + 1.0) * 0.5
        ob.set_param(T.CTL_WELSH_DCA_GAIN, val)
        gains.append(val)
        want.append(ob.render_bus(fr)); pos += fr
    want = np.concatenate(want, axis=0)
    assert np.sqrt(np.mean(want ** 2)) > 1e-2 and np.ptp(gains) > 0.9
    err_off, err_on = (float(np.sqrt(np.mean((g - want) ** 2))) for g in (off, on))
    blocks = len(gains)
    print(f"LFO -> dca-gain: bus RMS against the oracle off {err_off:.3e}, on {err_on:.3e}; host waits off {waits_off}, on {waits_on}, {blocks} blocks")
    assert err_off <= 1e-5 and err_on <= 1e-5
    assert waits_off - waits_on >= blocks, (waits_off, waits_on, blocks)     # no groove_bank_set_param, and so no host wait, per block


CLI_PROJECT = """// a synthetic project of this test's own, in the reference's project schema: an inline Welsh synth whose dca-pan a trip of a flat
// and a slope step (a half note each) automates
{
  title: "synthetic: four quarter notes under a pan trip", clock: {bpm: 120, "time-signature": [4, 4]},
  devices: [
    {instrument: ["pad", {"welsh-raw": [{"midi-in": 4}, {
        voice: {"oscillator-1": {waveform: {"pulse-width": 0.3}, "frequency-tune": 1.0},
                "oscillator-2": {waveform: "sawtooth", "frequency-tune": {osc: {octave: -1, semi: 0, cent: 4}}},
                "oscillator-2-sync": false, "oscillator-mix": 0.6,
                "amp-envelope": {attack: 0.01, decay: 0.2, sustain: 0.7, release: 0.3},
                lfo: {waveform: "square", frequency: 5.13}, "lfo-routing": "pitch", "lfo-depth": 0.05,
                filter: {cutoff: 900, "passband-ripple": 1.2}, "filter-cutoff-start": 0.4, "filter-cutoff-end": 0.5,
                "filter-envelope": {attack: 0.0, decay: 0.5, sustain: 0.3, release: 0.5}},
        dca: {gain: 0.8, pan: -0.25}}]}]},
  ],
  "patch-cables": [["pad", "main-mixer"]],
  patterns: [{id: "p4", "note-value": "quarter", notes: [[50, 62, 57, 55]]}],
  tracks: [{id: "t4", "midi-channel": 4, patterns: ["p4"]}],
  paths: [{id: "left-then-across", "note-value": "half", steps: [{flat: {value: 0.15}}, {slope: {start: 0.15, end: 0.95}}]}],
  trips: [{id: "pan", target: {id: "pad", param: "dca-pan"}, paths: ["left-then-across"]}],
}
"""
CLI_STEPS = [(LAW.FLAT, 0.15, 0.15, 2.0), (LAW.SLOPE, 0.15, 0.95, 2.0)]


def test_cli_with_device_instrument_controls_within_one_lsb_of_the_oracle_composition(tmp_path, oracle):
    proj = tmp_path / "pan.json5"
    proj.write_text(CLI_PROJECT)
    wavs = {}
    for name, flags in (("on", ["--device-instrument-controls"]), ("off", [])):
        r = subprocess.run([CLI, "--wav"] + flags + ["--assets", str(tmp_path), str(proj)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "Warning" not in r.stderr and "Warning" not in r.stdout, (name, r.stderr)
        wavs[name] = np.frombuffer((tmp_path / "pan.wav").read_bytes()[44:], dtype="<i2").reshape(-1, 2).astype(np.int32)
    bpm, block = 120.0, 256
    total = math.ceil(4.0 * 60 / bpm * SR)
    total -= total % block                                # run_performance drops the partial block
    assert wavs["on"].shape == wavs["off"].shape == (total, 2) and np.abs(wavs["on"]).max() > 2000
    assert np.array_equal(wavs["on"], wavs["off"])
    ob, al = oracle.Bank.welsh((T.WelshParams * 8)(*[_pad_patch()] * 8)), _Alloc(8, 0.3)
    events = []
    for i, k in enumerate([50, 62, 57, 55]):
        events.append((int(i * 1.0 * UPB + 0.5), len(events), k, True))
        events.append((int((i * 1.0 + 1.0) * UPB + 0.5), len(events), k, False))
    events.sort(key=lambda e: (e[0], e[1]))
    want, pos, last = [], 0, None
    while pos < total:
        t0, t1 = int(pos * bpm / 60.0 / SR * UPB), int((pos + block) * bpm / 60.0 / SR * UPB)
        for at, _, key, on in events:
            if t0 <= at < t1:
                for ev in (al.on(key, pos) if on else al.off(key, pos)):
                    ob.note_events(T.note_events([ev]))
        v = LAW.trip_value(0.0, CLI_STEPS, t0)
        if v is not None and v != last:
            ob.set_param(T.CTL_WELSH_DCA_PAN, v); last = v
        want.append(ob.render_bus(block)); pos += block
    want = _quantise(oracle, np.concatenate(want, axis=0))
    for name, pcm16 in wavs.items():
        worst = int(np.max(np.abs(pcm16 - want)))
        print(f"--device-instrument-controls {name}: worst |wav - oracle| = {worst} LSB")
        assert worst <= 1, (name, worst)
    q = total // 4
    on = wavs["on"].astype(np.float64)
    assert np.abs(on[:q, 0]).mean() > 1.5 * np.abs(on[:q, 1]).mean() and np.abs(on[-q:, 1]).mean() > 1.5 * np.abs(on[-q:, 0]).mean()    # left, then across
