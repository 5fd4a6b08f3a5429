"""GPU tier: wet-dry-mix links and trips through the compiled host layer (groove_amd/host/) — Orchestrator::set_wet_links_on_device,
Orchestrator::set_wet_reverb_run, `groove-cli-hip --device-wet-links --wet-reverb-run`.

The trip project is tests/test_gpu_orchestrator_trips.py's sweep project with its second trip, the one onto the SAME effect's
wet-dry-mix that keeps both trips on the host there; its steps here are slopes and a flat (STRAIGHT), so every block is comparable bit
for bit.  The CLI project is this test's own text in the reference's schema, the shape of tests/test_gpu_orchestrator_controllers.py's:
a sampler into the main mixer, a raw Welsh synth through a reverb, and an LFO device whose value a `controls` entry puts on the reverb's
wet-dry-mix."""
import math
import os
import subprocess

import numpy as np
import pytest

from groove_amd import abi_types as T
from tests import ctl_trip_law as LAW
from tests.test_ctl_core_cpu import _closed_form, _delta64
from tests.test_gpu_orchestrator import _mono_float, _quantise
from tests.test_gpu_orchestrator_controllers import PATTERNS, ROOT_HZ, SIDECHAIN, UPB, _Alloc, _pad_patch, _thump, _write_project
from tests.test_gpu_orchestrator_controllers import BPM as CLI_BPM
from tests.test_gpu_orchestrator_trips import BLOCK, BPM, SR, STRAIGHT, TOTAL, _build, _units

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(REPO, "groove_amd", "host", "groove-cli-hip")
WET_STEPS = [(LAW.SLOPE, 1.0, 0.4, 2.0), (LAW.SLOPE, 0.4, 0.9, 2.0)]      # _build's wet trip


def _render(trips_on, wet_on, ahead):
    """(bus, host waits of the run, {trip: on the device?})"""
    from groove_amd.host_binding import Orchestrator
    o = Orchestrator(0, SR, BPM)
    try:
        assert not o.wet_links_on_device() and not o.wet_reverb_run()      # both off by default
        o.set_render_ahead(ahead)
        o.set_trips_on_device(trips_on)
        o.set_wet_links_on_device(wet_on)
        assert o.wet_links_on_device() == wet_on
        trips = _build(o, STRAIGHT, wet_trip=True)
        assert all(o.control_trip_on_device(u) == 0 for u in trips.values())          # decided when a run starts, not before
        before = o.debug_info()["host_waits"]
        got = o.run(BLOCK)
        waits = o.debug_info()["host_waits"] - before
        assert o.debug_info()["zero_segments"] == 0
        return got, waits, {name: o.control_trip_on_device(u) for name, u in trips.items()}
    finally:
        o.close()


@pytest.mark.parametrize("ahead", [0, 1, 2])
def test_a_wet_trip_no_longer_keeps_its_effects_trips_on_the_host(ahead):
    """Both switches on: both trips are device-resident, the render is the switches-off render bit for bit (slopes and a flat: the f64
    law is the host trip's own), and the host waits fall by at least the number of blocks in which a value moved.  The wet switch alone
    moves nothing."""
    off, waits_off, dev_off = _render(False, False, ahead)
    on, waits_on, dev_on = _render(True, True, ahead)
    alone, _, dev_alone = _render(False, True, ahead)
    assert dev_off == {"cutoff": 0, "wet": 0} and dev_on == {"cutoff": 1, "wet": 1} and dev_alone == {"cutoff": 0, "wet": 0}
    assert off.shape == on.shape == (TOTAL, 2) and np.sqrt(np.mean(off.astype(np.float64) ** 2)) > 1e-2
    assert np.array_equal(off.view(np.uint32), on.view(np.uint32))
    assert np.array_equal(off.view(np.uint32), alone.view(np.uint32))
    moved, last = 0, {}
    for pos in range(0, TOTAL, BLOCK):
        at = _units(pos)
        changed = False
        for name, steps in (("cutoff", STRAIGHT), ("wet", WET_STEPS)):
            v = LAW.trip_value(0.0, steps, at)
            if v is not None and v != last.get(name):                   # the host trip sends a value when it changes
                changed, last[name] = True, v
        moved += changed
    print(f"render-ahead {ahead}: host waits off {waits_off}, on {waits_on}; a value moved in {moved} blocks")
    assert moved > 200
    assert waits_off - waits_on >= moved, (waits_off, waits_on, moved)


def test_link_control_onto_wet_dry_mix_with_the_switch_off_and_on():
    from groove_amd import host_binding as H
    o = H.Orchestrator(0, SR, BPM)
    try:
        tap, lfo = o.add_signal_passthrough(), o.add_lfo_controller(T.WAVE_SINE, 2.0)
        lp, verb, mixer = (o.add_effect(k, T.fx_params()) for k in (T.FX_BIQUAD_LP12, T.FX_REVERB, T.FX_MIXER))
        assert o.link_control(tap, lp, "wet-dry-mix") is False and "download per block" in o.last_error()      # the default: dropped
        assert o.link_control(lfo, verb, "wet-dry-mix") is True                                                   # (the host path, once per block)
        o.set_wet_links_on_device(True)
        assert o.link_control(tap, lp, "wet-dry-mix") is True
        assert o.link_control(tap, verb, "wet-dry-mix") is True and o.link_control(lfo, verb, "wet-dry-mix") is True
        assert o.link_control(tap, mixer, "wet-dry-mix") is False                                                 # the identity reads no mix
        assert o.link_control(tap, lp, "cutoff") is False                                                         # another switch's
        o.set_wet_links_on_device(False)
        assert o.link_control(tap, lp, "wet-dry-mix") is False and "download per block" in o.last_error()
        o.set_wet_reverb_run(True)
        assert o.wet_reverb_run()
        o.set_wet_reverb_run(False)
        assert not o.wet_reverb_run()
        assert o.debug_info()["zero_segments"] == 0
    finally:
        o.close()


WOBBLE_HZ = 2.5
BREATHING = (SIDECHAIN.replace('{effect: ["duck", {compressor: {threshold: 0.6, ratio: 0.25, attack: 0, release: 0}}]}',
                               '{effect: ["duck", {reverb: {attenuation: 0.6, seconds: 0.4}}]}')
             .replace('{controller: ["tap", {"signal-passthrough-controller": [{"midi-in": 0, "midi-out": 0}]}]},',
                      '{controller: ["tap", {"signal-passthrough-controller": [{"midi-in": 0, "midi-out": 0}]}]},\n'
                      '    {controller: ["wobble", {lfo: [{"midi-in": 0, "midi-out": 0}, {waveform: "triangle", frequency: 2.5}]}]},'))
CONTROLS = 'controls: [{id: "breathe", source: "wobble", target: {id: "duck", param: "wet-dry-mix"}}],'


def test_cli_with_device_wet_links_within_one_lsb_of_the_oracle_composition(tmp_path, oracle):
    """groove-cli-hip --wav --device-wet-links --wet-reverb-run against the oracle's pieces put together the way the project says: the
    reverb of block b is given the triangle LFO's closed form at the block's first frame as its wet-dry-mix.  Without the options the
    LFO goes through the host once per block: the same render at the same bar."""
    assert BREATHING.count("reverb") == 1 and BREATHING.count("wobble") == 1
    proj = _write_project(tmp_path)                        # (the sample file beside it)
    proj.write_text(BREATHING % CONTROLS)
    r = subprocess.run([CLI, "--wav", "--device-wet-links", "--wet-reverb-run", "--assets", str(tmp_path), str(proj)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "Warning" not in r.stderr, r.stderr
    pcm16 = np.frombuffer((tmp_path / "sidechain.wav").read_bytes()[44:], dtype="<i2").reshape(-1, 2).astype(np.int32)
    total = math.ceil(4.0 * 60 / CLI_BPM * SR)
    total -= total % BLOCK                                # run_performance drops the partial block
    assert len(pcm16) == total and np.abs(pcm16).max() > 2000

    pcm = _mono_float(_thump(), 1, 16)
    sp = (T.SamplerParams * 8)()
    for k in range(8):
        sp[k].sample_index, sp[k].one_shot, sp[k].gain = 0, 0, 1.0
    banks = {0: (oracle.Bank.sampler(pcm, (T.SampleDesc * 1)(T.SampleDesc(0, len(pcm), ROOT_HZ)), sp, SR), _Alloc(8, 0.0)),
             1: (oracle.Bank.welsh((T.WelshParams * 8)(*[_pad_patch()] * 8)), _Alloc(8, 0.3))}
    verb = lambda wet: (T.FxParams * 1)(T.fx_params(attenuation=0.6, reverb_seconds=0.4, wet=float(wet)))
    ofx = oracle.Fx(T.FX_REVERB, verb(1.0))
    events = []
    for ch, (beats, rows) in PATTERNS.items():
        for row in rows:
            for i, k in enumerate(row):
                if k:
                    events.append((int(i * beats * UPB + 0.5), len(events), ch, k, True))
                    events.append((int((i * beats + beats) * UPB + 0.5), len(events), ch, k, False))
    events.sort(key=lambda e: (e[0], e[1]))
    want, pos, values = [], 0, []
    while pos < total:
        t0, t1 = int(pos * CLI_BPM / 60.0 / SR * UPB), int((pos + BLOCK) * CLI_BPM / 60.0 / SR * UPB)
        for at, _, ch, key, on in events:
            if t0 <= at < t1:
                bank, al = banks[ch]
                for ev in (al.on(key, pos) if on else al.off(key, pos)):
                    bank.note_events(T.note_events([ev]))
        v = np.float32((_closed_form("triangle", (_delta64(WOBBLE_HZ, SR) * pos) % 2 ** 64) + 1.0) * 0.5)   # the control phase of the block
        ofx.set_params(verb(v))
        values.append(float(v))
        drums = banks[0][0].render_bus(BLOCK)
        pad = banks[1][0].render(BLOCK).sum(axis=2, keepdims=True)
        want.append(drums + oracle.mix(ofx.process(np.ascontiguousarray(pad))))
        pos += BLOCK
    assert np.ptp(values) > 0.9                            # the mix really moves
    want = _quantise(oracle, np.concatenate(want, axis=0))
    assert want.shape == pcm16.shape
    worst = int(np.max(np.abs(pcm16 - want)))
    print(f"--device-wet-links --wet-reverb-run: worst |wav - oracle| = {worst} LSB; value01 {min(values):.3f} .. {max(values):.3f}")
    assert worst <= 1, worst
    # the default: the host path, the same render to the LSB bar
    r = subprocess.run([CLI, "--wav", "--assets", str(tmp_path), str(proj)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "Warning" not in r.stderr, r.stderr
    off = np.frombuffer((tmp_path / "sidechain.wav").read_bytes()[44:], dtype="<i2").reshape(-1, 2).astype(np.int32)
    assert off.shape == pcm16.shape and np.max(np.abs(off - want)) <= 1
