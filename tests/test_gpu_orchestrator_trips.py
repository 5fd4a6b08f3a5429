"""GPU tier: device-resident control trips through the compiled host layer (groove_amd/host/) — Orchestrator::set_trips_on_device and
`groove-cli-hip --device-trips`.  With the switch on, a ControlTrip onto an effect parameter the library can reach lives in the library
(groove_ctl_trip_create) and costs no groove_fx_set_param, and so no host wait, per automated block; everything else — trips onto
instruments, onto wet-dry-mix, and every trip onto an effect that ANY control reaches through the host — takes the host path unchanged.

The sweep project is the one tests/test_gpu_orchestrator.py test_control_trip_sweep_matches_oracle builds (a toy source and a drumkit
into a 24 dB low-pass whose cutoff a trip sweeps), with slope, exponential and flat steps.  The renders with the switch off and on must
be the same sample for sample in every block whose start lies in a slope or flat step; in an exponential step the device's f64 log10
may differ from the C library's in the last place, so the blocks there that differ are counted, printed, and may be at most one in ten
(and once one HAS differed, the filter's state has too: the later blocks of that run are held to the oracle only)."""
import math
import os
import subprocess

import numpy as np
import pytest

from groove_amd import patches as P, abi_types as T
from tests import ctl_trip_law as LAW
from tests.test_gpu_orchestrator import _config1_notes, _oracle_config1, _quantise

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(REPO, "groove_amd", "host", "groove-cli-hip")
SR, BPM, BLOCK, BEATS = 44100, 128.0, 256, 4.0
SWEEP = [(LAW.SLOPE, 0.2, 0.8, 1.5), (LAW.EXP, 0.8, 0.1, 1.5), (LAW.FLAT, 0.35, 0.35, 1.0)]
STRAIGHT = [(LAW.SLOPE, 0.2, 0.8, 1.5), (LAW.FLAT, 0.35, 0.35, 1.0), (LAW.SLOPE, 0.8, 0.05, 1.5)]
TOTAL = math.ceil(BEATS * 60 / BPM * SR)


def _units(frame):
    return int(frame * BPM / 60.0 / SR * 65536)


def _build(o, steps, wet_trip=False, pan_trip=False):
    """The sweep project; returns the trips' uids by name."""
    from groove_amd import host_binding as H
    pcm, descs, k2s = H.synthetic_kit()
    src = o.add_toy_source(0.25)
    kit = o.add_drumkit(pcm, descs, k2s)
    lp = o.add_effect(T.FX_BIQUAD_LP24, T.fx_params(cutoff_hz=1000.0, passband_ripple=0.8))
    assert o.patch(src, lp) == 0 and o.patch(kit, lp) == 0 and o.patch(lp, o.MAIN_MIXER) == 0
    o.connect_midi_downstream(kit, 10)
    seq = o.add_sequencer()
    for k, s in _config1_notes(1):
        o.sequencer_insert(seq, 10, k, s, 0.25)
    o.sequencer_set_end(seq, BEATS)
    trips = {"cutoff": o.add_control_trip(lp, "cutoff", 0.0)}
    for st in steps:
        o.control_trip_add_step(trips["cutoff"], *st)
    if wet_trip:                                                        # a second trip onto the SAME effect, one only the host can work
        trips["wet"] = o.add_control_trip(lp, "wet-dry-mix", 0.0)
        o.control_trip_add_step(trips["wet"], LAW.SLOPE, 1.0, 0.4, 2.0)
        o.control_trip_add_step(trips["wet"], LAW.SLOPE, 0.4, 0.9, 2.0)
    if pan_trip:                                                        # a trip onto an instrument
        w = o.add_welsh(P.welsh_patch(3), voices=4)
        assert o.patch(w, o.MAIN_MIXER) == 0
        o.connect_midi_downstream(w, 0)
        for k, s_, d in ((60, 0.0, 1.9), (64, 0.5, 1.0), (67, 2.0, 1.5)):
            o.sequencer_insert(seq, 0, k, s_, d)
        trips["pan"] = o.add_control_trip(w, "dca-pan", 0.0)
        o.control_trip_add_step(trips["pan"], LAW.SLOPE, 0.1, 0.9, 4.0)
    return trips


def _render(on, ahead, steps, **kw):
    """(bus, host waits of the run, {trip: on the device?})"""
    from groove_amd.host_binding import Orchestrator
    o = Orchestrator(0, SR, BPM)
    try:
        o.set_render_ahead(ahead)
        o.set_trips_on_device(on)
        trips = _build(o, steps, **kw)
        assert all(o.control_trip_on_device(u) == 0 for u in trips.values())          # decided when a run starts, not before
        before = o.debug_info()["host_waits"]
        got = o.run(BLOCK)
        waits = o.debug_info()["host_waits"] - before
        assert o.debug_info()["zero_segments"] == 0
        return got, waits, {name: o.control_trip_on_device(u) for name, u in trips.items()}
    finally:
        o.close()


_ORACLE = {}


def _oracle_sweep(oracle):
    """The same graph on the oracle (two sources into one effect: it sums them, then transforms once), once for all the tests here."""
    if "bus" not in _ORACLE:
        from groove_amd import host_binding as H
        pcm, descs, k2s = H.synthetic_kit()
        sp = (T.SamplerParams * 128)()
        for k in range(128):
            sp[k].sample_index, sp[k].one_shot, sp[k].gain = (k2s[k] if k2s[k] >= 0 else 0), 1, (1.0 if k2s[k] >= 0 else 0.0)
        g = oracle.Graph()
        g.set_bpm(BPM)
        s_uid, k_uid = g.add_source(0.25), g.add_instrument(oracle.Bank.sampler(pcm, descs, sp))
        f_uid = g.add_effect(T.FX_BIQUAD_LP24, T.fx_params(cutoff_hz=1000.0, passband_ripple=0.8))
        assert g.patch(s_uid, f_uid) == 0 and g.patch(k_uid, f_uid) == 0 and g.patch(f_uid, g.MAIN_MIXER) == 0
        t = g.add_control_trip(f_uid, T.CTL_FX_CUTOFF, 0.0)
        for st in SWEEP:
            g.trip_add_step(t, *st)
        evs = sorted((int(s * 65536 + 0.5), k) for k, s in _config1_notes(1))
        want, pos = [], 0
        while pos < TOTAL:
            fr = min(BLOCK, TOTAL - pos)
            t0, t1 = _units(pos), _units(pos + fr)
            on = [(k, k, True) for at, k in evs if t0 <= at < t1]
            if on:
                g.note_events(k_uid, T.note_events(on))
            want.append(g.tick(fr))
            pos += fr
        _ORACLE["bus"] = _quantise(oracle, np.concatenate(want, axis=0))
    return _ORACLE["bus"]


@pytest.mark.parametrize("ahead", [0, 1, 2])
def test_sweep_switch_off_and_on(oracle, ahead):
    off, waits_off, dev_off = _render(False, ahead, SWEEP)
    on, waits_on, dev_on = _render(True, ahead, SWEEP)
    assert dev_off == {"cutoff": 0} and dev_on == {"cutoff": 1}
    assert off.shape == on.shape == (TOTAL, 2) and np.sqrt(np.mean(off.astype(np.float64) ** 2)) > 1e-2
    want = _oracle_sweep(oracle)
    for name, got in (("off", off), ("on", on)):
        worst = int(np.max(np.abs(_quantise(oracle, got) - want)))
        print(f"render-ahead {ahead}, switch {name}: worst |render - oracle| = {worst} LSB")
        assert worst <= 1, (name, worst)
    curved = differing = moved = 0
    diverged, last = False, None
    for pos in range(0, TOTAL, BLOCK):
        at = _units(pos)
        i, _ = LAW.scan(0.0, SWEEP, at)
        v = LAW.trip_value(0.0, SWEEP, at)
        if v is not None and v != last:                                 # the host trip sends a value when it changes
            moved, last = moved + 1, v
        same = np.array_equal(off[pos:pos + BLOCK].view(np.uint32), on[pos:pos + BLOCK].view(np.uint32))
        if i >= 0 and SWEEP[i][0] in (LAW.LOG, LAW.EXP):
            curved += 1
            if not same:
                differing, diverged = differing + 1, True
        elif not diverged:
            assert same, ("a slope / flat block differs between the switch's two sides", ahead, pos, i)
    print(f"render-ahead {ahead}: {differing} of {curved} exponential blocks differ" + ("; later blocks were held to the oracle only" if diverged else "") +
          f"; host waits off {waits_off}, on {waits_on}; the value moved in {moved} blocks")
    assert curved > 100 and differing * 10 <= curved, (differing, curved)
    assert moved > 200                                                  # (121 slope blocks, 121 exponential ones less the plateau past 1 - 10^(-12/5), one flat)
    assert waits_off - waits_on >= moved, (waits_off, waits_on, moved)


@pytest.mark.parametrize("ahead", [0, 2])
def test_a_host_path_trip_onto_the_same_effect_keeps_both_on_the_host(ahead):
    """wet-dry-mix chooses a kernel path on the host; one groove_fx_set_param for it would re-upload the host's stale cutoff over the one
    a device trip owns.  So both trips stay on the host, and the render is the switch-off render bit for bit."""
    off, _, dev_off = _render(False, ahead, SWEEP, wet_trip=True)
    on, _, dev_on = _render(True, ahead, SWEEP, wet_trip=True)
    assert dev_off == {"cutoff": 0, "wet": 0} and dev_on == {"cutoff": 0, "wet": 0}
    assert np.array_equal(off.view(np.uint32), on.view(np.uint32))
    plain, _, _ = _render(False, ahead, SWEEP)
    assert np.abs(off - plain).max() > 1e-3                              # the wet-dry-mix trip does something


def test_a_trip_onto_an_instrument_stays_on_the_host_and_the_render_is_unchanged():
    """dca-pan re-derives the bank's parameter tables (groove_bank_set_param): the host path.  The cutoff trip beside it targets another
    entity and is device-resident; its steps are slopes and a flat here, so the whole render is the same bit for bit."""
    off, _, dev_off = _render(False, 1, STRAIGHT, pan_trip=True)
    on, _, dev_on = _render(True, 1, STRAIGHT, pan_trip=True)
    assert dev_off == {"cutoff": 0, "pan": 0} and dev_on == {"cutoff": 1, "pan": 0}
    assert np.array_equal(off.view(np.uint32), on.view(np.uint32))
    assert np.abs(off[:, 0] - off[:, 1]).max() > 1e-3                    # the pan trip does something


PROJECT = """// a synthetic project of this test's own, in the reference's project schema: a drumkit through a 24 dB low-pass whose cutoff a trip of
// a flat, a slope, a logarithmic and an exponential step (a quarter note each) automates
{
  title: 'synthetic: one measure of shuffle under a four-step cutoff trip',
  clock: { bpm: 96, 'midi-ticks-per-second': 960, 'time-signature': [4, 4] },
  devices: [
    { instrument: ['kit', { drumkit: [{ 'midi-in': 10 }, { name: '707' }] }] },
    { effect: ['lp', { 'filter-low-pass-24db': { cutoff: 2400, 'passband-ripple': 0.55 } }] },
  ],
  'patch-cables': [['kit', 'lp', 'main-mixer']],
  patterns: [{ id: 'shuffle', 'note-value': 'eighth', notes: [[46, 0, 42, 42, 46, 0, 42, 44], [36, 0, 0, 36, 0, 0, 40, 0], [0, 0, 49, 0, 0, 45, 0, 47]] }],
  tracks: [{ id: 'kit-track', 'midi-channel': 10, patterns: ['shuffle'] }],
  paths: [{ id: 'four-shapes', 'note-value': 'quarter', steps: [{ flat: { value: 0.6 } }, { slope: { start: 0.6, end: 0.25 } },
                                                                  { logarithmic: { start: 0.25, end: 0.85 } }, { exponential: { start: 0.85, end: 0.3 } }] }],
  trips: [{ id: 'sweep', target: { id: 'lp', param: 'cutoff' }, paths: ['four-shapes'] }],
}
"""
PROJECT_ROWS = ([46, 0, 42, 42, 46, 0, 42, 44], [36, 0, 0, 36, 0, 0, 40, 0], [0, 0, 49, 0, 0, 45, 0, 47])
PROJECT_STEPS = [(LAW.FLAT, 0.6, 0.6, 1.0), (LAW.SLOPE, 0.6, 0.25, 1.0), (LAW.LOG, 0.25, 0.85, 1.0), (LAW.EXP, 0.85, 0.3, 1.0)]


def write_trip_project(directory):
    proj = directory / "trip.json5"
    proj.write_text(PROJECT)
    return proj


def test_cli_with_device_trips_within_one_lsb_of_the_oracle_composition(tmp_path, oracle):
    from groove_amd import host_binding as H
    proj = write_trip_project(tmp_path)
    r = subprocess.run([CLI, "--wav", "--device-trips", "--synthetic-kit", str(proj)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "Warning" not in r.stderr, r.stderr
    pcm16 = np.frombuffer((tmp_path / "trip.wav").read_bytes()[44:], dtype="<i2").reshape(-1, 2).astype(np.int32)
    total = math.ceil(4.0 * 60 / 96 * SR)
    assert len(pcm16) == total - total % BLOCK and np.abs(pcm16).max() > 500
    kpcm, kdescs, k2s = H.synthetic_kit()
    notes = [(k, i * 0.5) for row in PROJECT_ROWS for i, k in enumerate(row) if k]
    want = _quantise(oracle, _oracle_config1(oracle, kpcm, kdescs, k2s, notes, len(pcm16), BLOCK, bpm=96.0, cutoff=2400.0, ripple=0.55, trip_steps=PROJECT_STEPS))
    worst = int(np.max(np.abs(pcm16 - want)))
    print(f"--device-trips: worst |wav - oracle| = {worst} LSB")
    assert worst <= 1, worst
    # without the option: the host path, the same render to the LSB bar
    r = subprocess.run([CLI, "--wav", "--synthetic-kit", str(proj)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    off = np.frombuffer((tmp_path / "trip.wav").read_bytes()[44:], dtype="<i2").reshape(-1, 2).astype(np.int32)
    assert off.shape == pcm16.shape and np.max(np.abs(off - want)) <= 1
