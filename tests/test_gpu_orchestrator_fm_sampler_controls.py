"""GPU tier: controls onto FM synths and drumkits through the compiled host layer (groove_amd/host/).  With
Orchestrator::set_instrument_controls_on_device off, a ControlTrip or an LFO `controls` link onto an FM synth's pan, gain, depth or beta or
a drumkit's gain goes through groove_bank_set_param, which serves those banks now; with it on, the control lives in the library
(groove_ctl_bank_trip_create / groove_ctl_bank_link_create) and costs no re-upload of the bank and no host wait per automated block.

The project: a four-voice FM synth under a pan slope and a depth slope, and a drumkit (groove_amd.patches.drum_bank) under a gain fade,
both straight into the main mixer; 2 beats at 120 bpm.  Every trip is a slope — evaluated without a logarithm — so the renders on the two
sides of the switch must be the same sample for sample; and both differ from the project without its trips, which is what a library whose
FM and sampler banks expose no controls rendered whatever the trips said."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from groove_amd import abi_types as T, patches as P
from tests import ctl_trip_law as LAW

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(REPO, "groove_amd", "host", "groove-cli-hip")
PROJECT = os.path.join(REPO, "tests", "data", "synthetic-fm-pan-lfo.json5")
SR, BPM, BLOCK, BEATS = 44100, 120.0, 256, 2.0
TOTAL = math.ceil(BEATS * 60 / BPM * SR)
PAN, DEPTH, FADE = (LAW.SLOPE, 0.1, 0.9, 2.0), (LAW.SLOPE, 0.9, 0.1, 2.0), (LAW.SLOPE, 1.0, 0.25, 2.0)
_BANK = {}


def _kit():
    if not _BANK:
        pcm, descs, _ = P.drum_bank(scale=0.2)
        _BANK["kit"] = (pcm, descs, [k % P.BANK_BUFFERS for k in range(128)])
    return _BANK["kit"]


def _fm_patch():
    p = P.fm_patch(1)
    p.depth, p.beta = 1.0, 0.9
    p.carrier_envelope = T.EnvelopeParams(0.01, 0.2, 0.8, 0.3)
    p.dca_gain, p.dca_pan = 0.8, 0.0
    return p


def _units(frame):
    return int(frame * BPM / 60.0 / SR * 65536)


def _build(o, fm=True, kit=True, trips=True):
    """The project (or its FM synth or its drumkit alone); returns ({trip: uid}, {instrument: uid})."""
    seq = o.add_sequencer()
    uids, inst = {}, {}
    if fm:
        f = inst["fm"] = o.add_fm(_fm_patch(), voices=4)
        assert f > 0 and o.patch(f, o.MAIN_MIXER) == 0
        o.connect_midi_downstream(f, 0)
        for k, s_, d in ((57, 0.0, 1.9), (64, 0.5, 1.0), (69, 1.0, 0.9)):
            o.sequencer_insert(seq, 0, k, s_, d)
        if trips:
            for name, param, step in (("pan", "pan", PAN), ("depth", "depth", DEPTH)):
                uids[name] = o.add_control_trip(f, param, 0.0)
                o.control_trip_add_step(uids[name], *step)
    if kit:
        pcm, descs, k2s = _kit()
        d = inst["kit"] = o.add_drumkit(pcm, descs, k2s)
        assert d > 0 and o.patch(d, o.MAIN_MIXER) == 0
        o.connect_midi_downstream(d, 10)
        for i in range(8):                                            # a hit every quarter of a beat, eight drums in turn: every block sounds
            o.sequencer_insert(seq, 10, 36 + 5 * i, 0.25 * i, 0.2)
        if trips:
            uids["gain"] = o.add_control_trip(d, "gain", 0.0)
            o.control_trip_add_step(uids["gain"], *FADE)
    o.sequencer_set_end(seq, BEATS)
    return uids, inst


def _render(on, ahead, **kw):
    """(bus, host waits of the run, {trip: on the device?})"""
    from groove_amd.host_binding import Orchestrator
    o = Orchestrator(0, SR, BPM)
    try:
        o.set_render_ahead(ahead)
        o.set_instrument_controls_on_device(on)
        uids, _ = _build(o, **kw)
        before = o.debug_info()["host_waits"]
        got = o.run(BLOCK)
        waits = o.debug_info()["host_waits"] - before
        info = o.debug_info()
        assert info["zero_segments"] == 0 and info["fast_table_misses"] == 0
        return got, waits, {name: o.control_trip_on_device(u) for name, u in uids.items()}
    finally:
        o.close()


@pytest.mark.parametrize("ahead", [0, 1, 2])
def test_trips_onto_an_fm_synth_and_a_drumkit_switch_off_and_on(ahead):
    off, waits_off, dev_off = _render(False, ahead)
    on, waits_on, dev_on = _render(True, ahead)
    plain, _, _ = _render(False, ahead, trips=False)
    assert dev_off == {"pan": 0, "depth": 0, "gain": 0} and dev_on == {"pan": 1, "depth": 1, "gain": 1}
    assert off.shape == on.shape == plain.shape == (TOTAL, 2) and np.sqrt(np.mean(off.astype(np.float64) ** 2)) > 1e-2
    assert np.array_equal(off.view(np.uint32), on.view(np.uint32))                       # sample for sample
    assert np.abs(off - plain).max() > 1e-2 and np.abs(on - plain).max() > 1e-2          # the automation is rendered, on both sides
    q = TOTAL // 4
    e = on.astype(np.float64) ** 2
    assert e[:q, 0].sum() > e[:q, 1].sum() and e[-q:, 1].sum() > e[-q:, 0].sum()         # the image moves: left and right energy cross
    print(f"render-ahead {ahead}: host waits off {waits_off}, on {waits_on}")
    assert waits_on < waits_off, (waits_off, waits_on)


def test_the_drumkit_fades_by_the_trips_ratio_and_the_fm_synth_alone_moves():
    faded, _, dev = _render(True, 1, fm=False)
    plain, _, _ = _render(True, 1, fm=False, trips=False)
    assert dev == {"gain": 1}
    blocks = TOTAL // BLOCK
    rms = lambda x, k: float(np.sqrt(np.mean(x[k * BLOCK:(k + 1) * BLOCK].astype(np.float64) ** 2)))
    first, last = 0, blocks - 1
    assert rms(plain, first) > 1e-3 and rms(plain, last) > 1e-3
    want_last = float(np.float32(LAW.trip_value(0.0, [FADE], _units(last * BLOCK))))
    got_first, got_last = rms(faded, first) / rms(plain, first), rms(faded, last) / rms(plain, last)
    print(f"drumkit fade: first block x{got_first:.6f}, last block x{got_last:.6f} (the trip: x{want_last:.6f})")
    assert got_first == 1.0 and abs(got_last - want_last) <= 1e-6 and want_last < 0.3
    # the FM synth alone, depth and pan against pan alone: the depth trip changes the timbre, not only the level
    both, _, _ = _render(True, 1, kit=False)
    still, _, _ = _render(True, 1, kit=False, trips=False)
    assert np.abs(both - still).max() > 1e-2


def test_a_name_the_kind_lacks_is_refused_when_the_control_is_made():
    from groove_amd.host_binding import Orchestrator
    o = Orchestrator(0, SR, BPM)
    try:
        _, inst = _build(o, trips=False)
        lfo = o.add_lfo_controller(T.WAVE_TRIANGLE, 2.0)
        with pytest.raises(RuntimeError, match="unknown control name"):
            o.add_control_trip(inst["kit"], "cutoff", 0.0)
        with pytest.raises(RuntimeError, match="unknown control name"):
            o.link_control(lfo, inst["fm"], "cutoff")
        for name in ("pan", "depth", "beta", "dca-gain"):
            with pytest.raises(RuntimeError, match="unknown control name"):
                o.add_control_trip(inst["kit"], name, 0.0)
        assert o.add_control_trip(inst["kit"], "gain", 0.0) > 0
        for name in ("gain", "dca-gain", "pan", "dca-pan", "depth", "beta"):
            assert o.link_control(lfo, inst["fm"], name) is True
        assert o.link_control(lfo, inst["kit"], "gain") is True
        tap = o.add_signal_passthrough()
        assert o.link_control(tap, inst["fm"], "pan") is False          # a signal source onto an instrument stays dropped
    finally:
        o.close()


def test_cli_an_lfo_onto_an_fm_synths_pan_with_and_without_device_instrument_controls(tmp_path):
    proj = tmp_path / "sway.json5"
    shutil.copy(PROJECT, proj)
    wavs = {}
    for name, flags in (("on", ["--device-instrument-controls"]), ("off", [])):
        r = subprocess.run([CLI, "--wav"] + flags + ["--assets", str(tmp_path), str(proj)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "Warning" not in r.stderr and "Warning" not in r.stdout, (name, r.stderr)
        wavs[name] = np.frombuffer((tmp_path / "sway.wav").read_bytes()[44:], dtype="<i2").reshape(-1, 2).astype(np.int32)
    total = math.ceil(4.0 * 60 / 120.0 * SR)
    total -= total % BLOCK
    assert wavs["on"].shape == wavs["off"].shape == (total, 2) and np.abs(wavs["on"]).max() > 2000
    worst = int(np.abs(wavs["on"] - wavs["off"]).max())
    print(f"--device-instrument-controls on against off: worst difference {worst} LSB")
    assert worst <= 1                                                # the smooth LFO's host closed form is the device's only to 2e-7
    # the LFO is heard: a 1 Hz triangle swings the image to one side and to the other within every second
    e = wavs["on"].astype(np.float64) ** 2
    tenth = SR // 10
    ratio = [e[k * tenth:(k + 1) * tenth, 0].sum() / max(e[k * tenth:(k + 1) * tenth, 1].sum(), 1.0) for k in range(total // tenth)]
    assert max(ratio) > 4.0 and min(ratio) < 0.25, (min(ratio), max(ratio))
