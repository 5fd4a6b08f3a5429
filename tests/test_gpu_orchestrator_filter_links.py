"""GPU tier: filter links through the compiled host layer (groove_amd/host/) — Orchestrator::set_filter_links_on_device and
`groove-cli-hip --device-filter-links`: a controller device's link onto a filter's cutoff, q or passband-ripple stays on the device
(groove_ctl_filter_link_create), a signal source's among them, which is dropped with a warning while the switch is off (the default).

The synthetic project is this test's own text in the reference's schema, the shape of tests/test_gpu_orchestrator_controllers.py's: a
sampler (from a WAV file the test writes) through a passthrough into the main mixer, a raw Welsh synth through a 12 dB low-pass, and
one `controls` entry that puts the passthrough's value on the low-pass's cutoff."""
import math
import os
import subprocess

import numpy as np
import pytest

from groove_amd import patches as P, abi_types as T
from tests.test_ctl_core_cpu import signal_law_np
from tests.test_gpu_orchestrator import _mono_float, _quantise
from tests.test_gpu_orchestrator_controllers import (BLOCK, BPM, PATTERNS, ROOT_HZ, SIDECHAIN, SR, UPB, _Alloc, _pad_patch, _thump, _write_project)

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(REPO, "groove_amd", "host", "groove-cli-hip")
FILTERED = SIDECHAIN.replace('{effect: ["duck", {compressor: {threshold: 0.6, ratio: 0.25, attack: 0, release: 0}}]}',
                             '{effect: ["duck", {"filter-low-pass-12db": {cutoff: 900, q: 0.9}}]}')
CONTROLS = 'controls: [{id: "sweep-the-pad", source: "tap", target: {id: "duck", param: "cutoff"}}],'


def _project(tmp_path):
    assert FILTERED != SIDECHAIN
    proj = _write_project(tmp_path)                        # (the sample file beside it)
    proj.write_text(FILTERED % CONTROLS)
    return proj


def test_link_control_onto_a_filter_with_the_switch_off_and_on():
    from groove_amd import host_binding as H
    o = H.Orchestrator(0, SR, BPM)
    try:
        tap, lfo = o.add_signal_passthrough(), o.add_lfo_controller(T.WAVE_SINE, 2.0)
        lp, lp24, gain = (o.add_effect(k, T.fx_params()) for k in (T.FX_BIQUAD_LP12, T.FX_BIQUAD_LP24, T.FX_GAIN))
        assert o.link_control(tap, lp, "cutoff") is False and "download per block" in o.last_error()     # the default
        o.set_filter_links_on_device(True)
        assert o.link_control(tap, lp, "cutoff") is True
        assert o.link_control(tap, lp, "q") is True and o.link_control(tap, lp24, "passband-ripple") is True
        assert o.link_control(lfo, lp24, "cutoff") is True
        assert o.link_control(tap, lp24, "q") is False and "download per block" in o.last_error()       # not a parameter that kind derives from
        assert o.link_control(tap, lp, "wet-dry-mix") is False
        assert o.link_control(tap, gain, "ceiling") is True                                               # the plain links as before
        o.set_filter_links_on_device(False)
        assert o.link_control(tap, lp, "cutoff") is False and "download per block" in o.last_error()
        assert o.debug_info()["zero_segments"] == 0
    finally:
        o.close()


def test_cli_with_device_filter_links_within_one_lsb_of_the_oracle_composition(tmp_path, oracle):
    """groove-cli-hip --wav --device-filter-links against the oracle's pieces put together the way the project says: the sampler's bus is
    passed on as it is and its last frame of block b - 1 gives (numpy float32 law, bipolar; then the cutoff law) the cutoff the oracle's
    low-pass is given for block b.  Without the option the control is dropped with the warning, as before."""
    proj = _project(tmp_path)
    r = subprocess.run([CLI, "--wav", "--device-filter-links", "--assets", str(tmp_path), str(proj)], capture_output=True, text=True, timeout=120)
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
    lp = lambda hz: (T.FxParams * 1)(T.fx_params(cutoff_hz=float(hz), q=0.9))
    ofx = oracle.Fx(T.FX_BIQUAD_LP12, lp(900.0))
    events = []
    for ch, (beats, rows) in PATTERNS.items():
        for row in rows:
            for i, k in enumerate(row):
                if k:
                    events.append((int(i * beats * UPB + 0.5), len(events), ch, k, True))
                    events.append((int((i * beats + beats) * UPB + 0.5), len(events), ch, k, False))
    events.sort(key=lambda e: (e[0], e[1]))
    want, pos, v, values = [], 0, None, []
    while pos < total:
        t0, t1 = int(pos * BPM / 60.0 / SR * UPB), int((pos + BLOCK) * BPM / 60.0 / SR * UPB)
        for at, _, ch, key, on in events:
            if t0 <= at < t1:
                bank, al = banks[ch]
                for ev in (al.on(key, pos) if on else al.off(key, pos)):
                    bank.note_events(T.note_events([ev]))
        if v is not None:                                  # the control phase: what the passthrough captured from the block before
            ofx.set_params(lp(np.float32(25.0 * 800.0 ** float(v))))
            values.append(float(v))
        drums = banks[0][0].render_bus(BLOCK)
        pad = banks[1][0].render(BLOCK).sum(axis=2, keepdims=True)
        want.append(drums + oracle.mix(ofx.process(np.ascontiguousarray(pad))))
        last = drums[BLOCK - 1].astype(np.float32)
        _, vv = signal_law_np(T.CTL_LAW_BIPOLAR, last[0:1], last[1:2])
        v = vv[0]
        pos += BLOCK
    assert np.ptp(values) > 0.2                            # the cutoff really moves with the drums
    want = _quantise(oracle, np.concatenate(want, axis=0))
    assert want.shape == pcm16.shape
    worst = int(np.max(np.abs(pcm16 - want)))
    print(f"--device-filter-links: worst |wav - oracle| = {worst} LSB; value01 {min(values):.3f} .. {max(values):.3f}")
    assert worst <= 1, worst
    # the default: dropped, with the warning, and the render is another
    r = subprocess.run([CLI, "--wav", "--assets", str(tmp_path), str(proj)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "dropped: a signal source onto 'cutoff'" in r.stderr, r.stderr
    off = np.frombuffer((tmp_path / "sidechain.wav").read_bytes()[44:], dtype="<i2").reshape(-1, 2).astype(np.int32)
    assert off.shape == pcm16.shape and np.max(np.abs(off - pcm16)) > 30


def _lfo_run(on):
    from groove_amd import host_binding as H
    o = H.Orchestrator(0, SR, BPM)
    try:
        o.set_filter_links_on_device(on)
        w = o.add_welsh(P.welsh_patch(3), voices=4)
        lp = o.add_effect(T.FX_BIQUAD_LP12, T.fx_params(cutoff_hz=900.0, q=0.9))
        assert o.patch(w, lp) == 0 and o.patch(lp, o.MAIN_MIXER) == 0
        o.connect_midi_downstream(w, 0)
        seq = o.add_sequencer()
        for k, s_, d in ((60, 0.0, 1.9), (64, 0.5, 1.0)):
            o.sequencer_insert(seq, 0, k, s_, d)
        o.sequencer_set_end(seq, 2.0)
        lfo = o.add_lfo_controller(T.WAVE_TRIANGLE, 2.0)
        assert o.link_control(lfo, lp, "cutoff") is True
        before = o.debug_info()["host_waits"]
        got = o.run(BLOCK).astype(np.float64)
        waits = o.debug_info()["host_waits"] - before
        assert o.debug_info()["zero_segments"] == 0
        return got, waits
    finally:
        o.close()


def test_lfo_onto_a_cutoff_same_render_with_fewer_host_waits():
    """Switch off: the LFO's value is evaluated on the host in f64 and goes through groove_fx_set_param once per block (a wait for the
    ctx stream and a handful of copies).  Switch on: the fp32 law on the device, within 2e-7 of it, no wait.  The bar is the one
    test_lfo_onto_a_welsh_synths_pan_follows_the_oracle_bank holds its render to."""
    off, waits_off = _lfo_run(False)
    on, waits_on = _lfo_run(True)
    blocks = math.ceil(len(off) / BLOCK)
    assert off.shape == on.shape and len(off) == math.ceil(2.0 * 60 / BPM * SR)
    assert np.sqrt(np.mean(off ** 2)) > 1e-2
    rms = float(np.sqrt(np.mean((on - off) ** 2)))
    print(f"LFO -> cutoff: RMS(on - off) = {rms:.3e}; host waits over {blocks} blocks: off {waits_off}, on {waits_on}")
    assert rms <= 1e-5
    assert waits_off - waits_on >= blocks
