"""CPU tier: the project loader's controller devices and `controls` links (groove_amd/host/project.cpp; the schema's third device
class, settings/src/controllers.rs:103-112).  Parsing only — no GPU.  The project texts below are this test's own, written in the
reference's schema; the reference's controller demos are read from tests/golden/reference where they are stored."""
import ctypes as C
import json
import os

import pytest

from groove_amd import abi_types as T
from groove_amd.host_binding import HOST_LIB

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(REPO, "tests", "golden", "reference")


@pytest.fixture(scope="module")
def host():
    if not os.path.exists(HOST_LIB):
        import __graft_entry__ as g
        g.build()
    L = C.CDLL(HOST_LIB)
    for name in ("gh_project_describe", "gh_project_describe_text"):
        getattr(L, name).restype = C.c_void_p
        getattr(L, name).argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t]
    L.gh_free.argtypes = [C.c_void_p]
    return L


def describe(L, path=None, text=None, assets=""):
    err = C.create_string_buffer(512)
    p = L.gh_project_describe(path.encode(), assets.encode(), err, 512) if path else \
        L.gh_project_describe_text(text.encode(), assets.encode(), err, 512)
    if not p:
        raise RuntimeError(err.value.decode())
    s = C.string_at(p).decode()
    L.gh_free(p)
    return json.loads(s)


def project(controllers, controls, cables=None):
    """A small project: a toy instrument through a compressor, a second one through a passthrough and a low-pass, plus the given
    controller devices and controls."""
    cables = cables or '[["toy-a", "comp", "main-mixer"], ["toy-b", "tap", "lp", "main-mixer"]]'
    return """{
  title: "controllers", clock: {bpm: 100, "time-signature": [4, 4]},
  devices: [
    {instrument: ["toy-a", {"toy-instrument": [{"midi-in": 0}, {"fake-value": 0.5, dca: {gain: 0.5, pan: 0.0}}]}]},
    {instrument: ["toy-b", {"toy-instrument": [{"midi-in": 1}, {"fake-value": 0.5, dca: {gain: 0.5, pan: 0.0}}]}]},
    {effect: ["comp", {compressor: {threshold: 0.8, ratio: 0.25, attack: 0, release: 0}}]},
    {effect: ["lp", {"filter-low-pass-12db": {cutoff: 1200, q: 0.9}}]},
    {effect: ["verb", {reverb: {attenuation: 0.6, seconds: 0.4}}]},
    %s
  ],
  "patch-cables": %s,
  controls: [%s],
  patterns: [{id: "p", "note-value": "quarter", notes: [[60, 0, 64, 0]]}],
  tracks: [{id: "t0", "midi-channel": 0, patterns: ["p"]}, {id: "t1", "midi-channel": 1, patterns: ["p"]}],
}""" % (controllers, cables, controls)


LFO = '{controller: ["wobble", {lfo: [{"midi-in": 0, "midi-out": 0}, {waveform: "triangle", frequency: 2.5}]}]},'
TAP = '{controller: ["tap", {"signal-passthrough-controller": [{"midi-in": 0, "midi-out": 0}]}]},'


def test_lfo_and_passthrough_describe_without_warnings_and_both_links_resolve(host):
    d = describe(host, text=project(LFO + TAP,
                                    '{id: "duck", source: "tap", target: {id: "comp", param: "threshold"}},'
                                    '{id: "sweep", source: "wobble", target: {id: "lp", param: "cutoff"}}'))
    assert d["warnings"] == 0
    assert d["controllers"] == [{"id": "wobble", "kind": "lfo", "waveform": T.WAVE_TRIANGLE, "duty": 0.5, "frequency": 2.5},
                                {"id": "tap", "kind": "signal-passthrough-controller", "waveform": T.WAVE_SINE, "duty": 0.5, "frequency": 1}]
    assert d["controls"] == [{"id": "duck", "source": "tap", "target": "comp", "param": "threshold", "route": "device"},
                             {"id": "sweep", "source": "wobble", "target": "lp", "param": "cutoff", "route": "per-block"}]
    # `devices` is what it was: instruments and effects only, and the cable still names the passthrough
    assert [x["id"] for x in d["devices"]] == ["toy-a", "toy-b", "comp", "lp", "verb"]
    assert ["toy-b", "tap", "lp", "main-mixer"] in d["patch_cables"]


def test_lfo_waveform_forms_and_device_routes(host):
    lfo = '{controller: ["pw", {lfo: [{"midi-in": 0, "midi-out": 0}, {waveform: {"pulse-width": 0.25}, frequency: 0.5}]}]},'
    d = describe(host, text=project(lfo, '{id: "a", source: "pw", target: {id: "verb", param: "attenuation"}},'
                                         '{id: "b", source: "pw", target: {id: "toy-a", param: "pan"}},'
                                         '{id: "c", source: "pw", target: {id: "comp", param: "wet-dry-mix"}}'))
    assert d["warnings"] == 0
    assert d["controllers"] == [{"id": "pw", "kind": "lfo", "waveform": T.WAVE_PULSE_WIDTH, "duty": 0.25, "frequency": 0.5}]
    assert [(c["id"], c["route"]) for c in d["controls"]] == [("a", "device"), ("b", "per-block"), ("c", "per-block")]


def test_unknown_source_id_warns(host):
    d = describe(host, text=project(LFO, '{id: "x", source: "no-such-lfo", target: {id: "comp", param: "threshold"}}'))
    assert d["warnings"] == 1 and d["controls"] == []
    # a source that is a device of another class is no controller either
    d = describe(host, text=project(LFO, '{id: "x", source: "comp", target: {id: "verb", param: "attenuation"}}'))
    assert d["warnings"] == 1 and d["controls"] == []


def test_unknown_target_or_parameter_warns(host):
    d = describe(host, text=project(LFO, '{id: "x", source: "wobble", target: {id: "nobody", param: "threshold"}},'
                                         '{id: "y", source: "wobble", target: {id: "comp", param: "no-such-param"}}'))
    assert d["warnings"] == 2 and d["controls"] == []


def test_arpeggiator_and_test_controllers_stay_warned(host):
    arp = '{controller: ["arp", {arpeggiator: [{"midi-in": 1, "midi-out": 0}, {bpm: 100}]}]},'
    d = describe(host, text=project(arp, ""))
    assert d["warnings"] == 1 and d["controllers"] == []
    d = describe(host, text=project(arp + '{controller: ["t", {test: [{"midi-in": 0, "midi-out": 0}]}]},', ""))
    assert d["warnings"] == 2 and d["controllers"] == []


def test_noise_lfo_is_skipped_with_a_warning(host):
    noise = '{controller: ["hiss", {lfo: [{"midi-in": 0, "midi-out": 0}, {waveform: "noise", frequency: 3}]}]},'
    d = describe(host, text=project(noise, ""))
    assert d["warnings"] == 1 and d["controllers"] == []
    # ... and a control from it then has no source
    d = describe(host, text=project(noise, '{id: "x", source: "hiss", target: {id: "comp", param: "threshold"}}'))
    assert d["warnings"] == 2 and d["controls"] == []


def test_signal_onto_a_host_derived_parameter_warns(host):
    d = describe(host, text=project(TAP, '{id: "x", source: "tap", target: {id: "lp", param: "cutoff"}}'))
    assert d["warnings"] == 1 and d["controls"] == []
    assert d["controllers"][0]["id"] == "tap"   # the device itself stays (it is patched in a cable)
    d = describe(host, text=project(TAP, '{id: "x", source: "tap", target: {id: "toy-a", param: "pan"}}'))
    assert d["warnings"] == 1 and d["controls"] == []


def test_reference_controller_demos(host):
    """projects/demos/controllers of the reference: the sidechain (a passthrough in a patch cable onto a compressor's threshold) and the
    panning LFO load whole; the arpeggiator — whose behaviour is not in the reference tree — stays the one warning of its project."""
    base = f"{REF}/projects/demos/controllers"
    side = describe(host, path=f"{base}/sidechain.json", assets=f"{REF}/assets")
    assert side["warnings"] == 0
    assert [c["id"] for c in side["controllers"]] == ["sidechain-2"]
    assert side["controls"] == [{"id": "sidechain-drums-to-instrument-2", "source": "sidechain-2", "target": "compressor-2",
                                 "param": "threshold", "route": "device"}]
    assert ["drum-1", "sidechain-2", "main-mixer"] in side["patch_cables"]
    pan = describe(host, path=f"{base}/stereo-automation.json", assets=f"{REF}/assets")
    assert pan["warnings"] == 0
    assert pan["controllers"] == [{"id": "panning-lfo", "kind": "lfo", "waveform": T.WAVE_TRIANGLE, "duty": 0.5, "frequency": 2}]
    assert pan["controls"] == [{"id": "lfo-pan-1", "source": "panning-lfo", "target": "lead", "param": "pan", "route": "per-block"}]
    arp = describe(host, path=f"{base}/arpeggiator.json", assets=f"{REF}/assets")
    assert arp["warnings"] == 1 and arp["controllers"] == []
