"""CPU tier: the control links' route table and buffer layouts (groove_amd/csrc/ctl_core.h: ctl_fx_route, ctl_bank_route,
ctl_lanes_layout, ctl_trip_layout), compiled for the host through a small shim like test_ctl_core_cpu.py's.

The routes are held, over every effect kind x control index 0..99 and every bank kind x 0..99, against a table written out below from
the rule include/groove_hip.h documents for the groove_ctl_*_create calls; the predicates the older shims ask must agree with them.
The layouts are held as exact integers: the sections in order, none overlapping, the uint32 tail aligned, the total the allocation."""
import ctypes as C
import os
import subprocess

import pytest

from groove_amd import abi_types as T

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHIM = r'''
#include "groove_amd/csrc/ctl_core.h"
using namespace groove;
extern "C" {
uint32_t shim_fx_class(uint32_t index) { return ctl_fx_class(index); }
uint32_t shim_fx_route(uint32_t kind, uint32_t index) { return ctl_fx_route(kind, index); }
uint32_t shim_bank_route(uint32_t bank_kind, uint32_t index) { return ctl_bank_route(bank_kind, index); }
int shim_target_linkable(uint32_t index) { return ctl_target_linkable(index) ? 1 : 0; }
int shim_target_is_uint(uint32_t index) { return ctl_target_is_uint(index) ? 1 : 0; }
int shim_target_derived(uint32_t kind, uint32_t index) { return ctl_target_derived(kind, index) ? 1 : 0; }
int shim_bank_target_ok(uint32_t index) { return ctl_bank_target_ok(index) ? 1 : 0; }
int shim_fm_target_ok(uint32_t index) { return ctl_fm_target_ok(index) ? 1 : 0; }
int shim_sampler_target_ok(uint32_t index) { return ctl_sampler_target_ok(index) ? 1 : 0; }
void shim_lanes_layout(uint32_t n_src, uint64_t* out) {
  const CtlLanesLayout l = ctl_lanes_layout(n_src);
  out[0] = l.delta64; out[1] = l.duty64; out[2] = l.waveform; out[3] = l.law; out[4] = l.bytes;
}
void shim_trip_layout(uint32_t n_src, uint32_t n_steps, uint64_t* out) {
  const CtlTripLayout l = ctl_trip_layout(n_src, n_steps);
  out[0] = l.begin; out[1] = l.start; out[2] = l.end; out[3] = l.beats; out[4] = l.kind; out[5] = l.bytes;
}
}
'''

NONE, FLOAT, UINT, DERIVED, WET, BANK = range(6)   # ctl_core.h: CtlRoute
BANK_WELSH, BANK_FM, BANK_SAMPLER = range(3)       # ctl_core.h: BankKind
FX_KINDS = list(range(17))                         # include/groove_types.h: groove_fx_kind
FILTERS = [T.FX_BIQUAD_LP12, T.FX_BIQUAD_LP24, T.FX_BIQUAD_HP12, T.FX_BIQUAD_BP12, T.FX_BIQUAD_BS12, T.FX_BIQUAD_AP12, T.FX_BIQUAD_PEAK12,
           T.FX_BIQUAD_LSHELF12, T.FX_BIQUAD_HSHELF12]

# include/groove_hip.h, the rule of the six creates: (control index) -> (route, the kinds that have the parameter)
FX_RULE = {
    T.CTL_FX_CEILING: (FLOAT, [T.FX_GAIN]),
    T.CTL_FX_BITS: (UINT, [T.FX_BITCRUSHER]),
    T.CTL_FX_ATTENUATION: (FLOAT, [T.FX_REVERB]),
    T.CTL_FX_THRESHOLD: (FLOAT, [T.FX_COMPRESSOR, T.FX_LIMITER]),
    T.CTL_FX_CUTOFF: (DERIVED, FILTERS),
    T.CTL_FX_Q: (DERIVED, [T.FX_BIQUAD_LP12, T.FX_BIQUAD_HP12, T.FX_BIQUAD_AP12]),
    T.CTL_FX_PASSBAND_RIPPLE: (DERIVED, [T.FX_BIQUAD_LP24]),
    T.CTL_FX_WET: (WET, [k for k in FX_KINDS if k != T.FX_MIXER]),
}
BANK_RULE = {BANK_WELSH: [32, 33, 34], BANK_FM: [48, 49, 50, 51], BANK_SAMPLER: [64]}


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("ctl_route")
    src, so = d / "shim.cpp", d / "libctl_route_shim.so"
    src.write_text(SHIM)
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Werror", "-I", REPO, str(src), "-o", str(so)], check=True)
    L = C.CDLL(str(so))
    u32, p64 = C.c_uint32, C.POINTER(C.c_uint64)
    for name, res, args in (("shim_fx_class", u32, [u32]), ("shim_fx_route", u32, [u32, u32]), ("shim_bank_route", u32, [u32, u32]),
                            ("shim_target_linkable", C.c_int, [u32]), ("shim_target_is_uint", C.c_int, [u32]), ("shim_target_derived", C.c_int, [u32, u32]),
                            ("shim_bank_target_ok", C.c_int, [u32]), ("shim_fm_target_ok", C.c_int, [u32]), ("shim_sampler_target_ok", C.c_int, [u32]),
                            ("shim_lanes_layout", None, [u32, p64]), ("shim_trip_layout", None, [u32, u32, p64])):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    return L


def test_the_kinds_and_indices_are_the_headers():
    """The literal numbers above are include/groove_types.h's."""
    text = open(os.path.join(REPO, "include", "groove_types.h")).read()
    assert "GROOVE_FX_BIQUAD_HSHELF12 = 16 " in text and "GROOVE_FX_GAIN = 0," in text and "GROOVE_FX_MIXER = 7," in text
    for name, value in (("WELSH_DCA_GAIN", 32), ("WELSH_DCA_PAN", 33), ("WELSH_CUTOFF", 34), ("FM_DCA_GAIN", 48), ("FM_DCA_PAN", 49), ("FM_DEPTH", 50),
                        ("FM_BETA", 51), ("SAMPLER_GAIN", 64)):
        assert f"GROOVE_CTL_{name} = {value}" in text, name
    assert len(FILTERS) == 9 and len(set(FILTERS)) == 9


def test_fx_routes_are_the_documented_rule(shim):
    for kind in FX_KINDS:
        for index in range(100):
            route, kinds = FX_RULE.get(index, (NONE, []))
            want = route if kind in kinds else NONE
            assert shim.shim_fx_route(kind, index) == want, (kind, index)
    for index in range(100):
        assert shim.shim_fx_class(index) == FX_RULE.get(index, (NONE, []))[0], index


def test_bank_routes_are_the_documented_rule(shim):
    for bank_kind, indices in BANK_RULE.items():
        for index in range(100):
            assert shim.shim_bank_route(bank_kind, index) == (BANK if index in indices else NONE), (bank_kind, index)
    for index in range(100):
        assert shim.shim_bank_route(3, index) == NONE   # no such bank kind


def test_the_predicates_are_the_routes(shim):
    for index in range(100):
        cls = shim.shim_fx_class(index)
        assert shim.shim_target_linkable(index) == (1 if cls in (FLOAT, UINT) else 0), index
        assert shim.shim_target_is_uint(index) == (1 if cls == UINT else 0), index
        for kind in FX_KINDS:
            assert shim.shim_target_derived(kind, index) == (1 if shim.shim_fx_route(kind, index) == DERIVED else 0), (kind, index)
        assert shim.shim_bank_target_ok(index) == (1 if shim.shim_bank_route(BANK_WELSH, index) == BANK else 0), index
        assert shim.shim_fm_target_ok(index) == (1 if shim.shim_bank_route(BANK_FM, index) == BANK else 0), index
        assert shim.shim_sampler_target_ok(index) == (1 if shim.shim_bank_route(BANK_SAMPLER, index) == BANK else 0), index


@pytest.mark.parametrize("n_src", [1, 2, 65])
def test_lanes_layout(shim, n_src):
    """delta64[n], duty64[n] as uint64, then waveform[n], law[n] as uint32: 24 bytes a lane."""
    out = (C.c_uint64 * 5)()
    shim.shim_lanes_layout(n_src, out)
    delta64, duty64, waveform, law, total = list(out)
    assert (delta64, duty64, waveform, law, total) == (0, 8 * n_src, 16 * n_src, 20 * n_src, 24 * n_src)
    sections = [(delta64, 8 * n_src), (duty64, 8 * n_src), (waveform, 4 * n_src), (law, 4 * n_src)]
    for (at, size), (nxt, _) in zip(sections, sections[1:]):
        assert at + size <= nxt                       # no overlap
    assert sections[-1][0] + sections[-1][1] == total  # the total is the allocation
    assert delta64 % 8 == 0 and duty64 % 8 == 0 and waveform % 4 == 0 and law % 4 == 0


@pytest.mark.parametrize("n_steps", [1, 3])
@pytest.mark.parametrize("n_src", [1, 2, 65])
def test_trip_layout(shim, n_src, n_steps):
    """begin[n_steps + 1][n_src], start, end, beats [n_steps][n_src] as f64, then kind[n_steps][n_src] as uint32, in whole 64-bit words."""
    out = (C.c_uint64 * 6)()
    shim.shim_trip_layout(n_src, n_steps, out)
    begin, start, end, beats, kind, total = list(out)
    rows = n_steps * n_src
    assert (begin, start, end, beats, kind) == (0, 8 * (rows + n_src), 8 * (2 * rows + n_src), 8 * (3 * rows + n_src), 8 * (4 * rows + n_src))
    sections = [(begin, 8 * (rows + n_src)), (start, 8 * rows), (end, 8 * rows), (beats, 8 * rows), (kind, 4 * rows)]
    for (at, size), (nxt, _) in zip(sections, sections[1:]):
        assert at + size <= nxt
    assert kind % 4 == 0 and all(at % 8 == 0 for at, _ in sections[:4])
    assert total % 8 == 0 and kind + 4 * rows <= total < kind + 4 * rows + 8
    assert total == 8 * (4 * rows + n_src + (rows + 1) // 2)   # what the create allocates and uploads
