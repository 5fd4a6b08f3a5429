"""CPU tier: the trip source of a control link (groove_amd/csrc/ctl_core.h ctl_trip_*; docs/DSP_SPEC.md section 13), compiled for the
host through a shim of this test's own and held, bit for bit, against the host trip's law restated in Python (tests/ctl_trip_law.py:
ControlTrip::work's first-match scan and ControlTrip::value_at; math.log10 is the same C library's)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from groove_amd import abi_types as T
from tests import ctl_trip_law as LAW

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHIM = r'''
#include "groove_amd/csrc/ctl_core.h"
using namespace groove;
extern "C" {
void shim_trip_begins(double start_beat, const double* beats, uint32_t n_steps, double* begin, size_t stride) {
  ctl_trip_begins(start_beat, beats, 1, n_steps, begin, stride);
}
int32_t shim_trip_find(const double* begin, size_t stride, uint32_t n_steps, uint64_t at_units) {
  return ctl_trip_find(begin, stride, n_steps, ctl_trip_now(at_units));
}
double shim_trip_now(uint64_t at_units) { return ctl_trip_now(at_units); }
double shim_trip_value(uint32_t kind, double start, double end, double begin, double beats, double now) {
  return ctl_trip_value(kind, start, end, begin, beats, now);
}
int shim_trip_kind_ok(uint32_t kind) { return ctl_trip_kind_ok(kind) ? 1 : 0; }
float shim_target_float_f64(double v) { return ctl_target_float_f64(v); }
uint32_t shim_target_bits_f64(double v) { return ctl_target_bits_f64(v); }
float shim_derived_param_f64(uint32_t index, double v) { return ctl_derived_param_f64(index, v); }
float shim_derived_param(uint32_t index, float v) { return ctl_derived_param(index, v); }
}
'''

KINDS = [LAW.FLAT, LAW.SLOPE, LAW.LOG, LAW.EXP]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("ctl_trip")
    src, so = d / "shim.cpp", d / "libctl_trip_shim.so"
    src.write_text(SHIM)
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Werror", "-I", REPO,
                    "-I", os.path.join(REPO, "include"), str(src), "-o", str(so)], check=True)
    L = C.CDLL(str(so))
    u64, u32, f32, f64, dp = C.c_uint64, C.c_uint32, C.c_float, C.c_double, C.POINTER(C.c_double)
    for name, res, args in (("shim_trip_begins", None, [f64, dp, u32, dp, C.c_size_t]), ("shim_trip_find", C.c_int32, [dp, C.c_size_t, u32, u64]),
                            ("shim_trip_now", f64, [u64]), ("shim_trip_value", f64, [u32, f64, f64, f64, f64, f64]), ("shim_trip_kind_ok", C.c_int, [u32]),
                            ("shim_target_float_f64", f32, [f64]), ("shim_target_bits_f64", u32, [f64]), ("shim_derived_param_f64", f32, [u32, f64]),
                            ("shim_derived_param", f32, [u32, f32])):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    return L


def _bits(x):
    return struct.pack("<d", x)


def _trip(n_steps, exact, seed):
    """start_beat and n_steps steps: `exact` beats are whole units (every begin is a time a block can start at exactly), the others
    are not (0.1, a third, ...), so that the f64 accumulation order matters."""
    rng = np.random.default_rng(seed)
    kinds = [KINDS[i % 4] for i in range(n_steps)]
    if exact:
        start = 3 * 65536 // 8 / 65536.0
        beats = [int(u) / 65536.0 for u in rng.integers(1, 3000, n_steps)]
    else:
        start = 0.1
        beats = [float(b) for b in rng.choice([0.1, 1.0 / 3.0, 0.7, 1e-3, 2.0 / 7.0, 1.25], n_steps)]
    return start, [(k, float(rng.uniform(0, 1)), float(rng.uniform(0, 1)), b) for k, b in zip(kinds, beats)]


def _shim_begins(shim, start, steps, stride=1):
    n = len(steps)
    beats = (C.c_double * n)(*[s[3] for s in steps])
    begin = (C.c_double * ((n + 1) * stride))()
    shim.shim_trip_begins(start, beats, n, begin, stride)
    return begin


@pytest.mark.parametrize("exact", [True, False], ids=["whole-units", "fractions"])
@pytest.mark.parametrize("n_steps", [1, 2, 7, 4096])
def test_step_search_finds_the_hosts_first_match(shim, n_steps, exact):
    start, steps = _trip(n_steps, exact, 11 * n_steps + exact)
    want_begins = LAW.begins(start, steps)
    for stride in (1, 3):                                             # the device table is [step][lane]: a stride of n_src
        begin = _shim_begins(shim, start, steps, stride)
        assert [_bits(begin[i * stride]) for i in range(n_steps + 1)] == [_bits(b) for b in want_begins]
        # each begin exactly (whole units) or the units either side of it, one unit before and after, before the start, at and after the end
        ats = {0, 1, int(want_begins[-1] * 65536) + 5, int(want_begins[-1] * 65536) + 70000}
        some = range(n_steps + 1) if n_steps <= 64 else sorted(set(range(0, n_steps + 1, 61)) | {1, n_steps - 1, n_steps})   # (the scan is O(steps))
        for b in (want_begins[i] for i in some):
            u = int(b * 65536)
            ats.update(a for a in (u - 1, u, u + 1, u + 2) if a >= 0)
        hit = set()
        for at in sorted(ats):
            want, _ = LAW.scan(start, steps, at)
            got = shim.shim_trip_find(begin, stride, n_steps, at)
            assert got == want, (n_steps, exact, stride, at, got, want)
            hit.add(got)
        assert hit >= set(range(-1, n_steps)) & ({-1} | set(some))      # every step looked at, and "no step", has been the answer
        if exact:
            for i, b in enumerate(want_begins[:-1]):
                at = int(b * 65536)
                assert at / 65536.0 == b and shim.shim_trip_find(begin, stride, n_steps, at) == i           # begin[i] itself opens step i
                assert shim.shim_trip_find(begin, stride, n_steps, at - 1) == i - 1                         # one unit earlier: the step before (or none)
            at_end = int(want_begins[-1] * 65536)
            assert shim.shim_trip_find(begin, stride, n_steps, at_end) == -1 and shim.shim_trip_find(begin, stride, n_steps, at_end - 1) == n_steps - 1
    assert shim.shim_trip_now(98765) == 98765 / 65536.0


def _ts():
    thr = LAW.THRESHOLD
    near = [thr, np.nextafter(thr, 0.0), np.nextafter(thr, 1.0), 1.0 - thr, np.nextafter(1.0 - thr, 0.0), np.nextafter(1.0 - thr, 2.0)]
    edge = [0.0, 1.0, -0.25, 1.25, 5e-324, np.nextafter(1.0, 0.0), 0.5, 1.0 / 3.0]
    return [float(t) for t in edge + near + list(np.linspace(0.0, 1.0, 1025)) + list(np.random.default_rng(3).uniform(0, 1, 2048))]


@pytest.mark.parametrize("kind", KINDS, ids=["flat", "slope", "logarithmic", "exponential"])
def test_value_is_value_at_bit_for_bit(shim, kind):
    for start, end in ((0.0, 1.0), (0.9, 0.2), (0.3, 0.3), (0.15, 0.9), (-0.5, 1.5), (1.0 / 3.0, 0.7)):
        for t in _ts():
            # begin 0 and beats 1: (now - 0) / 1 is t itself
            got, want = shim.shim_trip_value(kind, start, end, 0.0, 1.0, t), LAW.value_at(kind, start, end, t)
            assert _bits(got) == _bits(want), (kind, start, end, t, got, want)
    assert LAW.value_at(LAW.LOG, 0.0, 1.0, np.nextafter(LAW.THRESHOLD, 0.0)) == 0.0 and LAW.value_at(LAW.EXP, 0.0, 1.0, np.nextafter(1.0 - LAW.THRESHOLD, 2.0)) == 1.0
    for k in range(8):
        assert bool(shim.shim_trip_kind_ok(k)) == (k < 4)


@pytest.mark.parametrize("exact", [True, False], ids=["whole-units", "fractions"])
def test_a_whole_trip_at_every_block_start(shim, exact):
    """Search and value together, as the kernel puts them together: t is (now - begin[i]) / beats[i]."""
    start, steps = _trip(7, exact, 77)
    begin = _shim_begins(shim, start, steps)
    end_units = int(LAW.begins(start, steps)[-1] * 65536) + 300
    inside = 0
    for at in range(0, end_units, 97):
        i = shim.shim_trip_find(begin, 1, 7, at)
        want = LAW.trip_value(start, steps, at)
        assert (i < 0) == (want is None), at
        if i >= 0:
            kind, s, e, beats = steps[i]
            assert _bits(shim.shim_trip_value(kind, s, e, begin[i], beats, shim.shim_trip_now(at))) == _bits(want), at
            inside += 1
    assert inside > 50


def test_target_laws_in_f64_are_groove_fx_set_params(shim):
    vals = [0.0, 1.0, -0.5, 1.5, 0.0625, np.nextafter(0.0625, 0.0), 0.5, np.nextafter(1.0, 0.0), 1.0 / 3.0] + list(np.random.default_rng(5).uniform(-0.1, 1.1, 2048))
    for v in (float(x) for x in vals):
        assert shim.shim_target_float_f64(v) == LAW.param_of(T.CTL_FX_CEILING, v)[1]
        assert shim.shim_target_bits_f64(v) == LAW.param_of(T.CTL_FX_BITS, v)[1]
        for index in (T.CTL_FX_CUTOFF, T.CTL_FX_Q, T.CTL_FX_PASSBAND_RIPPLE):
            assert shim.shim_derived_param_f64(index, v) == LAW.param_of(index, v)[1], (index, v)
            f = float(np.float32(v))                                  # the float sources' form is the same law of the float
            assert shim.shim_derived_param(index, f) == shim.shim_derived_param_f64(index, f)


def test_the_gpu_comparisons_trip_gives_the_same_parameters_on_both_sides(shim):
    """The trip tests/test_gpu_ctl_trips.py runs: at every block start the shim (the device's text, compiled for the host) and the Python
    law (what that test's host arm sends) give the same parameter for every target — zero differing parameters, so whatever differs
    between the arms on the GPU comes from the device's math library."""
    steps, start = LAW.MAIN_STEPS, LAW.MAIN_START
    begin = _shim_begins(shim, start, steps)
    where = LAW.main_block_steps()
    assert where[:3] == [-1, -1, 0] and where[5:7] == [0, 1] and where[-2:] == [-1, -1] and set(where) == {-1, 0, 1, 2, 3}
    assert 2 * LAW.BLOCK_UNITS / 65536.0 == begin[0] and 6 * LAW.BLOCK_UNITS / 65536.0 == begin[1]       # blocks exactly on a begin
    differing = 0
    for k in range(LAW.MAIN_BLOCKS):
        at = k * LAW.BLOCK_UNITS
        i = shim.shim_trip_find(begin, 1, len(steps), at)
        assert i == where[k]
        if i < 0:
            continue
        kind, s, e, beats = steps[i]
        got, want = shim.shim_trip_value(kind, s, e, begin[i], beats, shim.shim_trip_now(at)), LAW.trip_value(start, steps, at)
        for index in (T.CTL_FX_CEILING, T.CTL_FX_BITS, T.CTL_FX_CUTOFF, T.CTL_FX_Q, T.CTL_FX_PASSBAND_RIPPLE):
            mine = {T.CTL_FX_CEILING: shim.shim_target_float_f64(got), T.CTL_FX_BITS: shim.shim_target_bits_f64(got)}.get(index)
            if mine is None:
                mine = shim.shim_derived_param_f64(index, got)
            differing += mine != LAW.param_of(index, want)[1]
    assert differing == 0
