"""CPU tier: the control links' value laws and target laws (groove_amd/csrc/ctl_core.h, docs/DSP_SPEC.md section 13), compiled for
the host through a small shim of this test's own and held against closed forms.

The LFO law is checked against the oscillator's closed form evaluated in Python integers and exact fractions from the SAME 64-bit
increment: the edge waveforms (square, pulse-width) exactly, the smooth ones within 2e-7 — the sine polynomial's stated 1e-7 bound
(dsp_core.h sin_turns_folded), halved by the law, plus two fp32 roundings near 1 (6e-8 each).  The signal laws and the target laws are
checked bit for bit against numpy float32."""
import ctypes as C
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from groove_amd import abi_types as T

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHIM = r'''
#include "groove_amd/csrc/ctl_core.h"
using namespace groove;
extern "C" {
uint64_t shim_delta64(double f, double sr) { return ctl_lfo_delta64(f, sr); }
uint64_t shim_duty64(uint32_t w, float duty) { return ctl_lfo_duty64(w, duty); }
int shim_lfo_waveform_ok(uint32_t w) { return ctl_lfo_waveform_ok(w) ? 1 : 0; }
uint64_t shim_lfo_phase(uint64_t delta, uint64_t n0) { return ctl_lfo_phase(delta, n0); }
float shim_lfo_value01(uint32_t w, uint64_t delta, uint64_t duty, uint64_t n0) { return ctl_lfo_value01(w, delta, duty, n0); }
double shim_lfo_value01_f64(uint32_t w, uint64_t delta, uint64_t duty, uint64_t n0) { return ctl_lfo_value01_f64(w, delta, duty, n0); }
void shim_signal(const float* l, const float* r, uint32_t law, float* m, float* v, size_t n) {
  for (size_t i = 0; i < n; ++i) { m[i] = ctl_signal_mono(l[i], r[i]); v[i] = ctl_signal_value01(law, m[i]); }
}
int shim_signal_law_ok(uint32_t law) { return ctl_signal_law_ok(law) ? 1 : 0; }
int shim_target_linkable(uint32_t index) { return ctl_target_linkable(index) ? 1 : 0; }
int shim_target_is_uint(uint32_t index) { return ctl_target_is_uint(index) ? 1 : 0; }
void shim_target(const float* v, float* as_float, uint32_t* as_bits, size_t n) {
  for (size_t i = 0; i < n; ++i) { as_float[i] = ctl_target_float(v[i]); as_bits[i] = ctl_target_bits(v[i]); }
}
}
'''

SR = 44100.0
SMOOTH = {"sine": T.WAVE_SINE, "triangle": T.WAVE_TRIANGLE, "sawtooth": T.WAVE_SAWTOOTH, "triangle-sine": T.WAVE_TRIANGLE_SINE}
FREQS = [0.0, 0.5, 2.0, 5.3, 37.25, 440.0]
N0S = [0, 1, 255, 256, 257, 44100 * 3 + 17, 2 ** 31 - 1, 2 ** 33 + 5, 2 ** 40 + 123]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("ctl_core")
    src, so = d / "shim.cpp", d / "libctl_shim.so"
    src.write_text(SHIM)
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Werror", "-I", REPO, str(src), "-o", str(so)], check=True)
    L = C.CDLL(str(so))
    u64, u32, f32, f64 = C.c_uint64, C.c_uint32, C.c_float, C.c_double
    fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    for name, res, args in (("shim_delta64", u64, [f64, f64]), ("shim_duty64", u64, [u32, f32]), ("shim_lfo_waveform_ok", C.c_int, [u32]),
                            ("shim_lfo_phase", u64, [u64, u64]), ("shim_lfo_value01", f32, [u32, u64, u64, u64]),
                            ("shim_lfo_value01_f64", f64, [u32, u64, u64, u64]), ("shim_signal", None, [fp, fp, u32, fp, fp, C.c_size_t]),
                            ("shim_signal_law_ok", C.c_int, [u32]), ("shim_target_linkable", C.c_int, [u32]), ("shim_target_is_uint", C.c_int, [u32]),
                            ("shim_target", None, [fp, fp, up, C.c_size_t])):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    return L


def _delta64(f, sr=SR):
    """turns_to_inc(f / SR) for f >= 0: the fraction of a turn per frame, as a 64-bit increment (the same f64 expression)."""
    t = f / sr
    return int((t - math.floor(t)) * 18446744073709551616.0)


def _closed_form(name, phase):
    """The oscillator of DSP_SPEC section 2 at position p = phase / 2^64, exactly (fractions), except the sine (f64 libm)."""
    p = Fraction(phase, 2 ** 64)
    if name == "sine":
        return math.sin(2.0 * math.pi * float(p)) if phase else 0.0
    if name == "triangle":
        return float(4 * abs(p - math.floor(p + Fraction(1, 2))) - 1)
    if name == "sawtooth":
        return float(2 * (p - math.floor(p + Fraction(1, 2))))
    if name == "triangle-sine":
        return float(4 * abs(p - math.floor(p + Fraction(3, 4)) + Fraction(1, 4)) - 1)
    raise AssertionError(name)


def test_increment_is_the_device_oscillators(shim):
    for f in FREQS + [SR - 1.0, 0.1]:
        assert shim.shim_delta64(f, SR) == _delta64(f), f
    assert shim.shim_delta64(2.0, 48000.0) == _delta64(2.0, 48000.0)


def test_phase_is_the_wrapped_product(shim):
    for f in FREQS:
        d = _delta64(f)
        for n0 in N0S:
            assert shim.shim_lfo_phase(d, n0) == (d * n0) % 2 ** 64
    assert shim.shim_lfo_phase(_delta64(2.0), 0) == 0  # the first-tick rule: frame 0 is at phase 0


@pytest.mark.parametrize("name", sorted(SMOOTH))
def test_smooth_lfo_waveforms_within_2e_7(shim, name):
    worst = 0.0
    for f in FREQS:
        d = _delta64(f)
        for n0 in N0S:
            phase = (d * n0) % 2 ** 64
            want = (_closed_form(name, phase) + 1.0) * 0.5
            got = shim.shim_lfo_value01(SMOOTH[name], d, 2 ** 63, n0)
            worst = max(worst, abs(got - want))
            assert abs(got - want) <= 2e-7, (name, f, n0, got, want)
            # the host's f64 form of the same law (links onto parameters the host derives) sits on the closed form
            assert abs(shim.shim_lfo_value01_f64(SMOOTH[name], d, 2 ** 63, n0) - want) <= 1e-12, (name, f, n0)
    print(f"{name}: worst |fp32 law - closed form| = {worst:.3e}")


def test_edge_lfo_waveforms_are_exact(shim):
    for f in FREQS:
        d = _delta64(f)
        for n0 in N0S:
            phase = (d * n0) % 2 ** 64
            assert shim.shim_lfo_value01(T.WAVE_SQUARE, d, shim.shim_duty64(T.WAVE_SQUARE, 0.1), n0) == (1.0 if phase < 2 ** 63 else 0.0), (f, n0)
            for duty in (0.25, 0.5, 0.9):
                duty64 = shim.shim_duty64(T.WAVE_PULSE_WIDTH, duty)
                assert duty64 == int(float(np.float32(duty)) * 18446744073709549568.0)
                assert shim.shim_lfo_value01(T.WAVE_PULSE_WIDTH, d, duty64, n0) == (1.0 if phase < duty64 else 0.0), (f, n0, duty)
    # an edge that lands exactly on a frame is decided by the exact counter: 11,025 Hz at 44,100 Hz steps a quarter turn per frame
    d = _delta64(11025.0)
    assert d == 2 ** 62
    assert [shim.shim_lfo_value01(T.WAVE_SQUARE, d, 2 ** 63, n) for n in range(5)] == [1.0, 1.0, 0.0, 0.0, 1.0]
    assert [shim.shim_lfo_value01(T.WAVE_SQUARE, d, 2 ** 63, 2 ** 33 + n) for n in range(5)] == [1.0, 1.0, 0.0, 0.0, 1.0]


def test_noise_and_none_are_no_lfo(shim):
    ok = {T.WAVE_SINE, T.WAVE_SQUARE, T.WAVE_PULSE_WIDTH, T.WAVE_TRIANGLE, T.WAVE_SAWTOOTH, T.WAVE_TRIANGLE_SINE}
    for w in range(16):
        assert bool(shim.shim_lfo_waveform_ok(w)) == (w in ok), w


def _signal_inputs():
    rng = np.random.default_rng(20240613)
    edge = np.array([0.0, -0.0, 1.0, -1.0, 0.5, -0.5, 1.5, -1.5, 3.0, -3.0, 1e-30, -1e-30, 0.99999994, -0.99999994, 1e-8, 0.33333334], dtype=np.float32)
    left = np.concatenate([np.repeat(edge, len(edge)), rng.uniform(-1.5, 1.5, 4096).astype(np.float32)])
    right = np.concatenate([np.tile(edge, len(edge)), rng.uniform(-1.5, 1.5, 4096).astype(np.float32)])
    return left, right


def signal_law_np(law, left, right):
    """(m, value01) of the three signal laws in numpy float32 — the reference the GPU tests use too."""
    one, half = np.float32(1.0), np.float32(0.5)
    m = np.clip((left.astype(np.float32) + right.astype(np.float32)) * half, -one, one).astype(np.float32)
    if law == T.CTL_LAW_AMPLITUDE:
        v = np.abs(m)
    elif law == T.CTL_LAW_AMPLITUDE_INVERTED:
        v = one - np.abs(m)
    else:
        v = (m + one) * half
    return m, v.astype(np.float32)


@pytest.mark.parametrize("law", [T.CTL_LAW_BIPOLAR, T.CTL_LAW_AMPLITUDE, T.CTL_LAW_AMPLITUDE_INVERTED])
def test_signal_laws_bit_for_bit(shim, law):
    left, right = _signal_inputs()
    m, v = np.empty_like(left), np.empty_like(left)
    fp = C.POINTER(C.c_float)
    shim.shim_signal(left.ctypes.data_as(fp), right.ctypes.data_as(fp), law, m.ctypes.data_as(fp), v.ctypes.data_as(fp), left.size)
    want_m, want_v = signal_law_np(law, left, right)
    assert np.array_equal(m.view(np.uint32), want_m.view(np.uint32))
    assert np.array_equal(v.view(np.uint32), want_v.view(np.uint32))
    assert shim.shim_signal_law_ok(law) and not shim.shim_signal_law_ok(3)


def test_target_laws_bit_for_bit(shim):
    rng = np.random.default_rng(7)
    v = np.concatenate([np.array([0.0, 1.0, 0.0625, 0.06249999, 0.5, 0.99999994, 1.9375, 2.0, 2.5, 1e-9], dtype=np.float32),
                        np.arange(0, 40, dtype=np.float32) / np.float32(16), rng.uniform(0.0, 1.0, 4096).astype(np.float32)])
    as_float, as_bits = np.empty_like(v), np.empty(v.size, dtype=np.uint32)
    shim.shim_target(v.ctypes.data_as(C.POINTER(C.c_float)), as_float.ctypes.data_as(C.POINTER(C.c_float)),
                     as_bits.ctypes.data_as(C.POINTER(C.c_uint32)), v.size)
    # ceiling, threshold, attenuation: the float itself
    assert np.array_equal(as_float.view(np.uint32), v.view(np.uint32))
    # bits: (uint32_t)(v * 16), capped at 31 — groove_fx_set_param's law followed by the upload's cap
    want = np.minimum((v * np.float32(16)).astype(np.uint32), np.uint32(31))
    assert np.array_equal(as_bits, want)
    assert as_bits.max() == 31 and as_bits.min() == 0
    linkable = {T.CTL_FX_CEILING, T.CTL_FX_BITS, T.CTL_FX_ATTENUATION, T.CTL_FX_THRESHOLD}
    for index in list(range(12)) + [T.CTL_WELSH_DCA_GAIN, T.CTL_WELSH_DCA_PAN, T.CTL_WELSH_CUTOFF]:
        assert bool(shim.shim_target_linkable(index)) == (index in linkable), index
        assert bool(shim.shim_target_is_uint(index)) == (index == T.CTL_FX_BITS)
