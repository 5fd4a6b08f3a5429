"""CPU tier: the target laws of a BANK link (groove_amd/csrc/ctl_core.h: ctl_bank_*_f64 and pan_gains, docs/DSP_SPEC.md section 13) and
the host-only decision about WF_FILTER_F32 under a cutoff link (groove_amd/csrc/welsh_plan.h welsh_flag_filter_f32), compiled for the
host through a shim of this test's own.

The laws are checked bit for bit against the same float64 expressions, in the same order, rounded to float32 — and pan_gains, which
moved out of derive.h, against what derive_welsh puts into gl / gr for the same dca_gain / dca_pan: the words the host path uploads
are the words the link's kernel writes."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

from groove_amd import abi_types as T, patches as P
from tests import ctl_bank_law as LAW

REPO = LAW.REPO
SR = float(T.DEFAULT_SAMPLE_RATE)

SHIM = r'''
#include "groove_amd/csrc/welsh_plan.h"
using namespace groove;
extern "C" {
int shim_bank_target_ok(uint32_t index) { return ctl_bank_target_ok(index) ? 1 : 0; }
void shim_bank_param(uint32_t index, const double* v, float* out, size_t n) {
  for (size_t i = 0; i < n; ++i) out[i] = ctl_bank_param_f64(index, v[i]);
}
void shim_pan_gains(const float* gain, const float* pan, float* gl, float* gr, size_t n) {
  for (size_t i = 0; i < n; ++i) pan_gains((double)gain[i], (double)pan[i], gl[i], gr[i]);
}
// what derive_welsh / derive_fm put into gl, gr for `patch` with its dca replaced
void shim_derive_gains(const groove_welsh_params* patch, const float* gain, const float* pan, float* gl, float* gr, float* fm_gl, float* fm_gr, size_t n, double sr) {
  for (size_t i = 0; i < n; ++i) {
    groove_welsh_params p = *patch;
    p.dca_gain = gain[i]; p.dca_pan = pan[i];
    WelshCold cold;
    const WelshParams o = derive_welsh(p, sr, cold);
    gl[i] = o.gl; gr[i] = o.gr;
    groove_fm_params f{};
    f.dca_gain = gain[i]; f.dca_pan = pan[i];
    const FmParams fo = derive_fm(f, sr);
    fm_gl[i] = fo.gl; fm_gr[i] = fo.gr;
  }
}
// flagged[i]: record i carries WF_FILTER_F32 after welsh_flag_filter_f32; measured[i]: welsh_filter_f32_ok of the record
void shim_flag(const groove_welsh_params* patches, size_t n, double sr, int enabled, uint32_t cutoff_links, uint32_t* flagged, uint32_t* measured) {
  std::vector<WelshParams> ext(n);
  WelshCold cold;
  for (size_t i = 0; i < n; ++i) { ext[i] = derive_welsh(patches[i], sr, cold); measured[i] = welsh_filter_f32_ok(ext[i], sr) ? 1u : 0u; }
  welsh_flag_filter_f32(ext, enabled != 0, cutoff_links, [&](const WelshParams& o) { return welsh_filter_f32_ok(o, sr); });
  for (size_t i = 0; i < n; ++i) flagged[i] = (ext[i].flags & WF_FILTER_F32) ? 1u : 0u;
}
}
'''

VALUES = [0.0, 1e-3, 0.1, 0.25, 0.5, 0.75, 1.0, -0.2, 1.3]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("ctl_bank_law")
    src, so = d / "shim.cpp", d / "libctl_bank_shim.so"
    src.write_text(SHIM)
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Werror", "-I", REPO, str(src), "-o", str(so)], check=True)
    L = C.CDLL(str(so))
    u32, f64 = C.c_uint32, C.c_double
    fp, dp, up, wp = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(T.WelshParams)
    for name, res, args in (("shim_bank_target_ok", C.c_int, [u32]), ("shim_bank_param", None, [u32, dp, fp, C.c_size_t]),
                            ("shim_pan_gains", None, [fp, fp, fp, fp, C.c_size_t]),
                            ("shim_derive_gains", None, [wp, fp, fp, fp, fp, fp, fp, C.c_size_t, f64]),
                            ("shim_flag", None, [wp, C.c_size_t, f64, C.c_int, u32, up, up])):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    return L


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def _param(shim, index, values):
    v = np.asarray(values, dtype=np.float64)
    out = np.empty(v.size, dtype=np.float32)
    shim.shim_bank_param(index, v.ctypes.data_as(C.POINTER(C.c_double)), _fp(out), v.size)
    return out


def test_only_the_three_welsh_controls_are_bank_targets(shim):
    ok = {T.CTL_WELSH_DCA_GAIN, T.CTL_WELSH_DCA_PAN, T.CTL_WELSH_CUTOFF}
    for index in list(range(12)) + [31, 32, 33, 34, 35, 0xFFFFFFFF]:
        assert bool(shim.shim_bank_target_ok(index)) == (index in ok), index


def test_the_three_target_laws_bit_for_bit(shim):
    rng = np.random.default_rng(11)
    values = VALUES + list(rng.uniform(-0.25, 1.25, 512)) + [float(np.float32(x)) for x in rng.uniform(0.0, 1.0, 512)]
    gain = _param(shim, T.CTL_WELSH_DCA_GAIN, values)
    pan = _param(shim, T.CTL_WELSH_DCA_PAN, values)
    hz = _param(shim, T.CTL_WELSH_CUTOFF, values)
    assert np.array_equal(_bits(gain), _bits([LAW.gain_param(v) for v in values]))
    assert np.array_equal(_bits(pan), _bits([LAW.pan_param(v) for v in values]))
    assert np.array_equal(_bits(hz), _bits([LAW.cutoff_param(v) for v in values]))
    # the ends: clamped like groove_bank_set_param
    assert gain[VALUES.index(-0.2)] == 0.0 and gain[VALUES.index(1.3)] == 1.0
    assert pan[VALUES.index(-0.2)] == -1.0 and pan[VALUES.index(1.3)] == 1.0 and pan[VALUES.index(0.5)] == 0.0
    assert hz[VALUES.index(-0.2)] == 25.0 and hz[VALUES.index(1.3)] == 20000.0
    assert LAW.cutoff_param(0.5) == np.float32(25.0 * math.pow(800.0, 0.5))


def test_pan_gains_bit_for_bit_and_equal_to_derive_welsh(shim):
    gains = np.array([LAW.gain_param(v) for v in VALUES for _ in VALUES], dtype=np.float32)
    pans = np.array([LAW.pan_param(v) for _ in VALUES for v in VALUES], dtype=np.float32)
    n = gains.size
    gl, gr = np.empty(n, np.float32), np.empty(n, np.float32)
    shim.shim_pan_gains(_fp(gains), _fp(pans), _fp(gl), _fp(gr), n)
    want_l, want_r = LAW.pan_gains(gains, pans)
    assert np.array_equal(_bits(gl), _bits(want_l))
    assert np.array_equal(_bits(gr), _bits(want_r))
    # the host path: derive_welsh (and derive_fm, which calls the same function) for the same dca_gain / dca_pan
    dl, dr, fl, fr = (np.empty(n, np.float32) for _ in range(4))
    patch = P.welsh_patch(2)
    shim.shim_derive_gains(C.byref(patch), _fp(gains), _fp(pans), _fp(dl), _fp(dr), _fp(fl), _fp(fr), n, SR)
    for got_l, got_r in ((dl, dr), (fl, fr)):
        assert np.array_equal(_bits(got_l), _bits(gl))
        assert np.array_equal(_bits(got_r), _bits(gr))
    # centre: both channels gain * 0.75; hard left / right: the other channel silent
    c = list(pans).index(0.0)
    assert gl[c] == gr[c] == np.float32(float(gains[c]) * 0.75)
    left, right = (gains == 1.0) & (pans == -1.0), (gains == 1.0) & (pans == 1.0)
    assert gl[left][0] == 1.0 and gr[left][0] == 0.0 and gl[right][0] == 0.0 and gr[right][0] == 1.0


def test_a_bank_with_a_cutoff_link_carries_no_fp32_filter_flag(shim):
    n = P.N_PATCHES
    patches = (T.WelshParams * n)(*[P.welsh_patch(j) for j in range(n)])

    def flags(enabled, links):
        flagged, measured = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        up = C.POINTER(C.c_uint32)
        shim.shim_flag(patches, n, SR, enabled, links, flagged.ctypes.data_as(up), measured.ctypes.data_as(up))
        return flagged, measured

    plain, measured = flags(1, 0)
    assert 0 < measured.sum() < n  # the corpus has patches on both sides of the measurement
    assert np.array_equal(plain, measured)  # without a link: whatever welsh_filter_f32_ok gave them
    for links in (1, 2, 7):
        linked, again = flags(1, links)
        assert np.array_equal(again, measured)
        assert not linked.any(), links
    off, _ = flags(0, 0)
    assert not off.any()  # the context's knob still has the last word
