"""CPU tier: the shared coefficient formulas (groove_amd/csrc/fx_coef.h) against derive.h's host entry points, bit for bit, and the
predicate that says which (kind, control index) pairs a filter link reaches (groove_amd/csrc/ctl_core.h ctl_target_derived).

The device's filter links (csrc/ctl_link.h ctl_filter_apply_kernel) derive coefficients by calling fx_coef.h with the lane's five
parameter floats widened to f64; the host (fx_upload_params) calls rbj_for_kind_h / lp24_coeffs_h with a groove_fx_params.  One
compiler, one text: the two give the same bits for every kind over the grid below, or the text differs — there is no tolerance."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

from groove_amd import abi_types as T

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHIM = r'''
#include "groove_amd/csrc/fx_coef.h"
#include "groove_amd/csrc/ctl_core.h"
#include "groove_amd/csrc/derive.h"
using namespace groove;
extern "C" {
// the host's path: groove_fx_set_param's laws into a groove_fx_params, then derive.h
int shim_host(uint32_t kind, double v_cut, double v_q, double v_rip, float bw, float db, double fs, double* c6) {
  groove_fx_params p{};
  p.cutoff_hz = (float)percent_to_frequency_h(v_cut);
  p.q = (float)(v_q * v_q * 10.0 + 0.707);
  p.passband_ripple = (float)(v_rip * v_rip * 10.0 + 0.707);
  p.bandwidth_hz = bw; p.db_gain = db;
  if (kind == GROOVE_FX_BIQUAD_LP24) { lp24_coeffs_h(p.cutoff_hz, p.passband_ripple, fs, c6); return 6; }
  return rbj_for_kind_h(kind, p, fs, c6) ? 5 : 0;
}
// the link kernel's path: the laws of ctl_core.h from the fp32 control value, five floats, then fx_coef.h
int shim_shared(uint32_t kind, float v_cut, float v_q, float v_rip, float bw, float db, double fs, double* c6) {
  float w[CTL_SHADOW_WORDS];
  w[ctl_shadow_word(GROOVE_CTL_FX_CUTOFF)] = ctl_derived_param(GROOVE_CTL_FX_CUTOFF, v_cut);
  w[ctl_shadow_word(GROOVE_CTL_FX_Q)] = ctl_derived_param(GROOVE_CTL_FX_Q, v_q);
  w[ctl_shadow_word(GROOVE_CTL_FX_PASSBAND_RIPPLE)] = ctl_derived_param(GROOVE_CTL_FX_PASSBAND_RIPPLE, v_rip);
  w[CTL_SHADOW_BANDWIDTH] = bw; w[CTL_SHADOW_DB_GAIN] = db;
  if (kind == GROOVE_FX_BIQUAD_LP24) { fx_lp24_coeffs((double)w[CTL_SHADOW_CUTOFF], (double)w[CTL_SHADOW_RIPPLE], fs, c6); return 6; }
  return fx_rbj_for_kind(kind, (double)w[CTL_SHADOW_CUTOFF], (double)w[CTL_SHADOW_Q], (double)w[CTL_SHADOW_BANDWIDTH], (double)w[CTL_SHADOW_DB_GAIN], fs, c6) ? 5 : 0;
}
void shim_laws(float v, float* cutoff, float* q) { *cutoff = ctl_derived_param(GROOVE_CTL_FX_CUTOFF, v); *q = ctl_derived_param(GROOVE_CTL_FX_Q, v); }
void shim_lp24_clamped(double fc, double ripple, double fs, double* shared, double* host) { fx_lp24_coeffs(fc, ripple, fs, shared); lp24_coeffs_h(fc, ripple, fs, host); }
int shim_target_derived(uint32_t kind, uint32_t index) { return ctl_target_derived(kind, index) ? 1 : 0; }
int shim_target_linkable(uint32_t index) { return ctl_target_linkable(index) ? 1 : 0; }
}
'''

BIQUAD12 = [T.FX_BIQUAD_LP12, T.FX_BIQUAD_HP12, T.FX_BIQUAD_BP12, T.FX_BIQUAD_BS12, T.FX_BIQUAD_AP12, T.FX_BIQUAD_PEAK12,
            T.FX_BIQUAD_LSHELF12, T.FX_BIQUAD_HSHELF12]
FILTERS = BIQUAD12 + [T.FX_BIQUAD_LP24]
VALUES = [0.0, 1e-3, 0.1, 0.25, 0.5, 0.75, 0.95, 1.0]
BANDWIDTHS = [10.0, 500.0, 5000.0]
DB_GAINS = [-30.0, 0.0, 30.0]
RATES = [44100.0, 48000.0]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("fx_coef")
    src, so = d / "shim.cpp", d / "libfx_coef_shim.so"
    src.write_text(SHIM)
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Werror", "-I", REPO, str(src), "-o", str(so)], check=True)
    L = C.CDLL(str(so))
    u32, f32, f64, dp, fp = C.c_uint32, C.c_float, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_float)
    for name, res, args in (("shim_host", C.c_int, [u32, f64, f64, f64, f32, f32, f64, dp]), ("shim_shared", C.c_int, [u32, f32, f32, f32, f32, f32, f64, dp]),
                            ("shim_laws", None, [f32, fp, fp]), ("shim_lp24_clamped", None, [f64, f64, f64, dp, dp]),
                            ("shim_target_derived", C.c_int, [u32, u32]), ("shim_target_linkable", C.c_int, [u32])):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    return L


@pytest.mark.parametrize("kind", FILTERS)
def test_shared_formulas_give_the_hosts_bits(shim, kind):
    a, b = np.zeros(6), np.zeros(6)
    dp = C.POINTER(C.c_double)
    checked = 0
    for fs, v_cut, v_q, bw, db in itertools.product(RATES, VALUES, VALUES, BANDWIDTHS, DB_GAINS):
        v32 = [float(np.float32(v)) for v in (v_cut, v_q, v_q)]                      # the control value is fp32 on both sides (the ripple law at the q values)
        na = shim.shim_host(kind, v32[0], v32[1], v32[2], bw, db, fs, a.ctypes.data_as(dp))
        nb = shim.shim_shared(kind, v32[0], v32[1], v32[2], bw, db, fs, b.ctypes.data_as(dp))
        assert na == nb == (6 if kind == T.FX_BIQUAD_LP24 else 5)
        assert np.array_equal(a[:na].view(np.uint64), b[:nb].view(np.uint64)), (kind, fs, v_cut, v_q, bw, db, a, b)
        assert np.all(np.isfinite(a[:na]))
        checked += 1
    assert checked == 2 * 8 * 8 * 3 * 3


def test_not_a_filter_kind_is_refused_by_both(shim):
    c = np.zeros(6)
    for kind in (T.FX_GAIN, T.FX_BITCRUSHER, T.FX_CHORUS, T.FX_DELAY, T.FX_REVERB, T.FX_MIXER, T.FX_LIMITER, T.FX_COMPRESSOR, 17, 99):
        assert shim.shim_host(kind, 0.5, 0.5, 0.5, 500.0, 0.0, 44100.0, c.ctypes.data_as(C.POINTER(C.c_double))) == 0
        assert shim.shim_shared(kind, 0.5, 0.5, 0.5, 500.0, 0.0, 44100.0, c.ctypes.data_as(C.POINTER(C.c_double))) == 0


def test_parameter_laws_are_set_params(shim):
    """cutoff = (float)(25 * 800^v), q = ripple = (float)(10 v^2 + 0.707), v clamped to [0, 1] — in f64 from the fp32 value."""
    cut, q = C.c_float(), C.c_float()
    for v in VALUES + [-0.5, 1.5, 0.33333334]:
        v32 = float(np.float32(v))
        shim.shim_laws(v32, C.byref(cut), C.byref(q))
        c = min(max(v32, 0.0), 1.0)
        assert q.value == float(np.float32(c * c * 10.0 + 0.707)), v
        want = 25.0 * 800.0 ** c
        assert abs(cut.value - want) <= want * 2.0 ** -23, v                         # (libm's pow against Python's: the rounding to fp32 may differ in the last place)
    shim.shim_laws(0.0, C.byref(cut), C.byref(q))
    assert cut.value == 25.0 and q.value == float(np.float32(0.707))
    shim.shim_laws(1.0, C.byref(cut), C.byref(q))
    assert cut.value == 20000.0


def test_lp24_clamps_its_cutoff_like_the_host(shim):
    a, b = np.zeros(6), np.zeros(6)
    dp = C.POINTER(C.c_double)
    for fs in RATES:
        for fc in (0.0, 0.5, 1.0, 0.49 * fs, 0.5 * fs, 30000.0, -3.0):
            shim.shim_lp24_clamped(fc, 1.2, fs, a.ctypes.data_as(dp), b.ctypes.data_as(dp))
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64)) and np.all(np.isfinite(a)), (fs, fc)
        shim.shim_lp24_clamped(30000.0, 1.2, fs, a.ctypes.data_as(dp), b.ctypes.data_as(dp))
        top = a.copy()
        shim.shim_lp24_clamped(0.49 * fs, 1.2, fs, a.ctypes.data_as(dp), b.ctypes.data_as(dp))
        assert np.array_equal(top.view(np.uint64), a.view(np.uint64))


def test_derived_targets_are_exactly_the_listed_pairs(shim):
    want = {(k, T.CTL_FX_CUTOFF) for k in FILTERS}
    want |= {(k, T.CTL_FX_Q) for k in (T.FX_BIQUAD_LP12, T.FX_BIQUAD_HP12, T.FX_BIQUAD_AP12)}
    want |= {(T.FX_BIQUAD_LP24, T.CTL_FX_PASSBAND_RIPPLE)}
    assert len(want) == 13
    for kind in range(20):
        for index in list(range(12)) + [T.CTL_WELSH_DCA_GAIN, T.CTL_WELSH_DCA_PAN, T.CTL_WELSH_CUTOFF]:
            assert bool(shim.shim_target_derived(kind, index)) == ((kind, index) in want), (kind, index)
    linkable = {T.CTL_FX_CEILING, T.CTL_FX_BITS, T.CTL_FX_ATTENUATION, T.CTL_FX_THRESHOLD}
    for index in range(8):
        assert bool(shim.shim_target_linkable(index)) == (index in linkable), index
