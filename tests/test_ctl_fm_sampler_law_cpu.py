"""CPU tier: the target laws of a link onto an FM or a sampler bank (groove_amd/csrc/ctl_core.h ctl_fm_*_f64, ctl_sampler_gain_f64,
docs/DSP_SPEC.md section 13) and the text the links' kernels store with (ctl_fm_store, ctl_sampler_store), compiled for the host through a
shim of this test's own, like tests/test_ctl_bank_law_cpu.py.

The laws are held bit for bit against the float64 expressions groove_bank_set_param stores into groove_fm_params / groove_sampler_params
(tests/ctl_fm_sampler_law.py).  The store is run over a word-major parameter array exactly as the kernel runs it — one call per voice — and
the rows it leaves must be the rows derive_fm gives for the same four public floats: gl, gr, and depth_beta, an f64 spread over two
32-bit rows."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from groove_amd import abi_types as T
from tests import ctl_fm_sampler_law as LAW

REPO = LAW.REPO
SR = float(T.DEFAULT_SAMPLE_RATE)

SHIM = r'''
#include <vector>
#include <cstring>
#include "groove_amd/csrc/derive.h"
using namespace groove;
extern "C" {
int shim_fm_target_ok(uint32_t index) { return ctl_fm_target_ok(index) ? 1 : 0; }
int shim_sampler_target_ok(uint32_t index) { return ctl_sampler_target_ok(index) ? 1 : 0; }
uint32_t shim_fm_shadow_word(uint32_t index) { return ctl_fm_shadow_word(index); }
void shim_fm_param(uint32_t index, const double* v, float* out, size_t n) {
  for (size_t i = 0; i < n; ++i) out[i] = ctl_fm_param_f64(index, v[i]);
}
void shim_sampler_gain(const double* v, float* out, size_t n) {
  for (size_t i = 0; i < n; ++i) out[i] = ctl_sampler_gain_f64(v[i]);
}
uint32_t shim_fm_words() { return sizeof(FmParams) / 4; }
uint32_t shim_sampler_words() { return sizeof(SamplerParams) / 4; }
// derive_fm of n voices {gain, pan, depth, beta} (shadow: [4][n]) as the word-major array the library uploads
void shim_fm_derive_soa(const float* shadow, uint32_t n, double sr, uint32_t* soa) {
  const uint32_t W = sizeof(FmParams) / 4;
  for (uint32_t v = 0; v < n; ++v) {
    groove_fm_params p{};
    p.ratio = 2.0;
    p.carrier_envelope = groove_envelope_params{0.01, 0.1, 0.7, 0.2};
    p.modulator_envelope = groove_envelope_params{0.02, 0.3, 0.5, 0.1};
    p.dca_gain = shadow[0 * (size_t)n + v]; p.dca_pan = shadow[1 * (size_t)n + v]; p.depth = shadow[2 * (size_t)n + v]; p.beta = shadow[3 * (size_t)n + v];
    const FmParams o = derive_fm(p, sr);
    uint32_t w[sizeof(FmParams) / 4];
    std::memcpy(w, &o, sizeof(o));
    for (uint32_t i = 0; i < W; ++i) soa[(size_t)i * n + v] = w[i];
  }
}
// the kernel's store: one call per voice with that voice's parameter
void shim_fm_store(uint32_t* soa, float* shadow, uint32_t n, uint32_t index, const float* mine) {
  for (uint32_t e = 0; e < n; ++e) ctl_fm_store(soa, shadow, n, e, index, mine[e]);
}
void shim_sampler_store(uint32_t* soa, uint32_t n, const float* mine) {
  for (uint32_t e = 0; e < n; ++e) ctl_sampler_store(soa, n, e, mine[e]);
}
uint32_t shim_sampler_gain_row() { return offsetof(SamplerParams, gain) / 4; }
uint32_t shim_fm_row(int which) { return (uint32_t)((which == 0 ? offsetof(FmParams, depth_beta) : which == 1 ? offsetof(FmParams, gl) : offsetof(FmParams, gr)) / 4); }
}
'''

VALUES = [0.0, 1.0, 1e-3, 0.1, 0.25, 0.5, 0.75, -0.2, 1.3, -1e300, 1e300]
FM = (T.CTL_FM_DCA_GAIN, T.CTL_FM_DCA_PAN, T.CTL_FM_DEPTH, T.CTL_FM_BETA)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("ctl_fm_sampler_law")
    src, so = d / "shim.cpp", d / "libctl_fm_sampler_shim.so"
    src.write_text(SHIM)
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Werror", "-I", REPO, str(src), "-o", str(so)], check=True)
    L = C.CDLL(str(so))
    u32, f64 = C.c_uint32, C.c_double
    fp, dp, up = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_uint32)
    for name, res, args in (("shim_fm_target_ok", C.c_int, [u32]), ("shim_sampler_target_ok", C.c_int, [u32]), ("shim_fm_shadow_word", u32, [u32]),
                            ("shim_fm_param", None, [u32, dp, fp, C.c_size_t]), ("shim_sampler_gain", None, [dp, fp, C.c_size_t]),
                            ("shim_fm_words", u32, []), ("shim_sampler_words", u32, []), ("shim_fm_derive_soa", None, [fp, u32, f64, up]),
                            ("shim_fm_store", None, [up, fp, u32, u32, fp]), ("shim_sampler_store", None, [up, u32, fp]),
                            ("shim_sampler_gain_row", u32, []), ("shim_fm_row", u32, [C.c_int])):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    return L


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _up(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def _values():
    rng = np.random.default_rng(48)
    return VALUES + list(rng.uniform(-0.25, 1.25, 2048)) + [float(np.float32(x)) for x in rng.uniform(0.0, 1.0, 2048)]


def test_the_indices_and_which_bank_kind_they_belong_to(shim):
    assert FM == (48, 49, 50, 51) and T.CTL_SAMPLER_GAIN == 64
    for index in list(range(12)) + [31, 32, 33, 34, 35, 47, 48, 49, 50, 51, 52, 63, 64, 65, 0xFFFFFFFF]:
        assert bool(shim.shim_fm_target_ok(index)) == (index in FM), index
        assert bool(shim.shim_sampler_target_ok(index)) == (index == T.CTL_SAMPLER_GAIN), index
    assert [shim.shim_fm_shadow_word(i) for i in FM] == [0, 1, 2, 3]                        # gain, pan, depth, beta


def test_the_five_laws_bit_for_bit(shim):
    values = _values()
    v = np.asarray(values, dtype=np.float64)
    got = {}
    for index in FM:
        out = np.empty(v.size, dtype=np.float32)
        shim.shim_fm_param(index, v.ctypes.data_as(C.POINTER(C.c_double)), _fp(out), v.size)
        got[index] = out
    sg = np.empty(v.size, dtype=np.float32)
    shim.shim_sampler_gain(v.ctypes.data_as(C.POINTER(C.c_double)), _fp(sg), v.size)
    assert np.array_equal(_bits(got[T.CTL_FM_DCA_GAIN]), _bits([LAW.gain_param(x) for x in values]))
    assert np.array_equal(_bits(got[T.CTL_FM_DCA_PAN]), _bits([LAW.pan_param(x) for x in values]))
    assert np.array_equal(_bits(got[T.CTL_FM_DEPTH]), _bits([LAW.depth_param(x) for x in values]))
    assert np.array_equal(_bits(got[T.CTL_FM_BETA]), _bits([LAW.beta_param(x) for x in values]))
    assert np.array_equal(_bits(sg), _bits([LAW.sampler_gain_param(x) for x in values]))
    # the ends: clamped like groove_bank_set_param; pans at -1, 0 and +1
    lo, hi, mid = VALUES.index(-0.2), VALUES.index(1.3), VALUES.index(0.5)
    for index in (T.CTL_FM_DCA_GAIN, T.CTL_FM_DEPTH, T.CTL_FM_BETA):
        assert got[index][lo] == 0.0 and got[index][hi] == 1.0 and got[index][0] == 0.0 and got[index][1] == 1.0
    pan = got[T.CTL_FM_DCA_PAN]
    assert pan[lo] == -1.0 and pan[0] == -1.0 and pan[hi] == 1.0 and pan[1] == 1.0 and pan[mid] == 0.0
    assert sg[lo] == 0.0 and sg[hi] == 1.0 and sg[VALUES.index(-1e300)] == 0.0 and sg[VALUES.index(1e300)] == 1.0


def _shadow(n, seed):
    """[4][n] public floats after the laws: gain, pan (with the ends -1 and +1), depth, beta."""
    rng = np.random.default_rng(seed)
    vals = np.array(_values())
    pick = lambda: vals[rng.integers(0, vals.size, n)]
    rows = [[f(x) for x in pick()] for f in (LAW.gain_param, LAW.pan_param, LAW.depth_param, LAW.beta_param)]
    sh = np.array(rows, dtype=np.float32)
    sh[:, 0] = (1.0, -1.0, 1.0, 1.0)
    sh[:, 1] = (1.0, 1.0, 0.0, 1.0)
    return np.ascontiguousarray(sh)


@pytest.mark.parametrize("index", FM)
def test_the_store_leaves_the_rows_derive_fm_gives(shim, index):
    """From shadow words (gain, pan, depth, beta) and a new value of one of them, per voice: the array after ctl_fm_store is the array
    derive_fm builds from the four floats — every row, so the rows the store must not touch are held too."""
    n = 3001                                                                               # odd: a row is no multiple of anything
    W = shim.shim_fm_words()
    before = _shadow(n, 5)
    soa = np.empty(W * n, dtype=np.uint32)
    shim.shim_fm_derive_soa(_fp(before), n, SR, _up(soa))
    word = shim.shim_fm_shadow_word(index)
    mine = np.ascontiguousarray(_shadow(n, 6)[word])
    shadow = before.copy()
    shim.shim_fm_store(_up(soa), _fp(shadow), n, index, _fp(mine))
    after = before.copy()
    after[word] = mine
    assert np.array_equal(_bits(shadow), _bits(after))                                     # its own word written, the others as they were
    want = np.empty(W * n, dtype=np.uint32)
    shim.shim_fm_derive_soa(_fp(after), n, SR, _up(want))
    assert np.array_equal(soa, want)
    # ... and against the law restated: gl, gr, and the f64 index from its low and its high row
    rows = soa.reshape(W, n)
    r_idx, r_gl, r_gr = (shim.shim_fm_row(k) for k in range(3))
    gl, gr = LAW.pan_gains(after[0], after[1])
    assert np.array_equal(rows[r_gl], _bits(gl)) and np.array_equal(rows[r_gr], _bits(gr))
    idx = (rows[r_idx].astype(np.uint64) | (rows[r_idx + 1].astype(np.uint64) << np.uint64(32))).view(np.float64)
    assert np.array_equal(idx, LAW.depth_beta(after[2], after[3]))
    changed = np.flatnonzero((rows != _soa_of(shim, before, n).reshape(W, n)).any(axis=1))
    allowed = {r_gl, r_gr} if word < 2 else {r_idx, r_idx + 1}
    assert set(changed.tolist()) <= allowed and len(changed) > 0, (index, changed)


def _soa_of(shim, shadow, n):
    soa = np.empty(shim.shim_fm_words() * n, dtype=np.uint32)
    shim.shim_fm_derive_soa(_fp(np.ascontiguousarray(shadow)), n, SR, _up(soa))
    return soa


def test_the_sampler_store_writes_the_gain_row_alone(shim):
    n, W = 777, shim.shim_sampler_words()
    rng = np.random.default_rng(9)
    soa = rng.integers(0, 2 ** 32, W * n, dtype=np.uint64).astype(np.uint32)
    before = soa.copy()
    mine = np.array([LAW.sampler_gain_param(x) for x in rng.uniform(-0.25, 1.25, n)], dtype=np.float32)
    shim.shim_sampler_store(_up(soa), n, _fp(mine))
    row = shim.shim_sampler_gain_row()
    assert np.array_equal(soa.reshape(W, n)[row], _bits(mine))
    keep = np.ones(W, dtype=bool)
    keep[row] = False
    assert np.array_equal(soa.reshape(W, n)[keep], before.reshape(W, n)[keep])
