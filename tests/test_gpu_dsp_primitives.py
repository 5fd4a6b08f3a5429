"""GPU tier: the DEVICE side of csrc/dsp_core.h, primitive by primitive, through tests/probe (one bounds-guarded element-wise kernel
per primitive, built with the library's own flags; no kernel of the library runs here).

  a. bit for bit against the host build (which tests/test_dsp_primitives_cpu.py holds to exact and high-precision references), on the
     same inputs: everything integer or written in explicit fma / fmaf calls and single operations, where the compiler has nothing to
     contract and a device-only builtin must agree with the C on its domain;
  b. the hand-written v_fma sequences of the filter steps against their C bodies, bit for bit, 64 steps a lane;
  c. the two approximate instructions (v_exp_f32, v_rcp_f32) within 1 ulp, v_med3_f32 equal to min(max());
  d. the coefficient paths, where contraction and v_rcp_f32 meet, at the bars of
     test_emul_numerics.py::test_filter_coefficients_keep_the_poles_distance_from_the_unit_circle;
  e. the interpolation and cutoff-percent formulas against f64.
In (d) and (e) the distance between the device and the host build is counted and PRINTED (docs/DSP_SPEC.md section 14 records it).

References are numpy float64 and Python integers only."""
import functools

import numpy as np
import pytest

from tests import dsp_primitive_cases as K
from tests.probe import probe as PR

pytestmark = pytest.mark.gpu


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same_bits(name, got, want, inputs):
    g, w = _bits(got), _bits(want)
    bad = np.nonzero((g != w).reshape(g.shape[0], -1).any(axis=1))[0]
    assert bad.size == 0, (name, int(bad.size), [tuple(np.asarray(a).reshape(g.shape[0], -1)[i].tolist() for a in inputs) + (got[i].tolist(), want[i].tolist()) for i in bad[:4]])


def _ulps32(a, b):
    """Distance in units in the last place between two float32 arrays of the same sign pattern (monotone integer mapping)."""
    def key(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def _ulps64(a, b):
    def key(x):
        i = np.ascontiguousarray(x, dtype=np.float64).view(np.int64)
        return np.where(i < 0, -(i & np.int64(0x7FFFFFFFFFFFFFFF)), i).astype(np.float64)   # (a count: 53 bits are plenty)
    return np.abs(key(a) - key(b))


def _distance(label, dev, host, small=None):
    """The measured distance between the device and the emulation tier's build: reported, not asserted.  In ulps of the values; for
    coefficient sets (small = _small_quantities) relative to the quantities that matter, since an ulp of a1 next to -2 says nothing."""
    if small is not None:
        differ = (_bits(dev) != _bits(host)).any(axis=1)
        rel = np.abs(small(dev) - small(host)) / np.abs(small(host))
        print(f"device vs host build, {label}: {int(np.count_nonzero(differ))} of {differ.size} inputs differ, by at most {rel.max():.3e} of 1 + a2, 2 - |a1| or b0")
        return
    u = (_ulps32 if dev.dtype == np.float32 else _ulps64)(dev, host)
    lanes = u.reshape(u.shape[0], -1).max(axis=1)
    print(f"device vs host build, {label}: {int(np.count_nonzero(lanes))} of {lanes.size} inputs differ, by at most {int(u.max())} ulp")


# ------------------------------------------------------------------ a. bit for bit with the host build
ROWS = {
    "f64_to_u64": lambda: (K.f64_to_u64_inputs(),),
    "fract_f64": lambda: (K.fract_inputs(),),
    "turns_to_inc": lambda: (K.turns_inputs(),),
    "turns_to_phase": lambda: (K.turns_inputs(),),
    "fold_quarter": lambda: (K.fold32_inputs(),),
    "fold_quarter64": lambda: (K.fold64_inputs(),),
    "osc_value": K.osc_inputs,
    "osc_value_f64": K.osc_inputs,
    "noise_tick": lambda: (np.arange(K.NOISE_TICKS + 1, dtype=np.uint32),),
    "env_frames": lambda: (K.env_frames_inputs(),),
    "sin_turns_folded": lambda: (K.sin_f32_inputs(),),
    "sin_turns_folded_f64": lambda: (K.sin_f64_inputs(),),
    "exp2_small_f64": lambda: (K.exp2_small_inputs(),),
    "exp_tiny_f64": lambda: (K.exp_tiny_inputs(),),
    "tan_of_reduced": lambda: (K.tan_inputs(),),
    "tan_reduced": lambda: (K.tan_reduced_inputs(),),
}


@pytest.mark.parametrize("name", sorted(ROWS))
def test_device_equals_host_build_bit_for_bit(name):
    inputs = ROWS[name]()
    _same_bits(name, PR.device(name, *inputs), PR.host(name, *inputs), inputs)


EXACT = {
    "f64_to_u64": (lambda: (K.f64_to_u64_inputs(),), K.f64_to_u64_exact),
    "turns_to_inc": (lambda: (K.turns_inputs(),), K.turns_to_inc_exact),
    "turns_to_phase": (lambda: (K.turns_inputs(),), K.turns_to_inc_exact),
    "fold_quarter": (lambda: (K.fold32_inputs(),), lambda: K.fold_exact(K.fold32_inputs(), 32)),
    "fold_quarter64": (lambda: (K.fold64_inputs(),), lambda: K.fold_exact(K.fold64_inputs(), 64)),
    "noise_tick": (lambda: (np.arange(K.NOISE_TICKS + 1, dtype=np.uint32),), K.noise_exact),
    "env_frames": (lambda: (K.env_frames_inputs(),), K.env_frames_exact),
    "fract_f64": (lambda: (K.fract_inputs(),), K.fract_exact),
}


@pytest.mark.parametrize("name", sorted(EXACT))
def test_device_integer_rows_equal_the_python_integers(name):
    """The exact rows against Python's integers and fractions directly, not only through the host build."""
    make, exact = EXACT[name]
    inputs = make()
    _same_bits(name, PR.device(name, *inputs), exact(), inputs)


def test_env_shape_device_equals_host_build():
    """Frames 0 .. 4095 of stages with len in {1, 2.5, 441, 7938.0003, 13230} and D in {1, -0.4, -1} (attack from 0, decay and release from 1)."""
    n, A, D, inv = [], [], [], []
    for ln in (1.0, 2.5, 441.0, 7938.0003, 13230.0):
        for d in (1.0, -0.4, -1.0):
            n.append(np.arange(4096, dtype=np.float32))
            A.append(np.full(4096, 0.0 if d > 0 else 1.0, dtype=np.float32))
            D.append(np.full(4096, d, dtype=np.float32))
            inv.append(np.full(4096, np.float32(1.0) / np.float32(ln), dtype=np.float32))
    inputs = tuple(np.concatenate(v) for v in (n, A, D, inv))
    _same_bits("env_shape", PR.device("env_shape", *inputs), PR.host("env_shape", *inputs), inputs)


def test_bitcrush_device_equals_host_build():
    rng = np.random.default_rng(31)
    x = np.concatenate([np.array([0.0, -0.0, 1.0, -1.0, 3.0e-5, -3.0e-5, 0.999985, 2.5], dtype=np.float32),
                        (0.5 * rng.standard_normal(K.RANDOM - 1000)).astype(np.float32), (rng.standard_normal(1000) * 10.0 ** rng.uniform(-8, 12, 1000)).astype(np.float32)])
    depths = (0, 1, 4, 8, 13, 15)
    xs, bits = np.tile(x, len(depths)), np.repeat(np.array(depths, dtype=np.uint32), x.size)
    _same_bits("bitcrush", PR.device("bitcrush", xs, bits), PR.host("bitcrush", xs, bits), (xs, bits))


def test_sample_interp_nearest_is_the_tap():
    rng = np.random.default_rng(32)
    taps = rng.uniform(-1.0, 1.0, (K.RANDOM, 4)).astype(np.float32)
    t = (rng.integers(0, 1 << 24, K.RANDOM) * 2.0 ** -24).astype(np.float32)
    got = PR.device("sample_interp_nearest", taps, t)
    _same_bits("sample_interp_nearest", got, taps[:, 0].copy(), (taps, t))
    _same_bits("sample_interp_nearest", got, PR.host("sample_interp_nearest", taps, t), (taps, t))


# ------------------------------------------------------------------ b. the hand-written recurrences
SETS, LANES, SR = 64, 4096, 44100.0


@functools.lru_cache(None)
def _coefficient_sets():
    """64 (ripple, cutoff) pairs: ripples {0.1, 0.707, 3.2, 7.1, 10.7} x cutoffs {20 .. 21609} Hz, padded out with random draws; their
    coefficients from the host build's lp24_coefd_from_fc / lp24_coeff_from_fc at 44,100 Hz."""
    pairs = [(r, f) for r in (0.1, 0.707, 3.2, 7.1, 10.7) for f in (20.0, 99.0, 1000.0, 5000.0, 11025.0, 19000.0, 21609.0)]
    rng = np.random.default_rng(33)
    while len(pairs) < SETS:
        pairs.append((float(rng.uniform(0.1, 11.0)), float(min(20.0 * 1100.0 ** rng.random(), 0.49 * SR))))
    ripple, fc = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs], dtype=np.float32)
    sr = np.full(SETS, SR, dtype=np.float32)
    d, f = PR.host("lp24_coefd_from_fc", ripple, fc, sr), PR.host("lp24_coeff_from_fc", ripple, fc, sr)
    assert np.all(np.isfinite(d)) and np.all(np.isfinite(f)) and np.unique(d, axis=0).shape[0] == SETS
    return pairs, d, f


def _lanes(dtype, seed):
    """States in +-4 and inputs in +-1; lane 0 all zero, lane 1 all -0.0, lane 2 zero state, lane 3 zero input, signed zeros sprinkled."""
    rng = np.random.default_rng(seed)
    state = rng.uniform(-4.0, 4.0, (LANES, 4)).astype(dtype)
    x = rng.uniform(-1.0, 1.0, (LANES, PR.STEPS)).astype(dtype)
    state[0], x[0] = 0.0, 0.0
    state[1], x[1] = -0.0, -0.0
    state[2] = 0.0
    x[3] = 0.0
    x[4:64, ::7] = 0.0
    x[64:128, ::5] = -0.0
    state[128:192, 1] = -0.0
    return state, x


@pytest.mark.parametrize("kind", ["f64", "f32"])
def test_filter_step_asm_equals_its_c_body_bit_for_bit(kind):
    """lp24_step<false>, lp24_step<true> (f64) / lp24_step_f32<false>, lp24_step_f32<true> (f32): the ten written-out instructions against
    the ten operations of the C body — every output and all four state words after each of 64 consecutive steps, 4,096 lanes for each of
    64 coefficient sets.  The SCALAR_COEF form takes its set as kernel arguments, one launch a set."""
    pairs, cd, cf = _coefficient_sets()
    dtype, coefs, step = (np.float64, cd, "lp24_step") if kind == "f64" else (np.float32, cf, "lp24_step_f32")
    for k in range(SETS):
        state, x = _lanes(dtype, 100 + k)
        tiled = np.tile(coefs[k], (LANES, 1))
        want = PR.host(step, tiled, state, x)
        assert np.all(np.isfinite(want)), pairs[k]
        for form, got in (("per-lane coefficients", PR.device(step, tiled, state, x)), ("SCALAR_COEF", PR.device(step + "_scalar", coefs[k], state, x))):
            bad = np.nonzero((_bits(got) != _bits(want)).any(axis=1))[0]
            assert bad.size == 0, (step, form, pairs[k], int(bad.size), int(bad[0]), got[bad[0]][:10].tolist(), want[bad[0]][:10].tolist())


# ------------------------------------------------------------------ c. the approximate instructions
def _within_one_ulp(label, y, exact, x):
    """y within 1 ulp of the fp32 result: at most one step in the last place from the float64 reference rounded to fp32, AND no further
    than one unit in the last place (of that rounded result) from the float64 reference itself."""
    nearest = exact.astype(np.float32)
    u = _ulps32(y, nearest)
    err = np.abs(y.astype(np.float64) - exact) / np.spacing(np.abs(nearest)).astype(np.float64)
    i = int(np.argmax(err))
    print(f"{label}: at most {int(u.max())} ulp from the rounded fp32 result on {y.size} points; worst error {err[i]:.3f} ulp at x = {float(x[i])!r}")
    assert int(u.max()) <= 1, (label, float(x[int(np.argmax(u))]), float(y[int(np.argmax(u))]), float(nearest[int(np.argmax(u))]))
    assert err[i] <= 1.0, (label, float(x[i]), float(y[i]), float(exact[i]), float(err[i]))


def test_fast_exp2_within_one_ulp():
    """v_exp_f32 on [-16, 16], the kernels' domain (dsp_core.h lp24_t_from_pct, lp24_consts_from_ripple), against 2**x in float64."""
    x = np.concatenate([np.linspace(-16.0, 16.0, (1 << 22) - 64), np.arange(-16.0, 16.0, 0.5)]).astype(np.float32)
    assert x.size == 1 << 22
    _within_one_ulp("fast_exp2", PR.device("fast_exp2", x), np.exp2(x.astype(np.float64)), x)


def test_fast_rcp_within_one_ulp():
    """v_rcp_f32 on |x| in [2^-20, 2^20], both signs, against 1 / x in float64."""
    rng = np.random.default_rng(34)
    n = 1 << 22
    mag = 2.0 ** rng.uniform(-20.0, 20.0, n - 4)
    x = np.concatenate([mag * rng.choice([-1.0, 1.0], n - 4), [2.0 ** -20, -2.0 ** -20, 2.0 ** 20, -2.0 ** 20]]).astype(np.float32)
    _within_one_ulp("fast_rcp", PR.device("fast_rcp", x), 1.0 / x.astype(np.float64), x)


def test_med3f_is_min_of_max():
    rng = np.random.default_rng(35)
    a, b = rng.standard_normal(K.RANDOM).astype(np.float32), rng.standard_normal(K.RANDOM).astype(np.float32)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    x = (2.0 * rng.standard_normal(K.RANDOM)).astype(np.float32)
    x[:1000], x[1000:2000] = lo[:1000], hi[1000:2000]            # on the bounds themselves
    lo[2000:3000] = hi[2000:3000]                               # an empty interval's one point
    x[3000:3010] = [np.float32(v) for v in (3.0e38, -3.0e38, 1e-45, -1e-45, 1e-38, -1e-38, 65504.0, -65504.0, 1.0, -1.0)]
    got = PR.device("med3f", x, lo, hi)
    _same_bits("med3f", got, np.minimum(np.maximum(x, lo), hi), (x, lo, hi))
    _same_bits("med3f", got, PR.host("med3f", x, lo, hi), (x, lo, hi))


# ------------------------------------------------------------------ d. the coefficient paths
@functools.lru_cache(None)
def _coefficient_draw():
    """The draw of test_filter_coefficients_keep_the_poles_distance_from_the_unit_circle: 20,000 cases, seed 7, three rates."""
    rng = np.random.default_rng(7)
    ripple, sr, fc = [], [], []
    for _ in range(20000):
        ripple.append(float(rng.choice([0.1 + 1.3 * rng.random(), 11.0 * rng.random()])))
        sr.append(float(rng.choice([22050.0, 44100.0, 96000.0])))
        fc.append(float(min(20.0 * 1100.0 ** rng.random(), 0.49 * sr[-1])))
    return np.array(ripple), np.array(fc, dtype=np.float32), np.array(sr, dtype=np.float32)


def _small_quantities(c):
    """[n, 6] coefficients (b0, a1, a2 twice) -> [n, 6]: per section 1 + a2, the smaller of 2 - a1 and 2 + a1, and b0, in float64."""
    c = c.astype(np.float64)
    cols = []
    for s in (0, 3):
        cols += [1.0 + c[:, s + 2], np.minimum(2.0 - c[:, s + 1], 2.0 + c[:, s + 1]), c[:, s]]
    return np.stack(cols, axis=1)


def _coefficient_errors(label, got, want, fc, sr):
    """Relative errors of the small quantities [n, 6] and which cases lie up to 0.4 SR (bar 2e-6; above: 2e-5)."""
    rel = np.abs(_small_quantities(got) - _small_quantities(want)) / np.abs(_small_quantities(want))
    low = fc.astype(np.float64) <= 0.4 * sr.astype(np.float64)
    print(f"{label}: worst relative error {rel[low].max():.3e} up to 0.4 SR (bar 2e-6), {rel[~low].max():.3e} above (bar 2e-5)")
    assert rel.max() > 1e-9 and np.any(low) and np.any(~low)
    return rel, low


def _assert_bar(label, rel, bar, which, ripple, fc, sr):
    r = np.where(which[:, None], rel, 0.0)
    i, j = np.unravel_index(int(np.argmax(r)), r.shape)
    assert r[i, j] <= bar, (label, bar, float(ripple[i]), float(fc[i]), float(sr[i]), int(j), float(r[i, j]))


def test_lp24_coefd_from_fc_on_the_device_keeps_the_emulation_tiers_bars():
    ripple, fc, sr = _coefficient_draw()
    want = PR.host("ref_lp24_coeffs_h", ripple, fc.astype(np.float64), sr.astype(np.float64))
    got = PR.device("lp24_coefd_from_fc", ripple, fc, sr)
    _distance("lp24_coefd_from_fc", got, PR.host("lp24_coefd_from_fc", ripple, fc, sr), _small_quantities)
    rel, low = _coefficient_errors("lp24_coefd_from_fc", got, want, fc, sr)
    _assert_bar("lp24_coefd_from_fc", rel, 2e-6, low, ripple, fc, sr)
    _assert_bar("lp24_coefd_from_fc", rel, 2e-5, ~low, ripple, fc, sr)


def _percents_of(fc):
    """The cutoff percents whose 25 x 800^pct are the cutoffs (fp32, clamped to [0, 1] as the device clamps them), and the cutoffs those
    fp32 percents stand for, in float64: the reference is evaluated THERE, so that the rounding of the input is nobody's error."""
    pct = np.clip(np.log(fc.astype(np.float64) / 25.0) / np.log(800.0), 0.0, 1.0).astype(np.float32)
    return pct, 25.0 * 800.0 ** pct.astype(np.float64)


@functools.lru_cache(None)
def _pct_form():
    """lp24_coefd_from_pct on the device, with `wide` as derive_welsh sets it, at the percents whose 25 x 800^pct are the draw's cutoffs,
    against derive.h's lp24_coeffs_h at the cutoff the fp32 percent stands for."""
    ripple, fc, sr = _coefficient_draw()
    pct, fc_of_pct = _percents_of(fc)
    sr64 = sr.astype(np.float64)
    fc_ref = np.clip(fc_of_pct, 1.0, 0.49 * sr64)
    want = PR.host("ref_lp24_coeffs_h", ripple, fc_ref, sr64)
    got = PR.device("lp24_coefd_from_pct", ripple, pct, sr)
    _distance("lp24_coefd_from_pct", got, PR.host("lp24_coefd_from_pct", ripple, pct, sr), _small_quantities)
    rel, low = _coefficient_errors("lp24_coefd_from_pct", got, want, fc_ref, sr)
    return rel, low, ripple, fc_ref, sr


def test_lp24_coefd_from_pct_on_the_device_keeps_the_upper_bar_everywhere():
    """The bar the emulation tier sets above 0.4 SR, 2e-5, held there (measured 6.556e-6) — and, as the ceiling of what the expected
    failure below may hide, on the lower side too (measured 3.148e-6): that side's own bar is the next test's."""
    rel, low, ripple, fc, sr = _pct_form()
    _assert_bar("lp24_coefd_from_pct", rel, 2e-5, ~low, ripple, fc, sr)
    _assert_bar("lp24_coefd_from_pct", rel, 2e-5, low, ripple, fc, sr)


@pytest.mark.xfail(strict=True, reason="ripple 3.7053, cutoff 3940.99 Hz (pct 0.75709) at 22,050 Hz: section b's 2 + a1 is 3.148e-6 off on the device, bar 2e-6 "
                   "(host build: 2.578e-6 at ripple 3.3511, 11000.82 Hz, 44,100 Hz; 6 of the 20,000 cases miss, all with ripples 3.18 - 3.78 and all in section b). "
                   "The one-sided a1 of lp24_coefd_from_t just below the WF_COEF_WIDE threshold (c0 < 1/512, ripple ~3.8): 4 b0 rounds at 2^-24 against "
                   "a distance from -2 of 0.1.  Moving the threshold changes which per-frame body those patches run: a pull request of its own")
def test_lp24_coefd_from_pct_on_the_device_keeps_the_lower_bar():
    """The 2e-6 bar up to 0.4 SR, and nothing else.  Measured on an MI355X: 3.148e-6 (missed, see the mark)."""
    rel, low, ripple, fc, sr = _pct_form()
    _assert_bar("lp24_coefd_from_pct", rel, 2e-6, low, ripple, fc, sr)


@functools.lru_cache(None)
def _f32_form():
    ripple, fc, sr = _coefficient_draw()
    exact = PR.host("ref_lp24_coeffs_h", ripple, fc.astype(np.float64), sr.astype(np.float64))
    got = PR.device("lp24_coeff_from_fc", ripple, fc, sr)
    _distance("lp24_coeff_from_fc (lp24_t_from_fc, lp24_coeff_from_t)", got, PR.host("lp24_coeff_from_fc", ripple, fc, sr), _small_quantities)
    return got, exact


def test_lp24_coeff_from_t_on_the_device_holds_what_fp32_can_hold():
    """lp24_t_from_fc then lp24_coeff_from_t (the fp32 filter kind's coefficients) against derive.h's f64 coefficients, to what the
    arithmetic admits.  The form computes the fp32 quotients b0 and q2 = 1 + a2 (upper side: 1 / D', q2, P / D') of the f64 form, which
    the test above holds to a relative `bar` (2e-6 up to 0.4 SR, 2e-5 above), and finishes them in fp32:
      b0                      no further operation:                  |error| <= bar b0 + 2^-25 b0 (the comparison's own rounding of b0)
      a2 = q2 - 1             one rounding of a value below 1:       |error| <= bar (1 + a2) + 2^-25
      a1 = +-(2 - q2 - 4 b0)  2 - q2 rounds at <= 2^-24 (a value <= 2), the fma at <= 2^-24; q2 + 4 b0 (upper side q2 + 4 P / D') is
                              2 - a1 or 2 + a1, never more than 2 + |a1|:   |error| <= bar (2 + |a1|) + 2^-23
    The references are the f64 coefficients themselves, so no rounding of theirs enters."""
    ripple, fc, sr = _coefficient_draw()
    got, exact = _f32_form()
    g = got.astype(np.float64)
    bar = np.where(fc.astype(np.float64) <= 0.4 * sr.astype(np.float64), 2e-6, 2e-5)
    for s in (0, 3):
        for col, allowed in ((s, bar * exact[:, s] + 2.0 ** -25 * exact[:, s]), (s + 2, bar * (1.0 + exact[:, s + 2]) + 2.0 ** -25),
                             (s + 1, bar * (2.0 + np.abs(exact[:, s + 1])) + 2.0 ** -23)):
            err = np.abs(g[:, col] - exact[:, col])
            i = int(np.argmax(err / allowed))
            print(f"lp24_coeff_from_t: column {col}: worst share of its bound {err[i] / allowed[i]:.3f}")
            assert err[i] <= allowed[i], (col, float(ripple[i]), float(fc[i]), float(sr[i]), float(g[i, col]), float(exact[i, col]), float(allowed[i]))


@pytest.mark.xfail(strict=True, reason="ripple 10.708, cutoff 8169.42 Hz at 22,050 Hz: section b's 2 - |a1| is 4.03e-3 off (bar 2e-6), and 4.88e-3 above 0.4 SR (bar 2e-5), "
                   "on the device and in the host build alike: an fp32 a1 or a2 cannot hold a small quantity finer than its own ulp (6e-8 against 1 + a2 = 1e-5), "
                   "neither can the reference rounded once.  The library promises the fp32 recurrence patch by patch, by measurement (derive.h "
                   "welsh_filter_f32_ok), not by these bars; holding them would mean carrying q1 and q2 in the fp32 step, which changes the timed kernels")
def test_lp24_coeff_from_t_on_the_device_against_the_f64_coefficients_rounded_once():
    """The same coefficients at the bars of the f64 form, as the issue of this test sets them: against derive.h's f64 coefficients rounded
    once to fp32.  Measured on an MI355X: 4.032e-3 / 4.878e-3 (see the mark); what the form does hold is the test above."""
    ripple, fc, sr = _coefficient_draw()
    got, exact = _f32_form()
    rel, low = _coefficient_errors("lp24_coeff_from_t", got, exact.astype(np.float32), fc, sr)
    _assert_bar("lp24_coeff_from_t", rel, 2e-6, low, ripple, fc, sr)
    _assert_bar("lp24_coeff_from_t", rel, 2e-5, ~low, ripple, fc, sr)


# ------------------------------------------------------------------ e. the contracted functions
@pytest.mark.parametrize("cubic", [False, True], ids=["linear", "cubic"])
def test_sample_interp_against_the_f64_formula(cubic):
    """10^5 tap sets with |tap| <= 1 and t = k 2^-24 against the float64 formula (tests/test_gpu_sampler_interp.py's, stated in
    tests/dsp_primitive_cases.py) and that file's bound 2^-18 M (M the largest |tap|); at t = 0 the bits of tap 0."""
    rng = np.random.default_rng(37 + cubic)
    n = K.RANDOM
    taps = rng.uniform(-1.0, 1.0, (n, 4)).astype(np.float32)
    taps[:100] *= np.float32(1e-3)
    taps[100:200, 1:] = taps[100:200, :1]                       # flat
    taps[200] = [1.0, -1.0, 1.0, -1.0]
    t = (rng.integers(0, 1 << 24, n) * 2.0 ** -24).astype(np.float32)
    t[300:400] = 0.0
    t[400], t[401] = 2.0 ** -24, 1.0 - 2.0 ** -24
    name = "sample_interp_cubic" if cubic else "sample_interp_linear"
    first = -1 if cubic else 0                                  # the probe's taps are q[0..]: tap `first` of the frame onwards
    ref, m = K.interp_f64(cubic, taps, t)
    got = PR.device(name, taps, t)
    _distance(name, got, PR.host(name, taps, t))
    err = np.abs(got.astype(np.float64) - ref)
    i = int(np.argmax(err - 2.0 ** -18 * m))
    print(f"{name}: worst error {err.max():.3e}, worst share of the bound {np.max(err / np.maximum(2.0 ** -18 * m, 1e-300)):.3f}")
    assert np.all(err <= 2.0 ** -18 * m), (name, taps[i].tolist(), float(t[i]), float(got[i]), float(ref[i]))
    zero = t == 0.0
    assert np.count_nonzero(zero) >= 100
    assert np.array_equal(_bits(got[zero]), _bits(taps[zero, -first].copy()))


@pytest.mark.parametrize("name", ["welsh_env_cutoff_pct", "welsh_lfo_cutoff_pct"])
def test_cutoff_percent_laws_within_4_ulp_of_the_f64_formula(name):
    rng = np.random.default_rng(37)
    n = K.RANDOM
    start = rng.uniform(0.0, 1.0, n).astype(np.float32)
    if name == "welsh_env_cutoff_pct":   # start + (1 - start) end env
        b, c = rng.uniform(0.0, 1.0, n).astype(np.float32), rng.uniform(0.0, 1.0, n).astype(np.float32)
        start[:4], b[:4], c[:4] = [0.0, 1.0, 0.5, 0.1], [1.0, 1.0, 0.0, 1.0], [1.0, 0.5, 1.0, 0.0]
        ref = start.astype(np.float64) + (1.0 - start.astype(np.float64)) * b.astype(np.float64) * c.astype(np.float64)
    else:                                # start (1 + lfo depth)
        b, c = rng.uniform(0.0, 1.0, n).astype(np.float32), rng.uniform(-1.0, 1.0, n).astype(np.float32)
        start[:4], b[:4], c[:4] = [0.0, 1.0, 0.5, 0.1], [1.0, 1.0, 0.0, 1.0], [1.0, -1.0, 1.0, -0.999]
        ref = start.astype(np.float64) * (1.0 + c.astype(np.float64) * b.astype(np.float64))
    got = PR.device(name, start, b, c)
    _distance(name, got, PR.host(name, start, b, c))
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    err = np.abs(got.astype(np.float64) - ref) / ulp
    i = int(np.argmax(err))
    print(f"{name}: worst error {err[i]:.3f} ulp")
    assert err[i] <= 4.0, (name, float(start[i]), float(b[i]), float(c[i]), float(got[i]), float(ref[i]))
