"""The inputs of the dsp_core.h primitive tests and their EXACT references, shared by the CPU tier (tests/test_dsp_primitives_cpu.py: the
host build against these references) and the GPU tier (tests/test_gpu_dsp_primitives.py: the device against the host build, bit for bit,
on the same inputs).  References are Python integers, fractions and single numpy roundings; nothing here needs mpmath or a GPU.
Every set is drawn once (fixed seeds) and cached."""
import functools
import math
from fractions import Fraction

import numpy as np

RANDOM = 100_000
TWO64 = 1 << 64
WAVE_NONE, WAVE_SINE, WAVE_SQUARE, WAVE_PULSE_WIDTH, WAVE_TRIANGLE, WAVE_SAWTOOTH, WAVE_NOISE = 0, 1, 2, 3, 4, 5, 6
WAVE_DEBUG_ZERO, WAVE_DEBUG_MAX, WAVE_DEBUG_MIN, WAVE_TRIANGLE_SINE = 7, 8, 9, 10
EXACT_WAVES = (WAVE_NONE, WAVE_SQUARE, WAVE_PULSE_WIDTH, WAVE_TRIANGLE, WAVE_SAWTOOTH, WAVE_DEBUG_ZERO, WAVE_DEBUG_MAX, WAVE_DEBUG_MIN, WAVE_TRIANGLE_SINE, 11)
F32_PI_4 = np.float32(0.78539816339744831)
F32_PI_2 = np.float32(1.57079632679489662)


def _rng(seed):
    return np.random.default_rng(seed)


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------ f64_to_u64
@functools.lru_cache(None)
def f64_to_u64_inputs():
    x = [0.0, 0.5, 1.0 - 2.0 ** -53, 2.0 ** 32 - 0.5, 2.0 ** 53 - 1.0, 2.0 ** 53, 2.0 ** 53 + 2.0, float(2 ** 53 + 1), math.nextafter(2.0 ** 64, 0.0)]
    for k in range(64):
        p = 2.0 ** k
        x += [math.nextafter(p, 0.0), p, math.nextafter(p, math.inf)]
    r = 2.0 ** _rng(11).uniform(-10.0, 64.0, RANDOM)     # log-uniform in [2^-10, 2^64)
    x = np.concatenate([np.array(x), np.minimum(r, math.nextafter(2.0 ** 64, 0.0))])
    assert np.all((x >= 0.0) & (x < 2.0 ** 64))
    return x


@functools.lru_cache(None)
def f64_to_u64_exact():
    return np.array([int(v) for v in f64_to_u64_inputs()], dtype=np.uint64)


# ------------------------------------------------------------------ fract_f64 (x >= 0, its only use)
@functools.lru_cache(None)
def fract_inputs():
    ints = [0, 1, 2, 3, 7, 100, 44100, 2 ** 31 - 1, 2 ** 31, 2 ** 32, 2 ** 52 - 1, 2 ** 52, 2 ** 53 - 1, 2 ** 53] + [2 ** k for k in range(2, 53, 5)]
    x = [0.0, 2.0 ** -1022, 5e-324, 0.5, 1.0 - 2.0 ** -53] + [float(n) for n in ints]
    x += [math.nextafter(float(n + 1), 0.0) for n in ints if n < 2 ** 52]      # n + the largest fraction a double holds there (n = 0: 1 - 2^-53)
    r = _rng(12)
    x = np.concatenate([np.array(x), 2.0 ** r.uniform(-30.0, 53.0, RANDOM // 2), r.uniform(0.0, 4.0, RANDOM // 2)])
    assert np.all(x >= 0.0)
    return x


@functools.lru_cache(None)
def fract_exact():
    """x - floor(x) in rationals; always a double for x >= 0 (checked)."""
    out = np.empty(fract_inputs().size)
    for i, v in enumerate(fract_inputs()):
        f = Fraction(float(v)) % 1
        out[i] = float(f)
        assert Fraction(float(out[i])) == f
    return out


# ------------------------------------------------------------------ turns_to_inc, turns_to_phase
@functools.lru_cache(None)
def turns_inputs():
    mags = [0.0, 2.0 ** -70, 2.0 ** -65, 2.0 ** -64, 0.25, 0.5, 1.0 - 2.0 ** -53, 1.0, 1.5, 101.25, 2.0 ** 31 - 0.5]
    r = _rng(13)
    rnd = np.concatenate([r.uniform(-2.0, 2.0, RANDOM // 2), r.choice([-1.0, 1.0], RANDOM // 2) * 2.0 ** r.uniform(-40.0, 31.0, RANDOM // 2)])
    x = np.concatenate([np.array(mags), -np.array(mags), rnd])
    assert np.all(np.abs(x) < 2.0 ** 31)
    return x


def _frac_times_2_64(a):
    """floor(frac(a) 2^64) for a double a >= 0, exactly: fmod by 1 and a scaling by a power of two are exact in doubles."""
    return int(math.fmod(a, 1.0) * 2.0 ** 64)


@functools.lru_cache(None)
def turns_to_inc_exact():
    """floor(frac(t) 2^64) for t >= 0, the two's complement of floor(frac(-t) 2^64) for t < 0 (-0.0 is 0): turns_to_inc's and
    turns_to_phase's exact integer alike."""
    return np.array([_frac_times_2_64(t) if t >= 0.0 else (-_frac_times_2_64(-t)) % TWO64 for t in turns_inputs().tolist()], dtype=np.uint64)


# ------------------------------------------------------------------ fold_quarter, fold_quarter64
def _fold_inputs(bits, seed):
    q, top = 1 << (bits - 2), 1 << (bits - 1)
    v = [0, 1, -1, q - 1, q, q + 1, -q - 1, -q, -q + 1, top - 1, -top + 1, top - 2, 2 * q // 3, -2 * q // 3]
    dt = np.int32 if bits == 32 else np.int64
    r = _rng(seed).integers(-top + 1, top, RANDOM, dtype=np.int64, endpoint=False)
    return np.concatenate([np.array(v, dtype=np.int64), r]).astype(dt)


def fold_exact(q, bits):
    """The fold restated on Python integers: |p| >= a quarter turn -> half a turn - p, wrapped into the signed range."""
    quarter, half, full = 1 << (bits - 2), 1 << (bits - 1), 1 << bits
    out = []
    for v in q.tolist():
        if v >= quarter or v < -quarter:
            v = (half - v) % full
            v = v - full if v >= half else v
        out.append(v)
    return np.array(out, dtype=q.dtype)


@functools.lru_cache(None)
def fold32_inputs():
    return _fold_inputs(32, 14)


@functools.lru_cache(None)
def fold64_inputs():
    return _fold_inputs(64, 15)


# ------------------------------------------------------------------ osc_value, osc_value_f64 (every waveform but sine and noise)
@functools.lru_cache(None)
def osc_inputs():
    """(waveform, phase, duty64), each [n]: the named phases under every waveform and three duties, then random draws."""
    duties = [1 << 63, 0, TWO64 - 1, 0x3333333333333000, 12345]
    phases = [0, 1, (1 << 62) - 1, 1 << 62, (1 << 62) + 1, (1 << 63) - 1, 1 << 63, (1 << 63) + 1, TWO64 - 1, (3 << 62) - 1, 3 << 62, (3 << 62) + 1,
              (1 << 32) - 1, 1 << 32, 0x7FFFFF8000000000, 0x8000008000000000]
    w, p, d = [], [], []
    for wave in EXACT_WAVES:
        for duty in duties:
            for ph in phases + [(duty - 1) % TWO64, duty, (duty + 1) % TWO64]:
                w.append(wave); p.append(ph); d.append(duty)
    r = _rng(16)
    n = RANDOM
    w = np.concatenate([np.array(w, dtype=np.uint32), r.choice(np.array(EXACT_WAVES, dtype=np.uint32), n)])
    p = np.concatenate([np.array(p, dtype=np.uint64), r.integers(0, TWO64, n, dtype=np.uint64, endpoint=False)])
    d = np.concatenate([np.array(d, dtype=np.uint64), r.integers(0, TWO64, n, dtype=np.uint64, endpoint=False)])
    return w, p, d


@functools.lru_cache(None)
def osc_value_exact():
    """fp32: q = the phase's top 32 bits as a signed integer; (float)q is one rounding (numpy's int32 -> float32 is the C cast), the
    scalings by powers of two are exact, and 4 |a| 2^-32 - 1 is exact in a double (a multiple of 2^-30 in [-1, 1]), rounded once."""
    w, p, d = osc_inputs()
    q = (p >> np.uint64(32)).astype(np.uint32).view(np.int32)
    a = q.astype(np.float32).astype(np.float64)
    r = (q.view(np.uint32) + np.uint32(0x40000000)).view(np.int32).astype(np.float32).astype(np.float64)
    out = np.zeros(w.size, dtype=np.float32)
    pulse = np.where(p < d, np.float32(1.0), np.float32(-1.0))
    out = np.where((w == WAVE_SQUARE) | (w == WAVE_PULSE_WIDTH), pulse, out)
    out = np.where(w == WAVE_TRIANGLE, (np.abs(a) * 2.0 ** -30 - 1.0).astype(np.float32), out)
    out = np.where(w == WAVE_TRIANGLE_SINE, (np.abs(r) * 2.0 ** -30 - 1.0).astype(np.float32), out)
    out = np.where(w == WAVE_SAWTOOTH, (a * 2.0 ** -31).astype(np.float32), out)
    out = np.where(w == WAVE_DEBUG_MAX, np.float32(1.0), out)
    out = np.where(w == WAVE_DEBUG_MIN, np.float32(-1.0), out)
    return out.astype(np.float32)


@functools.lru_cache(None)
def osc_value_f64_exact():
    """f64: (double)(int64)phase is one rounding, the scalings are exact, and the triangle's fma rounds 4 |a| 2^-64 - 1 once: in rationals."""
    w, p, d = osc_inputs()
    q = p.view(np.int64)
    a = q.astype(np.float64)
    r = (p + np.uint64(1 << 62)).view(np.int64).astype(np.float64)
    out = np.zeros(w.size)
    out = np.where((w == WAVE_SQUARE) | (w == WAVE_PULSE_WIDTH), np.where(p < d, 1.0, -1.0), out)
    out = np.where(w == WAVE_SAWTOOTH, a * 2.0 ** -63, out)
    out = np.where(w == WAVE_DEBUG_MAX, 1.0, out)
    out = np.where(w == WAVE_DEBUG_MIN, -1.0, out)
    for wave, src in ((WAVE_TRIANGLE, a), (WAVE_TRIANGLE_SINE, r)):
        idx = np.nonzero(w == wave)[0]
        out[idx] = [float(abs(Fraction(v)) / (1 << 62) - 1) for v in src[idx].tolist()]
    return out


# ------------------------------------------------------------------ noise_tick
NOISE_TICKS = 1000


@functools.lru_cache(None)
def noise_exact():
    """The integer generator restated: [NOISE_TICKS + 1, 3] = (bits of the last tick's value, x1, x2) after k ticks from osc_reset."""
    x1, x2, v = 0x70F4F854, 0xE1E9F0A7, np.float32(0.0)
    rows = [(int(v.view(np.uint32)), x1, x2)]
    for _ in range(NOISE_TICKS):
        x1 ^= x2
        s = x2 - (1 << 32) if x2 >= (1 << 31) else x2
        v = np.float32(np.float32(s) * np.float32(2.0 ** -31))
        x2 = (x2 + x1) & 0xFFFFFFFF
        rows.append((int(v.view(np.uint32)), x1, x2))
    return np.array(rows, dtype=np.uint32)


# ------------------------------------------------------------------ env_frames
@functools.lru_cache(None)
def env_frames_inputs():
    k = np.arange(1, 10001, dtype=np.float32)
    return np.concatenate([np.array([0.0, -0.0, -1.0, np.nan, 7938.0003, 4.1e9, 4.0e9, 3.9e9, 1e-30, np.inf], dtype=np.float32), k,
                           k * np.float32(1.0 + 2.0 ** -16)]).astype(np.float32)


@functools.lru_cache(None)
def env_frames_exact():
    """docs/DSP_SPEC.md section 3: N = ceil(len (1 - 2^-16)) with the product rounded to fp32; 0 for a length that is not positive
    (NaN included); capped at 4e9."""
    x = env_frames_inputs()
    with np.errstate(invalid="ignore"):
        c = np.ceil((x * np.float32(1.0 - 2.0 ** -16)).astype(np.float32)).astype(np.float64)
        pos = x > 0
    return np.where(pos, np.minimum(np.where(pos, c, 0.0), 4.0e9), 0.0).astype(np.uint32)


# ------------------------------------------------------------------ sine, exponentials, tangent: inputs (references: the CPU test's)
@functools.lru_cache(None)
def sin_f32_inputs():
    """float(fold_quarter(q)) 2^-32: every q that is a multiple of 2^9 in [-2^30, 2^30], and every q within 64 of 0 and of +-2^30."""
    q = np.concatenate([np.arange(-(1 << 30), (1 << 30) + 1, 1 << 9, dtype=np.int64), np.arange(-64, 65, dtype=np.int64),
                        (1 << 30) + np.arange(-64, 65, dtype=np.int64), -(1 << 30) + np.arange(-64, 65, dtype=np.int64)])
    over = (q >= (1 << 30)) | (q < -(1 << 30))
    q = np.where(over, np.where(q > 0, (1 << 31) - q, -(1 << 31) - q), q)      # fold_quarter on integers (tested by itself)
    assert np.all(np.abs(q) <= (1 << 30))
    return (q.astype(np.int32).astype(np.float32) * np.float32(2.0 ** -32)).astype(np.float32)


def _f64_points(lo, hi, seed, extra):
    r = _rng(seed)
    n = 1_000_000
    x = np.concatenate([np.linspace(lo, hi, n // 2), r.uniform(lo, hi, n // 2 - len(extra)), np.array(extra)])
    return x


@functools.lru_cache(None)
def sin_f64_inputs():
    return _f64_points(-0.25, 0.25, 17, [-0.25, 0.25, 0.0, 2.0 ** -60, -2.0 ** -60])


@functools.lru_cache(None)
def exp2_small_inputs():
    return _f64_points(-1.0, 1.0, 18, [-1.0, 1.0, 0.0, 2.0 ** -60, -2.0 ** -60])


@functools.lru_cache(None)
def exp_tiny_inputs():
    return _f64_points(-1.5e-3, 1.5e-3, 19, [-1.5e-3, 1.5e-3, 0.0])


@functools.lru_cache(None)
def tan_inputs():
    """2^16 mantissas in every binade from 2^-20 up to pi/4 (the last one cut at fl(pi/4)), both ends."""
    m = 1.0 + np.arange(1 << 16, dtype=np.float64) / (1 << 16)
    z = np.concatenate([m * 2.0 ** e for e in range(-20, 0)]).astype(np.float32)
    z = z[z <= F32_PI_4]
    return np.concatenate([z, np.array([2.0 ** -20, F32_PI_4, np.nextafter(F32_PI_4, np.float32(0))], dtype=np.float32)])


@functools.lru_cache(None)
def tan_reduced_inputs():
    """... and their mirror images pi/2 - z (fp32), with the neighbours of pi/4 on both sides."""
    z = tan_inputs()
    edge = np.array([F32_PI_4, np.nextafter(F32_PI_4, np.float32(1)), np.nextafter(F32_PI_4, np.float32(0))], dtype=np.float32)
    return np.concatenate([z, (F32_PI_2 - z).astype(np.float32), edge])


def tan_reduced_argument(x):
    """What tan_reduced hands to tan_of_reduced, as its text states it: hi = x > fl(pi/4); hi ? fl(fl(pi/2) - x) : x."""
    hi = x > F32_PI_4
    return hi, np.where(hi, (F32_PI_2 - x).astype(np.float32), x).astype(np.float32)


# ------------------------------------------------------------------ sample_interp
def interp_f64(cubic, q, t):
    """The interpolation formulas in float64 (docs/DSP_SPEC.md section 7; the same formula as tests/test_gpu_sampler_interp.py's
    reference, stated here so that this tier loads nothing of the library).  q: [n, 4] taps from the mode's first tap on (linear: the
    frame's taps 0 and 1; cubic: -1, 0, 1, 2), t: [n].  Returns the value and M, the largest |tap| the mode reads."""
    q, t = q.astype(np.float64), t.astype(np.float64)
    if not cubic:
        p0, p1 = q[:, 0], q[:, 1]
        return p0 + t * (p1 - p0), np.maximum(np.abs(p0), np.abs(p1))
    pm, p0, p1, p2 = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    c1 = 0.5 * (p1 - pm)
    c2 = pm - 2.5 * p0 + 2.0 * p1 - 0.5 * p2
    c3 = 0.5 * (p2 - pm) + 1.5 * (p0 - p1)
    return ((c3 * t + c2) * t + c1) * t + p0, np.max(np.abs(q), axis=1)
