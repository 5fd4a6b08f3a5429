"""Inputs and references of the cross-lane probes (tests/probe/wave_probe.hip): the DPP scans, tp_shfl, bq_tp_wave and the scalar noise
generator of csrc/welsh_tp.h; dpp_add / FusedAcc::flush, the wave sums, wave_min_u32 and tp_reduce_prev of csrc/kernels.h.
tests/test_gpu_wave_primitives.py plays the tables on the device; tests/test_wave_primitive_refs_cpu.py checks the references
themselves.  References are Python integers, fractions.Fraction and (numpy) float64 only; `fma` below is the f64 fused multiply-add,
pinned against Fractions by the CPU test.

Exact families: every value of every bracketing is representable, so the device is held bit for bit.  Real families (docs/DSP_SPEC.md
section 14): per case X, the exact result in rationals; S, the serial f64 fold in the serial kernels' order; T, an f64 model of the
scan with the device's bracketing and without contraction; the yardstick y = max(|S - X|, |T - X|, 2^-53 |X|) over the case."""
import ctypes
import ctypes.util
import functools
import math
from fractions import Fraction as Fr

import numpy as np

from tests import dsp_primitive_cases as K
from tests.mix_bodies import FILTERS

f32, f64, u32, u64, i32 = np.float32, np.float64, np.uint32, np.uint64, np.int32
TWO64 = 1 << 64
SR = 44100.0
FC_MAX = 0.49 * SR
LPVS = (64, 32)
PRIMITIVES = ("tp_scan_add_u64", "tp_scan_max_i32", "tp_scan_affine", "tp_shfl", "bq_tp_wave", "tp_noise_ticks", "wave_sum_lane63",
              "wave_sum", "FusedAcc::flush", "wave_min_u32", "tp_reduce_prev")   # the rows of the probe table


def _rng(seed):
    return np.random.default_rng(0x57A7E + seed)


_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fma.restype = ctypes.c_double
_libm.fma.argtypes = [ctypes.c_double] * 3
fma = _libm.fma


def round_frac(x, bits):
    """The Fraction x rounded to a float of `bits` significand bits, ties to even (no subnormals, no overflow: asserted by range)."""
    if x == 0:
        return 0.0
    n, d = abs(x.numerator), x.denominator
    shift = bits - (n.bit_length() - d.bit_length())
    q, r = divmod(n << shift, d) if shift >= 0 else divmod(n, d << -shift)
    den = d if shift >= 0 else d << -shift
    if q >= 1 << bits:   # one bit too many: n / d >= 2^k exactly at the boundary
        shift -= 1
        q, r = divmod(n << shift, d) if shift >= 0 else divmod(n, d << -shift)
        den = d if shift >= 0 else d << -shift
    if 2 * r > den or (2 * r == den and q & 1):
        q += 1
    assert -1000 < -shift < 1000
    v = math.ldexp(q, -shift)
    return -v if x < 0 else v


def representable(x, bits):
    return Fr(round_frac(x, bits)) == x


# ================================================================== groups of lanes
def groups(lpv):
    return [range(g, g + lpv) for g in range(0, 64, lpv)]


# ------------------------------------------------------------------ tp_scan_add_u64
@functools.lru_cache(None)
def scan_add_inputs():
    """[cases, 64, 2] uint64: the pair of sums; names per case."""
    r = _rng(1)
    cases, names = [], []
    for k in range(64):   # one nonzero lane, at every position (the second sum: the mirrored lane, another value)
        a = np.zeros((64, 2), dtype=u64)
        a[k, 0] = 0xFFFFFFFF00000001
        a[63 - k, 1] = 0x00000001FFFFFFFF
        cases.append(a); names.append(f"one lane {k}")
    cases.append(np.full((64, 2), TWO64 - 1, dtype=u64)); names.append("all 2^64 - 1")
    cases.append(np.zeros((64, 2), dtype=u64)); names.append("zeros")
    c = np.full((64, 2), 0xFFFFFFFF, dtype=u64); c[:, 1] = 0x80000000
    cases.append(c); names.append("low halves that carry")
    for i in range(8):
        cases.append(r.integers(0, TWO64, (64, 2), dtype=u64, endpoint=False)); names.append(f"random {i}")
    return np.stack(cases), names


def scan_add_exact(lpv):
    x, _ = scan_add_inputs()
    out = np.empty_like(x)
    for c in range(len(x)):
        for g in groups(lpv):
            for w in range(2):
                run = 0
                for l in g:
                    run = (run + int(x[c, l, w])) % TWO64
                    out[c, l, w] = run
    return out


# ------------------------------------------------------------------ tp_scan_max_i32
@functools.lru_cache(None)
def scan_max_inputs():
    r = _rng(2)
    cases, names = [], []
    cases.append(np.full(64, -1, dtype=i32)); names.append("all -1")
    for k in range(64):
        a = np.full(64, -1, dtype=i32)
        a[k] = (0, 255, 7 + k)[k % 3]
        cases.append(a); names.append(f"one lane {k}")
    cases.append(np.arange(255, 255 - 64, -1).astype(i32)); names.append("descending")
    cases.append(np.arange(62, -2, -1).astype(i32)); names.append("descending to -1")
    for i in range(8):
        cases.append(r.integers(-1, 256, 64).astype(i32)); names.append(f"random {i}")
    a = r.integers(-1, 256, 64).astype(i32); a[r.random(64) < 0.8] = -1
    cases.append(a); names.append("sparse")
    return np.stack(cases), names


def scan_max_exact(lpv):
    x, _ = scan_max_inputs()
    out = np.empty_like(x)
    for g in groups(lpv):
        out[:, g.start:g.stop] = np.maximum.accumulate(np.maximum(x[:, g.start:g.stop], -1), axis=1)
    return out


# ================================================================== the filter's affine maps (Lp24Affine: c0[4], c1[4], c2[2], c3[2], z[4])
IDENTITY = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0)


def affine_mul(m, v, with_z):
    """lp24_affine_mul: Phi v (+ z), the fma nest of the source."""
    z = m[12:16] if with_z else (0.0, 0.0, 0.0, 0.0)
    return [fma(m[0], v[0], fma(m[4], v[1], z[0])),
            fma(m[1], v[0], fma(m[5], v[1], z[1])),
            fma(m[2], v[0], fma(m[6], v[1], fma(m[8], v[2], fma(m[10], v[3], z[2])))),
            fma(m[3], v[0], fma(m[7], v[1], fma(m[9], v[2], fma(m[11], v[3], z[3]))))]


def affine_compose(later, e):
    """lp24_affine_compose: later o e (e first)."""
    c0 = affine_mul(later, e[0:4], False)
    c1 = affine_mul(later, e[4:8], False)
    t2 = affine_mul(later, (0.0, 0.0, e[8], e[9]), False)
    t3 = affine_mul(later, (0.0, 0.0, e[10], e[11]), False)
    z = affine_mul(later, e[12:16], True)
    return tuple(c0 + c1 + t2[2:] + t3[2:] + z)


def lp24_step_v(s, c, x):
    """dsp_core.h lp24_step / welsh_tp.h lp24_step_v on a state list; c = b0a, a1a, a2a, b0b, a1b, a2b.  -> y2, the new state."""
    bx = c[0] * x
    y1 = bx + s[0]
    s0 = fma(c[1], y1, 2.0 * bx + s[1])
    s1 = fma(c[2], y1, bx)
    by = c[3] * y1
    y2 = by + s[2]
    s2 = fma(c[4], y2, 2.0 * by + s[3])
    s3 = fma(c[5], y2, by)
    return y2, [s0, s1, s2, s3]


def _step_h(s, c):
    y1 = s[0]
    by = c[3] * y1
    y2 = by + s[2]
    return [fma(c[1], y1, s[1]), c[2] * y1, fma(c[4], y2, 2.0 * by + s[3]), fma(c[5], y2, by)]


def _step_h2(s, c):
    return [fma(c[4], s[0], s[1]), c[5] * s[0]]


def affine_push(m, c, x):
    """lp24_affine_push: one more frame with coefficients c and input x."""
    _, z = lp24_step_v(list(m[12:16]), c, x)
    return tuple(_step_h(list(m[0:4]), c) + _step_h(list(m[4:8]), c) + _step_h2(list(m[8:10]), c) + _step_h2(list(m[10:12]), c) + z)


def scan_affine_model(lpv, maps):
    """T: tp_scan_affine<lpv> on the 64 records of a wavefront, step by step as the DPP controls move them — rows of 16 lanes by
    row_shr 1, 2, 4, 8 (a lane with no source composes with the identity), row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2 and
    3 when a voice spans the wavefront."""
    m = [tuple(x) for x in maps]
    for k in (1, 2, 4, 8):
        m = [affine_compose(m[l], m[l - k] if (l & 15) >= k else IDENTITY) for l in range(64)]
    m = [affine_compose(m[l], m[(l & ~15) - 1] if (l >> 4) in (1, 3) else IDENTITY) for l in range(64)]
    if lpv == 64:
        m = [affine_compose(m[l], m[31] if l >= 32 else IDENTITY) for l in range(64)]
    return m


def _to_matrix(m):
    P = [[Fr(m[0]), Fr(m[4]), Fr(0), Fr(0)], [Fr(m[1]), Fr(m[5]), Fr(0), Fr(0)],
         [Fr(m[2]), Fr(m[6]), Fr(m[8]), Fr(m[10])], [Fr(m[3]), Fr(m[7]), Fr(m[9]), Fr(m[11])]]
    return P, [Fr(v) for v in m[12:16]]


def _from_matrix(P, z):
    assert P[0][2] == P[0][3] == P[1][2] == P[1][3] == 0   # the record's block shape survives composition
    return (P[0][0], P[1][0], P[2][0], P[3][0], P[0][1], P[1][1], P[2][1], P[3][1], P[2][2], P[3][2], P[2][3], P[3][3], z[0], z[1], z[2], z[3])


def scan_affine_exact(lpv, maps):
    """The inclusive composition in lane order per group of lpv lanes, in rationals: 64 records of 16 Fractions."""
    out = []
    for g in groups(lpv):
        P = z = None
        for l in g:
            M, w = _to_matrix(maps[l])
            if P is None:
                P, z = M, w
            else:
                P, z = ([[sum(M[i][k] * P[k][j] for k in range(4)) for j in range(4)] for i in range(4)],
                        [sum(M[i][k] * z[k] for k in range(4)) + w[i] for i in range(4)])
            out.append(_from_matrix(P, z))
    return out


def _exact_generators():
    """Maps with small dyadic entries whose products stay small: signed permutations and quarter turns of each section (norm-preserving,
    so the coupling block grows linearly with the lanes), a coupling block of small integers, integer z."""
    blocks = [(1, 0, 0, 1), (-1, 0, 0, -1), (0, 1, 1, 0), (0, 1, -1, 0), (0, -1, 1, 0), (1, 0, 0, -1)]   # (m00, m10, m01, m11) column-wise
    r = _rng(3)
    gens = []
    for i in range(24):
        a, b = blocks[r.integers(len(blocks))], blocks[r.integers(len(blocks))]
        cpl = r.integers(-2, 3, 4)
        z = r.integers(-4, 5, 4)
        gens.append(tuple(float(v) for v in (a[0], a[1], cpl[0], cpl[1], a[2], a[3], cpl[2], cpl[3], b[0], b[1], b[2], b[3], z[0], z[1], z[2], z[3])))
    return gens


SHEAR = (1.0, 1.0, 0.0, 1.0, 0.0, 1.0, 1.0, 0.0, 1.0, 1.0, 0.0, 1.0, 1.0, -1.0, 2.0, 0.5)   # accumulates: entries grow with the lanes
LONE = (0.0, 1.0, 2.0, -1.0, -1.0, 0.0, 0.5, 3.0, 0.0, -1.0, 1.0, 0.0, 1.0, -2.0, 3.0, -4.0)   # the one map of "identity but lane k"
PAIR_A = (1.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 1.0, 0.0, 0.0, 0.0)   # A B != B A
PAIR_B = (0.0, 1.0, 0.0, 0.0, -1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


@functools.lru_cache(None)
def affine_exact_inputs():
    """[cases, 64, 16] float64, the start states [cases, 4], names."""
    gens = _exact_generators()
    r = _rng(4)
    cases, names = [], []
    for k in range(64):
        cases.append([LONE if l == k else IDENTITY for l in range(64)]); names.append(f"identity but lane {k}")
    cases.append([SHEAR] * 64); names.append("the same shear in every lane")
    cases.append([PAIR_A if l & 1 else PAIR_B for l in range(64)]); names.append("a pair that does not commute, alternating")
    cases.append([PAIR_B if l & 1 else PAIR_A for l in range(64)]); names.append("the pair the other way round")
    for i in range(8):
        pick = r.integers(len(gens), size=64)
        m = [gens[j] for j in pick]
        if i >= 4:   # a few lanes scaled by 1/2 (dyadic, not integer)
            for l in r.choice(64, 6, replace=False):
                m[l] = tuple(0.5 * v for v in m[l])
        cases.append(m); names.append(f"random generators {i}")
    s0 = r.integers(-3, 4, (len(cases), 4)).astype(f64)
    s0[0] = (1.0, -2.0, 3.0, 0.5)
    return np.array(cases, dtype=f64), s0, names


@functools.lru_cache(None)
def affine_exact_refs(lpv):
    """Records [cases, 64, 16] and states [cases, 64, 4] as Fractions (object arrays)."""
    maps, s0, _ = affine_exact_inputs()
    rec = np.empty(maps.shape, dtype=object)
    st = np.empty(maps.shape[:2] + (4,), dtype=object)
    for c in range(len(maps)):
        rows = scan_affine_exact(lpv, [tuple(m) for m in maps[c].tolist()])
        for l, row in enumerate(rows):
            rec[c, l] = row
            P, z = _to_matrix(row)
            st[c, l] = [sum(P[i][k] * Fr(float(s0[c, k])) for k in range(4)) + z[i] for i in range(4)]
    return rec, st


def filter_coefs(ripple, fc):
    """The library's own f64 coefficients of a cutoff (lp24_coefd_from_fc, host build): [n, 6]."""
    from tests.probe import probe as PR
    fc = np.atleast_1d(np.asarray(fc, dtype=f32))
    return PR.host("lp24_coefd_from_fc", np.full(fc.size, ripple, dtype=f64), fc, np.full(fc.size, SR, dtype=f32))


REAL_CUTOFFS = (25.0, 40.0, 100.0, 440.0, 2500.0, 8000.0, 15000.0, FC_MAX)
REAL_RIPPLES = (0.707, 4.0)


@functools.lru_cache(None)
def affine_real_voices():
    """Voices of 256 frames: (name, coefficients [256, 6], inputs [256] as f32 widened, start state [4]).  Cutoffs 25 Hz .. fc_max at two
    ripples (mix_bodies.FILTERS' 2,500 Hz and 40 Hz sets among them), noise and a step; two swept cutoffs (coefficients per frame)."""
    assert {h for h, _, _, rp in FILTERS.values()} <= set(REAL_CUTOFFS) and {rp for _, _, _, rp in FILTERS.values()} <= set(REAL_RIPPLES)
    r = _rng(5)
    voices = []
    for ripple in REAL_RIPPLES:
        for i, fc in enumerate(REAL_CUTOFFS):
            coef = np.repeat(filter_coefs(ripple, fc), 256, axis=0)
            kind = ("noise", "step")[(i + (ripple > 1.0)) & 1]
            x = r.uniform(-1.0, 1.0, 256).astype(f32) if kind == "noise" else np.where(np.arange(256) >= 37, 1.0, 0.0).astype(f32)
            voices.append((f"ripple {ripple} fc {fc:.0f} {kind}", coef, x.astype(f64), r.uniform(-1.0, 1.0, 4)))
    sweep = 25.0 * 800.0 ** np.linspace(0.02, 0.98, 256)
    voices.append(("sweep up, noise", filter_coefs(0.707, sweep), r.uniform(-1.0, 1.0, 256).astype(f32).astype(f64), r.uniform(-1.0, 1.0, 4)))
    voices.append(("sweep down, step", filter_coefs(4.0, sweep[::-1].copy()), np.where(np.arange(256) >= 5, -1.0, 0.5), np.zeros(4)))
    return voices


def affine_real_cases(lpv):
    """(names, maps [cases, 64, 16], s0 [cases, 4], frames of every lane): lpv = 64: a voice a case, four frames a lane; lpv = 32: two
    voices a case, eight frames a lane, both from the first voice's start state."""
    voices = affine_real_voices()
    per = 256 // lpv
    names, maps, s0, lanes = [], [], [], []
    sets = [(v,) for v in voices] if lpv == 64 else [(voices[i], voices[i + 1]) for i in range(0, len(voices), 2)]
    for vs in sets:
        case_maps, case_lanes = [], []
        for _, coef, x, _ in vs:
            for l in range(lpv):
                fr = [(tuple(coef[f].tolist()), float(x[f])) for f in range(l * per, (l + 1) * per)]
                m = IDENTITY
                for c, xv in fr:
                    m = affine_push(m, c, xv)
                case_maps.append(m); case_lanes.append(fr)
        names.append(" | ".join(v[0] for v in vs)); maps.append(case_maps); s0.append(vs[0][3]); lanes.append(case_lanes)
    return names, np.array(maps, dtype=f64), np.array(s0, dtype=f64), lanes


@functools.lru_cache(None)
def affine_real_refs(lpv):
    """names, maps, s0 and X (Fractions), S, T (float64): [cases, 64, 4], the state after every lane."""
    names, maps, s0, lanes = affine_real_cases(lpv)
    X = np.empty(maps.shape[:2] + (4,), dtype=object)
    S = np.empty(maps.shape[:2] + (4,), dtype=f64)
    T = np.empty_like(S)
    for c in range(len(maps)):
        ms = [tuple(m) for m in maps[c].tolist()]
        start = [float(v) for v in s0[c]]
        for g in groups(lpv):
            xs, ss = [Fr(v) for v in start], list(start)
            for l in g:
                P, z = _to_matrix(ms[l])
                xs = [sum(P[i][k] * xs[k] for k in range(4)) + z[i] for i in range(4)]
                for cf, xv in lanes[c][l]:
                    _, ss = lp24_step_v(ss, cf, xv)
                X[c, l], S[c, l] = xs, ss
        for l, m in enumerate(scan_affine_model(lpv, ms)):
            T[c, l] = affine_mul(m, start, True)
    return names, maps, s0, X, S, T


def yardstick(X, S, T):
    """y of a case (leading axis): max(|S - X|, |T - X|, 2^-53 |X|) over everything behind the leading axis, as floats."""
    def dist(A):
        return np.array([[float(abs(Fr(float(a)) - x)) for a, x in zip(ra.reshape(-1), rx.reshape(-1))] for ra, rx in zip(A, X)])
    mag = np.array([[float(abs(x)) for x in rx.reshape(-1)] for rx in X]) * 2.0 ** -53
    return np.maximum(np.maximum(dist(S), dist(T)), mag).max(axis=1)


def ratios(D, X, y):
    """|D - X| / y per case."""
    return np.array([max(float(abs(Fr(float(a)) - x)) for a, x in zip(rd.reshape(-1), rx.reshape(-1))) for rd, rx in zip(D, X)]) / y


def rel_to_serial(D, S):
    """max |D - S| / max |S| per case: the distance welsh_tp.h's header speaks of."""
    n = len(D)
    return np.abs(D.reshape(n, -1) - S.reshape(n, -1)).max(axis=1) / np.abs(S.reshape(n, -1)).max(axis=1)


# ================================================================== tp_shfl
SHFL_DISTANCES = tuple(range(0, 33))


@functools.lru_cache(None)
def shfl_inputs():
    """d [cases], 32-bit values [cases, 64], 64-bit values [cases, 64] whose halves differ."""
    r = _rng(6)
    d = np.array(SHFL_DISTANCES, dtype=i32)
    v32 = r.integers(0, 1 << 32, (d.size, 64), dtype=u64).astype(u32)
    lanes = np.arange(64, dtype=u64)
    v64 = np.stack([((lanes * u64(3) + u64(0x80000001 + 977 * i)) << u64(32)) | (u64(0x7FFFFFF0) - lanes * u64(5) + u64(i)) for i in range(d.size)])
    v64[1::2] = r.integers(0, TWO64, (len(v64[1::2]), 64), dtype=u64, endpoint=False)
    return d, v32, v64


def shfl_judged(d):
    """[cases, 64]: the lanes whose source lane - d is inside the wavefront, and that source."""
    src = np.arange(64)[None, :] - np.asarray(d)[:, None]
    return (src >= 0) & (src < 64), np.clip(src, 0, 63)


# ================================================================== bq_tp_wave
BQ_FRAMES = (1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 252, 253, 255, 256)
BQ_WETS = (1.0, 0.3)
# b0, b1, b2, a1, a2 (y = b0 x + b1 x1 + b2 x2 - a1 y1 - a2 y2): integrators, sign alternators, quarter and sixth turns — every power of the
# recurrence's matrix stays small — and two with a half in the feedback, for blocks short enough for the dyadic depth
BQ_EXACT_COEFS = ((1.0, 0.0, 0.0, -1.0, 0.0), (1.0, -1.0, 0.5, 1.0, 0.0), (0.5, 0.5, 0.0, 0.0, 1.0), (1.0, 0.0, -1.0, 0.0, -1.0),
                  (-1.0, 1.0, 1.0, -1.0, 1.0), (0.5, 0.0, 0.5, 1.0, 1.0), (1.0, 1.0, 1.0, 0.0, 0.0))
BQ_EXACT_SHORT = ((1.0, 0.5, 0.0, 0.5, 0.0), (1.0, 0.0, 0.0, -0.5, 0.5))
BQ_SHORT_FRAMES = 9


def _bq_voices(exact):
    r = _rng(7 if exact else 8)
    voices = []
    designs = None if exact else bq_real_designs()
    i = 0
    for wet in BQ_WETS:
        for frames in BQ_FRAMES:
            for rep in range(2):
                if exact:
                    pool = BQ_EXACT_COEFS + (BQ_EXACT_SHORT if frames <= BQ_SHORT_FRAMES else ())
                    name, c = "exact", pool[i % len(pool)]
                    x = r.integers(-3, 4, 256).astype(f32)
                    st = r.integers(-2, 3, 4).astype(f64)
                else:
                    name, c = designs[i % len(designs)]
                    x = r.uniform(-1.0, 1.0, 256).astype(f32)
                    st = r.uniform(-1.0, 1.0, 4)
                    st[:2] = st[:2].astype(f32)   # x1, x2: earlier inputs
                if rep == 1 and frames > 2:
                    x[frames - 1] = x[frames - 2] + f32(1.0)   # the last two inputs differ, whatever was drawn
                voices.append((f"{name} {tuple(c)} frames {frames} wet {wet}", frames, float(f32(wet)), tuple(float(v) for v in c), x, st))
                i += 1
    return voices


@functools.lru_cache(None)
def bq_real_designs():
    """The nine IIR modes of fx_coef.h (eight cookbook biquads; the 24 dB low-pass's first section, as a biquad) and the hard corners: a
    low cutoff at high Q, a high cutoff, a narrow band."""
    from tests.probe import wave_probe as WP
    from groove_amd import abi_types as T
    out = []
    for kind, cut, q, bw, gain in ((T.FX_BIQUAD_LP12, 1000.0, 0.707, 0, 0), (T.FX_BIQUAD_HP12, 300.0, 2.0, 0, 0), (T.FX_BIQUAD_BP12, 800.0, 0, 200.0, 0),
                                   (T.FX_BIQUAD_BS12, 5000.0, 0, 1000.0, 0), (T.FX_BIQUAD_AP12, 2000.0, 1.0, 0, 0), (T.FX_BIQUAD_PEAK12, 1200.0, 0, 0, 6.0),
                                   (T.FX_BIQUAD_LSHELF12, 200.0, 0, 0, -9.0), (T.FX_BIQUAD_HSHELF12, 6000.0, 0, 0, 4.0),
                                   (T.FX_BIQUAD_LP12, 30.0, 10.707, 0, 0), (T.FX_BIQUAD_HP12, 25.0, 10.707, 0, 0), (T.FX_BIQUAD_LP12, 21000.0, 0.707, 0, 0),
                                   (T.FX_BIQUAD_BP12, 60.0, 0, 2.0, 0)):
        out.append((f"kind {kind} {cut:.0f} Hz", tuple(WP.rbj_for_kind(kind, cut, q, bw, gain, SR).tolist())))
    for fc, ripple in ((40.0, 0.707), (2500.0, 4.0)):
        b0, a1, a2 = WP.fx_lp24_coeffs(fc, ripple, SR)[:3].tolist()
        out.append((f"24 dB section {fc:.0f} Hz", (b0, 2.0 * b0, b0, -a1, -a2)))
    return out


@functools.lru_cache(None)
def bq_exact_voices():
    return _bq_voices(True)


@functools.lru_cache(None)
def bq_real_voices():
    return _bq_voices(False)


def bq_cases(lpv, voices):
    """xf [cases, 64 / lpv, 256], par [cases, 64 / lpv, 11], the voice index of every lane-channel [cases, 64 / lpv]."""
    g = 64 // lpv
    if g == 2:   # pair a voice with one of another length
        order = list(range(len(voices)))
        idx = [(i, order[(i + len(order) // 2 + 3) % len(order)]) for i in order[::2]] + [(i, order[(i + 7) % len(order)]) for i in order[1::2]]
    else:
        idx = [(i,) for i in range(len(voices))]
    xf = np.array([[voices[i][4] for i in t] for t in idx], dtype=f32)
    par = np.array([[(voices[i][1], voices[i][2]) + voices[i][3] + tuple(voices[i][5]) for i in t] for t in idx], dtype=f64)
    return xf, par, np.array(idx)


def _wet_mix(y32, x32, wm):
    """o = (float)y, then fmaf(o, wm, x * (1 - wm)) where wm < 1: fp32 operations, each rounded once (in rationals)."""
    if wm >= 1.0:
        return y32
    dry = round_frac(Fr(x32) * Fr(float(f32(1.0) - f32(wm))), 24)
    return round_frac(Fr(y32) * Fr(wm) + Fr(dry), 24)


def bq_exact_ref(voice):
    """The exact recurrence (Fractions): outputs after the wet mix (floats holding fp32 values), the f64 values y before it (Fractions),
    and ns = x1, x2, y1, y2 after the block (Fractions)."""
    _, frames, wm, c, x, st = voice
    b0, b1, b2, a1, a2 = (Fr(v) for v in c)
    x1, x2, y1, y2 = (Fr(float(v)) for v in st)
    ys, o = [], []
    for f in range(frames):
        xv = Fr(float(x[f]))
        y = b0 * xv + b1 * x1 + b2 * x2 - a1 * y1 - a2 * y2
        x2, x1, y2, y1 = x1, xv, y1, y
        ys.append(y)
        o.append(_wet_mix(round_frac(y, 24), float(x[f]), wm))
    return o, ys, [x1, x2, y1, y2]


def bq_serial(voice):
    """S: biquad_step in f64, left to right.  -> y [frames], the state after the block."""
    _, frames, _, (b0, b1, b2, a1, a2), x, st = voice
    x1, x2, y1, y2 = (float(v) for v in st)
    ys = []
    for f in range(frames):
        xv = float(x[f])
        y = b0 * xv + b1 * x1 + b2 * x2 - a1 * y1 - a2 * y2
        x2, x1, y2, y1 = x1, xv, y1, y
        ys.append(y)
    return np.array(ys), [x1, x2, y1, y2]


def bq_model(lpv, voice):
    """T: bq_tp_wave<256 / lpv, lpv> of one lane-channel in numpy float64, its bracketing and no contraction: the maps of the lanes'
    frames (bq_affine_push), the shuffle scan (d = 1, 2, 4, ...: lanes at or above d compose with lane - d), pass B from the scanned
    start values.  -> y [frames] (f64, before the conversion), the state after the block."""
    _, frames, _, (b0, b1, b2, a1, a2), x, st = voice
    ch = 256 // lpv
    sx1, sx2, sy1, sy2 = (float(v) for v in st)
    n0 = np.arange(lpv) * ch
    cnt = np.clip(frames - n0, 0, ch)
    xf = np.where(np.arange(ch)[None, :] < cnt[:, None], x.astype(f64).reshape(lpv, ch), 0.0)
    px1 = np.concatenate([[sx1], xf[:-1, ch - 1]])
    px2 = np.concatenate([[sx2], xf[:-1, ch - 2]])
    m00, m01, m10, m11, z0, z1 = np.ones(lpv), np.zeros(lpv), np.zeros(lpv), np.ones(lpv), np.zeros(lpv), np.zeros(lpv)
    w = np.empty((lpv, ch))
    x1, x2 = px1.copy(), px2.copy()
    for j in range(ch):
        xv = xf[:, j]
        w[:, j] = b0 * xv + b1 * x1 + b2 * x2
        on = j < cnt
        n00, n01, nz0 = -a1 * m00 - a2 * m10, -a1 * m01 - a2 * m11, (w[:, j] - a1 * z0) - a2 * z1
        m10, m11, z1 = np.where(on, m00, m10), np.where(on, m01, m11), np.where(on, z0, z1)
        m00, m01, z0 = np.where(on, n00, m00), np.where(on, n01, m01), np.where(on, nz0, z0)
        x2, x1 = x1, xv
    d = 1
    while d < lpv:
        def sh(a):
            return np.concatenate([np.zeros(d), a[:-d]])
        e00, e01, e10, e11, ez0, ez1 = sh(m00), sh(m01), sh(m10), sh(m11), sh(z0), sh(z1)
        on = np.arange(lpv) >= d
        r00, r01 = m00 * e00 + m01 * e10, m00 * e01 + m01 * e11
        r10, r11 = m10 * e00 + m11 * e10, m10 * e01 + m11 * e11
        rz0, rz1 = m00 * ez0 + m01 * ez1 + z0, m10 * ez0 + m11 * ez1 + z1
        m00, m01, m10, m11, z0, z1 = (np.where(on, a, b) for a, b in ((r00, m00), (r01, m01), (r10, m10), (r11, m11), (rz0, z0), (rz1, z1)))
        d <<= 1
    e1, e2 = m00 * sy1 + m01 * sy2 + z0, m10 * sy1 + m11 * sy2 + z1
    y1, y2 = np.concatenate([[sy1], e1[:-1]]), np.concatenate([[sy2], e2[:-1]])
    ys = np.zeros((lpv, ch))
    for j in range(ch):
        y = w[:, j] - a1 * y1 - a2 * y2
        on = j < cnt
        y2, y1 = np.where(on, y1, y2), np.where(on, y, y1)
        ys[:, j] = y
    end = (frames - 1) // ch
    c = int(cnt[end])
    ns = [xf[end, c - 1], xf[end, c - 2] if c >= 2 else px1[end], y1[end], y2[end]]
    return ys.reshape(-1)[:frames], [float(v) for v in ns]


# ================================================================== tp_noise_ticks
@functools.lru_cache(None)
def noise_starts():
    """(x1, x2) [cases, 2]: osc_reset's state and what every further 64 ticks leave of it (dsp_primitive_cases.noise_exact), then random."""
    rows = K.noise_exact()
    chain = [rows[k, 1:3] for k in range(0, K.NOISE_TICKS - 63, 64)]
    r = _rng(9)
    rnd = r.integers(0, 1 << 32, (40, 2), dtype=u64).astype(u32)
    edge = np.array([[0, 0], [0xFFFFFFFF, 0xFFFFFFFF], [0x80000000, 0x7FFFFFFF], [1, 0xFFFFFFFF]], dtype=u32)
    return np.concatenate([np.array(chain, dtype=u32), edge, rnd]), len(chain)


def noise_exact(starts):
    """Lane I: x2 before tick I's add, as int32; the state after 64 ticks."""
    vals = np.empty((len(starts), 64), dtype=i32)
    end = np.empty((len(starts), 2), dtype=u32)
    for c, (x1, x2) in enumerate(np.asarray(starts).tolist()):
        for i in range(64):
            x1 ^= x2
            vals[c, i] = x2 - (1 << 32) if x2 >= (1 << 31) else x2
            x2 = (x2 + x1) & 0xFFFFFFFF
        end[c] = (x1, x2)
    return vals, end


# ================================================================== the wave sums and wave_min_u32
@functools.lru_cache(None)
def sum_integer_inputs():
    """Integer-valued floats below 2^15 in magnitude: every order of summation is exact (64 x 2^15 < 2^24)."""
    r = _rng(10)
    cases = [np.where(np.arange(64) == k, 1.0 + 3 * k, 0.0) for k in range(64)]
    cases += [r.integers(-(1 << 15) + 1, 1 << 15, 64).astype(f64) for _ in range(12)]
    cases += [np.full(64, float((1 << 15) - 1)), np.full(64, -float((1 << 15) - 1)), np.zeros(64)]
    return np.array(cases, dtype=f32)


@functools.lru_cache(None)
def sum_random_inputs():
    r = _rng(11)
    scale = np.exp2(r.integers(-20, 20, (32, 1)).astype(f64))
    return (r.standard_normal((32, 64)) * scale).astype(f32)


@functools.lru_cache(None)
def min_inputs():
    r = _rng(12)
    cases = []
    for k in range(64):   # the minimum at every lane: below 2^31 among values on both sides of it (a signed comparison would pick one at or above 2^31), or all at or above 2^31
        a = r.integers((1 << 31) + 1 if k & 1 else 1000, 1 << 32, 64, dtype=u64)
        a[k] = (1 << 31) if k & 1 else k * 7
        cases.append(a)
    ties = r.integers(5, 1 << 32, 64, dtype=u64); ties[[3, 17, 40, 63]] = 5
    cases += [ties, np.zeros(64, dtype=u64), np.full(64, 0xFFFFFFFF, dtype=u64)]
    one = np.full(64, 0xFFFFFFFF, dtype=u64); one[31] = 0xFFFFFFFE
    hi = r.integers(1 << 31, 1 << 32, 64, dtype=u64)
    zero = r.integers(0, 1 << 32, 64, dtype=u64); zero[48] = 0
    cases += [one, hi, zero]
    return np.array(cases).astype(u32)


# ================================================================== FusedAcc
FUSED_ROW_PAIRS, FUSED_FRAMES, FUSED_SENTINEL = 3, 16, -999.0
FUSED_PSIZE = FUSED_ROW_PAIRS * 2 * FUSED_FRAMES


@functools.lru_cache(None)
def fused_cases():
    """tile [cases, 8, 256, 2], par [cases, 4] = count, f0, prow, frames.  One nonzero (thread, frame slot) at each of the 2,048 positions
    (count 8); integer-valued random tiles at every count 1 .. 8, on either tile turn of a 16-frame and a 13-frame block, row pairs 0 - 2."""
    r = _rng(13)
    n_one = 8 * 256
    tile = np.zeros((n_one, 8, 256, 2), dtype=f32)
    pos = np.arange(n_one)
    tile[pos, pos // 256, pos % 256, 0] = 1.0 + pos % 7
    tile[pos, pos // 256, pos % 256, 1] = -2.0 - pos % 5
    par = [(8, 8 * (p & 1), (p >> 1) % 3, 16) for p in range(n_one)]
    rnd = []
    for count in range(1, 9):
        for f0, frames in ((0, 16), (8, 16), (8, 13), (0, count)):
            if f0 + count > frames:
                continue
            rnd.append(r.integers(-200, 201, (8, 256, 2)).astype(f32))
            par.append((count, f0, len(rnd) % 3, frames))
    return np.concatenate([tile, np.array(rnd, dtype=f32)]), np.array(par, dtype=u32)


def fused_exact():
    """partial [cases, FUSED_PSIZE] afterwards: the sentinel everywhere but rows f0 .. f0 + count - 1 of the case's row pair."""
    tile, par = fused_cases()
    out = np.full((len(tile), FUSED_PSIZE), FUSED_SENTINEL, dtype=f64)
    sums = tile.astype(f64).sum(axis=2)   # [cases, slot, ch]
    for c, (count, f0, prow, frames) in enumerate(par.tolist()):
        for k in range(count):
            for ch in range(2):
                out[c, (prow * 2 + ch) * frames + f0 + k] = sums[c, (f0 + k) & 7, ch]
    return out.astype(f32)


# ================================================================== tp_reduce_prev
REDUCE_ROWS = (1, 7, 8, 9, 63, 64, 65, 512, 513, 2048)
REDUCE_FRAMES = (1, 3, 64, 255, 256)
REDUCE_GRIDS = (1, 2, 3, 8, 64, 129, 512)   # and 2 frames + 1: more workgroups than columns
REDUCE_GUARD, REDUCE_SENTINEL, REDUCE_PREFILL = 16, float(1 << 20), 3.0


def reduce_cp(frames, grid):
    """The columns per pass tp_reduce_prev picks, and whether some workgroup of the grid has no column."""
    cols = 2 * frames
    per = -(-cols // grid)
    return (1 if per <= 1 else 2 if per <= 2 else 4 if per <= 4 else 8), per * (grid - 1) >= cols


@functools.lru_cache(None)
def reduce_cases():
    """rows (flat), desc [workgroups, 8], combos = (n_rows, frames, grid, accumulate, rows offset, bus offset), bus size."""
    r = _rng(14)
    rows, roff, off = [], {}, 0
    for n_rows in REDUCE_ROWS:
        for frames in REDUCE_FRAMES:
            a = r.integers(-8, 9, n_rows * 2 * frames).astype(f32)
            roff[(n_rows, frames)] = off
            rows.append(a); off += a.size
    combos, desc, boff = [], [], 0
    for n_rows in REDUCE_ROWS:
        for frames in REDUCE_FRAMES:
            for grid in REDUCE_GRIDS + (2 * frames + 1,):
                for acc in (0, 1):
                    combos.append((n_rows, frames, grid, acc, roff[(n_rows, frames)], boff))
                    desc += [(roff[(n_rows, frames)], boff, n_rows, frames, acc, wg, grid, 0) for wg in range(grid)]
                    boff += 2 * frames + REDUCE_GUARD
    return np.concatenate(rows), np.array(desc, dtype=u32), combos, boff


def reduce_prefill_and_exact():
    rows, _, combos, size = reduce_cases()
    pre = np.full(size, REDUCE_SENTINEL, dtype=f32)
    want = pre.astype(f64)
    for n_rows, frames, _, acc, ro, bo in combos:
        s = rows[ro:ro + n_rows * 2 * frames].astype(f64).reshape(n_rows, 2, frames).sum(axis=0)   # [ch, frame]
        if acc:
            pre[bo:bo + 2 * frames] = REDUCE_PREFILL
        want[bo:bo + 2 * frames] = s.T.reshape(-1) + (REDUCE_PREFILL if acc else 0.0)   # bus[frame][ch]
    return pre, want.astype(f32)
