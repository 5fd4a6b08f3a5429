"""The effect kernel forms (groove_hip.hip fx_form_of, reported by groove_fx_kernel_form) and the cases that reach each of them, on
both sides of every switch that picks one.  A plain table: tests/test_fx_form_coverage.py (CPU) checks that it covers every form and
every threshold, tests/test_gpu_fx_forms.py plays it and asserts, before every block, that the library takes the form written here.

A form is named by a TAG, a substring of exactly one of the library's strings (the strings themselves live in the library only:
groove_fx_kernel_form_name lists them)."""
import math
from collections import namedtuple

import numpy as np

from groove_amd import abi_types as T

IDENT = "identity"
RUN = "a stage of the fused run"
DIR_AP = "direct all-pass on the all-pass stream"
DIR = "direct all-pass behind it"
CHK = "chunked all-pass"
SEQ = "sequential all-pass"
BQ_TP = "fx_biquad_tp_kernel"
BQ_SEG = "fx_biquad_seg_kernel"
BQ_SER = "fx_biquad_kernel<16>"
LP_TP = "fx_lp24_tp_kernel"
LP_SER = "fx_lp24_kernel<16>"
D16 = "fx_delay_kernel<16>"
D1 = "fx_delay_kernel<1>"
C16 = "fx_chorus_kernel<16>"
C1 = "fx_chorus_kernel<1>"
R8 = "fx_reverb_kernel<8>"
R1 = "fx_reverb_kernel<1>"
TAGS = [IDENT, RUN, DIR_AP, DIR, CHK, SEQ, BQ_TP, BQ_SEG, BQ_SER, LP_TP, LP_SER, D16, D1, C16, C1, R8, R1]

# Forms and switch sides no case reaches at an audio sample rate, and why (nothing is built for them).
UNREACHABLE_REASONS = {
    R1: "the serial reverb kernel takes chunk 1 only when a line is under 8 frames: the 1.7 ms all-pass at a sample rate below 4.7 kHz",
    "reverb all-pass line under 32 frames": "the fused run is refused to an all-wet reverb whose 1.7 ms all-pass is under 32 frames: a sample rate "
                                            "below 18.6 kHz, and below 4.7 kHz before the serial kernel that then runs differs from the partly-wet one's",
}

SR = 44100.0


# ---- the line lengths, as the library derives them (csrc/derive.h) ----
def delay_frames(seconds, sr=SR):
    """delay_frames_h: the parameter is an fp32 field, the product and the rounding are f64."""
    n = math.floor(float(np.float32(seconds)) * sr + 0.5)
    return int(n) if n >= 1.0 else 1


COMB_SECONDS = (0.0297, 0.0371, 0.0411, 0.0437)   # kCombDelaysH / kAllpassDelaysH: f64 constants, not parameters
ALLPASS_SECONDS = (0.005, 0.0017)


def _const_frames(seconds, sr):
    return max(1, int(math.floor(seconds * sr + 0.5)))


def comb_frames(sr=SR):
    return [_const_frames(s, sr) for s in COMB_SECONDS]


def allpass_frames(sr=SR):
    return [_const_frames(s, sr) for s in ALLPASS_SECONDS]


def chorus_geometry(seconds, voices, sr=SR):
    """(N, spacing, nearest): the ring, the distance between taps, and how long ago the newest tap was pushed (fx_form_of's two limits)."""
    n = delay_frames(seconds, sr)
    spacing = n // voices
    return n, spacing, n - (voices - 1) * spacing


# ---- the cases ----
# knobs: "tp" False = time_parallel_max_voices 0 (restored afterwards); "ap" True = the all-pass stream on; "env" = a variable a
# context of its own is created under.  params: keyword arguments of abi_types.fx_params; a value that is a function takes the lane
# index.  walk / expect: block lengths in playing order and the form each takes.
Case = namedtuple("Case", "name kind params n knobs walk expect")

IIR_WALK = [256, 257, 16, 15, 1, 300, 255, 64, 512, 17, 253, 1024, 3]
IIR_BIG_WALK = [256, 100, 300, 15, 16]


def _short(form, serial, walk=IIR_WALK):          # a form of blocks of up to 256 frames, the serial kernel above
    return [form if f <= 256 else serial for f in walk]


def _seg(walk=IIR_WALK):                          # the four-segment kernel's window, 16 - 256 frames
    return [BQ_SEG if 16 <= f <= 256 else BQ_SER for f in walk]


def _third_partly_wet(i):
    return 0.6 if i % 3 == 0 else 1.0


def _log_lanes(lo, hi, period):                   # lo .. hi, geometrically, over `period` lanes and again
    return lambda i: lo * (hi / lo) ** ((i % period) / (period - 1.0))


_LP12 = dict(cutoff_hz=_log_lanes(40.0, 6000.0, 97), q=_log_lanes(0.5, 20.0, 61), wet=_third_partly_wet)
_PEAK = dict(cutoff_hz=_log_lanes(40.0, 6000.0, 97), q=_log_lanes(0.5, 20.0, 61), db_gain=lambda i: -12.0 + 24.0 * ((i * 7) % 50) / 49.0 + 0.3, wet=_third_partly_wet)
_LP24 = dict(cutoff_hz=_log_lanes(40.0, 6000.0, 97), passband_ripple=_log_lanes(0.71, 3.0, 53), wet=_third_partly_wet)


def _iir_cases():
    out = []
    for name, kind, params, tp, ser in (("lp12", T.FX_BIQUAD_LP12, _LP12, BQ_TP, BQ_SER), ("peak12", T.FX_BIQUAD_PEAK12, _PEAK, BQ_TP, BQ_SER),
                                        ("lp24", T.FX_BIQUAD_LP24, _LP24, LP_TP, LP_SER)):
        for n in (3, 130):
            out.append(Case(f"{name}-n{n}", kind, params, n, {}, IIR_WALK, _short(tp, ser)))
            out.append(Case(f"{name}-n{n}-tp0", kind, params, n, {"tp": False}, IIR_WALK, _seg() if ser == BQ_SER else [LP_SER] * len(IIR_WALK)))
    out += [Case("lp12-n2048", T.FX_BIQUAD_LP12, _LP12, 2048, {}, IIR_WALK, _short(BQ_TP, BQ_SER)),
            Case("lp12-n2049", T.FX_BIQUAD_LP12, _LP12, 2049, {}, IIR_WALK, _seg()),
            Case("peak12-n2048", T.FX_BIQUAD_PEAK12, _PEAK, 2048, {}, IIR_WALK, _short(BQ_TP, BQ_SER)),
            Case("peak12-n2049", T.FX_BIQUAD_PEAK12, _PEAK, 2049, {}, IIR_WALK, _seg()),
            Case("lp24-n1024", T.FX_BIQUAD_LP24, _LP24, 1024, {}, IIR_WALK, _short(LP_TP, LP_SER)),
            Case("lp24-n1025", T.FX_BIQUAD_LP24, _LP24, 1025, {}, IIR_WALK, [LP_SER] * len(IIR_WALK)),
            Case("lp12-n24576", T.FX_BIQUAD_LP12, _LP12, 24576, {}, IIR_BIG_WALK, _seg(IIR_BIG_WALK)),
            Case("lp12-n24577", T.FX_BIQUAD_LP12, _LP12, 24577, {}, IIR_BIG_WALK, [BQ_SER] * len(IIR_BIG_WALK))]
    return out


def _delay_cases(sr=SR):
    out = []
    for n in (6, 64):
        for seconds in (0.004, 0.012):
            N = delay_frames(seconds, sr)
            walk = [N - 1, N, N + 1, 256, 2 * N + 3, 1, 1024]
            out.append(Case(f"delay-{seconds}-n{n}", T.FX_DELAY, dict(delay_seconds=seconds, wet=_third_partly_wet), n, {}, walk,
                            [RUN, RUN, D16, RUN if N >= 256 else D16, D16, RUN, D16]))
        out.append(Case(f"delay-0.0002-n{n}", T.FX_DELAY, dict(delay_seconds=0.0002, wet=_third_partly_wet), n, {}, [256, 1, 1024, 37], [D1, RUN, D1, D1]))
    return out


def _chorus_cases(sr=SR):
    out = []
    for n in (6, 64):
        N, spacing, nearest = chorus_geometry(0.03, 3, sr)
        walk = [spacing - 1, spacing, spacing + 1, 256, nearest - 1, nearest, nearest + 1, 2048, 1]
        out.append(Case(f"chorus-3x0.03-n{n}", T.FX_CHORUS, dict(voices=3, delay_seconds=0.03, wet=_third_partly_wet), n, {}, walk,
                        [RUN, RUN, C16, RUN] + [RUN if f <= spacing else C16 for f in walk[4:7]] + [C16, RUN]))
        # one voice: the spacing limit does not apply and the nearest tap (= N) binds alone; with more voices it never does (nearest >= spacing)
        N1 = delay_frames(0.004, sr)
        out.append(Case(f"chorus-1x0.004-n{n}", T.FX_CHORUS, dict(voices=1, delay_seconds=0.004, wet=_third_partly_wet), n, {},
                        [N1 - 1, N1, N1 + 1, 256, 1], [RUN, RUN, C16, RUN if N1 >= 256 else C16, RUN]))
        out.append(Case(f"chorus-4x0.0005-n{n}", T.FX_CHORUS, dict(voices=4, delay_seconds=0.0005, wet=_third_partly_wet), n, {}, [256, 1, 1024], [C1, RUN, C1]))
    return out


def reverb_walk(sr=SR):
    nap, ncomb = min(allpass_frames(sr)), min(comb_frames(sr))
    return [256, 8 * nap, 8 * nap + 1, ncomb, ncomb + 1, 100, 2048, 1, nap, ncomb + 2, 256]


def _reverb_cases(sr=SR):
    walk = reverb_walk(sr)
    wet = [DIR, DIR, CHK, CHK, R8, DIR, R8, DIR, DIR, R8, DIR]
    out = []
    for n in (1, 12, 72):
        p = dict(attenuation=0.9, reverb_seconds=0.8)
        out.append(Case(f"reverb-n{n}", T.FX_REVERB, p, n, {}, walk, wet))
        out.append(Case(f"reverb-n{n}-ap", T.FX_REVERB, p, n, {"ap": True}, walk, [DIR_AP if f == DIR else f for f in wet]))
        out.append(Case(f"reverb-n{n}-one-lane-half-wet", T.FX_REVERB, dict(p, wet=lambda i: 0.5 if i == 0 else 1.0), n, {}, walk, [R8] * len(walk)))
    out.append(Case("reverb-n12-sequential", T.FX_REVERB, dict(attenuation=0.9, reverb_seconds=0.8), 12, {"env": "GROOVE_FX_SEQ_ALLPASS"}, walk,
                    [SEQ if f in (DIR, CHK) else f for f in wet]))
    return out


def _other_cases():
    return [Case("mixer-n6", T.FX_MIXER, {}, 6, {}, [256, 1, 1024], [IDENT] * 3),
            Case("gain-n6", T.FX_GAIN, dict(ceiling=lambda i: 0.5 + 0.05 * i), 6, {}, [256, 1, 1024], [RUN] * 3)]


CASES = _iir_cases() + _delay_cases() + _chorus_cases() + _reverb_cases() + _other_cases()


def fx_params(case):
    arr = (T.FxParams * case.n)()
    for i in range(case.n):
        arr[i] = T.fx_params(**{k: (v(i) if callable(v) else v) for k, v in case.params.items()})
    return arr


# ---- the switches: which side of each a (case, block length, form) sits on ----
_BIQUADS = (T.FX_BIQUAD_LP12, T.FX_BIQUAD_PEAK12)


def _tp(c):
    return c.knobs.get("tp", True)


def _side(below):
    return "below" if below else "above"


def _delay_n(c):
    return delay_frames(c.params["delay_seconds"])


def _chorus_g(c):
    return chorus_geometry(c.params["delay_seconds"], c.params["voices"])


def _all_wet(c):
    return "wet" not in c.params


# name -> f(case, frames, form) -> "below" | "above" | None.  Every switch of fx_form_of, and the two branch switches inside the
# kernels it picks (the four-segment kernel's straight-line code, the serial biquad's whole chunks).
THRESHOLDS = {
    "biquad block length 15 | 16 (serial | four-segment)":
        lambda c, f, form: _side(f == 15) if c.kind in _BIQUADS and not _tp(c) and f in (15, 16) else None,
    "biquad block length 256 | 257, time-parallel | serial":
        lambda c, f, form: _side(f == 256) if c.kind in _BIQUADS and _tp(c) and c.n <= 2048 and f in (256, 257) else None,
    "biquad block length 256 | 257, four-segment | serial":
        lambda c, f, form: _side(f == 256) if c.kind in _BIQUADS and not _tp(c) and f in (256, 257) else None,
    "lp24 block length 256 | 257 (time-parallel | serial)":
        lambda c, f, form: _side(f == 256) if c.kind == T.FX_BIQUAD_LP24 and _tp(c) and c.n <= 1024 and f in (256, 257) else None,
    "time-parallel knob on | off":
        lambda c, f, form: _side(_tp(c)) if c.kind in _BIQUADS + (T.FX_BIQUAD_LP24,) and c.n in (3, 130) and f <= 256 else None,
    "four-segment kernel: a predicated last segment (253 - 255) | four whole segments (256)":
        lambda c, f, form: _side(f < 256) if form == BQ_SEG and 253 <= f <= 256 else None,
    "serial biquad: tail chunk only (under 16 frames) | whole chunks":
        lambda c, f, form: _side(f < 16) if form == BQ_SER else None,
    "serial biquad: no tail (a multiple of 16) | whole chunks and a tail":
        lambda c, f, form: _side(f % 16 == 0) if form == BQ_SER and f >= 16 else None,
    "biquad lanes 2,048 | 2,049 (time-parallel | four-segment)":
        lambda c, f, form: _side(c.n == 2048) if c.kind in _BIQUADS and c.n in (2048, 2049) and 16 <= f <= 256 else None,
    "lp24 lanes 1,024 | 1,025 (time-parallel | serial)":
        lambda c, f, form: _side(c.n == 1024) if c.kind == T.FX_BIQUAD_LP24 and c.n in (1024, 1025) and f <= 256 else None,
    "biquad lanes 24,576 | 24,577 (four-segment | serial)":
        lambda c, f, form: _side(c.n == 24576) if c.kind in _BIQUADS and c.n in (24576, 24577) and 16 <= f <= 256 else None,
    "delay line N | N + 1 frames in the block (fused run | serial)":
        lambda c, f, form: _side(f == _delay_n(c)) if c.kind == T.FX_DELAY and f in (_delay_n(c), _delay_n(c) + 1) else None,
    "delay line under 16 | at least 16 frames (chunk 1 | 16)":
        lambda c, f, form: _side(_delay_n(c) < 16) if c.kind == T.FX_DELAY and form in (D1, D16) else None,
    "chorus of several voices: spacing | spacing + 1 frames in the block (fused run | serial)":
        lambda c, f, form: _side(f == _chorus_g(c)[1]) if c.kind == T.FX_CHORUS and c.params["voices"] > 1 and f in (_chorus_g(c)[1], _chorus_g(c)[1] + 1) else None,
    "chorus of one voice: nearest tap | nearest + 1 frames in the block (fused run | serial; with more voices the spacing limit is never the looser one)":
        lambda c, f, form: _side(f == _chorus_g(c)[2]) if c.kind == T.FX_CHORUS and c.params["voices"] == 1 and f in (_chorus_g(c)[2], _chorus_g(c)[2] + 1) else None,
    "chorus spacing under 16 | at least 16 frames (chunk 1 | 16)":
        lambda c, f, form: _side(_chorus_g(c)[1] < 16) if c.kind == T.FX_CHORUS and form in (C1, C16) else None,
    "all-wet reverb: shortest comb | one frame more (fused run | serial)":
        lambda c, f, form: _side(f == min(comb_frames())) if c.kind == T.FX_REVERB and _all_wet(c) and f in (min(comb_frames()), min(comb_frames()) + 1) else None,
    "all-wet reverb: 8 x the shorter all-pass | one frame more (direct | chunked)":
        lambda c, f, form: _side(f == 8 * min(allpass_frames())) if c.kind == T.FX_REVERB and _all_wet(c) and not c.knobs.get("env")
        and f in (8 * min(allpass_frames()), 8 * min(allpass_frames()) + 1) else None,
    "reverb partly wet | all wet (serial | fused run)":
        lambda c, f, form: _side(not _all_wet(c)) if c.kind == T.FX_REVERB and f <= min(comb_frames()) else None,
    "all-pass stream off | on":
        lambda c, f, form: _side(form == DIR) if form in (DIR, DIR_AP) else None,
    "fused run: scalar | 16-byte accesses (lanes no multiple | a multiple of 4)":
        lambda c, f, form: _side(c.n % 4 != 0) if form in (RUN, DIR, DIR_AP, CHK) else None,
}


def library_forms():
    """Every string groove_fx_kernel_form can return, from the library's own table (no device needed)."""
    import ctypes as C
    import os
    from groove_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    so = C.CDLL(lib.LIB_PATH)
    so.groove_fx_kernel_form_name.restype = C.c_char_p
    so.groove_fx_kernel_form_name.argtypes = [C.c_uint32]
    out = []
    while (s := so.groove_fx_kernel_form_name(len(out))) is not None:
        out.append(s.decode())
    return out


def form_of_tag(tag, forms):
    """The one library string a tag names."""
    hits = [f for f in forms if tag in f]
    assert len(hits) == 1, (tag, hits)
    return hits[0]
