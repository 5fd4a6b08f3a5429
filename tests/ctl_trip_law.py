"""The control trip's law restated in Python (groove_amd/host/groove_host.cpp ControlTrip::work / value_at; docs/DSP_SPEC.md section 13,
trip source), and the trip the GPU tests run — shared by tests/test_ctl_trip_cpu.py, which holds csrc/ctl_core.h to this text bit for
bit, and the GPU tests, which take their expected parameters from it.  Python floats are IEEE doubles and math.log10 / math.pow are
the C library's, so every figure here is the one the host trip computes."""
import math

import numpy as np

from groove_amd import abi_types as T

UNITS = T.CTL_UNITS_PER_BEAT
THRESHOLD = math.pow(10.0, -12.0 / 5.0)
FLAT, SLOPE, LOG, EXP = T.CTL_STEP_FLAT, T.CTL_STEP_SLOPE, T.CTL_STEP_LOGARITHMIC, T.CTL_STEP_EXPONENTIAL


def value_at(kind, start, end, t):
    """ControlTrip::value_at."""
    t = 0.0 if t < 0.0 else (1.0 if t > 1.0 else t)
    if kind == SLOPE:
        return start + (end - start) * t
    if kind == LOG:
        c = 0.0 if t < THRESHOLD else 1.0 + (5.0 / 12.0) * math.log10(t)
        return start + (end - start) * c
    if kind == EXP:
        c = 1.0 if t > 1.0 - THRESHOLD else -(5.0 / 12.0) * math.log10(1.0 - t)
        return start + (end - start) * c
    return start


def begins(start_beat, steps):
    b, out = start_beat, [start_beat]
    for _, _, _, beats in steps:
        b += beats
        out.append(b)
    return out


def scan(start_beat, steps, at_units):
    """ControlTrip::work's first-match scan: (step index, its begin), or (-1, None) where no step holds at_units."""
    now = at_units / float(UNITS)
    b = start_beat
    for i, (_, _, _, beats) in enumerate(steps):
        if now >= b and now < b + beats:
            return i, b
        b += beats
    return -1, None


def trip_value(start_beat, steps, at_units):
    """The value ControlTrip::work hands to the target for the block that starts at at_units, or None outside the steps."""
    i, b = scan(start_beat, steps, at_units)
    if i < 0:
        return None
    kind, start, end, beats = steps[i]
    return value_at(kind, start, end, (at_units / float(UNITS) - b) / beats)


def param_of(index, value):
    """What groove_fx_set_param makes of a value: (groove_fx_params field, the number it stores)."""
    v = 0.0 if value < 0.0 else (1.0 if value > 1.0 else value)
    if index == T.CTL_FX_BITS:
        return "bits", min(int(v * 16.0), 31)
    if index == T.CTL_FX_CUTOFF:
        return "cutoff_hz", float(np.float32(25.0 * math.pow(800.0, v)))
    if index in (T.CTL_FX_Q, T.CTL_FX_PASSBAND_RIPPLE):
        return ("q" if index == T.CTL_FX_Q else "passband_ripple"), float(np.float32(v * v * 10.0 + 0.707))
    return {T.CTL_FX_CEILING: "ceiling", T.CTL_FX_ATTENUATION: "attenuation", T.CTL_FX_THRESHOLD: "limit_min"}[index], float(np.float32(v))


# The trip of the GPU comparison: flat, slope, logarithmic, exponential.  Blocks start every 200 units (64 frames at 128 bpm and
# 44,100 Hz are 202.9); the trip starts at 400 units, so blocks 0 and 1 lie before it and block 2 exactly on its first begin; the flat
# step is 800 units long, so block 6 lies exactly on the boundary between flat and slope; the other boundaries (2,450, 4,080 and the
# end, 5,580) fall between block starts; blocks 28 and 29 lie after the end.
BLOCK_UNITS = 200
MAIN_START = 400.0 / UNITS
MAIN_STEPS = [(FLAT, 0.35, 0.35, 800.0 / UNITS), (SLOPE, 0.2, 0.8, 1250.0 / UNITS), (LOG, 0.8, 0.15, 1630.0 / UNITS), (EXP, 0.15, 0.9, 1500.0 / UNITS)]
MAIN_BLOCKS = 30


def main_block_steps():
    """Per block of the comparison: the index of the step that holds its start, or -1."""
    return [scan(MAIN_START, MAIN_STEPS, k * BLOCK_UNITS)[0] for k in range(MAIN_BLOCKS)]
