"""The target laws of a control link onto a Welsh bank restated in Python (groove_amd/csrc/ctl_core.h ctl_bank_*_f64 and pan_gains;
groove_hip.hip groove_bank_set_param; docs/DSP_SPEC.md section 13), and the trip, sources and shapes the GPU tests of those links run —
shared by tests/test_ctl_bank_law_cpu.py, which holds the C++ text to this one bit for bit, and tests/test_gpu_ctl_bank_links.py.
Python floats are IEEE doubles and math.pow is the C library's: every figure here is the one the host path computes.  The trip's own
law is tests/ctl_trip_law.py's, re-exported."""
import math
import os

import numpy as np

from groove_amd import abi_types as T
from tests.ctl_trip_law import (BLOCK_UNITS, EXP, FLAT, LOG, MAIN_START, MAIN_STEPS, SLOPE, UNITS, scan, trip_value)  # noqa: F401

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVED = (LOG, EXP)
INDEX = {"gain": T.CTL_WELSH_DCA_GAIN, "pan": T.CTL_WELSH_DCA_PAN, "cutoff": T.CTL_WELSH_CUTOFF}


def clamp01(v):
    return 0.0 if v < 0.0 else (1.0 if v > 1.0 else v)


def gain_param(v):
    """groove_welsh_params::dca_gain after a control value v."""
    return np.float32(clamp01(v))


def pan_param(v):
    """dca_pan: ControlValue 0..1 -> BipolarNormal."""
    return np.float32(clamp01(v) * 2.0 - 1.0)


def cutoff_param(v):
    """filter_cutoff_hz = WelshParams::cutoff_hz: percent_to_frequency."""
    return np.float32(25.0 * math.pow(800.0, clamp01(v)))


def pan_gains(gain, pan):
    """(gl, gr) of float32 gain and pan (arrays or scalars): float64 expressions in pan_gains' order, rounded to float32."""
    g, p = np.asarray(gain, dtype=np.float32).astype(np.float64), np.asarray(pan, dtype=np.float32).astype(np.float64)
    gl = g * (1.0 - 0.25 * (p + 1.0) * (p + 1.0))
    gr = g * (1.0 - (0.5 * p - 0.5) * (0.5 * p - 0.5))
    return gl.astype(np.float32), gr.astype(np.float32)


def steps_for(param):
    """The main trip for `param`.  A cutoff takes its values rescaled into 0.1 .. 1.0 (49 Hz up): the range
    tests/test_gpu_random_inputs.py records as the one inside the fp32-coefficient bar under a sounding voice."""
    if param != "cutoff":
        return list(MAIN_STEPS)
    return [(kind, 0.1 + 0.9 * start, 0.1 + 0.9 * end, beats) for kind, start, end, beats in MAIN_STEPS]


# The blocks of the main shape: ragged lengths, and trip times of the test's own choosing (the trip is a function of the time it is
# given, whatever the block's length): two blocks before the trip, block 2 on its first begin (400), block 5 on the boundary between flat
# and slope (1,200), five blocks in the logarithmic step, five in the exponential one — the first of them on the boundary between the
# two (4,080) — and two after the end (5,580).
MAIN_SIZES = [256, 256, 100, 37, 1, 256, 256, 100, 37, 1, 256, 256, 100, 37, 1, 256, 256, 100, 37, 1, 256, 256]
MAIN_ATS = [0, 200, 400, 700, 1000, 1200, 1500, 1800, 2100, 2400, 2600, 2900, 3200, 3500, 3800, 4080, 4400, 4700, 5000, 5300, 5600, 5900]
NOTE_ON_BLOCKS, NOTE_OFF_BLOCK = (0, 15), 9


def main_ats():
    return list(MAIN_ATS)


def lfo_source(frequency_hz=5.3, waveform=T.WAVE_SINE):
    return T.ctl_sources(1, source=T.CTL_SRC_LFO, waveform=waveform, frequency_hz=frequency_hz)
