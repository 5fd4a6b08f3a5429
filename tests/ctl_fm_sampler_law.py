"""The target laws of a control link onto an FM or a sampler bank restated in Python (groove_amd/csrc/ctl_core.h ctl_fm_*_f64,
ctl_sampler_gain_f64, fm_depth_beta, pan_gains; groove_hip.hip groove_bank_set_param; docs/DSP_SPEC.md section 13) — shared by
tests/test_ctl_fm_sampler_law_cpu.py, which holds the C++ text to this one bit for bit, and tests/test_gpu_ctl_fm_sampler_links.py.
Python floats are IEEE doubles: every figure here is the one the host path computes.  Gain and pan are the Welsh laws
(tests/ctl_bank_law.py), re-exported; the trip's own law is tests/ctl_trip_law.py's."""
import numpy as np

from groove_amd import abi_types as T
from tests.ctl_bank_law import CURVED, REPO, clamp01, gain_param, pan_gains, pan_param  # noqa: F401
from tests.ctl_trip_law import EXP, FLAT, LOG, SLOPE, scan, trip_value  # noqa: F401

FM_INDEX = {"gain": T.CTL_FM_DCA_GAIN, "pan": T.CTL_FM_DCA_PAN, "depth": T.CTL_FM_DEPTH, "beta": T.CTL_FM_BETA}
SAMPLER_INDEX = {"gain": T.CTL_SAMPLER_GAIN}


def depth_param(v):
    """groove_fm_params::depth after a control value v: a Normal."""
    return np.float32(clamp01(v))


def beta_param(v):
    """groove_fm_params::beta: set_beta(value.into()) on the ControlValue as it is."""
    return np.float32(clamp01(v))


def sampler_gain_param(v):
    """groove_sampler_params::gain."""
    return np.float32(clamp01(v))


def fm_param(name, v):
    return {"gain": gain_param, "pan": pan_param, "depth": depth_param, "beta": beta_param}[name](v)


def depth_beta(depth, beta):
    """FmParams::depth_beta of float32 depth and beta: the product of the two widened (exact in float64: 24 x 24 bits)."""
    return np.asarray(depth, dtype=np.float32).astype(np.float64) * np.asarray(beta, dtype=np.float32).astype(np.float64)
