"""ctypes binding of tests/probe (dsp_probe.hip built twice: libdsp_probe.so, the DEVICE side of every branch of csrc/dsp_core.h, one
element-wise kernel per primitive; libdsp_probe_host.so, the same functors looped by g++ with the emulation tier's flags).  Test
infrastructure only.

    device("fast_rcp", x)   host("fast_rcp", x)        x: numpy arrays, one per input, converted to the entry's types

Both return a fresh numpy array of the entry's output type, [n] or [n, words per lane]."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
STEPS = 64  # consecutive filter steps per lane of the lp24_step probes

f32, f64, u32, u64, i32, i64 = np.float32, np.float64, np.uint32, np.uint64, np.int32, np.int64

# name: (input dtypes, words per lane of each input, output dtype, output words per lane)
ENTRIES = {
    "fast_exp2": ((f32,), (1,), f32, 1),
    "fast_rcp": ((f32,), (1,), f32, 1),
    "f64_to_u64": ((f64,), (1,), u64, 1),
    "fract_f64": ((f64,), (1,), f64, 1),
    "turns_to_inc": ((f64,), (1,), u64, 1),
    "turns_to_phase": ((f64,), (1,), u64, 1),
    "fold_quarter": ((i32,), (1,), i32, 1),
    "fold_quarter64": ((i64,), (1,), i64, 1),
    "env_frames": ((f32,), (1,), u32, 1),
    "sin_turns_folded": ((f32,), (1,), f32, 1),
    "sin_turns_folded_f64": ((f64,), (1,), f64, 1),
    "exp2_small_f64": ((f64,), (1,), f64, 1),
    "exp_tiny_f64": ((f64,), (1,), f64, 1),
    "tan_of_reduced": ((f32,), (1,), f32, 1),
    "tan_reduced": ((f32,), (1,), f32, 2),                     # t, hi (1.0 / 0.0)
    "noise_tick": ((u32,), (1,), u32, 3),                      # ticks from osc_reset -> the last value's bits, x1, x2
    "med3f": ((f32, f32, f32), (1, 1, 1), f32, 1),             # x, lo, hi
    "osc_value": ((u32, u64, u64), (1, 1, 1), f32, 1),         # waveform, phase, duty64
    "osc_value_f64": ((u32, u64, u64), (1, 1, 1), f64, 1),
    "welsh_env_cutoff_pct": ((f32, f32, f32), (1, 1, 1), f32, 1),   # cutoff_start, cutoff_end, envelope value
    "welsh_lfo_cutoff_pct": ((f32, f32, f32), (1, 1, 1), f32, 1),   # cutoff_start, lfo_depth, lfo value
    "env_shape": ((f32, f32, f32, f32), (1, 1, 1, 1), f32, 1),      # frame counter, A, D, 1 / len
    "bitcrush": ((f32, u32), (1, 1), f32, 1),
    "sample_interp_nearest": ((f32, f32), (4, 1), f32, 1),     # 4 taps a lane (the mode reads its first N), t
    "sample_interp_linear": ((f32, f32), (4, 1), f32, 1),
    "sample_interp_cubic": ((f32, f32), (4, 1), f32, 1),
    "lp24_step": ((f64, f64, f64), (6, 4, STEPS), f64, 5 * STEPS),          # coefficients, state, inputs -> (y, s0..s3) per step
    "lp24_step_f32": ((f32, f32, f32), (6, 4, STEPS), f32, 5 * STEPS),
    "lp24_step_scalar": ((f64, f64, f64), (0, 4, STEPS), f64, 5 * STEPS),   # ONE coefficient set (6 words) a call
    "lp24_step_f32_scalar": ((f32, f32, f32), (0, 4, STEPS), f32, 5 * STEPS),
    "lp24_coefd_from_fc": ((f64, f32, f32), (1, 1, 1), f64, 6),             # ripple, cutoff Hz, rate Hz -> b0, a1, a2 twice
    "lp24_coeff_from_fc": ((f64, f32, f32), (1, 1, 1), f32, 6),
    "lp24_coefd_from_pct": ((f64, f32, f32), (1, 1, 1), f64, 6),            # ripple, cutoff percent, rate Hz
}
HOST_ONLY = {"ref_lp24_coeffs_h": ((f64, f64, f64), (1, 1, 1), f64, 6)}   # derive.h lp24_coeffs_h: ripple, cutoff Hz, rate Hz, f64 throughout

_LIBS = {}


def build():
    subprocess.run(["make", "-s", "-C", HERE], check=True)


def _lib(host):
    if host not in _LIBS:
        path = os.path.join(HERE, "libdsp_probe_host.so" if host else "libdsp_probe.so")
        if not os.path.exists(path):
            build()
        _LIBS[host] = C.CDLL(path)
    return _LIBS[host]


def _call(symbol, spec, host, arrays):
    in_types, in_words, out_type, out_words = spec
    assert len(arrays) == len(in_types), (symbol, len(arrays))
    ins = [np.ascontiguousarray(a, dtype=t).reshape(-1) for a, t in zip(arrays, in_types)]
    per_lane = [(a.size, w) for a, w in zip(ins, in_words) if w]
    n = per_lane[0][0] // per_lane[0][1]
    for a, w in zip(ins, in_words):
        assert a.size == (n * w if w else 6), (symbol, a.size, n, w)
    out = np.empty(n * out_words, dtype=out_type)
    fn = getattr(_lib(host), symbol)
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p] * (len(ins) + 1) + [C.c_size_t]
    err = fn(*[a.ctypes.data for a in ins], out.ctypes.data, n)
    if err != 0:
        raise RuntimeError(f"{symbol}: error code {err}")   # a missing kernel or a failed launch is an error, never a fall-back
    return out if out_words == 1 else out.reshape(n, out_words)


def device(name, *arrays):
    """The device side: one kernel launch on the current GPU."""
    return _call("probe_" + name, ENTRIES[name], False, arrays)


def host(name, *arrays):
    """The host side: the #else branches, as the emulation tier compiles them."""
    spec = HOST_ONLY.get(name) or ENTRIES[name]
    return _call("probe_host_" + name if name in ENTRIES else "probe_" + name, spec, True, arrays)
