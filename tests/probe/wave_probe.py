"""ctypes binding of tests/probe/libwave_probe.so (wave_probe.hip): the cross-lane routines of csrc/welsh_tp.h and csrc/kernels.h, one
kernel per primitive, ONE WORKGROUP PER CASE and many cases a launch.  Test infrastructure only.

Every device entry takes numpy arrays whose leading axis is the case and returns fresh arrays of what every lane held afterwards.
A missing symbol or a failed launch is an error, never a fall-back.  The host entries at the end (the workgroup-to-voice-group
mapping, the coefficient designs) run without a GPU."""
import ctypes as C
import os

import numpy as np

from tests.probe import probe as PR

HERE = os.path.dirname(os.path.abspath(__file__))
f32, f64, u32, u64, i32 = np.float32, np.float64, np.uint32, np.uint64, np.int32
NS_SENTINEL = -7777.0    # what bq_tp_wave's ns[] holds in a lane that does not hold the block's end
NOISE_TICKS = 64         # ticks per call of tp_noise_ticks<64>

_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        path = os.path.join(HERE, "libwave_probe.so")
        if not os.path.exists(path):
            PR.build()
        _LIB = C.CDLL(path)
    return _LIB


def _arr(a, dtype, shape):
    a = np.ascontiguousarray(a, dtype=dtype)
    assert a.shape == tuple(shape), (a.shape, shape)
    return a


def _call(symbol, *args):
    fn = getattr(lib(), "wave_probe_" + symbol)
    fn.restype = C.c_int
    conv = []
    for a in args:
        if isinstance(a, np.ndarray):
            conv.append(C.c_void_p(a.ctypes.data))
        elif isinstance(a, tuple):
            conv.append(a[0](a[1]))
        else:
            conv.append(C.c_size_t(a))
    err = fn(*conv)
    if err != 0:
        raise RuntimeError(f"wave_probe_{symbol}: error code {err}")


def _lanes(symbol, x, dtype, words=(), lpv=None):
    n = len(x)
    x = _arr(x, dtype, (n, 64) + tuple(words))
    out = np.empty_like(x)
    _call(symbol, *(((C.c_int, lpv),) if lpv else ()), x, out, n)
    return out


def scan_add_u64(lpv, ab):
    """ab: [cases, 64, 2] uint64, the pair of sums a lane carries."""
    return _lanes("scan_add_u64", ab, u64, (2,), lpv)


def scan_max_i32(lpv, x):
    return _lanes("scan_max_i32", x, i32, (), lpv)


def scan_affine(lpv, maps, s0):
    """maps: [cases, 64, 16] (c0[4], c1[4], c2[2], c3[2], z[4]); s0: [cases, 4].  -> the scanned records [cases, 64, 16] and
    lp24_affine_mul(record, s0, with z) [cases, 64, 4]."""
    n = len(maps)
    maps, s0 = _arr(maps, f64, (n, 64, 16)), _arr(s0, f64, (n, 4))
    out = np.empty((n, 64, 20), dtype=f64)
    _call("scan_affine", (C.c_int, lpv), maps, s0, out, n)
    return out[:, :, :16].copy(), out[:, :, 16:].copy()


def shfl(x, d):
    """x: [cases, 64] uint32 or uint64; d: [cases]; lane l receives lane l - d's value."""
    n = len(x)
    dtype = np.asarray(x).dtype
    assert dtype in (u32, u64)
    x, d = _arr(x, dtype, (n, 64)), _arr(d, i32, (n,))
    out = np.empty_like(x)
    _call("shfl32" if dtype == u32 else "shfl64", x, d, out, n)
    return out


def bq_tp_wave(lpv, xf, par):
    """xf: [cases, 64 / lpv, frames capacity] float32 (lane-channel, frame); par: [cases, 64 / lpv, 11] = frames, wet, b0, b1, b2, a1,
    a2, x1, x2, y1, y2.  -> outputs [cases, 64 / lpv, capacity] float32, holds_end [cases, 64] bool, ns [cases, 64, 4]."""
    n, ch, g = len(xf), {64: 4, 32: 8}[lpv], 64 // lpv
    xf = _arr(xf, f32, (n, g, 256))
    p = np.zeros((n, 2, 12), dtype=f64)
    p[:, :g, :11] = _arr(par, f64, (n, g, 11))
    o, ns = np.empty_like(xf), np.empty((n, 64, 5), dtype=f64)
    _call("bq_tp_wave", (C.c_int, lpv), xf, p, o, ns, n)
    assert ch * lpv == 256
    return o, ns[:, :, 0] != 0.0, ns[:, :, 1:].copy()


def noise_ticks(starts):
    """starts: [cases, 2] (x1, x2).  -> the accumulator's lanes [cases, 64] (as int32) and the state after the 64 ticks [cases, 2]."""
    n = len(starts)
    starts = _arr(starts, u32, (n, 2))
    out = np.empty((n, 66), dtype=u32)
    _call("noise_ticks", starts, out, n)
    return out[:, :64].view(i32).copy(), out[:, 64:].copy()


def wave_sum_lane63(x):
    return _lanes("wave_sum_lane63", x, f32)


def wave_sum(x):
    return _lanes("wave_sum", x, f32)


def wave_min_u32(x):
    return _lanes("wave_min_u32", x, u32)


def fused_acc(tile, par, partial):
    """tile: [cases, 8, 256, 2] float32 (frame slot, thread, L / R); par: [cases, 4] = count, f0, prow, frames; partial: [cases, psize]
    float32, the prefilled rows buffer of each case ([row pair][channel][frame]).  -> partial after FusedAcc::add x count and flush."""
    n = len(tile)
    tile, par = _arr(tile, f32, (n, 8, 256, 2)), _arr(par, u32, (n, 4))
    partial = np.array(partial, dtype=f32, order="C")
    assert partial.ndim == 2 and partial.shape[0] == n
    _call("fused_acc", tile, par, partial, partial.shape[1], n)
    return partial


def reduce_prev(rows, bus, desc):
    """rows: flat float32; bus: flat float32, prefilled; desc: [workgroups, 8] = rows offset, bus offset, n_rows, frames, accumulate,
    wg, n_wg, 0.  Every workgroup (256 threads) calls tp_reduce_prev once.  -> bus afterwards."""
    rows = np.ascontiguousarray(rows, dtype=f32).reshape(-1)
    bus = np.array(bus, dtype=f32, order="C").reshape(-1)
    desc = _arr(desc, u32, (len(desc), 8))
    _call("reduce_prev", rows, rows.size, bus, bus.size, desc, len(desc))
    return bus


# ------------------------------------------------------------------ host side (no GPU)
def voices_per_workgroup(vpw):
    fn = lib().wave_probe_voices_per_workgroup
    fn.restype, fn.argtypes = C.c_uint32, [C.c_uint32]
    return int(fn(vpw))


def welsh_tp_grid(n, vpw):
    fn = lib().wave_probe_welsh_tp_grid
    fn.restype, fn.argtypes = C.c_uint32, [C.c_uint32, C.c_uint32]
    return int(fn(n, vpw))


def groups_of_blocks(grid):
    """tp_group_of_block(i, grid) for i = 0 .. grid - 1."""
    fn = lib().wave_probe_groups_of_blocks
    fn.restype, fn.argtypes = None, [C.c_uint32, C.c_void_p]
    out = np.empty(grid, dtype=u32)
    fn(grid, out.ctypes.data)
    return out


def rbj_for_kind(kind, cutoff_hz, q, bandwidth_hz, db_gain, fs):
    """fx_coef.h fx_rbj_for_kind: b0, b1, b2, a1, a2."""
    fn = lib().wave_probe_rbj_for_kind
    fn.restype, fn.argtypes = C.c_int, [C.c_uint32] + [C.c_double] * 5 + [C.c_void_p]
    out = np.empty(5, dtype=f64)
    if fn(kind, cutoff_hz, q, bandwidth_hz, db_gain, fs, out.ctypes.data) != 0:
        raise RuntimeError(f"fx_rbj_for_kind: kind {kind} is no BiQuad 12 dB mode")
    return out


def fx_lp24_coeffs(fc, ripple, fs):
    """fx_coef.h fx_lp24_coeffs: b0, a1, a2 of section 1, then of section 2 (y = b0 x + 2 b0 x1 + b0 x2 + a1 y1 + a2 y2)."""
    fn = lib().wave_probe_fx_lp24_coeffs
    fn.restype, fn.argtypes = None, [C.c_double] * 3 + [C.c_void_p]
    out = np.empty(6, dtype=f64)
    fn(fc, ripple, fs, out.ctypes.data)
    return out
