"""GPU tier: the two (source, target, lane mapping) cells of csrc/ctl_link.h's ctl_apply_kernel<Source, Target> that no other test
launches and compares bits for — a live source's ONE lane broadcast onto a uint word (bits), and a trip with one lane per target lane
onto wet-dry-mix.  65 target lanes (one full wavefront and one lane), 8-frame blocks.  Arm A is the link; arm B is groove_fx_set_param
with the value the CPU shims of csrc/ctl_core.h give (tests/test_ctl_core_cpu.py, tests/test_ctl_trip_cpu.py); the two effects then
process the same block, which is how the neighbouring tests read a target word back, and must agree bit for bit."""
import numpy as np
import pytest

from groove_amd import abi_types as T
from tests import ctl_trip_law as LAW
from tests.test_ctl_core_cpu import shim  # noqa: F401  (the fixture that compiles csrc/ctl_core.h for the host)
from tests.test_ctl_trip_cpu import _shim_begins, shim as trip_shim  # noqa: F401  (... and its trip half)
from tests.test_gpu_ctl_links import _audio, _bitcrush_np, _params

pytestmark = pytest.mark.gpu

N, FRAMES = 65, 8


def _same(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _run(block, fx, x):
    block.upload(x)
    fx.transform_audio(block, x.shape[1])
    return block.download(x.shape[1])


def test_a_signal_lane_broadcast_onto_bits_is_set_param(gpu_ctx, shim):
    """|m| on and just under the sixteenths: bits = floor(16 |m|) takes 0 .. 16 over the blocks, the same in all 65 lanes."""
    import ctypes as C
    from groove_amd import entities as E
    a, b = (E.Effect(gpu_ctx, T.FX_BITCRUSHER, _params(N, bits=3)) for _ in range(2))
    link = E.ControlLink(gpu_ctx, T.ctl_sources(1, source=T.CTL_SRC_SIGNAL, law=T.CTL_LAW_AMPLITUDE), a, T.CTL_FX_BITS)
    side, io = gpu_ctx.block(1, FRAMES), gpu_ctx.block(N, FRAMES)
    rng = np.random.default_rng(65)
    ms = [np.float32(k / 16.0) for k in range(17)] + [np.nextafter(np.float32(k / 16.0), np.float32(0)) for k in range(1, 17)]
    seen = set()
    for m in ms:
        x = np.zeros((2, FRAMES, 1), dtype=np.float32)
        x[:, FRAMES - 1, 0] = m                                                   # L = R = m: (m + m) / 2 = m exactly
        side.upload(x)
        link.capture(side, FRAMES)
        link.work(0)
        left, right = (C.c_float * 1)(float(m)), (C.c_float * 1)(float(m))
        mono, v = (C.c_float * 1)(), (C.c_float * 1)()
        shim.shim_signal(left, right, T.CTL_LAW_AMPLITUDE, mono, v, 1)
        b.control_set_param_by_index(T.CTL_FX_BITS, float(v[0]))
        bits = min(int(np.float32(v[0]) * np.float32(16)), 31)
        seen.add(bits)
        probe = _audio(rng, N, FRAMES)
        probe[:, 0, :], probe[:, 1, :] = 1.0, 3.5                                 # 32767 tells bits 0 .. 15 apart, 114684 tells 15, 16 and 17 apart
        ga, gb = _run(io, a, probe), _run(io, b, probe)
        assert _same(ga, gb), float(m)
        assert _same(ga, _bitcrush_np(probe, np.uint32(bits))), float(m)
    assert seen == set(range(17))
    for x_ in (link, side, io, a, b):
        x_.destroy()


def test_a_trip_with_one_lane_per_target_lane_onto_wet_is_set_param(gpu_ctx, trip_shim):
    """Flat and slope steps (a closed form both sides round alike), values from -0.2 to 1.3 so that the clamp is reached, the lanes
    started up to 52 * 97 units apart: at one instant lanes sit before their trip, in either step, and after it."""
    from groove_amd import entities as E
    lanes = [[(LAW.FLAT, 0.35 + 0.004 * lane, 0.35 + 0.004 * lane, 800.0 / LAW.UNITS), (LAW.SLOPE, -0.2 + 0.003 * lane, 1.3 - 0.002 * lane, 1250.0 / LAW.UNITS)]
             for lane in range(N)]
    starts = [(400 + 97 * (lane % 53)) / LAW.UNITS for lane in range(N)]
    wet0 = [0.25 + 0.01 * lane for lane in range(N)]
    a, b = (E.Effect(gpu_ctx, T.FX_GAIN, _params(N, ceiling=0.5, wet=wet0)) for _ in range(2))
    trip = a.trip_wet(lanes, starts)
    io = gpu_ctx.block(N, FRAMES)
    rng = np.random.default_rng(66)
    begins = [_shim_begins(trip_shim, starts[s], lanes[s]) for s in range(N)]
    where_seen, clamped = set(), 0
    for at in range(0, 8000, 400):
        trip.work(at)
        where = []
        for s in range(N):
            i = trip_shim.shim_trip_find(begins[s], 1, 2, at)
            where.append(i)
            if i < 0:
                continue
            kind, s0, e0, beats = lanes[s][i]
            v = trip_shim.shim_trip_value(kind, s0, e0, begins[s][i], beats, trip_shim.shim_trip_now(at))
            clamped += not 0.0 <= v <= 1.0
            b.control_set_param_by_index(T.CTL_FX_WET, v, lane=s)
        where_seen.add(frozenset(where))
        x = _audio(rng, N, FRAMES)
        ga, gb = _run(io, a, x), _run(io, b, x)
        assert _same(ga, gb), (at, sorted(set(where)))
    assert frozenset({-1, 0, 1}) in where_seen and clamped > 0
    plain = E.Effect(gpu_ctx, T.FX_GAIN, _params(N, ceiling=0.5, wet=wet0))
    assert not _same(_run(io, a, x), _run(io, plain, x))                           # the trips really moved the mix
    for x_ in (trip, io, a, b, plain):
        x_.destroy()
