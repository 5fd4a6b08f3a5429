"""GPU tier: control trips resident on the device (include/groove_hip.h groove_ctl_trip_create / groove_ctl_trip_apply; csrc/ctl_link.h
ctl_trip_apply_kernel, ctl_trip_filter_apply_kernel; csrc/ctl_core.h ctl_trip_*).

Two effects of the same parameters run on the same noise, block after block.  Arm A has a device trip.  Arm B is the path that exists
without it: the host evaluates the trip's law (tests/ctl_trip_law.py, the host trip restated) and calls groove_fx_set_param, only while
a step holds.  O is the f64 oracle's effect, given the parameter groove_fx_set_param's law makes of that value.

A block whose start lies in a flat or slope step, or outside the trip, must come out of both arms bit for bit.  In a logarithmic or
exponential step the device's f64 log10 may differ from the C library's in the last place, which survives the rounding to the fp32
parameter about once in 2^28: there arm A is held to the oracle at the bar tests/test_gpu_ctl_filter_links.py uses (4e-6 of the larger
of 1 and the output's peak), and the number of such blocks that differ from arm B in any bit is printed and may be at most one in ten.
(tests/test_ctl_trip_cpu.py checks that the law's two texts give zero differing parameters for this trip on the CPU.)  Once a curved
block HAS differed, the parameter it left — and a filter's state — differ too, so the later blocks of that run are held to the oracle
only; the print says so."""
import ctypes as C

import numpy as np
import pytest

from groove_amd import abi_types as T, lib as _lib
from tests import ctl_trip_law as LAW, fx_forms as F
from tests.test_gpu_ctl_filter_links import BAR, KINDS as FILTERS
from tests.test_gpu_ctl_links import _audio, _params

pytestmark = pytest.mark.gpu

CAP = 64
BASE = {"gain": (T.FX_GAIN, dict(ceiling=0.75)), "bitcrusher": (T.FX_BITCRUSHER, dict(bits=8)),
        "reverb": (T.FX_REVERB, dict(attenuation=0.9, reverb_seconds=0.4)), "compressor": (T.FX_COMPRESSOR, dict(limit_min=0.3, limit_max=0.25)),
        "limiter": (T.FX_LIMITER, dict(limit_min=0.1, limit_max=1.0))}     # (the trip's threshold, at most 0.9, stays below the maximum)
BASE.update({k: (v, dict(cutoff_hz=1000.0, q=0.9, passband_ripple=1.1, bandwidth_hz=500.0, db_gain=6.0)) for k, v in FILTERS.items()})
INDEX = {"ceiling": T.CTL_FX_CEILING, "bits": T.CTL_FX_BITS, "attenuation": T.CTL_FX_ATTENUATION, "threshold": T.CTL_FX_THRESHOLD,
         "cutoff": T.CTL_FX_CUTOFF, "q": T.CTL_FX_Q, "passband-ripple": T.CTL_FX_PASSBAND_RIPPLE}
# every target groove_ctl_trip_create accepts
TARGETS = ([("ceiling", "gain"), ("bits", "bitcrusher"), ("attenuation", "reverb"), ("threshold", "compressor"), ("threshold", "limiter")] +
           [("cutoff", k) for k in FILTERS] + [("q", k) for k in ("lp12", "hp12", "ap12")] + [("passband-ripple", "lp24")])
CURVED = (LAW.LOG, LAW.EXP)


def _mk(n, kind, **per_lane):
    kw = dict(BASE[kind][1])
    kw.update({k: list(np.broadcast_to(v, (n,)).tolist()) for k, v in per_lane.items()})
    return _params(n, **kw)


def _run(block, fx, x):
    block.upload(x)
    fx.transform_audio(block, x.shape[1])
    return block.download(x.shape[1])


def _same(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _compare(gpu_ctx, oracle, param, kind, n, lanes, starts, ats, frames=64, seed=0, form=None, with_oracle=True):
    """The three arms over the blocks that start at `ats` (units).  `lanes` / `starts`: one trip per source lane (one: broadcast).
    Returns (curved blocks, curved blocks that differ between A and B, blocks in which A moved away from an untouched effect)."""
    from groove_amd import entities as E
    index, fxk = INDEX[param], BASE[kind][0]
    rng = np.random.default_rng(1000 + 31 * index + fxk + n + seed)
    a, b, plain = (E.Effect(gpu_ctx, fxk, _mk(n, kind)) for _ in range(3))
    ofx = oracle.Fx(fxk, _mk(n, kind)) if with_oracle else None
    trip = E.ControlTripLink(gpu_ctx, lanes, starts, a, index)
    io = gpu_ctx.block(n, CAP)
    field = LAW.param_of(index, 0.5)[0]
    cur = [BASE[kind][1][field]] * n                                  # the oracle's parameter, lane by lane
    curved = differing = moved = 0
    diverged = False
    for k, at in enumerate(ats):
        x = _audio(rng, n, frames)
        trip.work(at)
        where = [LAW.scan(starts[s], lanes[s], at)[0] for s in range(len(lanes))]
        vals = [LAW.trip_value(starts[s], lanes[s], at) for s in range(len(lanes))]
        if len(lanes) == 1:
            if vals[0] is not None:
                b.control_set_param_by_index(index, vals[0])
                cur = [LAW.param_of(index, vals[0])[1]] * n
        else:
            for lane in range(n):
                if vals[lane] is not None:
                    b.control_set_param_by_index(index, vals[lane], lane=lane)
                    cur[lane] = LAW.param_of(index, vals[lane])[1]
        if form is not None:
            for fx in (a, b):
                assert fx.kernel_form(io, frames) == form, (kind, n, frames)
        ga, gb, gp = _run(io, a, x), _run(io, b, x), _run(io, plain, x)
        if ofx is not None:
            ofx.set_params(_mk(n, kind, **{field: cur}))
            want = ofx.process(x.astype(np.float64))
            bar = BAR * max(1.0, float(np.abs(want).max()))
            err_b, err_a = float(np.abs(gb.astype(np.float64) - want).max()), float(np.abs(ga.astype(np.float64) - want).max())
            print(f"{param} -> {kind}, {n} lanes, block {k} at {at} (steps {sorted(set(where))}): |B - O| {err_b:.3e}  |A - O| {err_a:.3e}  bar {bar:.3e}")
            assert err_b <= bar, ("B against O: the inputs", param, kind, k)
            assert err_a <= bar, ("A against O", param, kind, k)
        is_curved = any(w >= 0 and lanes[s][w][0] in CURVED for s, w in enumerate(where))
        if is_curved:
            curved += 1
            if not _same(ga, gb):
                differing += 1
                diverged = True
        elif not diverged:
            assert _same(ga, gb), ("a flat / slope / outside block differs between the arms", param, kind, n, k, at, where)
        moved += (not _same(ga, gp)) and any(w >= 0 for w in where)
    print(f"{param} -> {kind}, {n} lanes: {differing} of {curved} logarithmic / exponential blocks differ between the arms" +
          ("; the blocks after the first of them were held to the oracle only" if diverged else ""))
    assert differing * 10 <= curved, (param, kind, differing, curved)
    assert gpu_ctx.debug_info()["zero_segments"] == 0
    for x_ in (trip, io, a, b, plain):
        x_.destroy()
    return curved, differing, moved


@pytest.mark.parametrize("param,kind", TARGETS, ids=[f"{p}-{k}" for p, k in TARGETS])
def test_trip_on_every_target_three_arms(gpu_ctx, oracle, param, kind):
    ats = [k * LAW.BLOCK_UNITS for k in range(LAW.MAIN_BLOCKS)]
    where = LAW.main_block_steps()
    assert where[:3] == [-1, -1, 0] and where[5:7] == [0, 1] and where[-2:] == [-1, -1]        # two before, one on a boundary, two after
    curved, _, moved = _compare(gpu_ctx, oracle, param, kind, 65, [LAW.MAIN_STEPS], [LAW.MAIN_START], ats)
    assert curved == sum(w in (2, 3) for w in where) == 15
    if kind != "reverb":     # (a reverb's attenuation scales what ENTERS its combs: it is heard a comb's delay later than these 1,920 frames)
        assert moved >= 13, moved


def _per_lane(n):
    """Every lane its own trip: the main trip's steps with other values, started up to 5,044 units apart, so that at one instant the
    lanes sit before the trip, in each of its steps, and after it."""
    lanes = [[(kind, (s0 + 0.003 * lane) % 1.0, (e0 + 0.002 * lane) % 1.0, beats) for kind, s0, e0, beats in LAW.MAIN_STEPS] for lane in range(n)]
    starts = [(400 + 97 * (lane % 53)) / 65536.0 for lane in range(n)]
    return lanes, starts


@pytest.mark.parametrize("param,kind", [("ceiling", "gain"), ("bits", "bitcrusher"), ("cutoff", "lp12")])
@pytest.mark.parametrize("n,per_lane", [(1, False), (257, False), (257, True)], ids=["1-lane", "257-broadcast", "257-per-lane"])
def test_lane_counts_broadcast_and_per_lane(gpu_ctx, oracle, param, kind, n, per_lane):
    """257 lanes: two workgroups and a ragged tail."""
    ats = list(range(0, 11200, 560))
    if per_lane:
        lanes, starts = _per_lane(n)
        at = 5000                                                       # one instant: before, flat, slope, logarithmic, exponential
        assert {LAW.scan(starts[s], lanes[s], at)[0] for s in range(n)} == {-1, 0, 1, 2, 3}
        assert {LAW.scan(starts[s], lanes[s], 10000)[0] for s in range(n)} == {-1, 3}
    else:
        lanes, starts = [LAW.MAIN_STEPS], [LAW.MAIN_START]
    curved, _, moved = _compare(gpu_ctx, oracle, param, kind, n, lanes, starts, ats, seed=7)
    assert curved >= 5 and moved >= 5


@pytest.mark.parametrize("n,frames", [(65, 64), (2049, 16), (24577, 8)])
@pytest.mark.parametrize("kind", ["lp12", "lp24"])
def test_every_iir_kernel_form_reads_what_the_trip_wrote(gpu_ctx, kind, n, frames):
    """Time-parallel, four-segment (12 dB; the 24 dB low-pass is serial from 1,025 lanes) and serial, the form asserted as
    tests/test_gpu_fx_forms.py does; the trip against groove_fx_set_param, a broadcast trip."""
    forms = F.library_forms()
    tag = {("lp12", 65): F.BQ_TP, ("lp12", 2049): F.BQ_SEG, ("lp12", 24577): F.BQ_SER,
           ("lp24", 65): F.LP_TP, ("lp24", 2049): F.LP_SER, ("lp24", 24577): F.LP_SER}[(kind, n)]
    ats = list(range(0, 6400, 640))
    curved, _, moved = _compare(gpu_ctx, None, "cutoff", kind, n, [LAW.MAIN_STEPS], [LAW.MAIN_START], ats, frames=frames, form=F.form_of_tag(tag, forms),
                                with_oracle=False)
    assert curved >= 4 and moved >= 6


def test_two_trips_onto_one_filter_see_each_other(gpu_ctx, oracle):
    from groove_amd import entities as E
    n, frames = 63, 64
    rng = np.random.default_rng(63)
    q_steps = [(LAW.SLOPE, 0.1, 0.9, 2000.0 / 65536), (LAW.FLAT, 0.55, 0.55, 1500.0 / 65536), (LAW.EXP, 0.9, 0.2, 2000.0 / 65536)]
    q_start = 300.0 / 65536
    fxs = {name: E.Effect(gpu_ctx, T.FX_BIQUAD_LP12, _mk(n, "lp12")) for name in ("both", "cutoff", "q")}
    ofx = oracle.Fx(T.FX_BIQUAD_LP12, _mk(n, "lp12"))
    trips = {("both", "cutoff"): E.ControlTripLink(gpu_ctx, [LAW.MAIN_STEPS], LAW.MAIN_START, fxs["both"], T.CTL_FX_CUTOFF),
             ("both", "q"): E.ControlTripLink(gpu_ctx, [q_steps], q_start, fxs["both"], T.CTL_FX_Q),
             ("cutoff", "cutoff"): E.ControlTripLink(gpu_ctx, [LAW.MAIN_STEPS], LAW.MAIN_START, fxs["cutoff"], T.CTL_FX_CUTOFF),
             ("q", "q"): E.ControlTripLink(gpu_ctx, [q_steps], q_start, fxs["q"], T.CTL_FX_Q)}
    io = gpu_ctx.block(n, CAP)
    cutoff, q = BASE["lp12"][1]["cutoff_hz"], BASE["lp12"][1]["q"]
    apart = {"cutoff": 0.0, "q": 0.0}
    for blk, at in enumerate(range(0, 6000, 400)):
        x = _audio(rng, n, frames)
        for p in (("cutoff", "q") if blk % 2 == 0 else ("q", "cutoff")):        # both orders, in different blocks
            trips[("both", p)].work(at)
        trips[("cutoff", "cutoff")].work(at)
        trips[("q", "q")].work(at)
        vc, vq = LAW.trip_value(LAW.MAIN_START, LAW.MAIN_STEPS, at), LAW.trip_value(q_start, q_steps, at)
        cutoff = cutoff if vc is None else LAW.param_of(T.CTL_FX_CUTOFF, vc)[1]
        q = q if vq is None else LAW.param_of(T.CTL_FX_Q, vq)[1]
        ofx.set_params(_mk(n, "lp12", cutoff_hz=cutoff, q=q))
        got = {name: _run(io, fx, x).astype(np.float64) for name, fx in fxs.items()}
        want = ofx.process(x.astype(np.float64))
        assert np.abs(got["both"] - want).max() <= BAR * max(1.0, float(np.abs(want).max())), blk
        for name in apart:
            apart[name] = max(apart[name], float(np.abs(got["both"] - got[name]).max()))
    assert apart["cutoff"] > 1e-3 and apart["q"] > 1e-3, apart
    assert gpu_ctx.debug_info()["zero_segments"] == 0
    for x_ in list(trips.values()) + [io] + list(fxs.values()):
        x_.destroy()


def test_trip_applies_do_not_wait_on_the_host_and_set_param_does(gpu_ctx):
    from groove_amd import entities as E
    n = 65
    lp, gain = E.Effect(gpu_ctx, T.FX_BIQUAD_LP12, _mk(n, "lp12")), E.Effect(gpu_ctx, T.FX_GAIN, _mk(n, "gain"))
    t1 = E.ControlTripLink(gpu_ctx, [LAW.MAIN_STEPS], LAW.MAIN_START, lp, T.CTL_FX_CUTOFF)
    t2 = E.ControlTripLink(gpu_ctx, [LAW.MAIN_STEPS], LAW.MAIN_START, gain, T.CTL_FX_CEILING)
    waits = lambda: gpu_ctx.debug_info()["host_waits"]
    a = waits()
    own = waits() - a                                                # what reading the counter costs by itself
    a = waits()
    for k in range(10):
        t1.work(k * 600)
        t2.work(k * 600)
    assert waits() - a - own == 0                                   # twenty applies: not one host wait
    a = waits()
    lp.control_set_param_by_index(T.CTL_FX_CUTOFF, 0.5)
    assert waits() - a - own >= 1
    assert gpu_ctx.debug_info()["zero_segments"] == 0
    for x_ in (t1, t2, lp, gain):
        x_.destroy()


def test_refusals_each_with_its_message(gpu_ctx):
    from groove_amd import entities as E
    n = 4
    fx = {name: E.Effect(gpu_ctx, BASE[name][0], _mk(n, name)) for name in ("gain", "lp12", "bp12", "lp24", "reverb")}
    ok = [(LAW.SLOPE, 0.1, 0.9, 1.0)]
    trip = lambda target, index, lanes=None, starts=0.0: E.ControlTripLink(gpu_ctx, [ok] if lanes is None else lanes, starts, fx[target], index)
    for target, index, msg in (("lp12", T.CTL_FX_WET, "groove_ctl_trip_create: wet-dry-mix chooses a kernel path"),
                               ("gain", T.CTL_FX_WET, "kernel path"),
                               ("gain", T.CTL_FX_CUTOFF, "no such parameter .*cutoff: the nine filter kinds"),
                               ("bp12", T.CTL_FX_Q, "no such parameter .*q: low-pass, high-pass and all-pass 12 dB"),
                               ("lp12", T.CTL_FX_PASSBAND_RIPPLE, "no such parameter .*passband-ripple: low-pass 24 dB"),
                               ("lp12", T.CTL_FX_CEILING, "no such parameter .*ceiling: Gain"),
                               ("gain", T.CTL_FX_BITS, "no such parameter .*bits: Bitcrusher"),
                               ("reverb", T.CTL_FX_THRESHOLD, "no such parameter .*threshold: Compressor"),
                               ("lp12", 99, "unknown control index"), ("lp12", T.CTL_WELSH_CUTOFF, "unknown control index")):
        with pytest.raises(_lib.GrooveError, match=msg):
            trip(target, index)
    inf, nan = float("inf"), float("nan")
    for lanes, starts, msg in (([[]], 0.0, "at least one step"),
                               ([ok * 65537], 0.0, "more than 65,536 steps"),
                               ([[(LAW.SLOPE, 0.1, 0.9, 0.0)]], 0.0, "beats must be > 0"),
                               ([ok + [(LAW.FLAT, 0.1, 0.1, -1.0)]], 0.0, "beats must be > 0"),
                               ([[(LAW.SLOPE, 0.1, 0.9, inf)]], 0.0, "beats, start or end is not finite"),
                               ([[(LAW.SLOPE, 0.1, 0.9, nan)]], 0.0, "beats, start or end is not finite"),
                               ([[(LAW.SLOPE, nan, 0.9, 1.0)]], 0.0, "beats, start or end is not finite"),
                               ([[(LAW.SLOPE, 0.1, -inf, 1.0)]], 0.0, "beats, start or end is not finite"),
                               ([ok], nan, "start_beat is not finite"), ([ok], inf, "start_beat is not finite"),
                               ([[(4, 0.1, 0.9, 1.0)]], 0.0, "unknown step kind"), ([ok + [(7, 0.1, 0.9, 1.0)]], 0.0, "unknown step kind"),
                               ([ok] * 3, 0.0, "lane count")):
        with pytest.raises(_lib.GrooveError, match=msg):
            trip("lp12", T.CTL_FX_CUTOFF, lanes, starts)
    assert trip("lp12", T.CTL_FX_CUTOFF, [ok * 65536]).destroy() is None               # 65,536 steps are accepted
    # links of the wrong kind
    link = trip("lp12", T.CTL_FX_CUTOFF)
    lfo = E.ControlLink(gpu_ctx, T.ctl_sources(n, source=T.CTL_SRC_LFO, waveform=T.WAVE_SINE, frequency_hz=1.0), fx["gain"], T.CTL_FX_CEILING)
    side = gpu_ctx.block(n, CAP)
    L = gpu_ctx.L
    with pytest.raises(_lib.GrooveError, match="groove_ctl_link_apply: a trip link .*groove_ctl_trip_apply"):
        _lib.check(L.groove_ctl_link_apply(link.h, 0), gpu_ctx.h)
    with pytest.raises(_lib.GrooveError, match="groove_ctl_link_capture: a trip link captures nothing"):
        _lib.check(L.groove_ctl_link_capture(link.h, side.h, CAP), gpu_ctx.h)
    with pytest.raises(_lib.GrooveError, match="groove_ctl_trip_apply: not a trip link"):
        _lib.check(L.groove_ctl_trip_apply(lfo.h, 0), gpu_ctx.h)
    link.reset()                                                       # succeeds and does nothing
    link.work(0)
    # a dead target
    dead = C.c_void_p(fx["lp12"].h.value)                              # (only compared with the live effects' handles, never followed)
    fx["lp12"].destroy()
    with pytest.raises(_lib.GrooveError, match="groove_ctl_trip_apply: the target effect has been destroyed"):
        link.work(64)
    steps, n_steps = T.ctl_steps([ok])
    with pytest.raises(_lib.GrooveError, match="groove_ctl_trip_create: the target is not a live effect"):
        _lib.check(L.groove_ctl_trip_create(gpu_ctx.h, steps, n_steps, (C.c_double * 1)(0.0), 1, dead, T.CTL_FX_CUTOFF, C.byref(C.c_void_p())), gpu_ctx.h)
    assert gpu_ctx.debug_info()["zero_segments"] == 0
    for x_ in (link, lfo, side):
        x_.destroy()
    for name in ("gain", "bp12", "lp24", "reverb"):
        fx[name].destroy()
