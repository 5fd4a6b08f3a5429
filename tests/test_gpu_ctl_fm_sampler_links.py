"""GPU tier: controls on FM and sampler banks — groove_bank_set_param on them, and control links and trips that stay on the device
(include/groove_hip.h groove_ctl_bank_link_create / groove_ctl_bank_trip_create on an FM or a sampler bank; csrc/ctl_link.h
ctl_voices_apply_kernel, ctl_trip_voices_apply_kernel; csrc/ctl_core.h ctl_fm_store, ctl_sampler_store).

Arm A is a bank with a device link, arm B the path without it: the host evaluates the law (tests/ctl_fm_sampler_law.py) and calls
groove_bank_set_param at the same block starts.  The arms must agree BIT FOR BIT block by block in flat and slope steps, outside the
trip, and under LFO and signal sources.  In a logarithmic or exponential step the rule is tests/test_gpu_ctl_bank_links.py's: the device's
log10 may differ from the C library's in the last place: every such block that differs is counted and at most one in ten may.  An LFO's fp32 value is read back from the device through an ordinary link onto a Gain's
ceiling (tests/test_gpu_ctl_wet_links.py's way) and handed to arm B; square and pulse lanes are also held to their closed form, exactly.

Arm B against an independent truth.  gain, pan and a sampler's gain never feed back into state, so block k of the walk is block k of an
ORACLE bank created with the values in force at block k: one oracle walk per distinct value, stitched.  FM bar: 2e-6 of full scale
(tests/test_gpu_instruments.py / test_gpu_independent.py for voices of index < 10); sampler: bit for bit.  depth and beta feed the carrier
phase: the reference is tests/test_oracle_independent.py's extended-precision FM voice restated here with the modulation index as a
per-frame array, constant within a block, and the re-trigger (the phase sums carry on from the last sounding frame), bar 2e-6.

Every test ends on zero_segments == 0 and fast_table_misses == 0."""
import contextlib

import numpy as np
import pytest

from groove_amd import abi_types as T, lib as _lib, patches as P
from tests import ctl_fm_sampler_law as LAW
from tests.ctl_trip_law import MAIN_START, MAIN_STEPS
from tests.test_ctl_core_cpu import signal_law_np
from tests.test_gpu_ctl_links import _Probe, _lfo_want
from tests.test_oracle_independent import _closed_form_envelope

pytestmark = pytest.mark.gpu

SR = 44100.0
BLOCKS = 24
SIZES = [64] * BLOCKS
SIZES[7] = 37                                                     # one ragged block
ATS = [240 * k for k in range(BLOCKS)]                            # trip times: 2 blocks before, 3 flat, 6 slope (block 5 on the boundary), 6 log, 7 exp
STARTS = [int(x) for x in np.concatenate([[0], np.cumsum(SIZES)[:-1]])]
ON_BLOCKS, OFF_BLOCK = (0, 15), 9
FM_PARAMS = ("gain", "pan", "depth", "beta")
FORMS = {                                                         # name: (kind, voices, time_parallel_max_voices or None, what kernel_form says)
    "fm-tp-3": ("fm", 3, None, "fm_tp_kernel (time-parallel)"),
    "fm-vpw4-4100": ("fm", 4100, None, "four voices per wavefront"),
    "fm-serial-70": ("fm", 70, 0, "fm_render_kernel (serial"),
    "sampler-tp-5": ("sampler", 5, None, "sampler_tp_kernel"),
    "sampler-serial-70": ("sampler", 70, 0, "sampler_render_kernel (serial"),
}
_PCM = {}


def _drums():
    if not _PCM:
        _PCM["bank"] = P.drum_bank(scale=0.02)[:2]
    return _PCM["bank"]


def _fm_table(n):
    """FM patches whose index stays below 10 (beta 15 clamped out: the controls clamp to 1 anyway) and whose envelopes sound over the walk."""
    ps = []
    for j in range(n):
        p = P.fm_patch(j % 16)
        p.beta = min(p.beta, 1.0)
        p.depth = 0.8
        p.carrier_envelope = T.EnvelopeParams(0.002, 0.004, 0.7, 0.003)
        p.modulator_envelope = T.EnvelopeParams(0.001, 0.005, 0.8, 0.004)
        ps.append(p)
    return (T.FmParams * n)(*ps)


def _keys(n):
    return (45 + (7 * np.arange(n)) % 40).astype(np.uint8)


@contextlib.contextmanager
def _form(ctx, name):
    kind, n, tp, says = FORMS[name]
    old = ctx.time_parallel_max_voices
    try:
        if tp is not None:
            ctx.time_parallel_max_voices = tp
        yield kind, n, says
    finally:
        ctx.time_parallel_max_voices = old


def _make(ctx, kind, n, params=None):
    from groove_amd import entities as E
    if kind == "fm":
        return E.FmSynth(ctx, _fm_table(n) if params is None else params)
    pcm, descs = _drums()
    return E.Sampler(ctx, pcm, descs, P.sampler_voices(n) if params is None else params)


def _index(kind, param):
    return (LAW.FM_INDEX if kind == "fm" else LAW.SAMPLER_INDEX)[param]


def _clean(ctx):
    info = ctx.debug_info()
    assert info["zero_segments"] == 0 and info["fast_table_misses"] == 0, info


def _same(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float32).view(np.uint32), np.asarray(b, dtype=np.float32).view(np.uint32))


def _events(n, k):
    lanes, keys, out = np.arange(n, dtype=np.uint32), _keys(n), []
    if k in ON_BLOCKS:
        out.append(T.note_events_np(lanes, keys, True))
    if k == OFF_BLOCK:
        out.append(T.note_events_np(lanes, keys, False))
    return out


def _walk(ctx, synth, n, before_block, mode="sync", blocks=BLOCKS):
    """The walk's blocks [2][frames][n]: events, before_block(k) — the arm's control — and the render, in one of the render entries."""
    out = []
    if mode in ("sync", "async"):
        blks = [ctx.block(n, 64) for _ in range(2 if mode == "async" else 1)]
        for k in range(blocks):
            for ev in _events(n, k):
                synth.handle_midi_events(ev)
            before_block(k)
            blk = blks[k % len(blks)]
            if mode == "async":
                synth.generate_batch_values_async(blk, SIZES[k])
                if k:
                    out.append(blks[(k - 1) % 2].download(SIZES[k - 1]))
            else:
                synth.generate_batch_values(blk, SIZES[k])
                out.append(blk.download(SIZES[k]))
        if mode == "async":
            out.append(blks[(blocks - 1) % 2].download(SIZES[blocks - 1]))
        for blk in blks:
            blk.destroy()
        return out
    bus = ctx.bus(sum(SIZES[:blocks]))                            # "paced", "mix": fused onto one long bus, no host wait between blocks
    for k in range(blocks):
        for ev in _events(n, k):
            synth.handle_midi_events(ev)
        before_block(k)
        getattr(synth, {"paced": "render_mix_paced", "mix": "render_mix"}[mode])(bus, SIZES[k], at_frame=STARTS[k])
    ctx.flush_bus()
    got = bus.download()
    bus.destroy()
    return [got[STARTS[k]:STARTS[k] + SIZES[k]] for k in range(blocks)]


def _compare_arms(ga, gb, curved_blocks, what, feeds_state=False):
    """tests/test_gpu_ctl_bank_links.py's rule: EVERY logarithmic / exponential block that differs between the arms is counted, and at
    most one in ten may.  Every other block must have arm B's bits — also after a curved block has differed, unless the parameter feeds
    the voices' state (depth, beta: the carrier phase), where a difference lives on; there the later curved blocks differ too, are
    counted, and break the bound."""
    curved = differing = 0
    diverged = False
    for k, (x, y) in enumerate(zip(ga, gb)):
        if k in curved_blocks:
            curved += 1
            if not _same(x, y):
                differing, diverged = differing + 1, True
        elif not (diverged and feeds_state):
            assert _same(x, y), ("a flat / slope / outside / LFO / signal block differs between the arms", what, k)
    print(f"{what}: {differing} of {curved} logarithmic / exponential blocks differ between the arms")
    assert differing * 10 <= curved, (what, differing, curved)


def _trip_values():
    return [LAW.trip_value(MAIN_START, MAIN_STEPS, at) for at in ATS]


def _curved():
    return {k for k, at in enumerate(ATS) if (lambda i: i >= 0 and MAIN_STEPS[i][0] in LAW.CURVED)(LAW.scan(MAIN_START, MAIN_STEPS, at)[0])}


def test_the_walk_has_every_kind_of_block():
    where = [LAW.scan(MAIN_START, MAIN_STEPS, at)[0] for at in ATS]
    assert where[:2] == [-1, -1] and where.count(0) == 3 and where[5] == 1 and where.count(1) == 6 and where.count(2) == 6 and where.count(3) == 7
    assert 37 in SIZES and len(SIZES) == 24


# ---------------------------------------------------------------------------------------------------------------- arm A = arm B
def _params_of(kind):
    return FM_PARAMS if kind == "fm" else ("gain",)


@pytest.mark.parametrize("name", list(FORMS))
def test_a_four_step_trip_in_every_form_arm_a_is_arm_b(gpu_ctx, name):
    from groove_amd import entities as E
    vals = _trip_values()
    with _form(gpu_ctx, name) as (kind, n, says):
        for param in _params_of(kind):
            index = _index(kind, param)
            a, b = _make(gpu_ctx, kind, n), _make(gpu_ctx, kind, n)
            assert says in a.kernel_form(64, False), (name, a.kernel_form(64, False))
            trip = E.ControlTripLink(gpu_ctx, [list(MAIN_STEPS)], MAIN_START, a, index)
            ga = _walk(gpu_ctx, a, n, lambda k: trip.work(ATS[k]))
            gb = _walk(gpu_ctx, b, n, lambda k: vals[k] is not None and b.control_set_param_by_index(index, vals[k]))
            plain = _make(gpu_ctx, kind, n)
            gp = _walk(gpu_ctx, plain, n, lambda k: None, blocks=4)
            assert _same(ga[0], gp[0]) and _same(ga[1], gp[1]) and not _same(ga[2], gp[2]), (name, param)   # nothing before the trip; heard from its first step
            _compare_arms(ga, gb, _curved(), f"{name} {param} trip", feeds_state=param in ("depth", "beta"))
            _clean(gpu_ctx)
            for x in (trip, a, b, plain):
                x.destroy()


def _per_voice_trip(n):
    """One flat-then-slope lane per voice — its own values, its own start beat, no curved step: at a given block some lanes hold a step
    and some do not."""
    units = float(T.CTL_UNITS_PER_BEAT)
    lanes, starts = [], []
    for v in range(n):
        a, b = 0.1 + 0.8 * ((v * 37) % 101) / 100.0, 0.1 + 0.8 * ((v * 53 + 11) % 101) / 100.0
        lanes.append([(LAW.FLAT, a, a, (700.0 + 100.0 * (v % 5)) / units), (LAW.SLOPE, a, b, 3000.0 / units)])
        starts.append((300.0 + 60.0 * (v % 7)) / units)
    return lanes, starts


@pytest.mark.parametrize("name", list(FORMS))
def test_a_trip_with_one_lane_per_voice_arm_a_is_arm_b(gpu_ctx, name):
    """n_src == voices on the trip kernel.  Arm B sets voice by voice, only the voices whose lane holds a step; at 4,100 voices that is
    4,100 uploads per block, so there the walk is three blocks: before every lane, inside every lane's slope, after every lane."""
    from groove_amd import entities as E
    with _form(gpu_ctx, name) as (kind, n, says):
        blocks, ats = (3, [0, 1500, 5400]) if n > 1000 else (BLOCKS, ATS)
        lanes, starts = _per_voice_trip(n)
        vals = [[LAW.trip_value(starts[v], lanes[v], at) for v in range(n)] for at in ats]
        holds = [sum(x is not None for x in row) for row in vals]
        assert 0 in holds and n in holds and (n > 1000 or any(0 < h < n for h in holds))
        for param in _params_of(kind):
            index = _index(kind, param)
            a, b = _make(gpu_ctx, kind, n), _make(gpu_ctx, kind, n)
            assert says in a.kernel_form(64, False)
            trip = E.ControlTripLink(gpu_ctx, lanes, starts, a, index)

            def set_voices(k):
                for v, x in enumerate(vals[k]):
                    if x is not None:
                        b.control_set_param_by_index(index, x, voice=v)

            ga = _walk(gpu_ctx, a, n, lambda k: trip.work(ats[k]), blocks=blocks)
            gb = _walk(gpu_ctx, b, n, set_voices, blocks=blocks)
            _compare_arms(ga, gb, set(), f"{name} {param} per-voice trip")
            plain = _make(gpu_ctx, kind, n)
            first = next(k for k, h in enumerate(holds) if h)                       # nothing before the first lane's first step; heard from there
            gp = _walk(gpu_ctx, plain, n, lambda k: None, blocks=first + 1)
            assert all(_same(ga[k], gp[k]) for k in range(first)) and not _same(ga[first], gp[first]), (name, param)
            _clean(gpu_ctx)
            for x in (trip, a, b, plain):
                x.destroy()


def _lfo_lanes(n_src, smooth):
    """n_src LFO lanes: sine / triangle / sawtooth / triangle-sine, or square / pulse (53 Hz and up: they switch within the walk)."""
    waves = [T.WAVE_SINE, T.WAVE_TRIANGLE, T.WAVE_SAWTOOTH, T.WAVE_TRIANGLE_SINE] if smooth else [T.WAVE_SQUARE, T.WAVE_PULSE_WIDTH]
    desc = [(waves[i % len(waves)], 0.3, (5.3 if smooth else 53.0) + 1.913 * (i % 97)) for i in range(n_src)]
    arr = (T.CtlSource * n_src)()
    for s, (w, duty, f) in zip(arr, desc):
        s.source, s.waveform, s.duty, s.frequency_hz = T.CTL_SRC_LFO, w, duty, f
    return arr, desc


def _device_lfo_values(ctx, arr, desc, smooth, blocks):
    """[block][lane] fp32 value01 as the device computes it: the same lanes linked onto a Gain's ceiling, read back; square and pulse lanes
    are the closed form exactly."""
    from groove_amd import entities as E
    n_src = len(arr)
    gain = E.Effect(ctx, T.FX_GAIN, (T.FxParams * n_src)(*[T.fx_params(ceiling=0.5) for _ in range(n_src)]))
    link, probe = E.ControlLink(ctx, arr, gain, T.CTL_FX_CEILING), _Probe(ctx, n_src, 1.0)
    out = []
    for k in range(blocks):
        link.work(STARTS[k])
        v = probe.read(gain)
        want = _lfo_want(desc, STARTS[k])
        assert np.abs(v - want).max() <= 2e-7
        if not smooth:
            assert np.array_equal(v, want.astype(np.float32))
        out.append(v)
    for x in (link, probe, gain):
        x.destroy()
    return out


def _set_per_voice(b, index, values):
    if len(values) == 1:
        b.control_set_param_by_index(index, float(values[0]))
    else:
        for v, x in enumerate(values):
            b.control_set_param_by_index(index, float(x), voice=v)


@pytest.mark.parametrize("per_voice", [False, True], ids=["broadcast", "per-voice"])
@pytest.mark.parametrize("name", list(FORMS))
def test_lfo_sources_broadcast_and_one_lane_per_voice(gpu_ctx, name, per_voice):
    """Smooth and switching LFOs.  Arm B sets voice by voice where the source has a lane per voice; at 4,100 voices that is 4,100 uploads
    per controlled block, so there the per-voice walk is three blocks long with one of them controlled (the kernel takes no other path at
    another block)."""
    from groove_amd import entities as E
    with _form(gpu_ctx, name) as (kind, n, says):
        blocks = 3 if per_voice and n > 1000 else BLOCKS
        controlled = {1} if per_voice and n > 1000 else set(range(blocks))
        for smooth in (True, False):
            arr, desc = _lfo_lanes(n if per_voice else 1, smooth)
            vals = _device_lfo_values(gpu_ctx, arr, desc, smooth, blocks)
            assert np.ptp(np.array(vals)) > 0.4
            for param in _params_of(kind):
                index = _index(kind, param)
                a, b = _make(gpu_ctx, kind, n), _make(gpu_ctx, kind, n)
                assert says in a.kernel_form(64, False)
                link = E.ControlLink(gpu_ctx, arr, a, index)
                ga = _walk(gpu_ctx, a, n, lambda k: k in controlled and link.work(STARTS[k]), blocks=blocks)
                gb = _walk(gpu_ctx, b, n, lambda k: k in controlled and _set_per_voice(b, index, vals[k]), blocks=blocks)
                _compare_arms(ga, gb, set(), f"{name} {param} LFO {'smooth' if smooth else 'square / pulse'} {'per voice' if per_voice else 'broadcast'}")
                _clean(gpu_ctx)
                for x in (link, a, b):
                    x.destroy()


@pytest.mark.parametrize("name", list(FORMS))
def test_a_signal_source_and_nothing_before_a_capture(gpu_ctx, name):
    from groove_amd import entities as E
    rng = np.random.default_rng(64)
    law = T.CTL_LAW_AMPLITUDE_INVERTED
    side = rng.uniform(-1.0, 1.0, (BLOCKS, 2, 8, 1)).astype(np.float32)
    vals = [None, None] + [float(signal_law_np(law, side[k, 0, 7], side[k, 1, 7])[1][0]) for k in range(2, BLOCKS)]
    with _form(gpu_ctx, name) as (kind, n, says):
        for param in _params_of(kind):
            index = _index(kind, param)
            a, b, plain = (_make(gpu_ctx, kind, n) for _ in range(3))
            link, blk = E.ControlLink(gpu_ctx, T.ctl_sources(1, source=T.CTL_SRC_SIGNAL, law=law), a, index), gpu_ctx.block(1, 8)

            def work(k):
                if k >= 2:
                    blk.upload(side[k])
                    link.capture(blk, 8)
                link.work(STARTS[k])

            ga = _walk(gpu_ctx, a, n, work)
            gb = _walk(gpu_ctx, b, n, lambda k: vals[k] is not None and b.control_set_param_by_index(index, vals[k]))
            gp = _walk(gpu_ctx, plain, n, lambda k: None, blocks=3)
            assert _same(ga[0], gp[0]) and _same(ga[1], gp[1]) and not _same(ga[2], gp[2])
            _compare_arms(ga, gb, set(), f"{name} {param} signal")
            _clean(gpu_ctx)
            for x in (link, blk, a, b, plain):
                x.destroy()


# ---------------------------------------------------------------------------------------------------------------- arm B against a truth
def _stitched(oracle, kind, n, param, vals):
    """Block k of an oracle bank CREATED with the value in force at block k (None: the patch's own): one walk per distinct value."""
    walks, out = {}, []
    in_force, v = [], None
    for x in vals:
        v = x if x is not None else v
        in_force.append(v)
    for v in in_force:
        if v in walks:
            continue
        if kind == "fm":
            params = _fm_table(n)
            for p in params:
                if v is not None:
                    setattr(p, {"gain": "dca_gain", "pan": "dca_pan"}[param], LAW.fm_param(param, v))
            ob = oracle.Bank.fm(params)
        else:
            params = P.sampler_voices(n)
            for p in params:
                if v is not None:
                    p.gain = LAW.sampler_gain_param(v)
            pcm, descs = _drums()
            ob = oracle.Bank.sampler(pcm, descs, params)
        blocks = []
        for k in range(BLOCKS):
            for ev in _events(n, k):
                ob.note_events(ev)
            blocks.append(ob.render(SIZES[k]))
        walks[v] = blocks
    for k, v in enumerate(in_force):
        out.append(walks[v][k])
    return out


@pytest.mark.parametrize("name,param", [("fm-tp-3", "gain"), ("fm-tp-3", "pan"), ("fm-serial-70", "gain"), ("fm-serial-70", "pan"),
                                        ("sampler-tp-5", "gain"), ("sampler-serial-70", "gain")])
def test_set_param_on_gain_and_pan_is_the_oracle_bank_created_with_the_value(gpu_ctx, oracle, name, param):
    vals = _trip_values()
    with _form(gpu_ctx, name) as (kind, n, says):
        b = _make(gpu_ctx, kind, n)
        gb = _walk(gpu_ctx, b, n, lambda k: vals[k] is not None and b.control_set_param_by_index(_index(kind, param), vals[k]))
        _clean(gpu_ctx)
        b.destroy()
    want = _stitched(oracle, kind, n, param, vals)
    got, want = np.concatenate(gb, axis=1), np.concatenate(want, axis=1)
    assert np.sqrt(np.mean(want ** 2)) > 1e-2
    if kind == "sampler":
        assert np.array_equal(got, want.astype(np.float32))                              # bit for bit, as every sampler test here is
    else:
        worst = float(np.abs(got.astype(np.float64) - want).max())
        print(f"{name} {param}: worst |B - O| {worst:.3e}")
        assert worst <= 2e-6, (name, param, worst)


def _independent_fm_voice(p, key, n, off, index, again):
    """tests/test_oracle_independent.py _independent_fm_voice_of with the modulation index as a per-frame array (constant within a
    block) and a second note-on at frame `again`, after the voice has gone idle: carrier phase = running sum of
    f_c / SR (1 + modulator x modulator envelope x index), the first tick at phase 0; extended precision, nothing of oracle/.
    The oscillators do not tick while the carrier envelope is idle and a note-on does not reset them (docs/DSP_SPEC.md: FmVoice), so the
    second note continues both phase sums from the last sounding frame, under envelopes that start again from zero."""
    fc = 440.0 * 2.0 ** ((key - 69) / 12.0)
    dm, dc = np.longdouble(fc * p.ratio) / np.longdouble(SR), np.longdouble(fc) / np.longdouble(SR)
    ce, me = p.carrier_envelope, p.modulator_envelope
    pf = float(np.float32(p.dca_pan))
    want = np.zeros((2, n))

    def stretch(first, frames, ticks, cpos0, note_off):
        """`frames` frames from frame `first`, `ticks` oscillator ticks and the carrier sum cpos0 behind them."""
        i = np.arange(frames, dtype=np.longdouble) + np.longdouble(ticks)
        mpos = i * dm
        mod = np.sin(2.0 * np.pi * (mpos - np.floor(mpos)).astype(np.float64))
        cenv, idle_from = _closed_form_envelope(ce.attack, ce.decay, ce.sustain, ce.release, note_off, frames)
        menv, _ = _closed_form_envelope(me.attack, me.decay, me.sustain, me.release, note_off, frames)
        lfm = mod * menv * index[first:first + frames]
        delta = dc * (1.0 + lfm.astype(np.longdouble))
        if ticks == 0:
            cpos = np.concatenate([[np.longdouble(0.0)], np.cumsum(delta[1:])])      # the very first tick emits phase 0
        else:
            cpos = cpos0 + np.cumsum(delta)
        m = np.sin(2.0 * np.pi * (cpos - np.floor(cpos)).astype(np.float64)) * cenv * float(np.float32(p.dca_gain))
        sounding = min(idle_from, frames)
        want[0, first:first + sounding] = (m * (1.0 - 0.25 * (pf + 1.0) ** 2))[:sounding]
        want[1, first:first + sounding] = (m * (1.0 - (0.5 * pf - 0.5) ** 2))[:sounding]
        return idle_from, cpos[sounding - 1]

    idle_from, cpos_last = stretch(0, again, 0, None, off)
    assert idle_from < again                                       # idle before the second note: its envelopes start from zero
    stretch(again, n - again, idle_from, cpos_last, n - again)     # held to the end of the walk
    return want, idle_from


@pytest.mark.parametrize("param", ["depth", "beta"])
@pytest.mark.parametrize("name", ["fm-tp-3", "fm-serial-70"])
def test_set_param_on_depth_and_beta_against_the_independent_voice(gpu_ctx, name, param):
    """The whole walk: note-on, note-off, release to idle, the re-trigger, under the four-step trip's values."""
    vals = _trip_values()
    frames, off, again = sum(SIZES), STARTS[OFF_BLOCK], STARTS[ON_BLOCKS[1]]
    with _form(gpu_ctx, name) as (kind, n, says):
        b = _make(gpu_ctx, kind, n)
        assert says in b.kernel_form(64, False)
        gb = _walk(gpu_ctx, b, n, lambda k: vals[k] is not None and b.control_set_param_by_index(_index(kind, param), vals[k]))
        _clean(gpu_ctx)
        b.destroy()
    got = np.concatenate(gb, axis=1).astype(np.float64)
    table, keys = _fm_table(n), _keys(n)
    worst = worst_again = 0.0
    for v in range(n):
        p = table[v]
        depth, beta = np.full(frames, float(np.float32(p.depth))), np.full(frames, float(np.float32(p.beta)))
        for k in range(BLOCKS):
            if vals[k] is not None:
                (depth if param == "depth" else beta)[STARTS[k]:] = float(LAW.fm_param(param, vals[k]))
        want, _ = _independent_fm_voice(p, int(keys[v]), frames, off, depth * beta, again)
        assert np.abs(want[:, :again]).max() > 0.05 and np.abs(want[:, again:]).max() > 0.05
        worst = max(worst, float(np.abs(got[:, :again, v] - want[:, :again]).max()))
        worst_again = max(worst_again, float(np.abs(got[:, again:, v] - want[:, again:]).max()))
    print(f"{name} {param}: worst |B - independent voice| {worst:.3e} up to the re-trigger, {worst_again:.3e} from it on, over {n} voices")
    assert worst <= 2e-6 and worst_again <= 2e-6, (name, param, worst, worst_again)


@pytest.mark.parametrize("name", ["fm-tp-3", "fm-vpw4-4100", "fm-serial-70"])
def test_set_param_ahead_of_block_zero_is_a_bank_created_with_the_value(gpu_ctx, name):
    with _form(gpu_ctx, name) as (kind, n, says):
        for param, field, v in (("depth", "depth", 0.37), ("beta", "beta", 0.61), ("gain", "dca_gain", 0.45), ("pan", "dca_pan", 0.8)):
            made = _fm_table(n)
            for p in made:
                setattr(p, field, LAW.fm_param(param, v))
            a, b = _make(gpu_ctx, kind, n), _make(gpu_ctx, kind, n, made)
            a.control_set_param_by_index(_index(kind, param), v)
            ga, gb = _walk(gpu_ctx, a, n, lambda k: None, blocks=12), _walk(gpu_ctx, b, n, lambda k: None, blocks=12)
            assert all(_same(x, y) for x, y in zip(ga, gb)), (name, param)
            assert np.abs(np.concatenate(ga, axis=1)).max() > 0.05
            a.destroy(); b.destroy()
        _clean(gpu_ctx)


# ---------------------------------------------------------------------------------------------------------------- ordering, waits
@pytest.mark.parametrize("name", ["fm-tp-3", "fm-vpw4-4100", "fm-serial-70", "sampler-tp-5", "sampler-serial-70"])
def test_applies_between_asynchronous_and_fused_renders_give_the_synchronous_walks_samples(gpu_ctx, name):
    """groove_bank_render_async (two blocks in rotation) against the synchronous walk, block for block; render_mix_paced and render_mix —
    each a different order of additions onto the bus than a lane sum on the host — against their own arm B.  (Not the single bank's
    render_mix_deferred: arm B's set_param is a flush point, so its pending block goes through the reduction kernels where arm A's is
    carried by the next launch, a different order of additions at 257 rows whatever the applies do.)"""
    from groove_amd import entities as E
    vals = _trip_values()
    with _form(gpu_ctx, name) as (kind, n, says):
        param = "pan" if kind == "fm" else "gain"
        index = _index(kind, param)
        runs = {}
        for mode in ("sync", "async", "paced", "mix"):
            a = _make(gpu_ctx, kind, n)
            trip = E.ControlTripLink(gpu_ctx, [list(MAIN_STEPS)], MAIN_START, a, index)
            runs[mode] = _walk(gpu_ctx, a, n, lambda k: trip.work(ATS[k]), mode)
            trip.destroy(); a.destroy()
            if mode in ("paced", "mix"):
                b = _make(gpu_ctx, kind, n)
                gb = _walk(gpu_ctx, b, n, lambda k: vals[k] is not None and b.control_set_param_by_index(index, vals[k]), mode)
                b.destroy()
                _compare_arms(runs[mode], gb, _curved(), f"{name} {param} {mode}")
                assert np.abs(np.concatenate(runs[mode])).max() > 1e-2
        for k in range(BLOCKS):
            assert _same(runs["sync"][k], runs["async"][k]), (name, k)
        _clean(gpu_ctx)


def test_the_mixed_one_launch_form_with_links_onto_the_fm_and_the_sampler_bank(gpu_ctx):
    from groove_amd import entities as E
    vals = _trip_values()

    def run(linked):
        welsh = E.WelshSynth(gpu_ctx, P.welsh_voices_grouped(6)[0])
        fm, sampler = _make(gpu_ctx, "fm", 3), _make(gpu_ctx, "sampler", 5)
        welsh.handle_midi_events(P.note_on_all(6))
        links = [E.ControlTripLink(gpu_ctx, [list(MAIN_STEPS)], MAIN_START, fm, T.CTL_FM_DEPTH), E.ControlTripLink(gpu_ctx, [list(MAIN_STEPS)], MAIN_START, fm, T.CTL_FM_DCA_PAN),
                 E.ControlTripLink(gpu_ctx, [list(MAIN_STEPS)], MAIN_START, sampler, T.CTL_SAMPLER_GAIN)] if linked else []
        bus = gpu_ctx.bus(sum(SIZES))
        for k in range(BLOCKS):
            for s, n in ((fm, 3), (sampler, 5)):
                for ev in _events(n, k):
                    s.handle_midi_events(ev)
            if linked:
                for l in links:
                    l.work(ATS[k])
            elif vals[k] is not None:
                fm.control_set_param_by_index(T.CTL_FM_DEPTH, vals[k])
                fm.control_set_param_by_index(T.CTL_FM_DCA_PAN, vals[k])
                sampler.control_set_param_by_index(T.CTL_SAMPLER_GAIN, vals[k])
            gpu_ctx.render_mix_banks_deferred([welsh, fm, sampler], bus, SIZES[k], at_frame=STARTS[k])
        gpu_ctx.flush_bus()
        got = bus.download()
        for x in links + [welsh, fm, sampler, bus]:
            x.destroy()
        return [got[STARTS[k]:STARTS[k] + SIZES[k]] for k in range(BLOCKS)]

    ga, gb = run(True), run(False)
    _compare_arms(ga, gb, _curved(), "mixed one-launch form", feeds_state=True)
    assert np.abs(np.concatenate(ga)).max() > 1e-2 and not _same(ga[2], ga[1])
    _clean(gpu_ctx)


def test_applies_do_not_wait_on_the_host_and_set_param_does(gpu_ctx):
    from groove_amd import entities as E
    n = 70
    fm, sampler, other = _make(gpu_ctx, "fm", n), _make(gpu_ctx, "sampler", n), _make(gpu_ctx, "fm", n)
    trips = [E.ControlTripLink(gpu_ctx, [list(MAIN_STEPS)], MAIN_START, fm, LAW.FM_INDEX[p]) for p in ("pan", "depth")]
    trips.append(E.ControlTripLink(gpu_ctx, [list(MAIN_STEPS)], MAIN_START, sampler, T.CTL_SAMPLER_GAIN))
    lfo = E.ControlLink(gpu_ctx, _lfo_lanes(n, True)[0], fm, T.CTL_FM_DCA_GAIN)
    sig = E.ControlLink(gpu_ctx, T.ctl_sources(1, source=T.CTL_SRC_SIGNAL, law=T.CTL_LAW_BIPOLAR), sampler, T.CTL_SAMPLER_GAIN)
    blk, blk2, side = gpu_ctx.block(n, 64), gpu_ctx.block(n, 64), gpu_ctx.block(1, 8)
    side.upload(np.full((2, 8, 1), 0.25, dtype=np.float32))
    waits = lambda: gpu_ctx.debug_info()["host_waits"]
    fm.handle_midi_events(T.note_events_np(np.arange(n, dtype=np.uint32), _keys(n), True))
    fm.generate_batch_values_async(blk, 64)                         # renders in flight on side streams
    sampler.generate_batch_values_async(blk2, 64)
    before = waits()
    own = waits() - before                                          # what reading the counter costs by itself
    before = waits()
    for k in range(10):
        for t in trips:
            t.work(480 + 240 * k)
        lfo.work(64 * k)
        sig.capture(side, 8)
    assert waits() - before - own == 0                              # forty applies and ten captures: not one host wait
    for s, index in ((other, T.CTL_FM_DCA_PAN), (other, T.CTL_FM_DEPTH), (sampler, T.CTL_SAMPLER_GAIN)):
        before = waits()
        s.control_set_param_by_index(index, 0.5)
        assert waits() - before - own >= 1, index
    blk.download(64); blk2.download(64)
    _clean(gpu_ctx)
    for x in trips + [lfo, sig, blk, blk2, side, fm, sampler, other]:
        x.destroy()


# ---------------------------------------------------------------------------------------------------------------- staleness, refusals
def test_set_param_overwrites_until_the_next_apply(gpu_ctx):
    """The expected three stretches: a link onto one word (pan; depth), then set_param(ALL) on its partner (gain; beta) — the host's copy
    goes up again, with the HOST's value of the linked word — then the link's next apply: its value back, over the new partner (the shadow
    was refreshed).  The reference arm is given the same parameters through set_param alone, voice by voice where the host's copy differs
    between voices; depth feeds the carrier phase, so the arms are compared stretch by stretch from equal states."""
    from groove_amd import entities as E
    n, fr = 70, 64
    table = _fm_table(n)
    own = {"pan": lambda p: (float(p.dca_pan) + 1.0) / 2.0, "depth": lambda p: float(p.depth)}       # the control value that gives the patch's own float back
    for mine, other in (("pan", "gain"), ("depth", "beta")):
        i_mine, i_other = LAW.FM_INDEX[mine], LAW.FM_INDEX[other]
        a, ref, kept = (_make(gpu_ctx, "fm", n) for _ in range(3))
        trip = E.ControlTripLink(gpu_ctx, [[(LAW.FLAT, 0.35, 0.35, 1.0)]], 0.0, a, i_mine)
        blk = gpu_ctx.block(n, 64)
        on = T.note_events_np(np.arange(n, dtype=np.uint32), _keys(n), True)

        def render(s):
            s.generate_batch_values(blk, fr)
            return blk.download(fr)

        def host_copy_back(s):
            for v in range(n):
                assert LAW.fm_param(mine, own[mine](table[v])) == np.float32(getattr(table[v], "dca_pan" if mine == "pan" else "depth"))
                s.control_set_param_by_index(i_mine, own[mine](table[v]), voice=v)

        for s in (a, ref, kept):
            s.handle_midi_events(on)
        trip.work(100)
        ref.control_set_param_by_index(i_mine, 0.35)
        kept.control_set_param_by_index(i_mine, 0.35)
        got, want = render(a), render(ref)
        render(kept)
        assert _same(got, want), mine                                                                       # the link's value
        for s in (a, ref, kept):
            s.control_set_param_by_index(i_other, 0.5)
        host_copy_back(ref)
        stale, want, other_way = render(a), render(ref), render(kept)
        assert _same(stale, want) and not _same(stale, other_way), mine                                     # the host copy's value, the new partner
        trip.work(200)
        ref.control_set_param_by_index(i_mine, 0.35)
        assert _same(render(a), render(ref)), mine                                                          # the link's value again, over the new partner
        # a reset: shadow and records back to the host's copy
        a.reset(); ref.reset()
        host_copy_back(ref)
        for s in (a, ref):
            s.handle_midi_events(on)
        assert _same(render(a), render(ref)), mine
        for x in (trip, blk, a, ref, kept):
            x.destroy()
    # a sampler's gain: one word
    a, host = _make(gpu_ctx, "sampler", 5), _make(gpu_ctx, "sampler", 5)
    trip = E.ControlTripLink(gpu_ctx, [[(LAW.FLAT, 0.3, 0.3, 1.0)]], 0.0, a, T.CTL_SAMPLER_GAIN)
    blk = gpu_ctx.block(5, 64)
    for s in (a, host):
        s.handle_midi_events(T.note_events_np(np.arange(5, dtype=np.uint32), _keys(5), True))
    out = []
    for step in (lambda: trip.work(100), lambda: a.control_set_param_by_index(T.CTL_SAMPLER_GAIN, 0.9), lambda: trip.work(200)):
        step()
        a.generate_batch_values(blk, 64); ga = blk.download(64)
        host.generate_batch_values(blk, 64); gh = blk.download(64)
        out.append((ga, gh))
    assert _same(out[0][0], out[0][1] * np.float32(0.3)) and _same(out[1][0], out[1][1] * np.float32(0.9)) and _same(out[2][0], out[2][1] * np.float32(0.3))
    assert np.abs(out[0][1]).max() > 1e-3
    _clean(gpu_ctx)
    for x in (trip, blk, a, host):
        x.destroy()


def test_refusals_each_with_its_message(gpu_ctx):
    from groove_amd import entities as E
    welsh = E.WelshSynth(gpu_ctx, P.welsh_voices_grouped(8)[0])
    fm, sampler = _make(gpu_ctx, "fm", 4), _make(gpu_ctx, "sampler", 4)
    ok = [(LAW.SLOPE, 0.1, 0.9, 1.0)]
    lfo = lambda n=1: T.ctl_sources(n, source=T.CTL_SRC_LFO, waveform=T.WAVE_SINE, frequency_hz=1.0)
    link = lambda target, index, n=1: E.ControlLink(gpu_ctx, lfo(n), target, index)
    trip = lambda target, index, n=1: E.ControlTripLink(gpu_ctx, [ok] * n, 0.0, target, index)
    for make, who in ((link, "groove_ctl_bank_link_create"), (trip, "groove_ctl_bank_trip_create")):
        for target in (fm, sampler):
            for index in (T.CTL_WELSH_DCA_GAIN, T.CTL_WELSH_DCA_PAN, T.CTL_WELSH_CUTOFF):
                with pytest.raises(_lib.GrooveError, match=who + ": only Welsh banks expose controls"):
                    make(target, index)
        with pytest.raises(_lib.GrooveError, match=who + ": an FM bank's controls are 48 - 51"):
            make(fm, T.CTL_SAMPLER_GAIN)
        for index in LAW.FM_INDEX.values():
            with pytest.raises(_lib.GrooveError, match=who + ": a sampler bank's control is 64"):
                make(sampler, index)
            with pytest.raises(_lib.GrooveError, match=who + ": unknown control index .*dca-gain, dca-pan or filter-cutoff"):
                make(welsh, index)
        with pytest.raises(_lib.GrooveError, match=who + ": unknown control index .*dca-gain, dca-pan or filter-cutoff"):
            make(welsh, T.CTL_SAMPLER_GAIN)
        for index in (T.CTL_FX_CEILING, 47, 52, 63, 65, 99):
            with pytest.raises(_lib.GrooveError, match=who + ": unknown control index .*FM bank"):
                make(fm, index)
            with pytest.raises(_lib.GrooveError, match=who + ": unknown control index .*sampler bank"):
                make(sampler, index)
        for n_src in (2, 3, 5):                                          # neither 1 nor the four voices
            with pytest.raises(_lib.GrooveError, match=who + ": n_src must be the bank's voice count, or 1"):
                make(fm, T.CTL_FM_DEPTH, n_src)
            with pytest.raises(_lib.GrooveError, match=who + ": n_src must be the bank's voice count, or 1"):
                make(sampler, T.CTL_SAMPLER_GAIN, n_src)
        with pytest.raises(_lib.GrooveError, match=who + ": n_src must be 1"):
            make(welsh, T.CTL_WELSH_DCA_PAN, 8)
        for target, index in ((fm, T.CTL_FM_BETA), (sampler, T.CTL_SAMPLER_GAIN)):
            make(target, index, 4).destroy()                               # one lane per voice is accepted
    # groove_bank_set_param
    for target in (fm, sampler):
        with pytest.raises(_lib.GrooveError, match="^groove_bank_set_param: only Welsh banks expose controls"):
            target.control_set_param_by_index(T.CTL_WELSH_DCA_GAIN, 0.5)
    with pytest.raises(_lib.GrooveError, match="groove_bank_set_param: an FM bank's controls are 48 - 51"):
        fm.control_set_param_by_index(T.CTL_SAMPLER_GAIN, 0.5)
    with pytest.raises(_lib.GrooveError, match="groove_bank_set_param: a sampler bank's control is 64"):
        sampler.control_set_param_by_index(T.CTL_FM_DEPTH, 0.5)
    with pytest.raises(_lib.GrooveError, match="groove_bank_set_param: unknown control index"):
        fm.control_set_param_by_index(7, 0.5)
    with pytest.raises(_lib.GrooveError, match="groove_bank_set_param: unknown control index"):
        welsh.control_set_param_by_index(T.CTL_FM_DEPTH, 0.5)
    with pytest.raises(_lib.GrooveError, match="groove_bank_set_param: voice out of range"):
        fm.control_set_param_by_index(T.CTL_FM_DEPTH, 0.5, voice=4)
    # a dead bank
    t, l = trip(fm, T.CTL_FM_DEPTH), link(sampler, T.CTL_SAMPLER_GAIN)
    t.work(0); l.work(0)
    fm.destroy(); sampler.destroy()
    with pytest.raises(_lib.GrooveError, match="groove_ctl_trip_apply: the target bank has been destroyed"):
        t.work(64)
    with pytest.raises(_lib.GrooveError, match="groove_ctl_link_apply: the target bank has been destroyed"):
        l.work(64)
    _clean(gpu_ctx)
    for x in (t, l, welsh):
        x.destroy()
