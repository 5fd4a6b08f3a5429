"""GPU tier: control links and trips onto a Welsh bank's dca-gain, dca-pan and filter-cutoff, resident on the device
(include/groove_hip.h groove_ctl_bank_link_create / groove_ctl_bank_trip_create; csrc/ctl_link.h ctl_bank_apply_kernel,
ctl_trip_bank_apply_kernel; csrc/ctl_core.h ctl_bank_*_f64, pan_gains).

Three arms, as tests/test_gpu_ctl_trips.py has them.  Arm A is a bank with a device link.  Arm B is the path that exists without it: the
host evaluates the source's law (tests/ctl_bank_law.py) and calls groove_bank_set_param on all voices, only while a step holds.  O is
the f64 oracle's bank given the same set_param.  A and B against O: that of tests/test_gpu_random_inputs.py's control test — bus and
voices RMS <= 1e-5, every voice <= 2e-4.  A against B bit for bit in every block whose start lies in a flat or slope step or outside the
trip, at look-ahead 1 like the bit-identity tests across forms; in a logarithmic or exponential step the device's log10 may differ from
the C library's in the last place: the number of such blocks that differ is printed and may be at most one in ten, and once one HAS
differed the parameter it left differs too, so the later blocks of that run are held to the oracle only.

Every test ends on zero_segments == 0 and fast_table_misses == 0: the apply writes the records the wave-uniform kernels read, and a
record torn under a running wave is what those two counters have caught before."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from groove_amd import abi_types as T, lib as _lib, patches as P
from tests import ctl_bank_law as LAW
from tests.test_ctl_core_cpu import shim, signal_law_np  # noqa: F401  (shim: the fixture that compiles csrc/ctl_core.h for the host)

pytestmark = pytest.mark.gpu

FORMS = {"tp": "welsh_tp_kernel", "any": "uniform_any_kernel", "split": "split4_kernel", "per-kind": "one launch per base kind"}
PARAMS = ("gain", "pan", "cutoff")
SR = 44100.0


@contextlib.contextmanager
def _forced(ctx, form, look=1):
    """The three context knobs tests/test_gpu_random_inputs.py forces a kernel form with (None: the defaults), restored on the way out."""
    old = (ctx.time_parallel_max_voices, ctx.split_max_waves, ctx.pipeline_min_waves)
    try:
        if form is not None:
            ctx.time_parallel_max_voices = old[0] if form == "tp" else 0
            ctx.split_max_waves = (1 << 20) if form == "split" else 0
            ctx.pipeline_min_waves = 1 if form == "per-kind" else old[2]
        ctx.look_ahead = look
        yield
    finally:
        ctx.time_parallel_max_voices, ctx.split_max_waves, ctx.pipeline_min_waves = old
        ctx.look_ahead = 3


def _clean(ctx):
    info = ctx.debug_info()
    assert info["zero_segments"] == 0 and info["fast_table_misses"] == 0, info


def _same(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float32).view(np.uint32), np.asarray(b, dtype=np.float32).view(np.uint32))


def _keys(n):
    return (36 + (7 * np.arange(n)) % 49).astype(np.uint8)


class Shape:
    """A bank, its blocks and the trip times of the blocks; the oracle's render for each parameter is made once and shared."""

    def __init__(self, name, params, sizes, ats, on_blocks=(0,), off_block=None):
        self.name, self.params, self.n, self.sizes, self.ats = name, params, len(params), sizes, ats
        self.on_blocks, self.off_block = on_blocks, off_block
        self.lanes, self.keys = np.arange(self.n, dtype=np.uint32), _keys(self.n)
        self._want = {}

    def events(self, b):
        out = []
        if b in self.on_blocks:
            out.append(T.note_events_np(self.lanes, self.keys, True))
        if b == self.off_block:
            out.append(T.note_events_np(self.lanes, self.keys, False))
        return out

    def values(self, param):
        if param is None:                       # the uncontrolled bank
            return [None] * len(self.ats)
        steps = LAW.steps_for(param)
        return [LAW.trip_value(LAW.MAIN_START, steps, at) for at in self.ats]

    def want(self, oracle, param):
        if param not in self._want:
            ob = oracle.Bank.welsh(self.params)
            out = []
            for b, (fr, v) in enumerate(zip(self.sizes, self.values(param))):
                for ev in self.events(b):
                    ob.note_events(ev)
                if v is not None:
                    ob.set_param(LAW.INDEX[param], v)
                out.append(ob.render(fr))
            w = np.concatenate(out, axis=1)
            w.setflags(write=False)
            assert np.sqrt(np.mean(w ** 2)) > 1e-2
            self._want[param] = w
        return self._want[param]


_SHAPES = {}


def _shape(name):
    if name not in _SHAPES:
        if name == "main":          # 32 patches in runs of three; ragged blocks; note-off mid-way, a re-trigger later
            s = Shape(name, P.welsh_voices_grouped(96)[0], LAW.MAIN_SIZES, LAW.main_ats(), LAW.NOTE_ON_BLOCKS, LAW.NOTE_OFF_BLOCK)
        elif name == "2x70":        # two patches x 70 voices: waves of 64 + 6, padding waves — the per-wave copy
            table = [P.welsh_patch(2), P.welsh_patch(11)]
            s = Shape(name, (T.WelshParams * 140)(*[table[i // 70] for i in range(140)]), [256, 100, 37, 256, 1, 256, 256, 100],
                      [0, 400, 1000, 1200, 1800, 2600, 4400, 6000])
        else:                       # 4,096 voices of two patches interleaved voice by voice: kept patch-major inside the library
            table = [P.welsh_patch(2), P.welsh_patch(11)]
            s = Shape(name, (T.WelshParams * 4096)(*[table[i % 2] for i in range(4096)]), [64] * 6, [0, 400, 1200, 1800, 2600, 6000])
        _SHAPES[name] = s
    return _SHAPES[name]


def _bars(got, want, what):
    """tests/test_gpu_random_inputs.py's bars for a controlled, sounding bank."""
    n = want.shape[2]
    got = got.astype(np.float64)
    per_voice = np.sqrt(np.mean((got - want) ** 2, axis=(0, 1)))
    voices = float(np.sqrt(np.mean((got - want) ** 2)))
    bus = float(np.sqrt(np.mean(((got - want).sum(axis=2) / n) ** 2)))
    print(f"{what}: voices RMS {voices:.3e}  bus RMS {bus:.3e}  worst voice {float(per_voice.max()):.3e} (voice {int(np.argmax(per_voice))})")
    assert np.isfinite(got).all(), what
    assert voices <= 1e-5 and bus <= 1e-5 and per_voice.max() <= 2e-4, (what, voices, bus, float(per_voice.max()))


def _blocks_of(ctx, synth, shape, before_block, render_async=False):
    """The bank's blocks [2][frames][n], block by block: events, before_block(b) — the arm's control — and the render."""
    blks = [ctx.block(shape.n, 256) for _ in range(2 if render_async else 1)]
    out = []
    for b, fr in enumerate(shape.sizes):
        for ev in shape.events(b):
            synth.handle_midi_events(ev)
        before_block(b)
        blk = blks[b % len(blks)]
        if render_async:    # the render of block b is on its side stream while the host reads block b - 1 and applies b + 1's control
            synth.generate_batch_values_async(blk, fr)
            if b:
                out.append(blks[(b - 1) % 2].download(shape.sizes[b - 1]))
        else:
            synth.generate_batch_values(blk, fr)
            out.append(blk.download(fr))
    if render_async:
        out.append(blks[(len(shape.sizes) - 1) % 2].download(shape.sizes[-1]))
    for blk in blks:
        blk.destroy()
    return out


def _three_arms(ctx, oracle, shape, param, form, render_async=False):
    from groove_amd import entities as E
    index, steps, vals = LAW.INDEX[param], LAW.steps_for(param), shape.values(param)
    want = shape.want(oracle, param)
    with _forced(ctx, form):
        a, b = E.WelshSynth(ctx, shape.params), E.WelshSynth(ctx, shape.params)
        trip = E.ControlTripLink(ctx, [steps], LAW.MAIN_START, a, index)
        if form is not None:
            for s in (a, b):
                assert FORMS[form] in s.kernel_form(256, False), (form, s.kernel_form(256, False))
        ga = _blocks_of(ctx, a, shape, lambda k: trip.work(shape.ats[k]), render_async)
        gb = _blocks_of(ctx, b, shape, lambda k: vals[k] is not None and b.control_set_param_by_index(index, vals[k]))
        _clean(ctx)
        for x in (trip, a, b):
            x.destroy()
    what = f"{param} on {shape.name}, form {form or 'default'}" + (", asynchronous renders" if render_async else "")
    _bars(np.concatenate(gb, axis=1), want, what + ": B against O")
    _bars(np.concatenate(ga, axis=1), want, what + ": A against O")
    curved = differing = 0
    diverged = False
    for k, at in enumerate(shape.ats):
        i = LAW.scan(LAW.MAIN_START, steps, at)[0]
        if i >= 0 and steps[i][0] in LAW.CURVED:
            curved += 1
            if not _same(ga[k], gb[k]):
                differing, diverged = differing + 1, True
        elif not diverged:
            assert _same(ga[k], gb[k]), ("a flat / slope / outside block differs between the arms", what, k, at, i)
    print(f"{what}: {differing} of {curved} logarithmic / exponential blocks differ between the arms" +
          ("; the blocks after the first of them were held to the oracle only" if diverged else ""))
    assert differing * 10 <= curved, (what, differing, curved)
    # the control is heard: the arms move away from the uncontrolled oracle
    return ga


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("param", PARAMS)
def test_trip_in_every_kernel_form_three_arms(gpu_ctx, oracle, param, form):
    shape = _shape("main")
    where = [LAW.scan(LAW.MAIN_START, LAW.steps_for(param), at)[0] for at in shape.ats]
    assert where[:3] == [-1, -1, 0] and where[4:6] == [0, 1] and where[-2:] == [-1, -1]   # two before, one on a boundary, two after
    assert where.count(2) == 5 and where.count(3) == 5
    _three_arms(gpu_ctx, oracle, shape, param, form)


@pytest.mark.parametrize("form", [None, "any"], ids=["default", "any"])
@pytest.mark.parametrize("param", PARAMS)
@pytest.mark.parametrize("name", ["2x70", "4096"])
def test_partial_and_padding_waves_and_a_lane_permutation(gpu_ctx, oracle, name, param, form):
    """On the default form, and — banks this small render time-parallel by default, from the per-lane array alone — on the all-kinds
    kernel, which reads the per-wave copies."""
    shape = _shape(name)
    where = [LAW.scan(LAW.MAIN_START, LAW.steps_for(param), at)[0] for at in shape.ats]
    assert where[0] == -1 and where[-1] == -1 and {0, 1, 2} <= set(where)
    _three_arms(gpu_ctx, oracle, shape, param, form)


def test_the_trip_is_heard_and_asynchronous_renders_give_the_same_bits(gpu_ctx, oracle):
    """Blocks rendered on the side streams (groove_bank_render_async, two blocks in rotation) while the host applies the next block's
    value: the apply joins them by events, and every block has the bits of the synchronous walk."""
    shape = _shape("main")
    for form in ("any", "per-kind"):
        sync = _three_arms(gpu_ctx, oracle, shape, "pan", form)
        asyn = _three_arms(gpu_ctx, oracle, shape, "pan", form, render_async=True)
        for k, (x, y) in enumerate(zip(sync, asyn)):
            assert _same(x, y), (form, k)
    assert np.abs(shape.want(oracle, "pan") - shape.want(oracle, None)).max() > 1e-3       # block 2 on: away from the patches' own pan


@pytest.mark.parametrize("param", PARAMS)
def test_fused_render_mix_onto_a_bus(gpu_ctx, oracle, param):
    """groove_bank_render_mix with two banks alive: the pipelined form, renders on side streams, one long bus and no host wait between
    arm A's blocks — its applies are ordered against its renders by events alone.  The bus bar is _check_mix_bus's: the per-voice 1e-5
    of each voice's level (full scale at least), added in quadrature."""
    from groove_amd import entities as E
    shape = _shape("main")
    index, steps, vals = LAW.INDEX[param], LAW.steps_for(param), shape.values(param)
    want = shape.want(oracle, param)
    total = sum(shape.sizes)
    with _forced(gpu_ctx, None):
        a, b = E.WelshSynth(gpu_ctx, shape.params), E.WelshSynth(gpu_ctx, shape.params)
        trip = E.ControlTripLink(gpu_ctx, [steps], LAW.MAIN_START, a, index)
        bus_a, bus_b = gpu_ctx.bus(total), gpu_ctx.bus(total)
        for synth, bus, control in ((a, bus_a, lambda k: trip.work(shape.ats[k])),
                                    (b, bus_b, lambda k: vals[k] is not None and b.control_set_param_by_index(index, vals[k]))):
            at = 0
            for k, fr in enumerate(shape.sizes):
                for ev in shape.events(k):
                    synth.handle_midi_events(ev)
                control(k)
                synth.render_mix(bus, fr, at_frame=at)
                at += fr
        ga, gb = bus_a.download().astype(np.float64), bus_b.download().astype(np.float64)
        _clean(gpu_ctx)
        for x in (trip, a, b, bus_a, bus_b):
            x.destroy()
    want_bus = want.sum(axis=2).T
    level = np.maximum(1.0, np.sqrt(np.mean(want ** 2, axis=(0, 1))))
    bar = 1e-5 * float(np.sqrt(np.sum(level ** 2)))
    err_a, err_b = (float(np.sqrt(np.mean((g - want_bus) ** 2))) for g in (ga, gb))
    print(f"fused {param}: |A - O| {err_a:.3e}  |B - O| {err_b:.3e}  bar {bar:.3e}")
    assert np.isfinite(ga).all() and np.isfinite(gb).all()
    assert err_b <= bar and err_a <= bar, (param, err_a, err_b, bar)
    if param != "cutoff":       # with a cutoff link arm A filters in f64 where arm B may have been measured into fp32
        at, diverged = 0, False
        for k, fr in enumerate(shape.sizes):
            i = LAW.scan(LAW.MAIN_START, steps, shape.ats[k])[0]
            same = _same(ga[at:at + fr], gb[at:at + fr])
            if i >= 0 and steps[i][0] in LAW.CURVED:
                diverged = diverged or not same
            elif not diverged:
                assert same, ("fused: a flat / slope / outside block differs between the arms", param, k)
            at += fr


def _source_arms(ctx, oracle, shape, a_control, values, what, bitwise):
    """Arm A under a_control(block, first frame), arm B and O fed values[block] (None: nothing) through set_param on dca-gain."""
    from groove_amd import entities as E
    index = T.CTL_WELSH_DCA_GAIN
    starts = np.concatenate([[0], np.cumsum(shape.sizes)[:-1]])
    ob = oracle.Bank.welsh(shape.params)
    want = []
    for k, fr in enumerate(shape.sizes):
        for ev in shape.events(k):
            ob.note_events(ev)
        if values[k] is not None:
            ob.set_param(index, values[k])
        want.append(ob.render(fr))
    want = np.concatenate(want, axis=1)
    a, b = E.WelshSynth(ctx, shape.params), E.WelshSynth(ctx, shape.params)
    link = a_control(a)
    ga = _blocks_of(ctx, a, shape, lambda k: link(k, int(starts[k])))
    gb = _blocks_of(ctx, b, shape, lambda k: values[k] is not None and b.control_set_param_by_index(index, values[k]))
    _clean(ctx)
    a.destroy(); b.destroy()
    _bars(np.concatenate(gb, axis=1), want, what + ": B against O")
    _bars(np.concatenate(ga, axis=1), want, what + ": A against O")
    equal = sum(_same(x, y) for x, y in zip(ga, gb))
    print(f"{what}: {equal} of {len(ga)} blocks have arm B's bits")
    if bitwise:
        assert equal == len(ga), what
    return ga


def test_lfo_source_onto_dca_gain(gpu_ctx, oracle, shim):
    """A sine at 5.3 Hz (a third of a turn over the 3,100 frames: 0.5 up to 1.0): the device's fp32 value01 against the host's own
    evaluation of the same text (bars against the oracle: the two may differ in the last place of the sine polynomial, contraction being
    on in device code).  A square's value — 53 Hz here, so that it switches — is 0 or 1 from the exact phase counter on both sides: there
    arm B receives the identical float and the blocks must agree bit for bit."""
    from groove_amd import entities as E
    shape = _shape("main")
    starts = np.concatenate([[0], np.cumsum(shape.sizes)[:-1]])
    with _forced(gpu_ctx, None):
        for wave, hz, bitwise in ((T.WAVE_SINE, 5.3, False), (T.WAVE_SQUARE, 53.0, True)):
            delta, duty = shim.shim_delta64(hz, SR), shim.shim_duty64(wave, 0.5)
            values = [float(shim.shim_lfo_value01(wave, delta, duty, int(n0))) for n0 in starts]
            assert max(values) - min(values) > 0.4
            links = []

            def control(a):
                links.append(E.ControlLink(gpu_ctx, LAW.lfo_source(hz, wave), a, T.CTL_WELSH_DCA_GAIN))
                return lambda k, n0: links[0].work(n0)

            _source_arms(gpu_ctx, oracle, shape, control, values, f"LFO waveform {wave} -> dca-gain", bitwise)
            links[0].destroy()


def test_signal_source_onto_dca_gain_and_nothing_before_a_capture(gpu_ctx, oracle):
    from groove_amd import entities as E
    shape = _shape("2x70")
    rng = np.random.default_rng(70)
    law = T.CTL_LAW_AMPLITUDE_INVERTED
    side = rng.uniform(-1.0, 1.0, (len(shape.sizes), 2, 8, 1)).astype(np.float32)      # one lane, 8 frames: frame 7 is kept
    values = [None, None] + [float(signal_law_np(law, side[k, 0, 7], side[k, 1, 7])[1][0]) for k in range(2, len(shape.sizes))]
    with _forced(gpu_ctx, None):
        links, blk = [], gpu_ctx.block(1, 8)

        def control(a):
            links.append(E.ControlLink(gpu_ctx, T.ctl_sources(1, source=T.CTL_SRC_SIGNAL, law=law), a, T.CTL_WELSH_DCA_GAIN))

            def work(k, n0):
                if k >= 2:                    # blocks 0 and 1: applied with nothing captured — the bank stays as it is
                    blk.upload(side[k])
                    links[0].capture(blk, 8)
                links[0].work(n0)
            return work

        ga = _source_arms(gpu_ctx, oracle, shape, control, values, "signal -> dca-gain", True)
        # ... bit for bit what an unlinked bank renders
        plain = E.WelshSynth(gpu_ctx, shape.params)
        gp = _blocks_of(gpu_ctx, plain, shape, lambda k: None)
        assert _same(ga[0], gp[0]) and _same(ga[1], gp[1]) and not _same(ga[2], gp[2])
        links[0].reset()
        _clean(gpu_ctx)
        for x in (links[0], blk, plain):
            x.destroy()


def test_set_param_overwrites_until_the_next_apply(gpu_ctx):
    """The staleness rule: a pan link, then set_param(ALL, gain) — the host's copy goes up again, with the HOST's pan; the link's next
    apply puts its pan back, over the new gain (the shadow was refreshed)."""
    from groove_amd import entities as E
    shape = _shape("2x70")
    n, fr = shape.n, 100
    flat = [(LAW.FLAT, 0.8, 0.8, 1.0)]
    with _forced(gpu_ctx, None):
        a, host_pan, both = (E.WelshSynth(gpu_ctx, shape.params) for _ in range(3))
        trip = E.ControlTripLink(gpu_ctx, [flat], 0.0, a, T.CTL_WELSH_DCA_PAN)
        blk = gpu_ctx.block(n, 256)

        def render(s):
            s.generate_batch_values(blk, fr)
            return blk.download(fr)

        for s in (a, host_pan, both):
            s.handle_midi_events(T.note_events_np(shape.lanes, shape.keys, True))
        trip.work(100)
        both.control_set_param_by_index(T.CTL_WELSH_DCA_PAN, 0.8)
        first = render(a)
        assert _same(first, render(both)) and not _same(first, render(host_pan))
        for s in (a, host_pan, both):
            s.control_set_param_by_index(T.CTL_WELSH_DCA_GAIN, 0.5)
        both.control_set_param_by_index(T.CTL_WELSH_DCA_PAN, 0.8)       # (its host copy already holds it: the same upload)
        stale, hp, bt = render(a), render(host_pan), render(both)
        assert _same(stale, hp) and not _same(stale, bt)                # the host copy's pan
        trip.work(200)
        again, hp, bt = render(a), render(host_pan), render(both)
        assert _same(again, bt) and not _same(again, hp)                # arm A again
        # two links onto one bank see each other's last value: a gain trip now, then the pan trip again
        gain = E.ControlTripLink(gpu_ctx, [[(LAW.FLAT, 0.25, 0.25, 1.0)]], 0.0, a, T.CTL_WELSH_DCA_GAIN)
        gain.work(300)
        both.control_set_param_by_index(T.CTL_WELSH_DCA_GAIN, 0.25)
        assert _same(render(a), render(both))
        trip.work(400)
        assert _same(render(a), render(both))
        _clean(gpu_ctx)
        for x in (trip, gain, blk, a, host_pan, both):
            x.destroy()


def test_applies_do_not_wait_on_the_host_and_set_param_does(gpu_ctx):
    from groove_amd import entities as E
    shape = _shape("main")
    a, b = E.WelshSynth(gpu_ctx, shape.params), E.WelshSynth(gpu_ctx, shape.params)
    trips = [E.ControlTripLink(gpu_ctx, [LAW.steps_for(p)], LAW.MAIN_START, a, LAW.INDEX[p]) for p in PARAMS]
    lfo = E.ControlLink(gpu_ctx, LAW.lfo_source(), a, T.CTL_WELSH_DCA_GAIN)
    blk = gpu_ctx.block(shape.n, 256)
    waits = lambda: gpu_ctx.debug_info()["host_waits"]
    a.handle_midi_events(T.note_events_np(shape.lanes, shape.keys, True))
    a.generate_batch_values_async(blk, 256)                        # a render in flight on a side stream
    before = waits()
    own = waits() - before                                          # what reading the counter costs by itself
    before = waits()
    for k in range(10):
        for t in trips:
            t.work(400 + k * 300)
        lfo.work(k * 256)
    assert waits() - before - own == 0                              # forty applies: not one host wait
    for p in PARAMS:
        before = waits()
        b.control_set_param_by_index(LAW.INDEX[p], 0.5)
        assert waits() - before - own >= 1, p
    blk.download(256)
    _clean(gpu_ctx)
    for x in trips + [lfo, blk, a, b]:
        x.destroy()


def test_refusals_each_with_its_message(gpu_ctx):
    from groove_amd import entities as E
    L = gpu_ctx.L
    welsh = E.WelshSynth(gpu_ctx, P.welsh_voices_grouped(8)[0])
    fm = E.FmSynth(gpu_ctx, P.fm_voices(4))
    pcm, descs, _ = P.drum_bank(scale=0.01)
    sampler = E.Sampler(gpu_ctx, pcm, descs, P.sampler_voices(4))
    ok = [(LAW.SLOPE, 0.1, 0.9, 1.0)]
    lfo = lambda n=1, **kw: T.ctl_sources(n, **dict(dict(source=T.CTL_SRC_LFO, waveform=T.WAVE_SINE, frequency_hz=1.0), **kw))
    link = lambda target, index, src=None: E.ControlLink(gpu_ctx, lfo() if src is None else src, target, index)
    trip = lambda target, index, lanes=None, starts=0.0: E.ControlTripLink(gpu_ctx, [ok] if lanes is None else lanes, starts, target, index)
    for make, who in ((link, "groove_ctl_bank_link_create"), (trip, "groove_ctl_bank_trip_create")):
        for target in (fm, sampler):
            with pytest.raises(_lib.GrooveError, match=who + ": only Welsh banks expose controls"):
                make(target, T.CTL_WELSH_DCA_GAIN)
        for index in (T.CTL_FX_CEILING, T.CTL_FX_CUTOFF, T.CTL_FX_WET, 31, 35, 99):
            with pytest.raises(_lib.GrooveError, match=who + ": unknown control index .*dca-gain, dca-pan or filter-cutoff"):
                make(welsh, index)
    # one source, broadcast
    with pytest.raises(_lib.GrooveError, match="groove_ctl_bank_link_create: n_src must be 1"):
        link(welsh, T.CTL_WELSH_DCA_PAN, lfo(8))
    with pytest.raises(_lib.GrooveError, match="groove_ctl_bank_trip_create: n_src must be 1"):
        trip(welsh, T.CTL_WELSH_DCA_PAN, [ok] * 8)
    # what the effect creates refuse of sources and steps
    for src, msg in ((lfo(waveform=T.WAVE_NOISE), "an LFO source is sine"), (lfo(waveform=T.WAVE_NONE), "an LFO source is sine"),
                     (lfo(waveform=12), "an LFO source is sine"), (lfo(frequency_hz=float("nan")), "LFO frequency outside"),
                     (lfo(frequency_hz=44100.0), "LFO frequency outside"), (T.ctl_sources(1, source=T.CTL_SRC_SIGNAL, law=3), "unknown signal law"),
                     (T.ctl_sources(1, source=7), "unknown source kind")):
        with pytest.raises(_lib.GrooveError, match="groove_ctl_bank_link_create: " + msg):
            link(welsh, T.CTL_WELSH_DCA_GAIN, src)
    inf, nan = float("inf"), float("nan")
    for lanes, starts, msg in (([[]], 0.0, "at least one step"), ([ok * 65537], 0.0, "more than 65,536 steps"),
                               ([[(LAW.SLOPE, 0.1, 0.9, 0.0)]], 0.0, "beats must be > 0"), ([[(LAW.SLOPE, 0.1, 0.9, nan)]], 0.0, "beats, start or end is not finite"),
                               ([[(LAW.SLOPE, inf, 0.9, 1.0)]], 0.0, "beats, start or end is not finite"), ([[(LAW.SLOPE, 0.1, -inf, 1.0)]], 0.0, "beats, start or end is not finite"),
                               ([ok], nan, "start_beat is not finite"), ([[(4, 0.1, 0.9, 1.0)]], 0.0, "unknown step kind")):
        with pytest.raises(_lib.GrooveError, match="groove_ctl_bank_trip_create: .*" + msg):
            trip(welsh, T.CTL_WELSH_CUTOFF, lanes, starts)
    assert trip(welsh, T.CTL_WELSH_CUTOFF, [ok * 65536]).destroy() is None               # 65,536 steps are accepted
    # NULL arguments
    steps, n_steps = T.ctl_steps([ok])
    out = C.c_void_p()
    with pytest.raises(_lib.GrooveError, match="groove_ctl_bank_link_create: NULL argument"):
        _lib.check(L.groove_ctl_bank_link_create(gpu_ctx.h, lfo(), 1, None, T.CTL_WELSH_DCA_GAIN, C.byref(out)), gpu_ctx.h)
    with pytest.raises(_lib.GrooveError, match="groove_ctl_bank_trip_create: NULL argument"):
        _lib.check(L.groove_ctl_bank_trip_create(gpu_ctx.h, steps, n_steps, (C.c_double * 1)(0.0), 1, None, T.CTL_WELSH_DCA_GAIN, C.byref(out)), gpu_ctx.h)
    # the existing calls under their own rules
    t, l = trip(welsh, T.CTL_WELSH_DCA_PAN), link(welsh, T.CTL_WELSH_DCA_GAIN)
    side = gpu_ctx.block(1, 8)
    with pytest.raises(_lib.GrooveError, match="groove_ctl_link_apply: a trip link .*groove_ctl_trip_apply"):
        _lib.check(L.groove_ctl_link_apply(t.h, 0), gpu_ctx.h)
    with pytest.raises(_lib.GrooveError, match="groove_ctl_link_capture: a trip link captures nothing"):
        _lib.check(L.groove_ctl_link_capture(t.h, side.h, 8), gpu_ctx.h)
    with pytest.raises(_lib.GrooveError, match="groove_ctl_trip_apply: not a trip link"):
        _lib.check(L.groove_ctl_trip_apply(l.h, 0), gpu_ctx.h)
    with pytest.raises(_lib.GrooveError, match="groove_ctl_link_capture: not a signal link"):
        l.capture(side, 8)
    sig = link(welsh, T.CTL_WELSH_DCA_GAIN, T.ctl_sources(1, source=T.CTL_SRC_SIGNAL, law=T.CTL_LAW_BIPOLAR))
    wide = gpu_ctx.block(8, 8)
    with pytest.raises(_lib.GrooveError, match="groove_ctl_link_capture: block lanes != source lanes"):
        sig.capture(wide, 8)                                            # a signal link's capture block has one lane
    t.reset(); l.reset(); t.work(0); l.work(0)
    # a dead bank
    dead = C.c_void_p(welsh.h.value)                                   # (only compared with the live banks' handles, never followed)
    welsh.destroy()
    with pytest.raises(_lib.GrooveError, match="groove_ctl_trip_apply: the target bank has been destroyed"):
        t.work(64)
    with pytest.raises(_lib.GrooveError, match="groove_ctl_link_apply: the target bank has been destroyed"):
        l.work(64)
    with pytest.raises(_lib.GrooveError, match="groove_ctl_bank_trip_create: the target is not a live bank"):
        _lib.check(L.groove_ctl_bank_trip_create(gpu_ctx.h, steps, n_steps, (C.c_double * 1)(0.0), 1, dead, T.CTL_WELSH_CUTOFF, C.byref(out)), gpu_ctx.h)
    with pytest.raises(_lib.GrooveError, match="groove_ctl_bank_link_create: the target is not a live bank"):
        _lib.check(L.groove_ctl_bank_link_create(gpu_ctx.h, lfo(), 1, dead, T.CTL_WELSH_CUTOFF, C.byref(out)), gpu_ctx.h)
    _clean(gpu_ctx)
    for x in (t, l, sig, side, wide, fm, sampler):
        x.destroy()


@pytest.mark.parametrize("form", [None, "any", "per-kind"])
def test_a_cutoff_link_comes_and_goes_without_disturbing_sounding_voices(gpu_ctx, oracle, form):
    """Creating the first cutoff link re-plans the bank without WF_FILTER_F32, destroying the last one re-plans it with: render, create
    (no apply), render, destroy, render — every stretch on the oracle of the untouched bank, voice by voice and on the fused bus."""
    from groove_amd import entities as E
    shape = _shape("main")
    fr = 256
    ob = oracle.Bank.welsh(shape.params)
    ob.note_events(T.note_events_np(shape.lanes, shape.keys, True))
    want = ob.render(4 * fr)
    with _forced(gpu_ctx, form, look=3):
        for fused in (False, True):
            s = E.WelshSynth(gpu_ctx, shape.params)
            blk, bus = gpu_ctx.block(shape.n, fr), gpu_ctx.bus(4 * fr)
            s.handle_midi_events(T.note_events_np(shape.lanes, shape.keys, True))
            out = []

            def render(k):
                if fused:
                    s.render_mix(bus, fr, at_frame=k * fr)
                else:
                    s.generate_batch_values(blk, fr)
                    out.append(blk.download(fr))

            render(0)
            first = E.ControlTripLink(gpu_ctx, [LAW.steps_for("cutoff")], LAW.MAIN_START, s, T.CTL_WELSH_CUTOFF)
            render(1)
            second = E.ControlLink(gpu_ctx, LAW.lfo_source(), s, T.CTL_WELSH_CUTOFF)
            first.destroy()                                         # one of two: the bank stays on the f64 filter
            render(2)
            second.destroy()                                        # the last one
            render(3)
            if fused:
                got = bus.download().astype(np.float64)
                level = np.maximum(1.0, np.sqrt(np.mean(want ** 2, axis=(0, 1))))
                err = float(np.sqrt(np.mean((got - want.sum(axis=2).T) ** 2)))
                print(f"cutoff link lifetime, form {form or 'default'}, fused: |bus - O| {err:.3e}")
                assert np.isfinite(got).all() and err <= 1e-5 * float(np.sqrt(np.sum(level ** 2))), (form, err)
            else:
                _bars(np.concatenate(out, axis=1), want, f"cutoff link lifetime, form {form or 'default'}")
            _clean(gpu_ctx)
            for x in (blk, bus, s):
                x.destroy()
