"""GPU tier: links and trips onto wet-dry-mix, resident on the device (include/groove_hip.h groove_ctl_wet_link_create /
groove_ctl_wet_trip_create).

Two effects of the same parameters run on the same noise, block after block.  Arm A has a wet link or a wet trip.  Arm B is the path
that exists without it: groove_fx_set_param(lane, GROOVE_CTL_FX_WET, v).  O is the f64 oracle's effect with the same wet-dry mix.

Where v comes from: a signal link's from the numpy law tests/test_ctl_core_cpu.py holds the device's to bit for bit; a trip's from
tests/ctl_trip_law.py, the host trip restated; a square or pulse-width LFO's from the closed form, which is exact.  A smooth LFO
waveform's closed form is the device's value only to 2e-7 (tests/test_ctl_core_cpu.py), which cannot carry an assertion about bits: its
v is read back from the device — the same sources linked onto a Gain's ceiling, whose law is the same `value itself`
(csrc/ctl_core.h ctl_target_float) — and held to the closed form at that 2e-7.

Every LFO, signal, flat, slope and outside block must come out of both arms bit for bit — for a reverb target that is why a set-param
arm that takes the all-wet run whenever every lane is at 1 must equal a link arm that never does.  Logarithmic and exponential blocks:
tests/test_gpu_ctl_trips.py's condition (at most one in ten may differ; after a difference the later blocks are held to the oracle
only).  Both arms: within tests/test_gpu_ctl_trips.py's bar of the oracle, 4e-6 of the larger of 1 and the output's peak."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from groove_amd import abi_types as T, lib as _lib
from tests import ctl_trip_law as LAW, fx_forms as F
from tests.test_ctl_core_cpu import signal_law_np
from tests.test_gpu_ctl_filter_links import BAR
from tests.test_gpu_ctl_links import _Probe, _audio, _lfo_sources, _lfo_want, _params

pytestmark = pytest.mark.gpu

CAP, BLOCKS = 64, LAW.MAIN_BLOCKS
LP = dict(cutoff_hz=1000.0, q=0.9, passband_ripple=1.1)
TARGETS = {"gain": (T.FX_GAIN, dict(ceiling=0.75)),
           "delay-run": (T.FX_DELAY, dict(delay_seconds=0.012)),         # a stage of the fused run at 64 frames
           "delay-serial": (T.FX_DELAY, dict(delay_seconds=0.0002)),     # nine frames: the serial kernel
           "lp12": (T.FX_BIQUAD_LP12, LP), "lp24": (T.FX_BIQUAD_LP24, LP),
           "compressor": (T.FX_COMPRESSOR, dict(limit_min=0.3, limit_max=0.25)),
           "reverb": (T.FX_REVERB, dict(attenuation=0.9, reverb_seconds=0.4))}
FORM = {"gain": F.RUN, "delay-run": F.RUN, "delay-serial": F.D1, "lp12": F.BQ_TP, "lp24": F.LP_TP, "compressor": F.RUN}
# (target, the run knob, the all-pass stream)
CASES = [(k, False, False) for k in TARGETS if k != "reverb"] + [("reverb", run, ap) for run in (False, True) for ap in (False, True)]
SOURCES = ["lfo-per-lane", "lfo-square-broadcast", "signal", "trip"]
SQUARE_HZ = 44100.0 / (CAP * 6)      # a square LFO that flips every three blocks: wet exactly 1 and exactly 0
CURVED = (LAW.LOG, LAW.EXP)


def _mk(n, target, wet=None):
    kw = dict(TARGETS[target][1])
    if wet is not None:
        kw["wet"] = [float(w) for w in wet]
    return _params(n, **kw)


@contextlib.contextmanager
def _knobs(ctx, run, ap):
    assert not ctx.fx_wet_reverb_run and not ctx.fx_allpass_stream
    try:
        ctx.fx_allpass_stream = ap
        ctx.fx_wet_reverb_run = run
        yield
    finally:
        ctx.fx_wet_reverb_run = False
        ctx.fx_allpass_stream = False


def _run(block, fx, x):
    block.upload(x)
    fx.transform_audio(block, x.shape[1])
    return block.download(x.shape[1])


def _same(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


class _Source:
    """One control source in both forms: the link onto arm A's effect, and per block the values the host path would set (None: the
    block leaves the target untouched) with the index of the trip step that holds the block (-1: none or no trip)."""

    def __init__(self, ctx, mode, n, fx, rng):
        from groove_amd import entities as E
        self.ctx, self.mode, self.n, self.rng = ctx, mode, n, rng
        self.extra = []
        if mode == "lfo-per-lane":
            arr, self.desc = _lfo_sources(n)
            self.link = fx.link_wet(arr)
            arr2, _ = _lfo_sources(n)
            self.gain = E.Effect(ctx, T.FX_GAIN, _params(n, ceiling=0.5))          # reads the device's LFO values back (module docstring)
            self.glink = E.ControlLink(ctx, arr2, self.gain, T.CTL_FX_CEILING)
            self.probe = _Probe(ctx, n, 1.0)
            self.extra = [self.glink, self.gain, self.probe]
        elif mode == "lfo-square-broadcast":
            self.link = fx.link_wet(T.ctl_sources(1, source=T.CTL_SRC_LFO, waveform=T.WAVE_SQUARE, frequency_hz=SQUARE_HZ))
        elif mode == "signal":
            self.link = fx.link_wet(T.ctl_sources(n, source=T.CTL_SRC_SIGNAL, law=T.CTL_LAW_AMPLITUDE))
            self.side = ctx.block(n, CAP)
            self.captured = None
            self.extra = [self.side]
        else:
            self.link = fx.trip_wet([LAW.MAIN_STEPS], LAW.MAIN_START)

    def work(self, k):
        """The control phase of block k on arm A; returns (values for arm B: None, one number, or one per lane; the trip step)."""
        if self.mode == "lfo-per-lane":
            at = k * CAP * 37
            self.link.work(at)
            self.glink.work(at)
            v = self.probe.read(self.gain)
            want = _lfo_want(self.desc, at)
            assert np.abs(v.astype(np.float64) - want).max() <= 2e-7
            edge = np.array([w in (T.WAVE_SQUARE, T.WAVE_PULSE_WIDTH) for w, _, _ in self.desc])
            assert np.array_equal(v[edge].astype(np.float64), want[edge])
            return v, -1
        if self.mode == "lfo-square-broadcast":
            self.link.work(k * CAP)
            v = float(_lfo_want([(T.WAVE_SQUARE, 0.5, SQUARE_HZ)], k * CAP)[0])
            assert v in (0.0, 1.0)
            return v, -1
        if self.mode == "signal":
            self.link.work(k * CAP)
            return self.captured, -1
        at = k * LAW.BLOCK_UNITS
        self.link.work(at)
        return LAW.trip_value(LAW.MAIN_START, LAW.MAIN_STEPS, at), LAW.scan(LAW.MAIN_START, LAW.MAIN_STEPS, at)[0]

    def after_block(self):
        """A signal source's transform_audio: the side block of this tick is what the next tick's work hands on."""
        if self.mode != "signal":
            return
        x = self.rng.uniform(-1.2, 1.2, (2, CAP, self.n)).astype(np.float32)
        self.side.upload(x)
        self.link.capture(self.side, CAP)
        _, self.captured = signal_law_np(T.CTL_LAW_AMPLITUDE, x[0, CAP - 1, :], x[1, CAP - 1, :])

    def destroy(self):
        for x_ in [self.link] + self.extra:
            x_.destroy()


def _compare(gpu_ctx, oracle, target, run, ap, mode, n):
    from groove_amd import entities as E
    kind = TARGETS[target][0]
    rng = np.random.default_rng(4000 + 131 * kind + 7 * SOURCES.index(mode) + n + 2 * run + ap)
    forms = F.library_forms()
    with _knobs(gpu_ctx, run, ap):
        a, b = E.Effect(gpu_ctx, kind, _mk(n, target)), E.Effect(gpu_ctx, kind, _mk(n, target))
        ofx = oracle.Fx(kind, _mk(n, target))
        src = _Source(gpu_ctx, mode, n, a, rng)
        ia, ib = gpu_ctx.block(n, CAP), gpu_ctx.block(n, CAP)
        ia.release(); ib.release()                                     # (they have their events: a reverb may leave for the all-pass stream)
        if target == "reverb":
            tag_a = (F.DIR_AP if ap else F.DIR) if run else F.R8       # the link arm never takes the all-wet run
        else:
            tag_a = FORM[target] if n <= 1024 else None
        cur = np.ones(n, np.float32)
        curved = differing = 0
        diverged = False
        seen = set()
        for k in range(BLOCKS):
            x = _audio(rng, n, CAP)
            v, step = src.work(k)
            if v is not None:
                if np.ndim(v) == 0:
                    b.control_set_param_by_index(T.CTL_FX_WET, v)
                    cur[:] = np.float32(min(max(v, 0.0), 1.0))
                else:
                    for lane in range(n):
                        b.control_set_param_by_index(T.CTL_FX_WET, float(v[lane]), lane=lane)
                    cur[:] = v
            seen.update(cur.tolist())
            if tag_a is not None:
                assert a.kernel_form(ia, CAP) == F.form_of_tag(tag_a, forms), (target, run, ap, mode, k)
            if target == "reverb" and not run:
                assert b.kernel_form(ib, CAP) == F.form_of_tag(F.R8 if (cur < 1.0).any() else F.DIR_AP if ap else F.DIR, forms)
            ga, gb = _run(ia, a, x), _run(ib, b, x)
            src.after_block()
            ofx.set_params(_mk(n, target, wet=cur))
            want = ofx.process(x.astype(np.float64))
            bar = BAR * max(1.0, float(np.abs(want).max()))
            err_a, err_b = float(np.abs(ga - want).max()), float(np.abs(gb - want).max())
            assert err_b <= bar, ("B against O", target, mode, k, err_b, bar)
            assert err_a <= bar, ("A against O", target, mode, k, err_a, bar)
            if step >= 0 and LAW.MAIN_STEPS[step][0] in CURVED:
                curved += 1
                if not _same(ga, gb):
                    differing += 1
                    diverged = True
            elif not diverged:
                assert _same(ga, gb), ("an LFO / signal / flat / slope / outside block differs between the arms", target, run, ap, mode, n, k)
        print(f"wet-dry-mix -> {target} (run knob {run}, all-pass stream {ap}), {mode}, {n} lanes: {differing} of {curved} logarithmic / "
              f"exponential blocks differ between the arms" + ("; the blocks after the first of them were held to the oracle only" if diverged else ""))
        assert differing * 10 <= curved
        if mode == "trip":
            assert curved == 15
        if mode == "lfo-square-broadcast":
            assert seen == {0.0, 1.0}
        else:
            assert any(0.0 < w < 1.0 for w in seen)
        assert gpu_ctx.debug_info()["zero_segments"] == 0
        src.destroy()
        for x_ in (ia, ib, a, b):
            x_.destroy()


@pytest.mark.parametrize("mode", SOURCES)
@pytest.mark.parametrize("target,run,ap", CASES, ids=[f"{t}{'-run' if r else ''}{'-ap' if p else ''}" for t, r, p in CASES])
def test_wet_link_against_set_param_and_the_oracle(gpu_ctx, oracle, target, run, ap, mode):
    """65 lanes (scalar accesses in the fused run), 30 blocks of 64 frames: the trip tests' geometry."""
    _compare(gpu_ctx, oracle, target, run, ap, mode, 65)


@pytest.mark.parametrize("target,run,ap,mode", [("reverb", True, True, "lfo-per-lane"), ("reverb", True, False, "trip"), ("delay-run", False, False, "signal")])
def test_72_lanes_take_the_16_byte_accesses(gpu_ctx, oracle, target, run, ap, mode):
    _compare(gpu_ctx, oracle, target, run, ap, mode, 72)


def test_applies_and_captures_do_not_wait_on_the_host(gpu_ctx):
    """Forty applies and ten captures with a chain in flight: not one host wait, where one groove_fx_set_param has at least one."""
    from groove_amd import entities as E
    n = 65
    with _knobs(gpu_ctx, True, True):
        chain = [E.Effect(gpu_ctx, T.FX_GAIN, _mk(n, "gain")), E.Effect(gpu_ctx, T.FX_DELAY, _mk(n, "delay-run")), E.Effect(gpu_ctx, T.FX_REVERB, _mk(n, "reverb"))]
        links = [chain[0].link_wet(T.ctl_sources(1, source=T.CTL_SRC_LFO, waveform=T.WAVE_SINE, frequency_hz=3.0)),
                 chain[2].link_wet(_lfo_sources(n)[0])]
        sig = chain[1].link_wet(T.ctl_sources(n, source=T.CTL_SRC_SIGNAL, law=T.CTL_LAW_BIPOLAR))
        trip = chain[2].trip_wet([LAW.MAIN_STEPS], LAW.MAIN_START)
        blocks = [gpu_ctx.block(n, CAP) for _ in range(10)]
        side = gpu_ctx.block(n, CAP)
        x = _audio(np.random.default_rng(9), n, CAP)
        side.upload(x)
        for blk in blocks:
            blk.release()
            blk.upload(x)
        waits = lambda: gpu_ctx.debug_info()["host_waits"]
        a = waits()
        own = waits() - a                                                # what reading the counter costs by itself
        a = waits()
        for k, blk in enumerate(blocks):
            for l in links:
                l.work(k * CAP)
            sig.work(k * CAP)
            trip.work(k * LAW.BLOCK_UNITS + 400)
            gpu_ctx.transform_chain(chain, blk, CAP)
            sig.capture(side, CAP)
        assert waits() - a - own == 0
        a = waits()
        chain[2].control_set_param_by_index(T.CTL_FX_WET, 0.5)
        assert waits() - a - own >= 1
        assert np.isfinite(blocks[-1].download(CAP)).all()
        assert gpu_ctx.debug_info()["zero_segments"] == 0
        for x_ in links + [sig, trip, side] + blocks + chain:
            x_.destroy()


def test_a_reverb_counts_its_live_wet_links(gpu_ctx):
    """While a wet link lives the reverb is not all wet, whatever the host's copy says: serial with the run knob off, the run's form with
    it on.  Once the last link is destroyed and set_param(WET, 1.0) has been applied it reports the all-wet form again.  A link that
    outlives its effect is destroyed without touching it."""
    from groove_amd import entities as E
    n = 12
    forms = F.library_forms()
    blk = gpu_ctx.block(n, CAP)
    rv = E.Effect(gpu_ctx, T.FX_REVERB, _mk(n, "reverb"))
    form = lambda: rv.kernel_form(blk, CAP)
    direct, serial = F.form_of_tag(F.DIR, forms), F.form_of_tag(F.R8, forms)
    assert not gpu_ctx.fx_wet_reverb_run and form() == direct
    l1 = rv.link_wet(T.ctl_sources(1, source=T.CTL_SRC_LFO, waveform=T.WAVE_SQUARE, frequency_hz=SQUARE_HZ))
    l2 = rv.trip_wet([LAW.MAIN_STEPS], LAW.MAIN_START)
    assert form() == serial
    try:
        gpu_ctx.fx_wet_reverb_run = True
        assert form() == direct
    finally:
        gpu_ctx.fx_wet_reverb_run = False
    assert _lfo_want([(T.WAVE_SQUARE, 0.5, SQUARE_HZ)], 4 * CAP)[0] == 0.0
    l1.work(4 * CAP)                                                   # the square's low half: wet 0 on the device, 1 in the host's copy
    x = _audio(np.random.default_rng(3), n, CAP)
    assert _same(_run(blk, rv, x), x)                                  # fully dry: the serial kernel read the device's value
    l1.destroy()
    assert form() == serial                                            # the trip still lives
    l2.destroy()
    rv.control_set_param_by_index(T.CTL_FX_WET, 1.0)
    assert form() == direct
    l3 = rv.link_wet(T.ctl_sources(1, source=T.CTL_SRC_LFO, waveform=T.WAVE_SINE, frequency_hz=1.0))
    rv.destroy()
    with pytest.raises(_lib.GrooveError, match="groove_ctl_link_apply: the target effect has been destroyed"):
        l3.work(0)
    l3.destroy()
    blk.destroy()


def test_refusals_each_with_its_message(gpu_ctx):
    from groove_amd import entities as E
    n = 4
    L = gpu_ctx.L
    fx = {k: E.Effect(gpu_ctx, TARGETS[k][0], _mk(n, k)) for k in ("gain", "lp12", "reverb")}
    mixer = E.Effect(gpu_ctx, T.FX_MIXER, _params(n))
    lfo = lambda m: T.ctl_sources(m, source=T.CTL_SRC_LFO, waveform=T.WAVE_SINE, frequency_hz=1.0)
    ok = [(LAW.SLOPE, 0.1, 0.9, 1.0)]
    steps, n_steps = T.ctl_steps([ok])
    start = (C.c_double * 1)(0.0)
    out = C.c_void_p()
    # a Mixer
    with pytest.raises(_lib.GrooveError, match="groove_ctl_wet_link_create: a Mixer is the identity"):
        mixer.link_wet(lfo(1))
    with pytest.raises(_lib.GrooveError, match="groove_ctl_wet_trip_create: a Mixer is the identity"):
        mixer.trip_wet([ok], 0.0)
    # NULL arguments
    for args in ((None, lfo(1), 1, fx["gain"].h, C.byref(out)), (gpu_ctx.h, None, 1, fx["gain"].h, C.byref(out)),
                 (gpu_ctx.h, lfo(1), 1, None, C.byref(out)), (gpu_ctx.h, lfo(1), 1, fx["gain"].h, None)):
        assert L.groove_ctl_wet_link_create(*args) != 0
    with pytest.raises(_lib.GrooveError, match="groove_ctl_wet_link_create: NULL argument"):
        _lib.check(L.groove_ctl_wet_link_create(gpu_ctx.h, None, 1, fx["gain"].h, C.byref(out)), gpu_ctx.h)
    for args in ((None, steps, n_steps, start, 1, fx["gain"].h, C.byref(out)), (gpu_ctx.h, None, n_steps, start, 1, fx["gain"].h, C.byref(out)),
                 (gpu_ctx.h, steps, n_steps, None, 1, fx["gain"].h, C.byref(out)), (gpu_ctx.h, steps, n_steps, start, 1, None, C.byref(out)),
                 (gpu_ctx.h, steps, n_steps, start, 1, fx["gain"].h, None)):
        assert L.groove_ctl_wet_trip_create(*args) != 0
    with pytest.raises(_lib.GrooveError, match="groove_ctl_wet_trip_create: NULL argument"):
        _lib.check(L.groove_ctl_wet_trip_create(gpu_ctx.h, steps, n_steps, None, 1, fx["gain"].h, C.byref(out)), gpu_ctx.h)
    # a foreign context
    other = E.Context(0)
    try:
        with pytest.raises(_lib.GrooveError, match="groove_ctl_wet_link_create: the target is not a live effect of this context"):
            _lib.check(L.groove_ctl_wet_link_create(other.h, lfo(1), 1, fx["gain"].h, C.byref(out)), other.h)
        with pytest.raises(_lib.GrooveError, match="groove_ctl_wet_trip_create: the target is not a live effect of this context"):
            _lib.check(L.groove_ctl_wet_trip_create(other.h, steps, n_steps, start, 1, fx["gain"].h, C.byref(out)), other.h)
    finally:
        other.close()
    # n_src neither 1 nor the lane count
    with pytest.raises(_lib.GrooveError, match="groove_ctl_wet_link_create: n_src must be the target's lane count, or 1"):
        fx["lp12"].link_wet(lfo(3))
    with pytest.raises(_lib.GrooveError, match="groove_ctl_wet_trip_create: n_src must be the target's lane count, or 1"):
        fx["lp12"].trip_wet([ok] * 3, 0.0)
    # sources and steps are checked like the other creates'
    with pytest.raises(_lib.GrooveError, match="groove_ctl_wet_link_create: an LFO source is sine"):
        fx["gain"].link_wet(T.ctl_sources(1, source=T.CTL_SRC_LFO, waveform=T.WAVE_NOISE, frequency_hz=1.0))
    with pytest.raises(_lib.GrooveError, match="groove_ctl_wet_trip_create: a step's beats must be > 0"):
        fx["gain"].trip_wet([[(LAW.SLOPE, 0.1, 0.9, 0.0)]], 0.0)
    # the three old creates still refuse wet-dry-mix
    with pytest.raises(_lib.GrooveError, match="groove_ctl_link_create: wet-dry-mix chooses a kernel path on the host"):
        E.ControlLink(gpu_ctx, lfo(1), fx["reverb"], T.CTL_FX_WET)
    with pytest.raises(_lib.GrooveError, match="groove_ctl_filter_link_create: wet-dry-mix chooses a kernel path on the host"):
        E.ControlLink(gpu_ctx, lfo(1), fx["lp12"], T.CTL_FX_WET, derived=True)
    with pytest.raises(_lib.GrooveError, match="groove_ctl_trip_create: wet-dry-mix chooses a kernel path on the host"):
        E.ControlTripLink(gpu_ctx, [ok], 0.0, fx["gain"], T.CTL_FX_WET)
    # a wet link is an ordinary link: the calls of the wrong kind are refused as on any other
    link, trip = fx["gain"].link_wet(lfo(n)), fx["gain"].trip_wet([ok], 0.0)
    with pytest.raises(_lib.GrooveError, match="groove_ctl_link_apply: a trip link"):
        _lib.check(L.groove_ctl_link_apply(trip.h, 0), gpu_ctx.h)
    with pytest.raises(_lib.GrooveError, match="groove_ctl_trip_apply: not a trip link"):
        _lib.check(L.groove_ctl_trip_apply(link.h, 0), gpu_ctx.h)
    link.work(0); trip.work(0); link.reset(); trip.reset()
    assert gpu_ctx.debug_info()["zero_segments"] == 0
    for x_ in [link, trip, mixer] + list(fx.values()):
        x_.destroy()
