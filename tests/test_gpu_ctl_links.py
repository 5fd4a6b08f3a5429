"""GPU tier: device-resident control links through the C ABI (include/groove_hip.h groove_ctl_link_*; csrc/ctl_link.h).

A link's value is read back through the effect it drives: a Gain given a block of ones returns its per-lane ceiling, a Compressor with
ratio 0 given a block above every threshold returns its per-lane threshold — both exactly (x * c; fma(a - t, 0, t)).  The signal laws
are bit-exact against numpy float32, the LFO law within 2e-7 of the closed form (tests/test_ctl_core_cpu.py states where the bound
comes from)."""
import numpy as np
import pytest

from groove_amd import abi_types as T, lib as _lib
from tests.test_ctl_core_cpu import _closed_form, _delta64, signal_law_np

pytestmark = pytest.mark.gpu

CAP = 256
LANES = [1, 63, 64, 65, 257]
FRAMES = [1, 7, 256]
LAWS = [T.CTL_LAW_BIPOLAR, T.CTL_LAW_AMPLITUDE, T.CTL_LAW_AMPLITUDE_INVERTED]
SMOOTH = {T.WAVE_SINE: "sine", T.WAVE_TRIANGLE: "triangle", T.WAVE_SAWTOOTH: "sawtooth", T.WAVE_TRIANGLE_SINE: "triangle-sine"}


def _params(n, **kw):
    arr = (T.FxParams * n)()
    for i in range(n):
        arr[i] = T.fx_params(**{k: (v[i] if isinstance(v, (list, np.ndarray)) else v) for k, v in kw.items()})
    return arr


class _Probe:
    """Reads an effect's linked parameter back by processing a constant block (one frame)."""

    def __init__(self, ctx, n, level):
        self.block = ctx.block(n, 1)
        self.x = np.full((2, 1, n), level, dtype=np.float32)

    def read(self, fx):
        self.block.upload(self.x)
        fx.transform_audio(self.block, 1)
        out = self.block.download(1)
        assert np.array_equal(out[0], out[1])
        return out[0, 0, :].copy()

    def destroy(self):
        self.block.destroy()


def _signal_block(rng, n, frames):
    """A full-capacity block of one content with `frames` frames of ANOTHER content on top: a capture that looked at frame cap - 1, or
    stepped from channel to channel by frames * n, would see the first."""
    full = rng.uniform(-1.5, 1.5, (2, CAP, n)).astype(np.float32)
    part = rng.uniform(-1.5, 1.5, (2, frames, n)).astype(np.float32)
    return full, part


def _lfo_want(sources, at_frame, sr=44100.0):
    """Closed-form control values of LFO source lanes (waveform, duty, frequency) at a block start, in f64."""
    out = []
    for w, duty, f in sources:
        phase = (_delta64(f, sr) * at_frame) % 2 ** 64
        if w == T.WAVE_SQUARE:
            v = 1.0 if phase < 2 ** 63 else -1.0
        elif w == T.WAVE_PULSE_WIDTH:
            v = 1.0 if phase < int(float(np.float32(duty)) * 18446744073709549568.0) else -1.0
        else:
            v = _closed_form(SMOOTH[w], phase)
        out.append((v + 1.0) * 0.5)
    return np.array(out)


def _lfo_sources(n):
    waves = [T.WAVE_SINE, T.WAVE_TRIANGLE, T.WAVE_SAWTOOTH, T.WAVE_TRIANGLE_SINE, T.WAVE_SQUARE, T.WAVE_PULSE_WIDTH]
    desc = [(waves[i % 6], 0.3, 0.37 + 1.913 * i) for i in range(n)]
    arr = (T.CtlSource * n)()
    for s, (w, duty, f) in zip(arr, desc):
        s.source, s.waveform, s.duty, s.frequency_hz = T.CTL_SRC_LFO, w, duty, f
    return arr, desc


@pytest.mark.parametrize("n", LANES)
def test_signal_capture_reaches_a_gains_ceiling_bit_exact(gpu_ctx, n):
    from groove_amd import entities as E
    rng = np.random.default_rng(100 + n)
    gain = E.Effect(gpu_ctx, T.FX_GAIN, _params(n, ceiling=0.75))
    probe, src = _Probe(gpu_ctx, n, 1.0), gpu_ctx.block(n, CAP)
    for law in LAWS:
        link = E.ControlLink(gpu_ctx, T.ctl_sources(n, source=T.CTL_SRC_SIGNAL, law=law), gain, T.CTL_FX_CEILING)
        for frames in FRAMES:
            full, part = _signal_block(rng, n, frames)
            src.upload(full)
            src.upload(part)
            link.capture(src, frames)
            link.work(0)
            _, want = signal_law_np(law, part[0, frames - 1, :], part[1, frames - 1, :])
            got = probe.read(gain)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (n, law, frames)
            # the passthrough is the identity: the block is bit-unchanged, in and beyond the frames it was given
            after = src.download(CAP)
            assert np.array_equal(after[:, :frames].view(np.uint32), part.view(np.uint32))
            assert np.array_equal(after[:, frames:].view(np.uint32), full[:, frames:].view(np.uint32))
        link.destroy()
    probe.destroy(); src.destroy(); gain.destroy()


def test_one_source_lane_is_broadcast_to_65_target_lanes(gpu_ctx):
    from groove_amd import entities as E
    n = 65
    gain = E.Effect(gpu_ctx, T.FX_GAIN, _params(n, ceiling=[0.01 * i for i in range(n)]))
    probe, src = _Probe(gpu_ctx, n, 1.0), gpu_ctx.block(1, CAP)
    link = E.ControlLink(gpu_ctx, T.ctl_sources(1, source=T.CTL_SRC_SIGNAL, law=T.CTL_LAW_AMPLITUDE_INVERTED), gain, T.CTL_FX_CEILING)
    x = np.zeros((2, 7, 1), dtype=np.float32)
    x[0, 6, 0], x[1, 6, 0] = 0.3, -0.85
    src.upload(x)
    link.capture(src, 7)
    link.work(0)
    _, want = signal_law_np(T.CTL_LAW_AMPLITUDE_INVERTED, x[0, 6, :], x[1, 6, :])
    got = probe.read(gain)
    assert np.array_equal(got.view(np.uint32), np.repeat(want, n).view(np.uint32))
    # an LFO source too
    lfo = E.ControlLink(gpu_ctx, T.ctl_sources(1, source=T.CTL_SRC_LFO, waveform=T.WAVE_TRIANGLE, frequency_hz=3.0), gain, T.CTL_FX_CEILING)
    lfo.work(1234)
    got = probe.read(gain)
    assert np.all(got == got[0]) and abs(float(got[0]) - _lfo_want([(T.WAVE_TRIANGLE, 0.5, 3.0)], 1234)[0]) <= 2e-7
    for x_ in (link, lfo, probe, src, gain):
        x_.destroy()


def test_apply_before_any_capture_and_after_reset_leaves_the_target(gpu_ctx):
    from groove_amd import entities as E
    n = 65
    created = np.linspace(0.1, 0.9, n).astype(np.float32)
    gain = E.Effect(gpu_ctx, T.FX_GAIN, _params(n, ceiling=list(created)))
    probe, src = _Probe(gpu_ctx, n, 1.0), gpu_ctx.block(n, CAP)
    link = E.ControlLink(gpu_ctx, T.ctl_sources(n, source=T.CTL_SRC_SIGNAL, law=T.CTL_LAW_BIPOLAR), gain, T.CTL_FX_CEILING)
    link.work(0)
    assert np.array_equal(probe.read(gain), created)
    x = np.random.default_rng(5).uniform(-1, 1, (2, 7, n)).astype(np.float32)
    src.upload(x)
    link.capture(src, 0)            # no frames transformed: nothing captured
    link.work(0)
    assert np.array_equal(probe.read(gain), created)
    link.capture(src, 7)
    link.work(0)
    _, want = signal_law_np(T.CTL_LAW_BIPOLAR, x[0, 6], x[1, 6])
    assert np.array_equal(probe.read(gain), want)
    gain.set_params(_params(n, ceiling=list(created)))
    link.reset()
    link.work(0)
    assert np.array_equal(probe.read(gain), created)
    for x_ in (link, probe, src, gain):
        x_.destroy()


def test_lfo_reaches_a_compressors_threshold_within_2e_7(gpu_ctx):
    from groove_amd import entities as E
    n = 257
    comp = E.Effect(gpu_ctx, T.FX_COMPRESSOR, _params(n, limit_min=0.5, limit_max=0.0))   # ratio 0: |x| above the threshold comes out AS the threshold
    probe = _Probe(gpu_ctx, n, 2.0)
    sources, desc = _lfo_sources(n)
    link = E.ControlLink(gpu_ctx, sources, comp, T.CTL_FX_THRESHOLD)
    edge = np.array([w in (T.WAVE_SQUARE, T.WAVE_PULSE_WIDTH) for w, _, _ in desc])
    worst = 0.0
    for at in [b * 256 for b in range(40)] + [2 ** 33 + 5]:
        link.work(at)
        got = probe.read(comp).astype(np.float64)
        want = _lfo_want(desc, at)
        worst = max(worst, float(np.max(np.abs(got - want))))
        assert np.max(np.abs(got - want)) <= 2e-7, at
        assert np.array_equal(got[edge], want[edge]), at        # the edge waveforms are exact
    print(f"LFO -> threshold: worst |device - closed form| = {worst:.3e}")
    assert np.ptp(_lfo_want(desc, 39 * 256)[~edge]) > 0.5          # the lanes really are at different places
    for x_ in (link, probe, comp):
        x_.destroy()


def _bitcrush_np(x, bits):
    q = (np.abs(x).astype(np.float32) * np.float32(32767.0)).astype(np.uint32)
    q = (q >> bits) << bits
    return np.copysign(q.astype(np.float32) * np.float32(1.0 / 32767.0), x).astype(np.float32)


def test_bits_target_is_exact(gpu_ctx):
    from groove_amd import entities as E
    n = 65
    crush = E.Effect(gpu_ctx, T.FX_BITCRUSHER, _params(n, bits=3))
    src, io = gpu_ctx.block(n, CAP), gpu_ctx.block(n, 2)
    link = E.ControlLink(gpu_ctx, T.ctl_sources(n, source=T.CTL_SRC_SIGNAL, law=T.CTL_LAW_AMPLITUDE), crush, T.CTL_FX_BITS)
    # |m| on and just under every sixteenth: bits = floor(16 |m|), 0 .. 16
    m = np.array([(k // 2) / 16.0 if k % 2 == 0 else np.nextafter(np.float32((k // 2 + 1) / 16.0), np.float32(0)) for k in range(n)], dtype=np.float32)
    m = np.minimum(m, np.float32(1.0))
    x = np.stack([m, m])[:, None, :].astype(np.float32)            # L = R = m: (m + m) / 2 = m exactly
    src.upload(x)
    link.capture(src, 1)
    link.work(0)
    bits = np.minimum((m * np.float32(16)).astype(np.uint32), 31)
    assert bits.min() == 0 and bits.max() == 16 and len(set(bits.tolist())) == 17
    probe = np.empty((2, 2, n), dtype=np.float32)
    probe[:, 0, :], probe[:, 1, :] = 1.0, 3.5                        # 32767 tells bits 0 .. 15 apart, 114684 tells 15, 16 and 17 apart
    io.upload(probe)
    crush.transform_audio(io, 2)
    got = io.download(2)
    assert np.array_equal(got.view(np.uint32), _bitcrush_np(probe, bits[None, None, :]).view(np.uint32))
    for x_ in (link, src, io, crush):
        x_.destroy()


def test_refused_targets_sources_and_shapes_return_errors_with_messages(gpu_ctx):
    from groove_amd import entities as E
    n = 4
    gain = E.Effect(gpu_ctx, T.FX_GAIN, _params(n))
    lp = E.Effect(gpu_ctx, T.FX_BIQUAD_LP12, _params(n))
    lp24 = E.Effect(gpu_ctx, T.FX_BIQUAD_LP24, _params(n))
    lfo = lambda **kw: T.ctl_sources(n, source=T.CTL_SRC_LFO, waveform=T.WAVE_SINE, frequency_hz=1.0, **kw)
    for fx, index, msg in ((lp, T.CTL_FX_CUTOFF, "coefficients on the host"), (lp, T.CTL_FX_Q, "coefficients on the host"),
                           (lp24, T.CTL_FX_PASSBAND_RIPPLE, "coefficients on the host"), (gain, T.CTL_FX_WET, "kernel path"),
                           (gain, 99, "unknown control index"), (gain, T.CTL_WELSH_DCA_PAN, "unknown control index"),
                           (gain, T.CTL_FX_THRESHOLD, "no such parameter"), (lp, T.CTL_FX_CEILING, "no such parameter")):
        with pytest.raises(_lib.GrooveError, match=msg):
            E.ControlLink(gpu_ctx, lfo(), fx, index)
    for w in (T.WAVE_NOISE, T.WAVE_NONE, T.WAVE_DEBUG_MAX):
        with pytest.raises(_lib.GrooveError, match="no closed form"):
            E.ControlLink(gpu_ctx, T.ctl_sources(n, source=T.CTL_SRC_LFO, waveform=w, frequency_hz=1.0), gain, T.CTL_FX_CEILING)
    with pytest.raises(_lib.GrooveError, match="lane count"):
        E.ControlLink(gpu_ctx, T.ctl_sources(3, source=T.CTL_SRC_LFO, waveform=T.WAVE_SINE, frequency_hz=1.0), gain, T.CTL_FX_CEILING)
    mixed = lfo()
    mixed[2].source = T.CTL_SRC_SIGNAL
    with pytest.raises(_lib.GrooveError, match="one source kind"):
        E.ControlLink(gpu_ctx, mixed, gain, T.CTL_FX_CEILING)
    with pytest.raises(_lib.GrooveError, match="unknown signal law"):
        E.ControlLink(gpu_ctx, T.ctl_sources(n, source=T.CTL_SRC_SIGNAL, law=7), gain, T.CTL_FX_CEILING)
    link = E.ControlLink(gpu_ctx, lfo(), gain, T.CTL_FX_CEILING)
    blk, small = gpu_ctx.block(n, 8), gpu_ctx.block(n + 1, 8)
    with pytest.raises(_lib.GrooveError, match="not a signal link"):
        link.capture(blk, 8)
    sig = E.ControlLink(gpu_ctx, T.ctl_sources(n, source=T.CTL_SRC_SIGNAL), gain, T.CTL_FX_CEILING)
    with pytest.raises(_lib.GrooveError, match="lanes"):
        sig.capture(small, 8)
    with pytest.raises(_lib.GrooveError, match="capacity"):
        sig.capture(blk, 9)
    for x_ in (link, sig, blk, small, gain, lp, lp24):
        x_.destroy()


def test_set_param_overwrites_until_the_next_apply_and_a_destroyed_target_is_an_error(gpu_ctx):
    from groove_amd import entities as E
    n = 63
    gain = E.Effect(gpu_ctx, T.FX_GAIN, _params(n, ceiling=0.5))
    probe = _Probe(gpu_ctx, n, 1.0)
    sources, desc = _lfo_sources(n)
    link = E.ControlLink(gpu_ctx, sources, gain, T.CTL_FX_CEILING)
    link.work(512)
    linked = probe.read(gain)
    assert np.max(np.abs(linked - _lfo_want(desc, 512))) <= 2e-7 and np.ptp(linked) > 0.5
    gain.control_set_param_by_index(T.CTL_FX_CEILING, 0.25)          # the host's shadow is re-uploaded: the link's value is gone ...
    assert np.array_equal(probe.read(gain), np.full(n, 0.25, dtype=np.float32))
    link.work(512)                                                    # ... until the link's next apply
    assert np.array_equal(probe.read(gain), linked)
    gain.destroy()
    with pytest.raises(_lib.GrooveError, match="destroyed"):
        link.work(768)
    # a new effect may land on the freed one's address: the link still has no target
    other = E.Effect(gpu_ctx, T.FX_GAIN, _params(n, ceiling=0.5))
    with pytest.raises(_lib.GrooveError, match="destroyed"):
        link.work(768)
    assert np.array_equal(probe.read(other), np.full(n, 0.5, dtype=np.float32))
    for x_ in (link, probe, other):
        x_.destroy()


def _audio(rng, n, frames):
    t = np.arange(frames)[None, :, None]
    f = (110.0 * 2.0 ** (np.arange(n) % 29 / 12.0))[None, None, :]
    return (0.6 * np.sin(2 * np.pi * f * t / 44100.0 + np.arange(2)[:, None, None]) + 0.15 * rng.standard_normal((2, frames, n))).astype(np.float32)


@pytest.mark.parametrize("source", ["signal", "lfo"])
def test_sidechain_of_65_lanes_follows_the_oracle_compressor(gpu_ctx, oracle, source):
    """Six blocks: the compressor's threshold of block b is the control value of block b's control phase — what the passthrough captured
    from the last frame of block b - 1 (signal), or the LFO at the block's first frame — and the oracle's Fx is given that threshold, per
    lane, from the numpy law (signal) or the closed form (lfo).  Signal: the 1e-7 bar tests/test_gpu_fx.py holds the compressor to (the
    threshold is bit-exact).  LFO: 3e-7 = that bar plus the value's 2e-7, which the compressor scales by at most 1."""
    from groove_amd import entities as E
    n, frames, blocks = 65, 256, 6
    rng = np.random.default_rng(77)
    created = np.full(n, 0.4, dtype=np.float32)
    comp = E.Effect(gpu_ctx, T.FX_COMPRESSOR, _params(n, limit_min=list(created), limit_max=0.25))
    ofx = oracle.Fx(T.FX_COMPRESSOR, _params(n, limit_min=list(created), limit_max=0.25))
    if source == "signal":
        law = T.CTL_LAW_AMPLITUDE_INVERTED
        link = E.ControlLink(gpu_ctx, T.ctl_sources(n, source=T.CTL_SRC_SIGNAL, law=law), comp, T.CTL_FX_THRESHOLD)
        bar = 1e-7
    else:
        sources, desc = _lfo_sources(n)
        link = E.ControlLink(gpu_ctx, sources, comp, T.CTL_FX_THRESHOLD)
        bar = 3e-7
    side, io = gpu_ctx.block(n, CAP), gpu_ctx.block(n, CAP)
    thr, worst, moved = created, 0.0, 0
    for b in range(blocks):
        drums, synth = _audio(rng, n, frames), _audio(rng, n, frames)
        if source == "lfo":
            thr = _lfo_want(desc, b * frames).astype(np.float32)
        link.work(b * frames)
        io.upload(synth)
        comp.transform_audio(io, frames)
        got = io.download(frames).astype(np.float64)
        ofx.set_params(_params(n, limit_min=list(thr), limit_max=0.25))
        want = ofx.process(synth.astype(np.float64))
        worst = max(worst, float(np.max(np.abs(got - want))))
        assert np.max(np.abs(got - want)) <= bar, (source, b)
        moved += int(np.any(np.abs(want - synth) > 1e-3))
        if source == "signal":
            side.upload(drums)
            link.capture(side, frames)                              # heard by block b + 1
            _, thr = signal_law_np(law, drums[0, frames - 1], drums[1, frames - 1])
    print(f"sidechain ({source}): worst |device - oracle| = {worst:.3e}")
    assert moved == blocks                                           # the compressor really compresses
    for x_ in (link, side, io, comp):
        x_.destroy()


def test_linked_stages_inside_a_chain_match_stage_by_stage(gpu_ctx):
    from groove_amd import entities as E
    n, sizes = 64, [256, 100, 256, 1, 255, 256]
    rng = np.random.default_rng(31)
    chain = [(T.FX_GAIN, _params(n, ceiling=0.9)), (T.FX_COMPRESSOR, _params(n, limit_min=0.3, limit_max=0.2)),
             (T.FX_BITCRUSHER, _params(n, bits=6)), (T.FX_LIMITER, _params(n, limit_min=0.0, limit_max=0.8))]
    sources, _ = _lfo_sources(n)
    sets = []
    for _ in range(2):
        fx = [E.Effect(gpu_ctx, k, p) for k, p in chain]
        links = [E.ControlLink(gpu_ctx, sources, fx[0], T.CTL_FX_CEILING),
                 E.ControlLink(gpu_ctx, T.ctl_sources(n, source=T.CTL_SRC_SIGNAL, law=T.CTL_LAW_AMPLITUDE), fx[1], T.CTL_FX_THRESHOLD),
                 E.ControlLink(gpu_ctx, T.ctl_sources(1, source=T.CTL_SRC_LFO, waveform=T.WAVE_SAWTOOTH, frequency_hz=40.0), fx[2], T.CTL_FX_BITS)]
        sets.append((fx, links, gpu_ctx.block(n, CAP)))
    side = gpu_ctx.block(n, CAP)
    at = 0
    differs = False
    for fr in sizes:
        x, drums = _audio(rng, n, fr), _audio(rng, n, fr)
        side.upload(drums)
        outs = []
        for which, (fx, links, io) in enumerate(sets):
            for l in links:
                l.work(at)
            io.upload(x)
            if which == 0:
                for e in fx:
                    e.transform_audio(io, fr)
            else:
                gpu_ctx.transform_chain(fx, io, fr)
            links[1].capture(side, fr)
            outs.append(io.download(fr))
        assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32)), at
        differs = differs or not np.array_equal(outs[0], x * np.float32(0.9))
        at += fr
    assert differs
    for fx, links, io in sets:
        for x_ in links + fx + [io]:
            x_.destroy()
    side.destroy()


def test_reverb_attenuation_link_same_bits_with_the_allpass_stream_on_and_off(gpu_ctx):
    from groove_amd import entities as E
    n, frames, blocks = 64, 256, 6
    rng = np.random.default_rng(9)
    xs = [_audio(rng, n, frames) for _ in range(blocks)]
    params = _params(n, attenuation=0.9, reverb_seconds=0.6)
    old = gpu_ctx.fx_allpass_stream
    runs = {}
    try:
        for mode in ("off", "on", "unlinked"):
            gpu_ctx.fx_allpass_stream = mode == "on"
            verb = E.Effect(gpu_ctx, T.FX_REVERB, params)
            link = None if mode == "unlinked" else E.ControlLink(
                gpu_ctx, T.ctl_sources(1, source=T.CTL_SRC_LFO, waveform=T.WAVE_SINE, frequency_hz=23.0), verb, T.CTL_FX_ATTENUATION)
            io = gpu_ctx.block(n, CAP)
            io.release()                                             # a block with its events takes the all-pass stream
            out = []
            for b, x in enumerate(xs):
                if link:
                    link.work(b * frames)                            # behind the previous block's all-passes (fx_ap_settle), ahead of this run
                io.upload(x)
                gpu_ctx.transform_chain([verb], io, frames)
                out.append(io.download(frames))
                io.release()
            runs[mode] = np.concatenate(out, axis=1)
            for x_ in ([link] if link else []) + [io, verb]:
                x_.destroy()
    finally:
        gpu_ctx.fx_allpass_stream = old
    assert np.array_equal(runs["on"].view(np.uint32), runs["off"].view(np.uint32))
    assert np.max(np.abs(runs["on"] - runs["unlinked"])) > 1e-3


def test_applies_do_not_wait_on_the_host_and_set_param_does(gpu_ctx):
    from groove_amd import entities as E
    n = 65
    gain = E.Effect(gpu_ctx, T.FX_GAIN, _params(n, ceiling=0.5))
    src = gpu_ctx.block(n, CAP)
    lfo = E.ControlLink(gpu_ctx, T.ctl_sources(n, source=T.CTL_SRC_LFO, waveform=T.WAVE_SINE, frequency_hz=2.0), gain, T.CTL_FX_CEILING)
    sig = E.ControlLink(gpu_ctx, T.ctl_sources(n, source=T.CTL_SRC_SIGNAL), gain, T.CTL_FX_CEILING)
    waits = lambda: gpu_ctx.debug_info()["host_waits"]
    a = waits()
    own = waits() - a                                                # what reading the counter costs by itself
    a = waits()
    for b in range(10):
        lfo.work(b * 256)
        sig.capture(src, 256)
        sig.work(b * 256)
    assert waits() - a - own == 0                                   # twenty applies (and ten captures): not one host wait
    a = waits()
    for b in range(20):
        gain.control_set_param_by_index(T.CTL_FX_CEILING, 0.5)
    assert waits() - a - own >= 20
    assert gpu_ctx.debug_info()["zero_segments"] == 0
    for x_ in (lfo, sig, src, gain):
        x_.destroy()
