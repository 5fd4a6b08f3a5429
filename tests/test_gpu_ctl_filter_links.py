"""GPU tier: device-resident links onto a filter's cutoff, q and passband-ripple (include/groove_hip.h groove_ctl_filter_link_create;
csrc/ctl_link.h ctl_filter_apply_kernel, csrc/fx_coef.h).

Three arms where the text says so.  A: the new link (capture after a block, work before the next).  B: a second effect of the same
parameters driven lane by lane through groove_fx_set_param — the path that exists without the link, the host's f64 derivation.  O: the
f64 oracle's effect, given per block the parameters the law gives in numpy (cutoff = float32(25 * 800^v), q = ripple =
float32(10 v^2 + 0.707)).  The bar is the one tests/test_gpu_fx.py holds the IIR kinds to, 4e-6 of the larger of 1 and the output's
peak; B against O is asserted first (it validates the inputs with code that is not new), then A against O.  |A - B| — what the
device's math library and a possible last-place difference of the fp32 cutoff cost — is printed, not bounded beyond that.

Signal sources use the AMPLITUDE law on L = R = m, whose value |m| is exact in fp32 (tests/test_ctl_core_cpu.py signal_law_np)."""
import numpy as np
import pytest

from groove_amd import abi_types as T, lib as _lib
from tests import fx_forms as F
from tests.test_ctl_core_cpu import signal_law_np
from tests.test_gpu_ctl_links import _audio, _lfo_sources, _lfo_want, _params

pytestmark = pytest.mark.gpu

CAP = 64
BAR = 4e-6
BASE = dict(cutoff_hz=1000.0, q=0.9, passband_ripple=1.1, bandwidth_hz=500.0, db_gain=6.0)
KINDS = {"lp12": T.FX_BIQUAD_LP12, "hp12": T.FX_BIQUAD_HP12, "bp12": T.FX_BIQUAD_BP12, "bs12": T.FX_BIQUAD_BS12, "ap12": T.FX_BIQUAD_AP12,
         "peak12": T.FX_BIQUAD_PEAK12, "lshelf12": T.FX_BIQUAD_LSHELF12, "hshelf12": T.FX_BIQUAD_HSHELF12, "lp24": T.FX_BIQUAD_LP24}
FIELD = {T.CTL_FX_CUTOFF: "cutoff_hz", T.CTL_FX_Q: "q", T.CTL_FX_PASSBAND_RIPPLE: "passband_ripple"}
CASES = [("cutoff", k) for k in KINDS] + [("q", k) for k in ("lp12", "hp12", "ap12")] + [("passband-ripple", "lp24")]
INDEX = {"cutoff": T.CTL_FX_CUTOFF, "q": T.CTL_FX_Q, "passband-ripple": T.CTL_FX_PASSBAND_RIPPLE}


def law_np(index, v):
    """groove_fx_set_param's law of a fp32 control value, as the float groove_fx_params holds."""
    v = np.asarray(v, dtype=np.float64)
    if index == T.CTL_FX_CUTOFF:
        return np.array([np.float32(25.0 * 800.0 ** float(x)) for x in v.ravel()], dtype=np.float32).reshape(v.shape)
    return (v * v * 10.0 + 0.707).astype(np.float32)


def _with(n, **per_lane):
    kw = dict(BASE)
    kw.update({k: [float(x) for x in np.broadcast_to(v, (n,))] for k, v in per_lane.items()})
    return _params(n, **kw)


def _side_values(n, block, lo=0.1, hi=0.95, salt=0):
    """Per-lane m in [lo, hi], different in every lane and block; both ends are reached at 65 lanes."""
    k = (np.arange(n) * 7 + block * 13 + salt) % 65
    return (lo + (hi - lo) * k / 64.0).astype(np.float32)


def _side_block(n, frames, m):
    """A block whose last frame is L = R = m (so that (L + R) / 2 = m exactly) and whose other frames are something else."""
    x = np.full((2, frames, n), 0.77, dtype=np.float32)
    x[:, frames - 1, :] = m
    return x


def _run(block, fx, x):
    block.upload(x)
    fx.transform_audio(block, x.shape[1])
    return block.download(x.shape[1])


def _zero_segments(ctx):
    assert ctx.debug_info()["zero_segments"] == 0


@pytest.mark.parametrize("param,kind", CASES, ids=[f"{p}-{k}" for p, k in CASES])
def test_signal_link_on_every_kind_three_arms(gpu_ctx, oracle, param, kind):
    from groove_amd import entities as E
    n, frames, blocks = 65, 64, 6
    index, fxk = INDEX[param], KINDS[kind]
    rng = np.random.default_rng(500 + 17 * index + fxk)
    a, b, plain = (E.Effect(gpu_ctx, fxk, _with(n)) for _ in range(3))
    ofx = oracle.Fx(fxk, _with(n))
    link = E.ControlLink(gpu_ctx, T.ctl_sources(n, source=T.CTL_SRC_SIGNAL, law=T.CTL_LAW_AMPLITUDE), a, index, derived=True)
    side, io = gpu_ctx.block(n, CAP), gpu_ctx.block(n, CAP)
    v, seen = None, []
    worst_ab = worst_ao = worst_bo = 0.0
    for blk in range(blocks):
        x = _audio(rng, n, frames)
        link.work(blk * frames)
        if v is not None:
            seen.append(v)
            for lane in range(n):
                b.control_set_param_by_index(index, float(v[lane]), lane=lane)
            ofx.set_params(_with(n, **{FIELD[index]: law_np(index, v)}))
        ga, gb, gp = _run(io, a, x).astype(np.float64), _run(io, b, x).astype(np.float64), _run(io, plain, x)
        want = ofx.process(x.astype(np.float64))
        bar = BAR * max(1.0, float(np.abs(want).max()))
        worst_bo, worst_ao, worst_ab = max(worst_bo, np.abs(gb - want).max()), max(worst_ao, np.abs(ga - want).max()), max(worst_ab, np.abs(ga - gb).max())
        print(f"{param} -> {kind}, block {blk}: |B - O| {np.abs(gb - want).max():.3e}  |A - O| {np.abs(ga - want).max():.3e}  |A - B| {np.abs(ga - gb).max():.3e}  bar {bar:.3e}")
        assert np.abs(gb - want).max() <= bar, ("B against O: the inputs", param, kind, blk)
        assert np.abs(ga - want).max() <= bar, ("A against O", param, kind, blk)
        if blk == 0:
            assert np.array_equal(ga.astype(np.float32).view(np.uint32), gp.view(np.uint32))     # nothing captured yet
        else:
            assert np.abs(ga - gp).max() > 1e-3, (param, kind, blk)                                  # the output really moves
        m = _side_values(n, blk)
        side.upload(_side_block(n, frames, m))
        link.capture(side, frames)                                                                   # heard by block blk + 1
        _, v = signal_law_np(T.CTL_LAW_AMPLITUDE, m, m)
    print(f"{param} -> {kind}: worst |A - B| = {worst_ab:.3e}, |A - O| = {worst_ao:.3e}, |B - O| = {worst_bo:.3e}")
    seen = np.array(seen)
    assert seen.min() == np.float32(0.1) and seen.max() == np.float32(0.95)
    assert all(len(set(row.tolist())) == n for row in seen) and all(len(set(col.tolist())) == blocks - 1 for col in seen.T)
    _zero_segments(gpu_ctx)
    for x_ in (link, side, io, a, b, plain):
        x_.destroy()


def _lfo_lanes_in_range(n, ats, lo=0.1, hi=0.95):
    """The first n lanes of the existing test's LFO sources whose closed-form value lies in [lo, hi] at every block start in `ats`
    (the edge waveforms, 0 or 1, never do), as (ctypes array, descriptions, values[len(ats)][n]) — decided on the CPU."""
    _, desc = _lfo_sources(24 * n + 24)
    vals = np.array([_lfo_want(desc, at) for at in ats])
    keep = [i for i in range(len(desc)) if vals[:, i].min() >= lo and vals[:, i].max() <= hi][:n]
    assert len(keep) == n, (n, len(keep))
    arr = (T.CtlSource * n)()
    for s, i in zip(arr, keep):
        s.source, s.waveform, s.duty, s.frequency_hz = T.CTL_SRC_LFO, desc[i][0], desc[i][1], desc[i][2]
    return arr, [desc[i] for i in keep], vals[:, keep]


@pytest.mark.parametrize("n", [1, 257])
@pytest.mark.parametrize("kind", ["lp12", "lp24"])
def test_lfo_link_follows_the_oracle_at_the_closed_form(gpu_ctx, oracle, kind, n):
    """The oracle's cutoff is the law of the closed-form LFO value; the device's fp32 value is within 2e-7 of it
    (tests/test_ctl_core_cpu.py), which is 1.4e-6 of the cutoff (d cutoff / cutoff = ln 800 dv) — far inside the bar for values in
    [0.1, 0.95], which is what the lanes are chosen for."""
    from groove_amd import entities as E
    frames, blocks, at0 = 32, 8, 10000
    ats = [at0 + b * frames for b in range(blocks)]
    sources, desc, vals = _lfo_lanes_in_range(n, ats)
    assert vals.min() >= 0.1 and vals.max() <= 0.95
    if n > 1:
        assert np.ptp(vals[0]) > 0.5 and len({d[0] for d in desc}) == 4          # the lanes are at different places, on every smooth waveform
    fxk = KINDS[kind]
    rng = np.random.default_rng(900 + n + fxk)
    a, ofx = E.Effect(gpu_ctx, fxk, _with(n)), oracle.Fx(fxk, _with(n))
    link = E.ControlLink(gpu_ctx, sources, a, T.CTL_FX_CUTOFF, derived=True)
    io = gpu_ctx.block(n, CAP)
    worst = 0.0
    for blk, at in enumerate(ats):
        x = _audio(rng, n, frames)
        link.work(at)
        ofx.set_params(_with(n, cutoff_hz=law_np(T.CTL_FX_CUTOFF, _lfo_want(desc, at))))
        got, want = _run(io, a, x).astype(np.float64), ofx.process(x.astype(np.float64))
        worst = max(worst, float(np.abs(got - want).max()))
        assert np.abs(got - want).max() <= BAR * max(1.0, float(np.abs(want).max())), (kind, n, blk)
    print(f"LFO -> cutoff of {kind}, {n} lanes: worst |device - oracle| = {worst:.3e}")
    _zero_segments(gpu_ctx)
    for x_ in (link, io, a):
        x_.destroy()


@pytest.mark.parametrize("n,frames", [(65, 64), (2049, 16), (24577, 8)])
@pytest.mark.parametrize("kind", ["lp12", "lp24"])
def test_every_iir_kernel_form_reads_what_the_link_wrote(gpu_ctx, kind, n, frames):
    """Time-parallel, four-segment (the 12 dB kinds; the 24 dB low-pass has no such form and is serial from 1,025 lanes) and serial: the
    link against groove_fx_set_param, a broadcast signal source."""
    from groove_amd import entities as E
    forms = F.library_forms()
    tag = {("lp12", 65): F.BQ_TP, ("lp12", 2049): F.BQ_SEG, ("lp12", 24577): F.BQ_SER,
           ("lp24", 65): F.LP_TP, ("lp24", 2049): F.LP_SER, ("lp24", 24577): F.LP_SER}[(kind, n)]
    fxk = KINDS[kind]
    rng = np.random.default_rng(n + fxk)
    a, b, plain = (E.Effect(gpu_ctx, fxk, _with(n)) for _ in range(3))
    link = E.ControlLink(gpu_ctx, T.ctl_sources(1, source=T.CTL_SRC_SIGNAL, law=T.CTL_LAW_AMPLITUDE), a, T.CTL_FX_CUTOFF, derived=True)
    side, io = gpu_ctx.block(1, CAP), gpu_ctx.block(n, CAP)
    v, worst, moved = None, 0.0, 0.0
    for blk in range(4):
        x = _audio(rng, n, frames)
        link.work(blk * frames)
        if v is not None:
            b.control_set_param_by_index(T.CTL_FX_CUTOFF, float(v[0]))
        for fx in (a, b):
            assert fx.kernel_form(io, frames) == F.form_of_tag(tag, forms), (kind, n, frames)
        ga, gb = _run(io, a, x).astype(np.float64), _run(io, b, x).astype(np.float64)
        worst = max(worst, float(np.abs(ga - gb).max()))
        assert np.abs(ga - gb).max() <= BAR * max(1.0, float(np.abs(gb).max())), (kind, n, blk)
        if v is not None:
            moved = max(moved, float(np.abs(ga - _run(io, plain, x)).max()))
        m = _side_values(1, blk, salt=5 + 20 * blk)
        side.upload(_side_block(1, frames, m))
        link.capture(side, frames)
        _, v = signal_law_np(T.CTL_LAW_AMPLITUDE, m, m)
    print(f"{kind}, {n} lanes x {frames} frames ({tag}): worst |A - B| = {worst:.3e}")
    assert moved > 1e-3
    _zero_segments(gpu_ctx)
    for x_ in (link, side, io, a, b, plain):
        x_.destroy()


def test_two_links_onto_one_filter_see_each_other(gpu_ctx, oracle):
    from groove_amd import entities as E
    n, frames, blocks = 63, 64, 5
    rng = np.random.default_rng(63)
    fxs = {name: E.Effect(gpu_ctx, T.FX_BIQUAD_LP12, _with(n)) for name in ("both", "cutoff", "q")}
    ofx = oracle.Fx(T.FX_BIQUAD_LP12, _with(n))
    sig = lambda: T.ctl_sources(n, source=T.CTL_SRC_SIGNAL, law=T.CTL_LAW_AMPLITUDE)
    links = {("both", "cutoff"): E.ControlLink(gpu_ctx, sig(), fxs["both"], T.CTL_FX_CUTOFF, derived=True),
             ("both", "q"): E.ControlLink(gpu_ctx, sig(), fxs["both"], T.CTL_FX_Q, derived=True),
             ("cutoff", "cutoff"): E.ControlLink(gpu_ctx, sig(), fxs["cutoff"], T.CTL_FX_CUTOFF, derived=True),
             ("q", "q"): E.ControlLink(gpu_ctx, sig(), fxs["q"], T.CTL_FX_Q, derived=True)}
    side, io = gpu_ctx.block(n, CAP), gpu_ctx.block(n, CAP)
    vc = vq = None
    apart = {"cutoff": 0.0, "q": 0.0}
    for blk in range(blocks):
        x = _audio(rng, n, frames)
        order = ("cutoff", "q") if blk % 2 == 0 else ("q", "cutoff")      # both orders, in different blocks
        for p in order:
            links[("both", p)].work(blk * frames)
        links[("cutoff", "cutoff")].work(blk * frames)
        links[("q", "q")].work(blk * frames)
        if vc is not None:
            ofx.set_params(_with(n, cutoff_hz=law_np(T.CTL_FX_CUTOFF, vc), q=law_np(T.CTL_FX_Q, vq)))
        got = {name: _run(io, fx, x).astype(np.float64) for name, fx in fxs.items()}
        want = ofx.process(x.astype(np.float64))
        assert np.abs(got["both"] - want).max() <= BAR * max(1.0, float(np.abs(want).max())), blk
        if blk:
            for name in apart:
                apart[name] = max(apart[name], float(np.abs(got["both"] - got[name]).max()))
        mc, mq = _side_values(n, blk), _side_values(n, blk, salt=31)
        for p, m in (("cutoff", mc), ("q", mq)):
            side.upload(_side_block(n, frames, m))
            for key, l in links.items():
                if key[1] == p:
                    l.capture(side, frames)
        (_, vc), (_, vq) = signal_law_np(T.CTL_LAW_AMPLITUDE, mc, mc), signal_law_np(T.CTL_LAW_AMPLITUDE, mq, mq)
    assert apart["cutoff"] > 1e-3 and apart["q"] > 1e-3, apart
    _zero_segments(gpu_ctx)
    for x_ in list(links.values()) + [side, io] + list(fxs.values()):
        x_.destroy()


def test_the_shadow_follows_the_host(gpu_ctx, oracle):
    """groove_fx_set_param re-uploads the host's parameters: onto the device's shadow too, so that the link's next apply derives from the
    new q; and over the linked cutoff, which is gone until the link's next apply (docs/DSP_SPEC.md section 13, staleness)."""
    from groove_amd import entities as E
    n, frames = 65, 64
    rng = np.random.default_rng(65)
    a, ofx = E.Effect(gpu_ctx, T.FX_BIQUAD_LP12, _with(n)), oracle.Fx(T.FX_BIQUAD_LP12, _with(n))
    link = E.ControlLink(gpu_ctx, T.ctl_sources(n, source=T.CTL_SRC_SIGNAL, law=T.CTL_LAW_AMPLITUDE), a, T.CTL_FX_CUTOFF, derived=True)
    side, io = gpu_ctx.block(n, CAP), gpu_ctx.block(n, CAP)
    m = _side_values(n, 3)
    _, v = signal_law_np(T.CTL_LAW_AMPLITUDE, m, m)
    linked, q_new = law_np(T.CTL_FX_CUTOFF, v), float(law_np(T.CTL_FX_Q, 0.8))
    side.upload(_side_block(n, frames, m))
    link.capture(side, frames)

    def block(**oracle_params):
        x = _audio(rng, n, frames)
        ofx.set_params(_with(n, **oracle_params))
        got, want = _run(io, a, x).astype(np.float64), ofx.process(x.astype(np.float64))
        return float(np.abs(got - want).max()), BAR * max(1.0, float(np.abs(want).max()))

    link.work(0)
    err, bar = block(cutoff_hz=linked)
    assert err <= bar
    a.control_set_param_by_index(T.CTL_FX_Q, 0.8)               # the host's shadow: its own cutoff, the new q
    err, bar = block(q=q_new)
    assert err <= bar
    link.work(frames)                                           # the new q AND the linked cutoff
    err, bar = block(cutoff_hz=linked, q=q_new)
    assert err <= bar
    a.control_set_param_by_index(T.CTL_FX_CUTOFF, 0.3)          # no work behind it: the linked cutoff is gone
    err, bar = block(cutoff_hz=float(law_np(T.CTL_FX_CUTOFF, 0.3)), q=q_new)
    assert err <= bar
    link.work(2 * frames)                                       # ... until the next apply
    err, bar = block(cutoff_hz=linked, q=q_new)
    assert err <= bar
    _zero_segments(gpu_ctx)
    for x_ in (link, side, io, a):
        x_.destroy()


def test_apply_before_any_capture_and_after_reset_leaves_the_coefficients(gpu_ctx):
    from groove_amd import entities as E
    n, frames = 65, 64
    rng = np.random.default_rng(6)
    for kind in ("lp12", "lp24"):
        a, twin = E.Effect(gpu_ctx, KINDS[kind], _with(n)), E.Effect(gpu_ctx, KINDS[kind], _with(n))
        link = E.ControlLink(gpu_ctx, T.ctl_sources(n, source=T.CTL_SRC_SIGNAL, law=T.CTL_LAW_AMPLITUDE), a, T.CTL_FX_CUTOFF, derived=True)
        side, io = gpu_ctx.block(n, CAP), gpu_ctx.block(n, CAP)
        same = lambda x: np.array_equal(_run(io, a, x).view(np.uint32), _run(io, twin, x).view(np.uint32))
        link.work(0)
        assert same(_audio(rng, n, frames))
        side.upload(_side_block(n, frames, _side_values(n, 1)))
        link.capture(side, 0)                                   # no frames transformed: nothing captured
        link.work(frames)
        assert same(_audio(rng, n, frames))
        link.capture(side, frames)
        link.work(2 * frames)
        assert not same(_audio(rng, n, frames))
        a.set_params(_with(n))                                  # the host's coefficients again
        a.reset(); twin.reset()
        link.reset()
        link.work(3 * frames)
        assert same(_audio(rng, n, frames))
        for x_ in (link, side, io, a, twin):
            x_.destroy()
    _zero_segments(gpu_ctx)


def test_a_linked_filter_inside_a_chain_matches_stage_by_stage(gpu_ctx):
    from groove_amd import entities as E
    n, sizes = 64, [64, 1, 37, 64]
    rng = np.random.default_rng(7)
    chain = [(T.FX_BIQUAD_LP12, _with(n)), (T.FX_GAIN, _params(n, ceiling=0.9)), (T.FX_COMPRESSOR, _params(n, limit_min=0.3, limit_max=0.2))]
    sources, _ = _lfo_sources(n)
    sets = []
    for which in range(3):                                            # stage by stage, as a chain, and stage by stage without links
        fx = [E.Effect(gpu_ctx, k, p) for k, p in chain]
        links = [] if which == 2 else [
            E.ControlLink(gpu_ctx, sources, fx[0], T.CTL_FX_CUTOFF, derived=True),
            E.ControlLink(gpu_ctx, T.ctl_sources(n, source=T.CTL_SRC_SIGNAL, law=T.CTL_LAW_AMPLITUDE), fx[0], T.CTL_FX_Q, derived=True),
            E.ControlLink(gpu_ctx, T.ctl_sources(n, source=T.CTL_SRC_SIGNAL, law=T.CTL_LAW_AMPLITUDE), fx[2], T.CTL_FX_THRESHOLD)]
        sets.append((fx, links, gpu_ctx.block(n, CAP)))
    side = gpu_ctx.block(n, CAP)
    at, moved = 0, False
    for fr in sizes:
        x, drums = _audio(rng, n, fr), _audio(rng, n, fr)
        side.upload(drums)
        outs = []
        for which, (fx, links, io) in enumerate(sets):
            for l in links:
                l.work(at)
            io.upload(x)
            if which == 1:
                gpu_ctx.transform_chain(fx, io, fr)
            else:
                for e in fx:
                    e.transform_audio(io, fr)
            for l in links[1:]:
                l.capture(side, fr)
            outs.append(io.download(fr))
        assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32)), at
        moved = moved or float(np.abs(outs[0] - outs[2]).max()) > 1e-3
        at += fr
    assert moved
    _zero_segments(gpu_ctx)
    for fx, links, io in sets:
        for x_ in links + fx + [io]:
            x_.destroy()
    side.destroy()


def test_filter_applies_do_not_wait_on_the_host_and_set_param_does(gpu_ctx):
    from groove_amd import entities as E
    n = 65
    lp = E.Effect(gpu_ctx, T.FX_BIQUAD_LP12, _with(n))
    src = gpu_ctx.block(n, CAP)
    lfo = E.ControlLink(gpu_ctx, T.ctl_sources(n, source=T.CTL_SRC_LFO, waveform=T.WAVE_SINE, frequency_hz=2.0), lp, T.CTL_FX_CUTOFF, derived=True)
    sig = E.ControlLink(gpu_ctx, T.ctl_sources(n, source=T.CTL_SRC_SIGNAL), lp, T.CTL_FX_Q, derived=True)
    waits = lambda: gpu_ctx.debug_info()["host_waits"]
    a = waits()
    own = waits() - a                                                # what reading the counter costs by itself
    a = waits()
    for b in range(10):
        lfo.work(b * 64)
        sig.capture(src, 64)
        sig.work(b * 64)
    assert waits() - a - own == 0                                   # twenty applies (and ten captures): not one host wait
    a = waits()
    for b in range(20):
        lp.control_set_param_by_index(T.CTL_FX_CUTOFF, 0.5)
    assert waits() - a - own >= 20
    _zero_segments(gpu_ctx)
    for x_ in (lfo, sig, src, lp):
        x_.destroy()


def test_refusals_each_with_its_message(gpu_ctx):
    from groove_amd import entities as E
    n = 4
    fx = {name: E.Effect(gpu_ctx, kind, _params(n)) for name, kind in (("gain", T.FX_GAIN), ("lp12", T.FX_BIQUAD_LP12), ("bp12", T.FX_BIQUAD_BP12), ("lp24", T.FX_BIQUAD_LP24))}
    lfo = lambda k=n, **kw: T.ctl_sources(k, source=T.CTL_SRC_LFO, frequency_hz=1.0, **{"waveform": T.WAVE_SINE, **kw})
    for target, index, msg in (("bp12", T.CTL_FX_Q, "does not derive its coefficients from that parameter"),
                               ("lp12", T.CTL_FX_PASSBAND_RIPPLE, "passband-ripple: low-pass 24 dB"),
                               ("lp24", T.CTL_FX_Q, "q: low-pass, high-pass and all-pass 12 dB"),
                               ("gain", T.CTL_FX_CUTOFF, "cutoff: the nine filter kinds"),
                               ("lp12", T.CTL_FX_WET, "kernel path"), ("gain", T.CTL_FX_WET, "kernel path"),
                               ("lp12", 99, "unknown control index"), ("lp12", T.CTL_WELSH_CUTOFF, "unknown control index"),
                               ("gain", T.CTL_FX_CEILING, "use groove_ctl_link_create")):
        with pytest.raises(_lib.GrooveError, match=msg):
            E.ControlLink(gpu_ctx, lfo(), fx[target], index, derived=True)
    with pytest.raises(_lib.GrooveError, match="groove_ctl_filter_link_create: .*no closed form"):
        E.ControlLink(gpu_ctx, lfo(waveform=T.WAVE_NOISE), fx["lp12"], T.CTL_FX_CUTOFF, derived=True)
    with pytest.raises(_lib.GrooveError, match="groove_ctl_filter_link_create: .*lane count"):
        E.ControlLink(gpu_ctx, lfo(3), fx["lp12"], T.CTL_FX_CUTOFF, derived=True)
    with pytest.raises(_lib.GrooveError, match="unknown signal law"):
        E.ControlLink(gpu_ctx, T.ctl_sources(n, source=T.CTL_SRC_SIGNAL, law=7), fx["lp12"], T.CTL_FX_CUTOFF, derived=True)
    link = E.ControlLink(gpu_ctx, lfo(), fx["lp12"], T.CTL_FX_CUTOFF, derived=True)
    link.work(0)
    fx["lp12"].destroy()
    with pytest.raises(_lib.GrooveError, match="destroyed"):
        link.work(64)
    _zero_segments(gpu_ctx)
    link.destroy()
    for name in ("gain", "bp12", "lp24"):
        fx[name].destroy()
