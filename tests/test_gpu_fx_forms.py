"""GPU tier: every effect kernel form, on both sides of the switch that picks it (the case table of tests/fx_forms.py).

Every case plays a unit-scale pseudo-audio stream (test_gpu_fx._audio: the second half silent, so that tails ring out) block by block
through blocks of 2,048 frames' capacity, so that the channel stride differs from frames x lanes almost everywhere; before every block
the library is asked which form it takes (groove_fx_kernel_form) and the answer is held against the table.  Per case:

  - the f64 oracle stepping in the same blocks, at the bars tests/test_gpu_fx.py holds the kind to;
  - a reference that knows nothing of blocks (LP12: scipy's lfilter over the whole stream with the bilinear transform of the analog
    prototype, the design of tests/test_gpu_independent.py; the pure delay: the input shifted by N frames, exactly);
  - split invariance: the same stream in uniform 256-frame blocks, one form throughout;
  - the block's lane sums after the last block: groove_mix against the f64 lane sum of what the block holds.

The last test of the module lists how many blocks took each form."""
import collections
import contextlib
import functools
import math
import os

import numpy as np
import pytest

from groove_amd import abi_types as T
from tests import fx_forms as F
from tests.test_gpu_fx import _audio

pytestmark = pytest.mark.gpu

CAP = 2048
BLOCKS_OF_FORM = collections.Counter()   # library string -> blocks played in it, this session
PLAYED = set()                           # case names
ULP = 2.0 ** -23                         # fp32 spacing at unit scale


@functools.lru_cache(maxsize=None)
def _forms():
    return F.library_forms()


def _cases(prefix, pred=lambda c: True):
    return [c for c in F.CASES if c.name.startswith(prefix) and pred(c)]


@contextlib.contextmanager
def _knobs(gpu_ctx, knobs):
    """The context a case plays in: the session's with the case's knobs set (and restored), or one of its own under an environment variable."""
    from groove_amd import entities as E
    if knobs.get("env"):
        os.environ[knobs["env"]] = "1"
        try:
            ctx = E.Context(0)
        finally:
            del os.environ[knobs["env"]]
        try:
            yield ctx
        finally:
            ctx.close()
        return
    old_tp = gpu_ctx.time_parallel_max_voices
    if not knobs.get("tp", True):
        gpu_ctx.time_parallel_max_voices = 0
    if knobs.get("ap"):
        assert not gpu_ctx.fx_allpass_stream
        gpu_ctx.fx_allpass_stream = True
    try:
        yield gpu_ctx
    finally:
        gpu_ctx.time_parallel_max_voices = old_tp
        if knobs.get("ap"):
            gpu_ctx.fx_allpass_stream = False


def _expect(fx, block, frames, tag, where):
    got = fx.kernel_form(block, frames)
    want = F.form_of_tag(tag, _forms())
    assert got == want, (where, frames, got, want)
    BLOCKS_OF_FORM[want] += 1


def _play(ctx, fx, x, walk, expect=None, name="", reset_at=None, in_flight=False):
    """x[2][>= sum(walk)][n] through one effect, block by block.  in_flight: every block of the walk is a block of its own, all uploaded
    before the first launch and downloaded after the last, so that no host wait sits between the launches (and every block is released
    once, which is what lets a reverb's all-passes leave for the all-pass stream).  Returns (output, the last block, its frames)."""
    n = x.shape[2]
    blocks = [ctx.block(n, CAP) for _ in (walk if in_flight else walk[:1])]
    out, pos = [], 0
    if in_flight:
        for blk, fr in zip(blocks, walk):
            blk.release()
            blk.upload(np.ascontiguousarray(x[:, pos:pos + fr, :]))
            pos += fr
        pos = 0
    for i, fr in enumerate(walk):
        blk = blocks[i] if in_flight else blocks[0]
        if not in_flight:
            blk.upload(np.ascontiguousarray(x[:, pos:pos + fr, :]))
        if reset_at == i:
            fx.reset()
        if expect is not None:
            _expect(fx, blk, fr, expect[i], name)
        fx.transform_audio(blk, fr)
        if not in_flight:
            out.append(blk.download(fr))
        pos += fr
    if in_flight:
        out = [blk.download(fr) for blk, fr in zip(blocks, walk)]
        for blk in blocks[:-1]:
            blk.destroy()
    return np.concatenate(out, axis=1), blocks[-1], walk[-1]


def _oracle(oracle, case, x, walk, reset_at=None, sr=T.DEFAULT_SAMPLE_RATE):
    params = F.fx_params(case)
    ofx = oracle.Fx(case.kind, params, sr)
    out, pos = [], 0
    for i, fr in enumerate(walk):
        if reset_at == i:
            ofx = oracle.Fx(case.kind, params, sr)
        out.append(ofx.process(np.ascontiguousarray(x[:, pos:pos + fr, :]).astype(np.float64)))
        pos += fr
    return np.concatenate(out, axis=1)


def _uniform(total):
    return [256] * (total // 256) + ([total % 256] if total % 256 else [])


def _stream(case, seed):
    """The case's input, padded to whole 256-frame blocks for the uniform walk (silent like the rest of the second half)."""
    total = sum(case.walk)
    x = _audio(case.n, total, seed)
    pad = -total % 256
    return np.concatenate([x, np.zeros((2, pad, case.n), np.float32)], axis=1), total


def _check_block_sums(ctx, block, frames, name):
    """groove_mix of the block the case's last launch left (its row sums, where the form leaves them; the block itself otherwise)
    against the f64 lane sum of what the block holds: test_chain_leaves_the_blocks_lane_sums_for_the_mix's bar."""
    bus = ctx.bus(frames)
    ctx.mix([block], frames, bus)
    got = bus.download(frames).astype(np.float64)
    held = block.download(frames).astype(np.float64)
    want = held.sum(axis=2).T
    scale = max(1.0, float(np.abs(held).sum(axis=2).max()))
    bus.destroy()
    assert np.max(np.abs(got - want)) <= 2e-6 * scale, (name, frames, float(np.max(np.abs(got - want))))


def _differing(a, b):
    return int(np.count_nonzero(a.view(np.uint32) != b.view(np.uint32)))


def _split_invariance(name, got, uni, peak, exact):
    """The walk against the same stream in uniform blocks: the same bits, or (forms whose start states agree to f64 rounding, so that
    an output differs only where an f64 value sits on an fp32 rounding boundary) the fp32 spacing at the signal's scale."""
    worst = float(np.abs(got.astype(np.float64) - uni.astype(np.float64)).max())
    print(f"  {name}: {_differing(got, uni)} of {got.size} samples differ from the uniform walk's, worst {worst:.3e}")
    if exact:
        assert np.array_equal(got.view(np.uint32), uni.view(np.uint32)), (name, _differing(got, uni), worst)
    else:
        assert worst <= ULP * max(1.0, peak), (name, worst, peak)


def _wet(case):
    w = case.params.get("wet", 1.0)
    return np.array([np.float32(w(i) if callable(w) else w) for i in range(case.n)], dtype=np.float32)


def _lp12_whole_stream(case, x, lanes):
    """scipy's lfilter over the whole stream, lane by lane: the bilinear transform of H(s) = 1 / (s^2 + s / Q + 1), s -> s / k
    (tests/test_gpu_independent.py), then the wet / dry mix."""
    from scipy import signal
    xd = x.astype(np.float64)
    want = np.empty((2, x.shape[1], len(lanes)))
    wet = _wet(case).astype(np.float64)
    for j, i in enumerate(lanes):
        f0 = float(np.float32(case.params["cutoff_hz"](i))); q = float(np.float32(case.params["q"](i)))
        k = math.tan(math.pi * f0 / F.SR)
        b, a = signal.bilinear([1.0], [1.0 / k ** 2, 1.0 / (q * k), 1.0], fs=0.5)
        y = signal.lfilter(b / a[0], a / a[0], xd[:, :, i], axis=1)
        want[:, :, j] = y * wet[i] + xd[:, :, i] * (1.0 - wet[i])
    return want


def _iir_case(gpu_ctx, oracle, case, seed=21):
    from groove_amd import entities as E
    from tests.test_gpu_independent import _close
    x, total = _stream(case, seed)
    with _knobs(gpu_ctx, case.knobs) as ctx:
        fx, fu = E.Effect(ctx, case.kind, F.fx_params(case)), E.Effect(ctx, case.kind, F.fx_params(case))
        got, blk, last = _play(ctx, fx, x, case.walk, case.expect, case.name)
        _check_block_sums(ctx, blk, last, case.name)
        uni, bu, _ = _play(ctx, fu, x, _uniform(x.shape[1]))
        fx.destroy(); fu.destroy(); blk.destroy(); bu.destroy()
    want = _oracle(oracle, case, x, case.walk)
    peak = float(np.abs(want).max())
    err = float(np.abs(got - want).max())
    print(f"  {case.name}: worst error against the oracle {err:.3e}, peak {peak:.3f}")
    assert peak > 0.05 and np.isfinite(got).all()
    if case.kind in (T.FX_BIQUAD_LP12, T.FX_BIQUAD_HP12, T.FX_BIQUAD_LP24):
        assert err <= 2e-6, (case.name, err)
    else:
        assert err <= 4e-6 * max(1.0, peak), (case.name, err, peak)
    if case.kind == T.FX_BIQUAD_LP12:
        # (a bank of tens of thousands of lanes: every sixteenth lane and the last 512, the ragged end of the grid)
        lanes = list(range(case.n)) if case.n <= 4096 else sorted(set(range(0, case.n, 16)) | set(range(case.n - 512, case.n)))
        _close(got[:, :, lanes], _lp12_whole_stream(case, x[:, :total, :], lanes))
    _split_invariance(case.name, got, uni[:, :total, :], peak, exact=False)
    PLAYED.add(case.name)


@pytest.mark.parametrize("kind", ["lp12", "peak12", "lp24"])
def test_iir_forms_hand_a_stream_over(gpu_ctx, oracle, kind):
    """LP12, PEAK12 (all five coefficients non-zero) and the 24 dB low-pass, cutoffs 40 Hz - 6 kHz, q 0.5 - 20 (the demo projects'
    extreme), ripple 0.71 - 3, every third lane partly wet: a stream that moves between the time-parallel (or, with that knob at 0, the
    four-segment) form and the serial kernel over one [4][2n] f64 state record — block lengths on both sides of 15 | 16 and 256 | 257,
    across the four-segment kernel's straight-line / predicated switch (253 - 256), down to blocks shorter than a lane's four frames;
    3 lanes, 130 (a ragged 8-lane tile), and on both sides of the lane count that switches the form."""
    for case in _cases(kind + "-", lambda c: c.n <= 2049):
        _iir_case(gpu_ctx, oracle, case)


@pytest.mark.parametrize("n", [24576, 24577])
def test_biquad_bank_of_24576_lanes_and_one_more(gpu_ctx, oracle, n):
    """The largest bank the four-segment kernel takes and the first the serial kernel takes at every block length: its whole-chunk
    branch (feed-forward sweep first, feedback chain second) over 193 workgroups with a ragged last one."""
    (case,) = _cases(f"lp12-n{n}")
    _iir_case(gpu_ctx, oracle, case)


@pytest.mark.parametrize("n", [6, 64])
def test_delay_lines_as_long_as_the_block(gpu_ctx, oracle, n):
    """N - 1, N, N + 1 frames through a line of N (the fused run up to N, the serial kernel above), several trips round a short ring
    inside one launch (2N + 3, 1,024), a line under 16 frames (chunk 1).  Fully wet lanes are exact against the oracle and ARE the
    input N frames earlier; partly wet ones to 1e-6 (test_short_delay_and_ragged_blocks's bar: one fp32 mix); the uniform walk gives
    the same bits."""
    from groove_amd import entities as E
    for case in _cases("delay-", lambda c: c.n == n):
        x, total = _stream(case, 22)
        with _knobs(gpu_ctx, case.knobs) as ctx:
            fx, fu = E.Effect(ctx, case.kind, F.fx_params(case)), E.Effect(ctx, case.kind, F.fx_params(case))
            got, blk, last = _play(ctx, fx, x, case.walk, case.expect, case.name)
            _check_block_sums(ctx, blk, last, case.name)
            uni, bu, _ = _play(ctx, fu, x, _uniform(x.shape[1]))
            fx.destroy(); fu.destroy(); blk.destroy(); bu.destroy()
        want = _oracle(oracle, case, x, case.walk)
        full = _wet(case) == 1.0
        assert full.any() and not full.all()
        assert np.array_equal(got[:, :, full], want[:, :, full].astype(np.float32)), case.name
        assert np.abs(got[:, :, ~full] - want[:, :, ~full]).max() <= 1e-6, case.name
        N = F.delay_frames(case.params["delay_seconds"])
        shifted = np.zeros_like(got)
        shifted[:, N:, :] = x[:, :total - N, :]
        assert np.abs(shifted).max() > 0.1
        assert np.array_equal(got[:, :, full].view(np.uint32), shifted[:, :, full].view(np.uint32)), case.name
        _split_invariance(case.name, got, uni[:, :total, :], 1.0, exact=True)
        PLAYED.add(case.name)


# Whether the serial kernels and the fused run contract their multiply-adds alike is not something the source settles.  Measured on an
# MI355X (the first run of this module): for every chorus and reverb case 0 samples differ between the walk and the uniform walk, worst
# difference 0.0 — so bit equality is what is asserted.
CHORUS_SPLIT_EXACT = True
REVERB_SPLIT_EXACT = True


@pytest.mark.parametrize("n", [6, 64])
def test_chorus_taps_on_both_sides_of_the_block(gpu_ctx, oracle, n):
    """Three voices at 0.03 s around the tap spacing (with several voices the nearest tap is never nearer than the spacing, so that limit
    binds), one voice at 0.004 s around the nearest tap (N: the limit that binds alone there), a 2,048-frame block (more than a trip
    round the ring in one launch), four voices at 0.0005 s (spacing under 16: chunk 1).  2e-6 against the oracle.  Split invariance,
    measured: 0 samples of any case differ from the uniform walk's (59,412 / 15,372 at 6 lanes, 633,728 / 163,968 at 64), worst
    difference 0.0: the same bits are asserted."""
    from groove_amd import entities as E
    for case in _cases("chorus-", lambda c: c.n == n):
        x, total = _stream(case, 23)
        with _knobs(gpu_ctx, case.knobs) as ctx:
            fx, fu = E.Effect(ctx, case.kind, F.fx_params(case)), E.Effect(ctx, case.kind, F.fx_params(case))
            got, blk, last = _play(ctx, fx, x, case.walk, case.expect, case.name)
            _check_block_sums(ctx, blk, last, case.name)
            uni, bu, _ = _play(ctx, fu, x, _uniform(x.shape[1]))
            fx.destroy(); fu.destroy(); blk.destroy(); bu.destroy()
        want = _oracle(oracle, case, x, case.walk)
        peak = float(np.abs(want).max())
        assert peak > 0.1
        assert np.abs(got - want).max() <= 2e-6, (case.name, float(np.abs(got - want).max()))
        _split_invariance(case.name, got, uni[:, :total, :], peak, exact=CHORUS_SPLIT_EXACT)
        PLAYED.add(case.name)


@pytest.mark.parametrize("n", [1, 12, 72])
def test_reverb_forms_hand_the_lines_over(gpu_ctx, oracle, n):
    """All-wet reverb, 0.8 s: blocks on both sides of 8 x the shorter all-pass line (direct | chunked all-pass) and of the shortest comb
    (fused run | the serial kernel partly-wet reverbs take), a 2,048-frame block, single frames, with the all-pass stream off and on.
    The direct form keeps two copies of the all-pass rings and swaps their bases on the host after every block; with the all-pass
    stream on its kernel runs beside the ctx stream.  Every block of the walk is a block of its own and nothing waits on the host
    between the launches: the serial kernel of the next block must find the swapped base and wait for that stream by itself.  A second
    pass resets the effect in the middle.  One lane at wet 0.5 makes the reverb serial throughout: the control.  4e-6 against the
    oracle.  Split invariance, measured: 0 of 15,740 / 188,880 / 1,133,280 samples (1 / 12 / 72 lanes) differ from the uniform
    walk's in every case (all-pass stream off and on, sequential all-pass, the partly-wet control), worst difference 0.0: the same bits are
    asserted."""
    from groove_amd import entities as E
    for case in _cases("reverb-", lambda c: c.n == n):
        x, total = _stream(case, 24)
        reset_at = len(case.walk) // 2
        with _knobs(gpu_ctx, case.knobs) as ctx:
            fx, fu = E.Effect(ctx, case.kind, F.fx_params(case)), E.Effect(ctx, case.kind, F.fx_params(case))
            got, blk, last = _play(ctx, fx, x, case.walk, case.expect, case.name, in_flight=True)
            _check_block_sums(ctx, blk, last, case.name)
            blk.destroy()
            fx.reset()
            again, blk, _ = _play(ctx, fx, x, case.walk, case.expect, case.name, reset_at=reset_at, in_flight=True)
            uni, bu, _ = _play(ctx, fu, x, _uniform(x.shape[1]))
            fx.destroy(); fu.destroy(); blk.destroy(); bu.destroy()
        want = _oracle(oracle, case, x, case.walk)
        peak = float(np.abs(want).max())
        assert peak > 0.1
        assert np.abs(got - want).max() <= 4e-6, (case.name, float(np.abs(got - want).max()))
        want2 = _oracle(oracle, case, x, case.walk, reset_at=reset_at)
        assert np.abs(again - want2).max() <= 4e-6, (case.name, "second pass", float(np.abs(again - want2).max()))
        _split_invariance(case.name, got, uni[:, :total, :], peak, exact=REVERB_SPLIT_EXACT)
        PLAYED.add(case.name)


@pytest.mark.parametrize("n", [6, 64])
def test_chains_at_the_long_walk(gpu_ctx, n):
    """gain -> chorus -> delay -> reverb and reverb -> limiter over the reverb's walk (blocks of up to 2,048 frames, on both sides of
    every line length): groove_fx_chain_process, which groups the stages into fused runs as each block's length allows, is the
    stage-by-stage walk bit for bit at every block (test_chain_process_equals_stage_by_stage's property at <= 256 frames).  In the
    second chain the reverb is not the last launch, so it takes no all-pass stream."""
    from groove_amd import entities as E
    from tests.test_gpu_fx import _params
    walk = F.reverb_walk()
    part = [1.0 if i % 3 else 0.6 for i in range(n)]
    chains = {"gain-chorus-delay-reverb": [(T.FX_GAIN, _params(n, ceiling=[0.5 + 0.4 * i / n for i in range(n)])),
                                           (T.FX_CHORUS, _params(n, voices=3, delay_seconds=0.03, wet=part)),
                                           (T.FX_DELAY, _params(n, delay_seconds=0.012, wet=part)),
                                           (T.FX_REVERB, _params(n, attenuation=0.9, reverb_seconds=0.8))],
              "reverb-limiter": [(T.FX_REVERB, _params(n, attenuation=0.9, reverb_seconds=0.8)),
                                 (T.FX_LIMITER, _params(n, limit_min=0.0, limit_max=0.7))]}
    _, spacing, _ = F.chorus_geometry(0.03, 3)
    N, ncomb, nap = F.delay_frames(0.012), min(F.comb_frames()), min(F.allpass_frames())
    x = _audio(n, sum(walk), seed=25)
    for name, chain in chains.items():
        for ap in (False, True):
            with _knobs(gpu_ctx, {"ap": ap}) as ctx:
                a = [E.Effect(ctx, k, p) for k, p in chain]
                b = [E.Effect(ctx, k, p) for k, p in chain]
                ba, bb = ctx.block(n, CAP), ctx.block(n, CAP)
                ba.release(); bb.release()
                pos, peak = 0, 0.0
                for fr in walk:
                    chunk = np.ascontiguousarray(x[:, pos:pos + fr, :])
                    ba.upload(chunk); bb.upload(chunk)
                    for e, (k, _) in zip(a, chain):   # (stage by stage every launch is the last of its chain: the reverb rides the all-pass stream)
                        tag = {T.FX_GAIN: F.RUN, T.FX_LIMITER: F.RUN,
                               T.FX_CHORUS: F.RUN if fr <= spacing else F.C16,
                               T.FX_DELAY: F.RUN if fr <= N else F.D16,
                               T.FX_REVERB: F.R8 if fr > ncomb else F.CHK if fr > 8 * nap else F.DIR_AP if ap else F.DIR}[k]
                        _expect(e, ba, fr, tag, name)
                        e.transform_audio(ba, fr)
                    ctx.transform_chain(b, bb, fr)
                    ga, gb = ba.download(fr), bb.download(fr)
                    assert np.array_equal(ga.view(np.uint32), gb.view(np.uint32)), (name, ap, pos, fr, _differing(ga, gb))
                    peak = max(peak, float(np.abs(ga).max()))
                    pos += fr
                assert peak > 1e-2
                _check_block_sums(ctx, bb, walk[-1], name)
                for e in a + b:
                    e.destroy()
                ba.destroy(); bb.destroy()
    PLAYED.add(f"chains-n{n}")


def test_identity_and_element_wise_forms(gpu_ctx):
    """The Mixer launches nothing and an element-wise kind is always a stage of the fused run, whatever the block length."""
    from groove_amd import entities as E
    for case in _cases("mixer-") + _cases("gain-"):
        x, total = _stream(case, 26)
        fx = E.Effect(gpu_ctx, case.kind, F.fx_params(case))
        got, blk, last = _play(gpu_ctx, fx, x, case.walk, case.expect, case.name)
        _check_block_sums(gpu_ctx, blk, last, case.name)
        ceil = np.array([np.float32(case.params["ceiling"](i)) for i in range(case.n)]) if case.kind == T.FX_GAIN else np.float32(1.0)
        assert np.array_equal(got, x[:, :total, :] * ceil), case.name
        fx.destroy(); blk.destroy()
        PLAYED.add(case.name)


def test_every_form_was_played():
    """How many blocks took each form in this session; none that the table reaches may be zero.  (Asserted when the whole module ran.)"""
    forms = _forms()
    for form in forms:
        print(f"  {BLOCKS_OF_FORM[form]:5d} blocks  {form}")
    everything = {c.name for c in F.CASES} | {"chains-n6", "chains-n64"}
    if PLAYED != everything:
        print(f"  (a partial session: {len(PLAYED)} of {len(everything)} cases played)")
        return
    unreachable = {F.form_of_tag(t, forms) for t in F.UNREACHABLE_REASONS if t in F.TAGS}
    assert [f for f in forms if f not in unreachable and BLOCKS_OF_FORM[f] == 0] == []
    assert all(BLOCKS_OF_FORM[f] == 0 for f in unreachable)
