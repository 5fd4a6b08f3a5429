"""GPU tier: a partly wet reverb in the fused run (groove_set_fx_wet_reverb_run; kernels.h, the DRY instantiations).

With the knob on, a reverb with lanes below wet 1 takes the forms of an all-wet one — the table of tests/fx_forms.py — and must give
the bits of the serial kernel it takes with the knob off (the same wet-dry expression on the same operands).  Every case plays the
reverb walk of tests/fx_forms.py (7,870 frames at 44.1 kHz: six times the shortest comb, blocks on both sides of every switch), every
block a block of its own with nothing waiting on the host between the launches, as test_gpu_fx_forms.test_reverb_forms_hand_the_lines_over
does."""
import contextlib
import functools
import os

import numpy as np
import pytest

from groove_amd import abi_types as T
from tests import fx_forms as F
from tests.test_gpu_fx import _audio, _params
from tests.test_gpu_fx_forms import CAP, _check_block_sums, _differing, _oracle

pytestmark = pytest.mark.gpu

REVERB = dict(attenuation=0.9, reverb_seconds=0.8)
WALK = F.reverb_walk()
ALL_WET_FORMS = [F.DIR, F.DIR, F.CHK, F.CHK, F.R8, F.DIR, F.R8, F.DIR, F.DIR, F.R8, F.DIR]   # fx_forms._reverb_cases' `wet`
PATTERNS = {
    "one-lane-half": lambda i: 0.5 if i == 0 else 1.0,
    "every-third-0.6": lambda i: 0.6 if i % 3 == 0 else 1.0,
    "0.3-0.0-1.0": lambda i: (0.3, 0.0, 1.0)[i % 3],
}


@functools.lru_cache(maxsize=None)
def _forms():
    return F.library_forms()


def _all_wet_expectation(knobs):
    """What fx_forms._reverb_cases expects of an ALL-WET reverb under these knobs."""
    (case,) = [c for c in F.CASES if c.name == "reverb-n12" + ("-ap" if knobs.get("ap") else "-sequential" if knobs.get("env") else "")]
    assert case.walk == WALK
    return case.expect


def test_the_expectation_is_the_tables():
    assert _all_wet_expectation({}) == ALL_WET_FORMS
    assert _all_wet_expectation({"ap": True}) == [F.DIR_AP if f == F.DIR else f for f in ALL_WET_FORMS]
    assert _all_wet_expectation({"env": "GROOVE_FX_SEQ_ALLPASS"}) == [F.SEQ if f in (F.DIR, F.CHK) else f for f in ALL_WET_FORMS]


@contextlib.contextmanager
def _knobs(gpu_ctx, knobs, run):
    """The session's context with the all-pass stream and the run knob set (both off on entry, both restored), or a context of its own
    created under an environment variable."""
    from groove_amd import entities as E
    own = None
    if knobs.get("env"):
        os.environ[knobs["env"]] = "1"
        try:
            own = E.Context(0)
        finally:
            del os.environ[knobs["env"]]
    ctx = own or gpu_ctx
    assert not ctx.fx_wet_reverb_run and not ctx.fx_allpass_stream
    try:
        ctx.fx_allpass_stream = bool(knobs.get("ap"))
        ctx.fx_wet_reverb_run = run
        yield ctx
    finally:
        ctx.fx_wet_reverb_run = False
        ctx.fx_allpass_stream = False
        if own:
            own.close()


def _expect(fx, block, frames, tag, where):
    got, want = fx.kernel_form(block, frames), F.form_of_tag(tag, _forms())
    assert got == want, (where, frames, got, want)


def _play(ctx, fx, x, expect, name, reset_at=None, before_block=None):
    """x through the reverb over WALK, every block in flight; the form is asserted before every block.  Returns (output, last block)."""
    n = x.shape[2]
    blocks = [ctx.block(n, CAP) for _ in WALK]
    pos = 0
    for blk, fr in zip(blocks, WALK):
        blk.release()
        blk.upload(np.ascontiguousarray(x[:, pos:pos + fr, :]))
        pos += fr
    for i, (blk, fr) in enumerate(zip(blocks, WALK)):
        if reset_at == i:
            fx.reset()
        if before_block:
            before_block(i)
        _expect(fx, blk, fr, expect(i) if callable(expect) else expect[i], name)
        fx.transform_audio(blk, fr)
    out = [blk.download(fr) for blk, fr in zip(blocks, WALK)]
    for blk in blocks[:-1]:
        blk.destroy()
    return np.concatenate(out, axis=1), blocks[-1]


def _same_bits(a, b, what):
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (what, _differing(a, b), float(np.abs(a - b).max()))


@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("n", [1, 12, 72])
def test_partly_wet_reverb_takes_the_run_and_gives_the_serial_bits(gpu_ctx, oracle, n, pattern):
    """Forms and bits, and the lane sums the last launch leaves.  The knob-off arm is the serial kernel at every block (asserted: the
    knob off leaves a partly wet reverb where it was); the knob-on arms — all-pass stream off, on, and (12 lanes) the sequential
    all-pass in a context of its own — take the all-wet table's form at every block, give the knob-off bits, and sit within 4e-6 of
    the oracle (test_reverb_forms_hand_the_lines_over's bar).  A second pass resets the effect mid-walk.  groove_mix of the last
    block against the f64 lane sum of what it holds (2e-6 x scale) is what catches rows that sum the unmixed value."""
    from groove_amd import entities as E
    case = F.Case(f"wet-reverb-n{n}-{pattern}", T.FX_REVERB, dict(REVERB, wet=PATTERNS[pattern]), n, {}, WALK, None)
    x = _audio(n, sum(WALK), 24)
    reset_at = len(WALK) // 2
    with _knobs(gpu_ctx, {}, run=False) as ctx:
        fx = E.Effect(ctx, case.kind, F.fx_params(case))
        off, blk = _play(ctx, fx, x, [F.R8] * len(WALK), case.name + " knob off")
        _check_block_sums(ctx, blk, WALK[-1], case.name + " knob off")
        blk.destroy()
        fx.reset()
        off2, blk = _play(ctx, fx, x, [F.R8] * len(WALK), case.name + " knob off", reset_at=reset_at)
        fx.destroy(); blk.destroy()
    want, want2 = _oracle(oracle, case, x, WALK), _oracle(oracle, case, x, WALK, reset_at=reset_at)
    assert float(np.abs(want).max()) > 0.1
    err = float(np.abs(off - want).max())
    print(f"  {case.name}: knob off, worst error against the oracle {err:.3e}")
    assert err <= 4e-6 and np.abs(off2 - want2).max() <= 4e-6
    arms = [{}, {"ap": True}] + ([{"env": "GROOVE_FX_SEQ_ALLPASS"}] if n == 12 else [])
    for knobs in arms:
        name = f"{case.name} knob on {knobs}"
        expect = _all_wet_expectation(knobs)
        with _knobs(gpu_ctx, knobs, run=True) as ctx:
            fx = E.Effect(ctx, case.kind, F.fx_params(case))
            got, blk = _play(ctx, fx, x, expect, name)
            _check_block_sums(ctx, blk, WALK[-1], name)
            blk.destroy()
            fx.reset()
            again, blk = _play(ctx, fx, x, expect, name, reset_at=reset_at)
            fx.destroy(); blk.destroy()
        print(f"  {name}: {_differing(got, off)} of {got.size} samples differ from the knob-off arm's, worst error against the oracle "
              f"{float(np.abs(got - want).max()):.3e}")
        _same_bits(got, off, name)
        _same_bits(again, off2, name + ", second pass")
        assert np.abs(got - want).max() <= 4e-6 and np.abs(again - want2).max() <= 4e-6


@pytest.mark.parametrize("ap", [False, True])
@pytest.mark.parametrize("n", [1, 12])
def test_the_run_with_and_without_dry_alternate(gpu_ctx, n, ap):
    """groove_fx_set_param(ALL, WET, ...) between blocks, 1.0 -> 0.4 -> 1.0 -> 0.0 and round again: with the knob on the form is the
    all-wet table's at every block, launched without the dry store at 1.0 and with it below; the bits are the knob-off arm's, where the
    reverb moves between the run (at 1.0) and the serial kernel."""
    from groove_amd import entities as E
    wets = (1.0, 0.4, 1.0, 0.0)
    knobs = {"ap": ap}
    table = _all_wet_expectation(knobs)
    x = _audio(n, sum(WALK), 27)
    outs = {}
    for run in (False, True):
        with _knobs(gpu_ctx, knobs, run=run) as ctx:
            fx = E.Effect(ctx, T.FX_REVERB, _params(n, **REVERB))
            outs[run], blk = _play(ctx, fx, x, lambda i: table[i] if run or wets[i % 4] == 1.0 else F.R8, f"alternate n{n} ap={ap} run={run}",
                                   before_block=lambda i: fx.control_set_param_by_index(T.CTL_FX_WET, wets[i % 4]))
            _check_block_sums(ctx, blk, WALK[-1], f"alternate n{n} ap={ap} run={run}")
            fx.destroy(); blk.destroy()
    assert float(np.abs(outs[False]).max()) > 0.1
    _same_bits(outs[True], outs[False], f"alternate n{n} ap={ap}")


@pytest.mark.parametrize("n", [6, 64])
def test_chains_with_a_partly_wet_reverb(gpu_ctx, n):
    """gain -> chorus -> delay -> reverb and reverb -> limiter over the reverb's walk, the reverb partly wet, knob on: the chain
    (groove_fx_chain_process, the reverb's combs fused with the stages in front of it) is the stage-by-stage walk bit for bit at every
    block, and both are the chain with the knob off, where the run is cut in front of the serial reverb."""
    from groove_amd import entities as E
    part = [1.0 if i % 3 else 0.6 for i in range(n)]
    rev = (T.FX_REVERB, _params(n, wet=[(0.3, 0.0, 1.0)[i % 3] for i in range(n)], **REVERB))
    chains = {"gain-chorus-delay-reverb": [(T.FX_GAIN, _params(n, ceiling=[0.5 + 0.4 * i / n for i in range(n)])),
                                           (T.FX_CHORUS, _params(n, voices=3, delay_seconds=0.03, wet=part)),
                                           (T.FX_DELAY, _params(n, delay_seconds=0.012, wet=part)), rev],
              "reverb-limiter": [rev, (T.FX_LIMITER, _params(n, limit_min=0.0, limit_max=0.7))]}
    ncomb, nap = min(F.comb_frames()), min(F.allpass_frames())
    x = _audio(n, sum(WALK), seed=25)
    for name, chain in chains.items():
        ri = [k for k, _ in chain].index(T.FX_REVERB)
        with _knobs(gpu_ctx, {}, run=False) as ctx:   # the knob-off arm: the parent's path
            c = [E.Effect(ctx, k, p) for k, p in chain]
            bc = ctx.block(n, CAP)
            off, pos = [], 0
            for fr in WALK:
                bc.upload(np.ascontiguousarray(x[:, pos:pos + fr, :]))
                _expect(c[ri], bc, fr, F.R8, name + " knob off")
                ctx.transform_chain(c, bc, fr)
                off.append(bc.download(fr))
                pos += fr
            for e in c:
                e.destroy()
            bc.destroy()
        assert max(float(np.abs(o).max()) for o in off) > 1e-2
        for ap in (False, True):
            with _knobs(gpu_ctx, {"ap": ap}, run=True) as ctx:
                a = [E.Effect(ctx, k, p) for k, p in chain]
                b = [E.Effect(ctx, k, p) for k, p in chain]
                ba, bb = ctx.block(n, CAP), ctx.block(n, CAP)
                ba.release(); bb.release()
                pos = 0
                for i, fr in enumerate(WALK):
                    chunk = np.ascontiguousarray(x[:, pos:pos + fr, :])
                    ba.upload(chunk); bb.upload(chunk)
                    _expect(a[ri], ba, fr, F.R8 if fr > ncomb else F.CHK if fr > 8 * nap else F.DIR_AP if ap else F.DIR, name)
                    for e in a:
                        e.transform_audio(ba, fr)
                    ctx.transform_chain(b, bb, fr)
                    ga, gb = ba.download(fr), bb.download(fr)
                    _same_bits(ga, gb, (name, "chain against stage by stage", ap, pos, fr))
                    _same_bits(gb, off[i], (name, "knob on against knob off", ap, pos, fr))
                    pos += fr
                _check_block_sums(ctx, bb, WALK[-1], name)
                for e in a + b:
                    e.destroy()
                ba.destroy(); bb.destroy()


def test_knob_off_keeps_a_partly_wet_reverb_serial(gpu_ctx):
    """Default off, and off means today's form decision: serial for a partly wet reverb at a block length an all-wet one fuses."""
    from groove_amd import entities as E
    assert not gpu_ctx.fx_wet_reverb_run
    blk = gpu_ctx.block(12, CAP)
    part = E.Effect(gpu_ctx, T.FX_REVERB, _params(12, wet=[0.5] + [1.0] * 11, **REVERB))
    full = E.Effect(gpu_ctx, T.FX_REVERB, _params(12, **REVERB))
    try:
        _expect(part, blk, 256, F.R8, "knob off")
        _expect(full, blk, 256, F.DIR, "knob off")
        gpu_ctx.fx_wet_reverb_run = True
        assert gpu_ctx.fx_wet_reverb_run
        _expect(part, blk, 256, F.DIR, "knob on")
        _expect(full, blk, 256, F.DIR, "knob on")
    finally:
        gpu_ctx.fx_wet_reverb_run = False
    _expect(part, blk, 256, F.R8, "knob off again")
    part.destroy(); full.destroy(); blk.destroy()
