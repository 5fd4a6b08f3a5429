"""GPU tier: the SYNCHRONOUS block-writing walk over a big wave-uniform Welsh bank (csrc/groove_hip.hip launch_render: one kernel per
base kind present, 5 down to 0 — the first on the ctx stream, the others on forked side streams) against its asynchronous twin
(render_async_impl over big_pieces: the exact-f64 kinds 5 and 4 in a kernel each, then the MIX kernel's sections 2, 1, 0, every piece
on its side stream) bit for bit, and against the f64 oracle.  The two walks launch different kernels for kinds 0 - 3 — per-kind and
mix, both block-writing — around the same block bodies: that the bits agree is what lets either walk take the other's kernels.

pipeline_min_waves = 1 gives these small banks the big form.  Patches are representatives of tests/mix_bodies.py, whose key names the
base kind:
  A  seven patches of distinct class triples over kinds 0 - 3 (seven workgroups: sections of 3 / 2 / 2) and one each of kinds 4 and
     5, five voices per patch (partly filled waves): all six kinds, all five pieces;
  B  kinds 4 and 5 only: no mix section;
  C  kind 5 alone: one launch, no fork;
  D  one kind-0 patch: one workgroup, two empty sections;
  E  bank A's voices interleaved patch by patch (45 one-voice waves, which the plan sorts into workgroups by kind; a bank of this
     size keeps the caller's lane order: welsh_plan.h runs_are_long);
  F  the same interleaving at 228 voices per patch: 2,052 one-voice runs, past the 2,048 from which the library REGROUPS a bank
     patch-major, so that the walk writes the block's library-order buffer and the results are compared in the caller's lane order.
Blocks of 256, 37, 1 and 256 frames; every voice struck before block 0, every second one released before block 2.

For every bank and block: the generate_batch_values block, the voices' state and the groove_mix of the block onto a bus (through the
block's row sums) have the bits of the generate_batch_values_async twin's; every voice of the synchronous block is within 1e-5 RMS of
max(1, its level) of the oracle; the oracle sounds (RMS > 1e-3 over the timeline); no zero-frame segment was counted."""
import numpy as np
import pytest

from groove_amd import abi_types as T
from tests import mix_bodies as M

pytestmark = pytest.mark.gpu

SIZES = [256, 37, 1, 256]
RELEASE_BLOCK = 2
# body keys (base kind, LFO class, oscillator-1 class, oscillator-2 class, fp32-filter flag) of tests/mix_bodies.py
MIX_KEYS = [(0, 5, 2, 1, 0), (0, 4, 4, 3, 1), (1, 0, 0, 2, 0), (1, 3, 1, 4, 1), (2, 4, 2, 2, 0), (2, 3, 3, 1, 1), (3, 0, 4, 0, 0)]
KEY_4, KEY_5 = (4, 4, 2, 3, 0), (5, 2, 1, 2, 0)
PER_PATCH = 5
BANKS = {   # name: (keys, voices per patch, interleaved)
    "A five pieces": (MIX_KEYS + [KEY_4, KEY_5], PER_PATCH, False),
    "B exact-f64 kinds only": ([KEY_4, KEY_5], PER_PATCH, False),
    "C kind 5 alone": ([KEY_5], PER_PATCH, False),
    "D one kind-0 workgroup": ([MIX_KEYS[0]], PER_PATCH, False),
    "E interleaved": (MIX_KEYS + [KEY_4, KEY_5], PER_PATCH, True),
    "F interleaved and regrouped": (MIX_KEYS + [KEY_4, KEY_5], 228, True),
}
SOUNDS = 1e-3


def bank_params(name):
    keys, per_patch, interleaved = BANKS[name]
    assert len({k[1:4] for k in keys}) == len(keys)   # distinct class triples
    patches = [M.representative(k) for k in keys]
    assert all(p is not None and M.key(p) == k for p, k in zip(patches, keys))
    order = [p for _ in range(per_patch) for p in patches] if interleaved else [p for p in patches for _ in range(per_patch)]
    return (T.WelshParams * len(order))(*order)


def events_before(block, n):
    voices = np.arange(n, dtype=np.uint32)
    if block == RELEASE_BLOCK:
        voices = voices[::2]
    elif block != 0:
        return []
    keys = np.array([M.voice_key(v) for v in voices], dtype=np.uint8)
    return [T.note_events_np(voices, keys, block == 0)]


def oracle_blocks(oracle, params):
    """The oracle's blocks [2][frames][voices] float64 over the timeline."""
    ob = oracle.Bank.welsh(params)
    out = []
    for b, fr in enumerate(SIZES):
        for ev in events_before(b, len(params)):
            ob.note_events(ev)
        out.append(np.asarray(ob.render(fr), dtype=np.float64))
    return out


@pytest.fixture()
def big_form(gpu_ctx):
    old = gpu_ctx.time_parallel_max_voices, gpu_ctx.split_max_waves, gpu_ctx.pipeline_min_waves
    try:
        gpu_ctx.time_parallel_max_voices, gpu_ctx.split_max_waves, gpu_ctx.pipeline_min_waves = 0, 0, 1
        yield gpu_ctx
    finally:
        gpu_ctx.time_parallel_max_voices, gpu_ctx.split_max_waves, gpu_ctx.pipeline_min_waves = old


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


@pytest.mark.parametrize("name", list(BANKS))
def test_synchronous_walk_has_the_asynchronous_walks_bits(big_form, oracle, name):
    from groove_amd import entities as E
    ctx = big_form
    params = bank_params(name)
    n = len(params)
    want = oracle_blocks(oracle, params)
    level = float(np.sqrt(np.mean(np.concatenate(want, axis=1) ** 2)))
    print(f"{name}: {n} voices, oracle RMS {level:.3e}")
    assert level > SOUNDS, level
    sync, twin = E.WelshSynth(ctx, params), E.WelshSynth(ctx, params)
    blk_s, blk_a = ctx.block(n, max(SIZES)), ctx.block(n, max(SIZES))
    bus_s, bus_a = ctx.bus(max(SIZES)), ctx.bus(max(SIZES))
    try:
        for b, fr in enumerate(SIZES):
            for ev in events_before(b, n):
                sync.handle_midi_events(ev)
                twin.handle_midi_events(ev)
            sync.generate_batch_values(blk_s, fr)
            twin.generate_batch_values_async(blk_a, fr)
            ctx.mix([blk_s], fr, bus_s)   # (over the bus's first `fr` frames; what an earlier block left behind them was compared then)
            ctx.mix([blk_a], fr, bus_a)
            got, got_a = blk_s.download(fr), blk_a.download(fr)
            err = M.voice_errors(got, want[b])
            print(f"{name}: block {b} ({fr} frames): worst voice error {err.max():.3e} (bar {M.VOICE_BAR:g})")
            assert np.array_equal(_bits(got), _bits(got_a)), (name, b, "block", int(np.count_nonzero(_bits(got) != _bits(got_a))))
            assert np.array_equal(sync.download_state(), twin.download_state()), (name, b, "state")
            assert np.array_equal(_bits(bus_s.download()), _bits(bus_a.download())), (name, b, "bus")
            assert np.isfinite(got).all() and err.max() <= M.VOICE_BAR, (name, b, float(err.max()), int(err.argmax()))
        assert ctx.debug_info()["zero_segments"] == 0
    finally:
        sync.destroy(); twin.destroy(); blk_s.destroy(); blk_a.destroy(); bus_s.destroy(); bus_a.destroy()


def test_the_two_walks_are_named(big_form, name="A five pieces"):
    """The synchronous walk keeps the per-kind kernels (at 1,000,000 voices the mix kernel's three launches were 6 % slower there:
    docs/HISTORY.md section 17); the fused form names the mix kernel."""
    from groove_amd import entities as E
    s = E.WelshSynth(big_form, bank_params(name))
    try:
        form = s.kernel_form(256, False)
        assert "welsh_render_uniform_kernel" in form and "one launch per base kind" in form and "blocks pipelined" not in form, form
        fused = s.kernel_form(256, True)
        assert "mix_kernel" in fused and "blocks pipelined" in fused, fused
    finally:
        s.destroy()
