"""GPU tier: sampler and drumkit banks over STEREO sample memory (include/groove_hip.h groove_sampler_create_stereo,
groove_bank_sample_channels; csrc/dsp_core.h sampler_chunk_stereo; csrc/kernels.h sampler_render_kernel<FUSED, true>; csrc/welsh_tp.h
sampler_tp_body<FUSED, WAVES, true>).

The reference is numpy, docs/DSP_SPEC.md section 7 restated: per voice the events are replayed on (idx, step, playing), frame f of a
block reads i = (idx + f * step) >> 44 in exact 64-bit integers, and the voice's output is float32(pcm[offset + i, ch]) * float32(gain),
one fp32 multiply per channel.  The block-writing forms are held to it BIT FOR BIT; the fused buses to the f64 sum of those values within
the project's bar (section 10: bus RMS / V <= 1e-5 of full scale), and to themselves bit for bit under a swap of the bank's channels.

Forms: the time-parallel kernel at 5 voices (one partial wave), 70 (crosses a wave), 300 (several workgroups), 1,100 (two voices per
wavefront) and 4,100 (five per wavefront: one full group of four fetch sets and a partial one); the serial kernel at 70 and 300 (crosses a
256-thread workgroup).  Block lengths 64, 37, 17, 256 in one walk (17 and 37 straddle the 16-frame chunk and the 4-frame lane chunk);
samples of length 1, 100 and 5,000; keys below, at and above the root and a drumkit sample; a note-off a sampler voice obeys and a
one-shot ignores; a re-trigger of sounding voices; left and right are independent noise.

Every test ends on zero_segments == 0 and fast_table_misses == 0."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from groove_amd import abi_types as T, lib as _lib, patches as P

pytestmark = pytest.mark.gpu

SIZES = [64, 37, 17, 256, 64, 37, 17, 256]
STARTS = [int(x) for x in np.concatenate([[0], np.cumsum(SIZES)[:-1]])]
TOTAL = sum(SIZES)
ON_BLOCKS, OFF_BLOCK = (0, 3), 2                                   # on; off (one-shots play on); on again: a re-trigger of what still sounds
LENGTHS = (1, 100, 5000, 5000)                                     # the last one is the drumkit sample (root_hz 0: step 1 whatever the key)
ROOTS = (440.0, 440.0, 440.0, 0.0)
FORMS = {                                                          # name: (voices, time_parallel_max_voices or None, what kernel_form says)
    "tp-5": (5, None, "sampler_tp_kernel"), "tp-70": (70, None, "sampler_tp_kernel"), "tp-300": (300, None, "sampler_tp_kernel"),
    "tp-1100": (1100, None, "sampler_tp_kernel"), "tp-4100": (4100, None, "sampler_tp_kernel"),
    "serial-70": (70, 0, "sampler_render_kernel (serial"), "serial-300": (300, 0, "sampler_render_kernel (serial"),
}
_CACHE = {}


def _bank():
    """(pcm [frames, 2] float32, descs): left and right independent noise."""
    if "bank" not in _CACHE:
        rng = np.random.default_rng(20240607)
        pcm = (rng.standard_normal((sum(LENGTHS), 2)) * 0.3).astype(np.float32)
        descs = (T.SampleDesc * len(LENGTHS))()
        off = 0
        for k, ln in enumerate(LENGTHS):
            descs[k].offset, descs[k].length, descs[k].root_hz = off, ln, ROOTS[k]
            off += ln
        pcm.setflags(write=False)
        _CACHE["bank"] = (pcm, descs)
    return _CACHE["bank"]


def _keys(n):
    return (57 + (12 * np.arange(n)) % 25).astype(np.uint8)         # voice 0: 57 (step 1/2), 1: 69 (step 1), 2: 81 (step 2), ...


def _sample_of(n):
    return np.arange(n) % len(LENGTHS)


def _one_shot(n):
    return (np.arange(n) // len(LENGTHS)) % 2


def _gains(n):
    return (0.25 + 0.5 * ((np.arange(n) * 7) % 11) / 11.0).astype(np.float32)


def _params(n):
    arr = (T.SamplerParams * n)()
    raw = np.zeros(n, dtype=np.dtype([("sample_index", "<u4"), ("one_shot", "<u4"), ("gain", "<f4")]))
    raw["sample_index"], raw["one_shot"], raw["gain"] = _sample_of(n), _one_shot(n), _gains(n)
    C.memmove(arr, raw.tobytes(), n * C.sizeof(T.SamplerParams))
    return arr


def _events(n, k):
    lanes, keys, out = np.arange(n, dtype=np.uint32), _keys(n), []
    if k in ON_BLOCKS:
        out.append(T.note_events_np(lanes, keys, True))
    if k == OFF_BLOCK:
        out.append(T.note_events_np(lanes, keys, False))
    return out


def _reference(n, gain_from=None):
    """The walk in numpy: blocks [k] -> [2][frames][n] float32 (exact), and the final (idx, step, playing).  gain_from = (block, value):
    every voice's gain is float32(value) from that block on (groove_bank_set_param's law for a sampler's gain is the clamp to 0..1)."""
    key = (n, gain_from)
    if key in _CACHE:
        return _CACHE[key]
    pcm, descs = _bank()
    smp = _sample_of(n)
    offset = np.array([descs[s].offset for s in smp], dtype=np.int64)
    length = np.array([descs[s].length for s in smp], dtype=np.uint64)
    root = np.array([ROOTS[s] for s in smp], dtype=np.float64)
    one_shot, gain = _one_shot(n).astype(bool), _gains(n)
    freq = 440.0 * np.exp2((_keys(n).astype(np.float64) - 69.0) / 12.0)
    ratio = np.where(root > 0.0, freq / np.where(root > 0.0, root, 1.0), 1.0)
    note_step = (ratio * 17592186044416.0).astype(np.uint64)         # truncation, 2^44
    idx, step, playing = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=bool)
    blocks = []
    for k, frames in enumerate(SIZES):
        if k in ON_BLOCKS:
            idx[:], step[:], playing[:] = 0, note_step, True
        if k == OFF_BLOCK:
            playing &= one_shot
        if gain_from is not None and k == gain_from[0]:
            gain = np.full(n, np.float32(gain_from[1]), dtype=np.float32)
        f = np.arange(frames, dtype=np.uint64)
        i = (idx[None, :] + f[:, None] * step[None, :]) >> np.uint64(44)      # [frames][n], exact in 64 bits (idx < 2^57, f * step < 2^54)
        ok = playing[None, :] & (i < length[None, :])
        at = offset[None, :] + np.minimum(i, length[None, :] - np.uint64(1)).astype(np.int64)
        out = np.zeros((2, frames, n), dtype=np.float32)
        for ch in range(2):
            out[ch] = np.where(ok, pcm[at, ch] * gain[None, :], np.float32(0.0))
        blocks.append(out)
        valid = ok.sum(axis=0).astype(np.uint64)                                # a prefix: the index only moves forward
        idx = idx + valid * step
        playing = playing & (valid == np.uint64(frames))
    for b in blocks:
        b.setflags(write=False)
    _CACHE[key] = (blocks, (idx.copy(), step.copy(), playing.copy()))
    return _CACHE[key]


@contextlib.contextmanager
def _form(ctx, name):
    n, tp, says = FORMS[name]
    old = ctx.time_parallel_max_voices
    try:
        if tp is not None:
            ctx.time_parallel_max_voices = tp
        yield n, says
    finally:
        ctx.time_parallel_max_voices = old


def _make(ctx, n, pcm=None):
    from groove_amd import entities as E
    bank, descs = _bank()
    return E.Sampler(ctx, bank if pcm is None else pcm, descs, _params(n))


def _walk(ctx, synth, n, mode="blocks", before_block=None):
    """The walk through one render entry.  "blocks": list of [2][frames][n]; "mix" / "deferred" / "paced": the bus [TOTAL][2]."""
    if mode == "blocks":
        blk, out = ctx.block(n, 256), []
        for k, frames in enumerate(SIZES):
            for ev in _events(n, k):
                synth.handle_midi_events(ev)
            if before_block:
                before_block(k)
            synth.generate_batch_values(blk, frames)
            out.append(blk.download(frames))
        blk.destroy()
        return out
    bus = ctx.bus(TOTAL)
    render = getattr(synth, {"mix": "render_mix", "deferred": "render_mix_deferred", "paced": "render_mix_paced"}[mode])
    for k, frames in enumerate(SIZES):
        for ev in _events(n, k):
            synth.handle_midi_events(ev)
        render(bus, frames, at_frame=STARTS[k])
    ctx.flush_bus()
    got = bus.download()
    bus.destroy()
    return got


def _same(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float32).view(np.uint32), np.asarray(b, dtype=np.float32).view(np.uint32))


def _clean(ctx):
    info = ctx.debug_info()
    assert info["zero_segments"] == 0 and info["fast_table_misses"] == 0, info


def _state_words(idx, step, playing):
    """SamplerState as groove_bank_download_state gives it: [6][n] words (idx lo, hi; step lo, hi; playing; pad)."""
    return np.stack([(idx & np.uint64(0xFFFFFFFF)).astype(np.uint32), (idx >> np.uint64(32)).astype(np.uint32),
                     (step & np.uint64(0xFFFFFFFF)).astype(np.uint32), (step >> np.uint64(32)).astype(np.uint32), playing.astype(np.uint32)])


def test_the_walk_has_every_case():
    n = 70
    blocks, (idx, step, playing) = _reference(n)
    steps = step.astype(np.float64) / 2.0 ** 44
    pitched = _sample_of(n) != 3
    assert (steps[pitched] < 1).any() and (steps[pitched] == 1).any() and (steps[pitched] > 1).any() and (steps[~pitched] == 1).all()
    assert set(SIZES) == {64, 37, 17, 256} and set(LENGTHS) == {1, 100, 5000}
    sounding = [np.any(b != 0, axis=(0, 1)) for b in blocks]
    one_shot = _one_shot(n).astype(bool)
    long = _sample_of(n) >= 2                                                  # 5,000 frames: nothing but a note-off ends them inside the walk
    assert (long & sounding[1] & ~sounding[2] & ~one_shot).any()               # a note-off obeyed (silent in block 2 though sounding before it)
    assert (sounding[2] & one_shot).any()                                      # ... and ignored by a one-shot, which the next note-on re-triggers
    assert _same(blocks[3][:, :17, one_shot & sounding[2]], blocks[0][:, :17, one_shot & sounding[2]])
    col = np.any(blocks[0] != 0, axis=0)                                       # voices that end inside block 0, not on a chunk boundary
    last = np.array([np.flatnonzero(col[:, v]).max(initial=-1) + 1 for v in range(n)])
    assert ((last > 0) & (last < 64) & (last % 16 != 0)).any()
    assert not _same(blocks[0][0], blocks[0][1])                               # the channels differ


@pytest.mark.parametrize("name", list(FORMS))
def test_blocks_and_state_against_numpy_and_a_mono_bank(gpu_ctx, name):
    """Properties 1, 2, 3 (blocks and state) and 7 (reset): bit for bit."""
    pcm, _ = _bank()
    with _form(gpu_ctx, name) as (n, says):
        want, final = _reference(n)
        st = _make(gpu_ctx, n)
        assert st.sample_channels == 2 and says in st.kernel_form(64, False), st.kernel_form(64, False)
        got = _walk(gpu_ctx, st, n)
        for k in range(len(SIZES)):
            assert _same(got[k][0], want[k][0]) and _same(got[k][1], want[k][1]), (name, k)
        state = st.download_state()
        assert state.shape[0] == 6 and np.array_equal(state[:5], _state_words(*final)), name
        # a mono bank on the left channel: the same state words, and the stereo bank's left channel on both of its channels
        mono = _make(gpu_ctx, n, np.ascontiguousarray(pcm[:, 0]))
        assert mono.sample_channels == 1 and mono.kernel_form(64, False) == st.kernel_form(64, False) and mono.kernel_form(64, True) == st.kernel_form(64, True)
        gm = _walk(gpu_ctx, mono, n)
        assert np.array_equal(mono.download_state(), state), name
        # right == left: the mono bank's bits
        dup = _make(gpu_ctx, n, np.ascontiguousarray(np.stack([pcm[:, 0], pcm[:, 0]], axis=1)))
        gd = _walk(gpu_ctx, dup, n)
        for k in range(len(SIZES)):
            assert _same(gd[k], gm[k]) and _same(gm[k][0], want[k][0]) and _same(gm[k][1], want[k][0]), (name, k)
        assert np.array_equal(dup.download_state(), state)
        # reset: the same walk, the same blocks
        st.reset()
        again = _walk(gpu_ctx, st, n)
        assert all(_same(x, y) for x, y in zip(again, got)), name
        _clean(gpu_ctx)
        for x in (st, mono, dup):
            x.destroy()


@pytest.mark.parametrize("name", list(FORMS))
def test_fused_buses(gpu_ctx, name):
    """Properties 3 (buses) and 4: the three fused entries; a swap of the bank's channels swaps the bus's columns bit for bit; the f64 bar."""
    pcm, _ = _bank()
    with _form(gpu_ctx, name) as (n, says):
        want = np.concatenate([b.astype(np.float64).sum(axis=2).T for b in _reference(n)[0]])       # [TOTAL][2], the exact values summed in f64
        st, swapped = _make(gpu_ctx, n), _make(gpu_ctx, n, np.ascontiguousarray(pcm[:, ::-1]))
        mono, dup = _make(gpu_ctx, n, np.ascontiguousarray(pcm[:, 0])), _make(gpu_ctx, n, np.ascontiguousarray(np.stack([pcm[:, 0], pcm[:, 0]], axis=1)))
        assert says in st.kernel_form(64, True), st.kernel_form(64, True)
        # the deferred form's two row buffers grow at the first 256-frame block of a context, and growing flushes the pending block through
        # the reduction kernels, whose order of additions is not the carried reduction's (groove_hip.hip ensure_dpart): size them before
        # the walks that are compared bit for bit, so that both are the same call pattern
        warm = gpu_ctx.bus(256)
        st.render_mix_deferred(warm, 256)
        gpu_ctx.flush_bus()
        warm.destroy()
        for mode in ("mix", "deferred", "paced"):
            for x in (st, swapped, mono, dup):
                x.reset()
            got, got_sw = _walk(gpu_ctx, st, n, mode), _walk(gpu_ctx, swapped, n, mode)
            assert _same(got[:, 0], got_sw[:, 1]) and _same(got[:, 1], got_sw[:, 0]), (name, mode)
            assert not _same(got[:, 0], got[:, 1])
            rms = np.sqrt(np.mean((got.astype(np.float64) - want) ** 2, axis=0)) / n
            sig = np.sqrt(np.mean(want ** 2, axis=0)) / n
            print(f"{name} {mode}: bus RMS error / V = {rms[0]:.3e}, {rms[1]:.3e} (signal {sig[0]:.3e}, {sig[1]:.3e})")
            assert (sig > 1e-4).all() and (rms <= 1e-5).all(), (name, mode, rms, sig)
            gm, gd = _walk(gpu_ctx, mono, n, mode), _walk(gpu_ctx, dup, n, mode)
            assert _same(gd, gm) and _same(gm[:, 0], gm[:, 1]) and _same(gm[:, 0], got[:, 0]), (name, mode)   # right == left: the mono bank's bus
            assert np.array_equal(dup.download_state(), mono.download_state()) and np.array_equal(st.download_state(), mono.download_state())
        _clean(gpu_ctx)
        for x in (st, swapped, mono, dup):
            x.destroy()


def test_mixed_launch_takes_the_bank_by_bank_path(gpu_ctx):
    """Property 5: groove_banks_render_mix_deferred over {a small Welsh bank, a stereo sampler bank} against the two banks rendered one
    by one with groove_bank_render_mix_deferred; the tolerance of tests/test_gpu_configs.py's shard sum (1e-6 of the voice count)."""
    from groove_amd import entities as E
    nw, ns = 64, 300

    def run(together):
        welsh, sampler = E.WelshSynth(gpu_ctx, P.welsh_voices(nw)), _make(gpu_ctx, ns)
        welsh.handle_midi_events(P.note_on_all(nw))
        bus = gpu_ctx.bus(TOTAL)
        for k, frames in enumerate(SIZES):
            for ev in _events(ns, k):
                sampler.handle_midi_events(ev)
            if together:
                gpu_ctx.render_mix_banks_deferred([welsh, sampler], bus, frames, at_frame=STARTS[k])
            else:
                welsh.render_mix_deferred(bus, frames, at_frame=STARTS[k])
                sampler.render_mix_deferred(bus, frames, accumulate=True, at_frame=STARTS[k])
        gpu_ctx.flush_bus()
        got = bus.download().astype(np.float64)
        for x in (bus, welsh, sampler):
            x.destroy()
        return got

    a, b = run(True), run(False)
    alone = np.concatenate([blk.astype(np.float64).sum(axis=2).T for blk in _reference(ns)[0]])
    assert np.max(np.abs(a - b)) / (nw + ns) <= 1e-6
    assert np.abs(a - alone).max() > 1e-2                                      # the Welsh bank sounds ...
    assert np.abs(a[:, 0] - a[:, 1]).max() > 1e-2                              # ... and the sampler bank in stereo
    _clean(gpu_ctx)


@pytest.mark.parametrize("name", ["tp-70", "serial-70"])
def test_set_param_on_the_gain_mid_walk(gpu_ctx, name):
    """Property 6, first half: groove_bank_set_param(GROOVE_CTL_SAMPLER_GAIN) before block 4, bit for bit against numpy with the new gain."""
    with _form(gpu_ctx, name) as (n, _):
        want, final = _reference(n, gain_from=(4, 0.6))
        st = _make(gpu_ctx, n)
        got = _walk(gpu_ctx, st, n, before_block=lambda k: k == 4 and st.control_set_param_by_index(T.CTL_SAMPLER_GAIN, 0.6))
        for k in range(len(SIZES)):
            assert _same(got[k], want[k]), (name, k)
        assert not _same(want[4], _reference(n)[0][4])
        assert np.array_equal(st.download_state()[:5], _state_words(*final))
        _clean(gpu_ctx)
        st.destroy()


@pytest.mark.parametrize("name", ["tp-70", "serial-70"])
def test_a_four_step_trip_onto_the_gain_is_the_set_param_arm(gpu_ctx, name):
    """Property 6, second half: tests/test_gpu_ctl_fm_sampler_links.py's pattern on a stereo bank — arm A a device-resident bank trip onto
    the gain, arm B groove_bank_set_param with the law's value at the same block starts, compared block for block by that file's rule; the
    applies cost no host wait."""
    from groove_amd import entities as E
    from tests import test_gpu_ctl_fm_sampler_links as FS
    from tests.ctl_trip_law import MAIN_START, MAIN_STEPS
    vals = FS._trip_values()
    with _form(gpu_ctx, name) as (n, _):
        def walk(synth, before_block):
            blk, out = gpu_ctx.block(n, 64), []
            for k in range(FS.BLOCKS):
                if k in (0, 15):
                    synth.handle_midi_events(T.note_events_np(np.arange(n, dtype=np.uint32), _keys(n), True))
                before_block(k)
                synth.generate_batch_values(blk, FS.SIZES[k])
                out.append(blk.download(FS.SIZES[k]))
            blk.destroy()
            return out
        a, b = _make(gpu_ctx, n), _make(gpu_ctx, n)
        trip = E.ControlTripLink(gpu_ctx, [list(MAIN_STEPS)], MAIN_START, a, T.CTL_SAMPLER_GAIN)
        ga = walk(a, lambda k: trip.work(FS.ATS[k]))
        gb = walk(b, lambda k: vals[k] is not None and b.control_set_param_by_index(T.CTL_SAMPLER_GAIN, vals[k]))
        FS._compare_arms(ga, gb, FS._curved(), f"stereo {name} gain trip")
        assert any(not _same(x[0], x[1]) for x in ga)               # in stereo
        waits = lambda: gpu_ctx.debug_info()["host_waits"]
        blk = gpu_ctx.block(n, 64)
        a.generate_batch_values_async(blk, 64)                      # a render in flight on a side stream
        before = waits()
        own = waits() - before                                      # what reading the counter costs by itself
        before = waits()
        for k in range(10):
            trip.work(480 + 240 * k)
        assert waits() - before - own == 0
        blk.download(64)
        _clean(gpu_ctx)
        for x in (trip, blk, a, b):
            x.destroy()


def test_sample_rate_change_leaves_a_stereo_bank_stereo(gpu_ctx):
    """Property 7, second half: groove_update_sample_rate to 48,000 and back; the bank is still stereo and renders the walk's bits."""
    n = 70
    st = _make(gpu_ctx, n)
    rate = gpu_ctx.sample_rate
    try:
        gpu_ctx.update_sample_rate(48000)
        assert st.sample_channels == 2
        gpu_ctx.update_sample_rate(rate)
    finally:
        if gpu_ctx.sample_rate != rate:
            gpu_ctx.update_sample_rate(rate)
    assert st.sample_channels == 2
    got, want = _walk(gpu_ctx, st, n), _reference(n)[0]
    assert all(_same(x, y) for x, y in zip(got, want))
    _clean(gpu_ctx)
    st.destroy()


def test_refusals_by_message(gpu_ctx):
    """Property 8."""
    from groove_amd import entities as E
    L, h = gpu_ctx.L, gpu_ctx.h
    pcm, descs = _bank()
    fp = pcm.ctypes.data_as(C.POINTER(C.c_float))
    sp, out = _params(2), C.c_void_p()
    create = lambda *a: L.groove_sampler_create_stereo(h, *a)
    cases = [
        (lambda: create(None, pcm.shape[0], descs, len(descs), sp, 2, C.byref(out)), "groove_sampler_create_stereo: NULL argument"),
        (lambda: create(fp, pcm.shape[0], descs, len(descs), sp, 2, None), "groove_sampler_create_stereo: NULL argument"),
        (lambda: create(fp, pcm.shape[0], descs, 0, sp, 2, C.byref(out)), "groove_sampler_create_stereo: empty bank"),
        (lambda: create(fp, pcm.shape[0] - 1, descs, len(descs), sp, 2, C.byref(out)), "groove_sampler_create_stereo: sample descriptor exceeds bank"),
    ]
    for call, message in cases:
        assert call() != 0
        assert L.groove_last_error(h).decode() == message
    with pytest.raises(ValueError, match="a stereo bank is"):
        E.Sampler(gpu_ctx, np.zeros((8, 3), dtype=np.float32), descs, sp)
    welsh = E.WelshSynth(gpu_ctx, P.welsh_voices(4))
    assert L.groove_bank_sample_channels(welsh.h) == 0 and L.groove_bank_sample_channels(None) == 0
    welsh.destroy()
    _clean(gpu_ctx)
