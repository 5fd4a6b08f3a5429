"""GPU tier: sampler banks whose samples carry forward loops (include/groove_hip.h groove_bank_set_sample_loops; docs/DSP_SPEC.md
section 7; csrc/dsp_core.h sample_loop_fold, sample_loop_advance, sample_loop_tap, sampler_chunk_loop; csrc/kernels.h
sampler_render_kernel<FUSED, STEREO, MODE, LOOP>; csrc/welsh_tp.h sampler_tp_body<FUSED, WAVES, STEREO, MODE, LOOP>).

The reference is numpy, section 7 restated: per voice the events are replayed on (idx, step, playing) in exact integers.  A voice loops
in a block when its sample has a loop, it is no one-shot and it plays; frame f of such a voice is read at F(idx + f * step) with
F(x) = x below E = end << 44 and S + (x - S) mod (E - S) from there on, and the block leaves idx = F(idx + frames * step); every other
voice is the walk of tests/test_gpu_sampler_interp.py.  i = pos >> 44, t = ((pos >> 20) & 0xFFFFFF) * 2^-24; the taps are the bank's
float32 values — of a looping voice tap j >= end is read at start + (j - start) mod (end - start) and tap j < 0 is 0 — and the
formula, linear or Catmull-Rom, is evaluated in float64, times the gain.  NEAREST is float32(pcm) * float32(gain), exact.

Bounds: NEAREST bit for bit; LINEAR and CUBIC |gpu - ref| <= 2^-18 * M * gain + 2^-24 * |ref|, M the largest |tap| of the frame (the
derivation is test_gpu_sampler_interp.py's: ~12 rounded fp32 operations on intermediates <= 4 M), no value exempted; state words bit
for bit in every mode.  The samples lie adjacent in the bank, first and last frames of magnitude >= 0.2, so a tap read across a
sample's or a loop's boundary is an error of 1e-2 or more.

Shapes: the time-parallel kernel at 5, 70 and 1,100 voices (one voice per wavefront, several workgroups' worth, more than one voice
per wavefront), the serial one at 70; block lengths 64, 37, 17, 256, three times over; keys an octave below the root, on it, an octave
and three octaves above (step 8: longer than the loops of 1, 2 and 3 frames, a frame wraps several times); loops [0, 1), [0, 2),
[1, 4) of 6 frames, [90, 100) of 100, [1000, 3000) of 5,000, a sample without a loop and the drumkit sample (looped, so that its
one-shot voices show that they do not loop); one-shot and sampler voices on every sample; mono and stereo banks.

Every test ends on zero_segments == 0 and fast_table_misses == 0."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from groove_amd import abi_types as T, lib as _lib, patches as P

pytestmark = pytest.mark.gpu

SIZES = [64, 37, 17, 256] * 3                                      # three walks of the four block lengths
STARTS = [int(x) for x in np.concatenate([[0], np.cumsum(SIZES)[:-1]])]
TOTAL = sum(SIZES)
ON_BLOCKS, OFF_BLOCK = (0, 3), 2                                   # on; off (one-shots play on); on again; then held for two more walks
LENGTHS = (1, 2, 6, 100, 5000, 300, 5000)                          # the last one is the drumkit sample (root_hz 0: step 1 whatever the key)
LOOPS = ((0, 1), (0, 2), (1, 4), (90, 100), (1000, 3000), (0, 0), (100, 200))
ROOTS = (440.0, 440.0, 440.0, 440.0, 440.0, 440.0, 0.0)
NO_LOOP, DRUM = 5, 6
KEYS = (57, 69, 81, 105)                                           # steps 1/2, 1, 2, 8
NEAREST, LINEAR, CUBIC = T.SAMPLE_NEAREST, T.SAMPLE_LINEAR, T.SAMPLE_CUBIC
MODE_NAME = {NEAREST: "nearest", LINEAR: "linear", CUBIC: "cubic"}
FORMS = {                                                          # name: (voices, time_parallel_max_voices or None, what kernel_form says)
    "tp-5": (5, None, "sampler_tp_kernel"), "tp-70": (70, None, "sampler_tp_kernel"), "tp-1100": (1100, None, "sampler_tp_kernel"),
    "serial-70": (70, 0, "sampler_render_kernel (serial"),
}
_CACHE = {}


def _bank():
    """(pcm [frames, 2] float32, descs): left and right independent noise; every sample's first and last frame at least 0.2 in magnitude."""
    if "bank" not in _CACHE:
        rng = np.random.default_rng(20261020)
        pcm = (rng.standard_normal((sum(LENGTHS), 2)) * 0.3).astype(np.float32)
        descs = (T.SampleDesc * len(LENGTHS))()
        off = 0
        for k, ln in enumerate(LENGTHS):
            descs[k].offset, descs[k].length, descs[k].root_hz = off, ln, ROOTS[k]
            for at in (off, off + ln - 1):
                pcm[at] = np.where(pcm[at] < 0, -0.2, 0.2) + pcm[at]
            off += ln
        pcm.setflags(write=False)
        _CACHE["bank"] = (pcm, descs)
    return _CACHE["bank"]


def _keys(n):
    return np.array(KEYS, dtype=np.uint8)[np.arange(n) % 4]


def _sample_of(n):
    return (np.arange(n) + np.arange(n) // 4) % len(LENGTHS)         # (4 keys, 7 samples: the shift pairs every sample with every key)


def _one_shot(n):
    return (np.arange(n) // 28) % 2                                   # 28 voices: every (sample, key) pair; the next 28 are its one-shots


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


def _note_step(n):
    root = np.array([ROOTS[s] for s in _sample_of(n)], dtype=np.float64)
    freq = 440.0 * np.exp2((_keys(n).astype(np.float64) - 69.0) / 12.0)
    ratio = np.where(root > 0.0, freq / np.where(root > 0.0, root, 1.0), 1.0)
    return (ratio * 17592186044416.0).astype(np.uint64)               # truncation, 2^44


def _interp(mode, tap, t):
    """The mode's formula in float64.  tap(k): the frame's tap i + k as float64."""
    if mode == LINEAR:
        p0, p1 = tap(0), tap(1)
        return p0 + t * (p1 - p0), np.maximum(np.abs(p0), np.abs(p1))
    pm, p0, p1, p2 = tap(-1), tap(0), tap(1), tap(2)
    c1 = 0.5 * (p1 - pm)
    c2 = pm - 2.5 * p0 + 2.0 * p1 - 0.5 * p2
    c3 = 0.5 * (p2 - pm) + 1.5 * (p0 - p1)
    return ((c3 * t + c2) * t + c1) * t + p0, np.max(np.abs([pm, p0, p1, p2]), axis=0)


def _fold(x, s, e):
    """F(x), uint64 arrays; s, e in frames, e == 0: no loop (x as it is).  (x < 2^59 here: exact)"""
    big_s, big_e = s.astype(np.uint64) << np.uint64(44), e.astype(np.uint64) << np.uint64(44)
    lam = np.where(e > 0, big_e - big_s, np.uint64(1))
    over = (e > 0) & (x >= big_e)
    return np.where(over, big_s + (np.where(over, x - big_s, np.uint64(0)) % lam), x)


def _reference(n, plan="always"):
    """The walk in numpy.  {mode: blocks}, bounds, final state, looping: blocks[k] is [2][frames][n] — float32 and exact for NEAREST,
    float64 for LINEAR and CUBIC; bounds[mode][k] the allowed |gpu - ref|; looping[k] which voices looped in block k.  plan: "always",
    "never", or "mid" — no loops until block 4, LOOPS from there, cleared again from block 10 on."""
    key = (n, plan)
    if key in _CACHE:
        return _CACHE[key]
    pcm, descs = _bank()
    smp = _sample_of(n)
    offset = np.array([descs[s].offset for s in smp], dtype=np.int64)
    length = np.array([descs[s].length for s in smp], dtype=np.int64)
    one_shot, gain = _one_shot(n).astype(bool), _gains(n)
    note_step = _note_step(n)
    idx, step, playing = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=bool)
    blocks, bounds, looping = {m: [] for m in MODE_NAME}, {LINEAR: [], CUBIC: []}, []
    for k, frames in enumerate(SIZES):
        if k in ON_BLOCKS:
            idx[:], step[:], playing[:] = 0, note_step, True
        if k == OFF_BLOCK:
            playing &= one_shot
        loops = np.array(_loops_at(plan, k), dtype=np.int64)[smp]                 # [n][2]
        lp = (loops[:, 1] > 0) & ~one_shot & playing
        ls, le = np.where(lp, loops[:, 0], 0), np.where(lp, loops[:, 1], 0)
        lam = np.where(lp, le - ls, 1)
        f = np.arange(frames, dtype=np.uint64)
        pos = _fold(idx[None, :] + f[:, None] * step[None, :], ls[None, :], le[None, :])   # [frames][n]; idx + f * step < 2^59: exact in 64 bits
        i = (pos >> np.uint64(44)).astype(np.int64)
        t = ((pos >> np.uint64(20)) & np.uint64(0xFFFFFF)).astype(np.float64) * 2.0 ** -24
        ok = playing[None, :] & (i < length[None, :])
        assert ok[:, lp].all() and (i[:, lp] < le[None, lp]).all()
        near = np.zeros((2, frames, n), dtype=np.float32)
        out = {LINEAR: np.zeros((2, frames, n)), CUBIC: np.zeros((2, frames, n))}
        bnd = {LINEAR: np.zeros((2, frames, n)), CUBIC: np.zeros((2, frames, n))}
        g64 = gain.astype(np.float64)[None, :]
        for ch in range(2):
            def tap(d, ch=ch):
                j = i + d
                wrapped = ls[None, :] + (j - ls[None, :]) % lam[None, :]
                j = np.where(lp[None, :] & (j >= le[None, :]), wrapped, j)
                inside = ok & (j >= 0) & (j < length[None, :])
                return np.where(inside, pcm[offset[None, :] + np.clip(j, 0, length[None, :] - 1), ch].astype(np.float64), 0.0)
            near[ch] = np.where(ok, pcm[offset[None, :] + np.minimum(i, length[None, :] - 1), ch] * gain[None, :], np.float32(0.0))
            for mode in (LINEAR, CUBIC):
                y, m = _interp(mode, tap, t)
                out[mode][ch] = np.where(ok, y * g64, 0.0)
                bnd[mode][ch] = 2.0 ** -18 * m * g64 + 2.0 ** -24 * np.abs(out[mode][ch])
        blocks[NEAREST].append(near)
        for mode in (LINEAR, CUBIC):
            blocks[mode].append(out[mode])
            bounds[mode].append(bnd[mode])
        looping.append(lp)
        valid = ok.sum(axis=0).astype(np.uint64)                                 # a prefix, or the whole block of a looping voice
        idx = _fold(idx + valid * step, ls, le)
        playing = playing & (valid == np.uint64(frames))
    for m in blocks:
        for b in blocks[m]:
            b.setflags(write=False)
    _CACHE[key] = (blocks, bounds, (idx.copy(), step.copy(), playing.copy()), looping)
    return _CACHE[key]


NONE = tuple((0, 0) for _ in LOOPS)


def _loops_at(plan, k):
    if plan == "always":
        return LOOPS
    if plan == "never":
        return NONE
    return LOOPS if 4 <= k < 10 else NONE


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


def _make(ctx, n, channels=2, mode=None, loops=LOOPS):
    from groove_amd import entities as E
    pcm, descs = _bank()
    s = E.Sampler(ctx, pcm if channels == 2 else np.ascontiguousarray(pcm[:, 0]), descs, _params(n))
    if mode is not None:
        s.sample_interpolation = mode
    if loops is not None:
        s.sample_loops = loops
    return s


def _walk(ctx, synth, n, entry="blocks", before_block=None):
    """The walk through one render entry.  "blocks": list of [2][frames][n]; "mix" / "deferred" / "paced": the bus [TOTAL][2]."""
    if entry == "blocks":
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
    render = getattr(synth, {"mix": "render_mix", "deferred": "render_mix_deferred", "paced": "render_mix_paced"}[entry])
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


def _within(got, want, bound, what, channels=2):
    """Every value of a block [2][frames][n] within its bound of the reference; a mono bank plays the left reference on both channels."""
    for ch in range(2):
        rc = ch if channels == 2 else 0
        err = np.abs(got[ch].astype(np.float64) - want[rc])
        worst = np.unravel_index(np.argmax(err - bound[rc]), err.shape)
        assert (err <= bound[rc]).all(), (what, ch, worst, float(err[worst]), float(bound[rc][worst]), float(want[rc][worst]))


def _check_walk(got, mode, want, bounds, what, channels):
    for k in range(len(SIZES)):
        if mode == NEAREST:
            for ch in range(2):
                assert _same(got[k][ch], want[NEAREST][k][ch if channels == 2 else 0]), (what, k, ch)
        else:
            _within(got[k], want[mode][k], bounds[mode][k], (what, k), channels)


def _clean(ctx):
    info = ctx.debug_info()
    assert info["zero_segments"] == 0 and info["fast_table_misses"] == 0, info


def _state_words(idx, step, playing):
    """SamplerState as groove_bank_download_state gives it: [6][n] words (idx lo, hi; step lo, hi; playing; pad)."""
    return np.stack([(idx & np.uint64(0xFFFFFFFF)).astype(np.uint32), (idx >> np.uint64(32)).astype(np.uint32),
                     (step & np.uint64(0xFFFFFFFF)).astype(np.uint32), (step >> np.uint64(32)).astype(np.uint32), playing.astype(np.uint32)])


def _the_walk_has_every_case(n):
    """The numpy walk itself holds the cases the tests rely on (part of test_blocks_and_state_in_every_mode's set-up at 70 voices)."""
    blocks, bounds, (idx, step, playing), looping = _reference(n)
    pcm, descs = _bank()
    smp, one_shot = _sample_of(n), _one_shot(n).astype(bool)
    steps = step.astype(np.float64) / 2.0 ** 44
    pitched = smp != DRUM
    assert set(np.round(steps[pitched], 6)) == {0.5, 1.0, 2.0, 8.0} and (steps[~pitched] == 1).all()
    for s in range(len(LENGTHS)):                                                # every sample under every key, as a sampler voice and as a one-shot
        for key in KEYS:
            for os_ in (False, True):
                assert ((smp == s) & (_keys(n) == key) & (one_shot == os_)).any(), (s, key, os_)
    for k in range(len(LENGTHS)):                                                # adjacent samples, loud at both ends: a tap across a boundary shows
        o, ln = descs[k].offset, descs[k].length
        assert np.abs(pcm[o]).min() >= 0.2 and np.abs(pcm[o + ln - 1]).min() >= 0.2
        assert k == 0 or o == descs[k - 1].offset + descs[k - 1].length
    has_loop = np.array([LOOPS[s][1] > 0 for s in smp])
    sounding = [np.any(b != 0, axis=(0, 1)) for b in blocks[NEAREST]]
    assert (looping[0] == (has_loop & ~one_shot)).all() and not looping[2].any() and (looping[3] == looping[0]).all()
    assert (sounding[1] & ~sounding[2] & looping[1]).any()                       # a note-off stops a looping voice at the next block start
    assert (sounding[2] & one_shot).any()                                        # ... and is ignored by a one-shot
    assert sounding[-1][looping[-1]].all() and looping[-1].any() and (looping[-1] == looping[3]).all()   # two walks later: still sounding
    assert not sounding[-1][~looping[-1] & (smp != 4) & (smp != DRUM)].any()     # everything else but the one-shots of the 5,000-frame samples has ended
    assert playing[looping[-1]].all() and (idx[looping[-1]] >> np.uint64(44) < np.array([LOOPS[s][1] for s in smp])[looping[-1]]).all()
    wraps = steps * TOTAL / np.maximum(1, np.array([LOOPS[s][1] - LOOPS[s][0] for s in smp]))
    assert (wraps[looping[-1]] > 100).any()                                      # (step 8 on a loop of one frame: eight wraps per frame)
    assert max(b.max() for b in bounds[CUBIC]) < 2e-5                            # the bound is rounding, orders below a wrong tap


@pytest.mark.parametrize("name", list(FORMS))
def test_blocks_and_state_in_every_mode(gpu_ctx, name):
    """The block-writing forms against the reference, three modes, mono and stereo: NEAREST bit for bit, LINEAR and CUBIC within the
    bound, the state words bit for bit in every mode; groove_bank_kernel_form says "looped"; the voices that do not loop (one-shots on
    looped samples, every voice of the loop-free sample) are a never-looped bank's bits; and with the loops cleared the whole bank is."""
    with _form(gpu_ctx, name) as (n, says):
        want, bounds, final, looping = _reference(n)
        if n == 70:
            _the_walk_has_every_case(n)
        ever = np.any(looping, axis=0)
        for channels in (2, 1):
            bank, plain = _make(gpu_ctx, n, channels), _make(gpu_ctx, n, channels, loops=None)
            assert bank.sample_loops == [tuple(x) for x in LOOPS] and plain.sample_loops == [(0, 0)] * len(LOOPS)
            for mode in (NEAREST, LINEAR, CUBIC):
                bank.sample_interpolation = plain.sample_interpolation = mode
                form, pform = bank.kernel_form(64, False), plain.kernel_form(64, False)
                assert says in form and form.endswith(", looped)") and "looped" not in pform and form == pform[:-1] + ", looped)", (form, pform)
                bank.reset()
                plain.reset()
                assert bank.sample_loops == [tuple(x) for x in LOOPS]               # (kept by groove_bank_reset)
                got = _walk(gpu_ctx, bank, n)
                _check_walk(got, mode, want, bounds, (name, MODE_NAME[mode], channels), channels)
                assert np.array_equal(bank.download_state()[:5], _state_words(*final)), (name, MODE_NAME[mode], channels)
                never = _walk(gpu_ctx, plain, n)
                for k in range(len(SIZES)):
                    assert _same(got[k][:, :, ~looping[k]], never[k][:, :, ~looping[k]]), (name, MODE_NAME[mode], channels, k)
                assert np.array_equal(bank.download_state()[:, ~ever], plain.download_state()[:, ~ever])
                if mode == CUBIC:                                               # cleared: the bank ends where it ends today
                    bank.sample_loops = None
                    assert "looped" not in bank.kernel_form(64, False) and bank.sample_loops == [(0, 0)] * len(LOOPS)
                    bank.reset()
                    cleared = _walk(gpu_ctx, bank, n)
                    assert all(_same(a, b) for a, b in zip(cleared, never)) and np.array_equal(bank.download_state(), plain.download_state())
            bank.destroy()
            plain.destroy()
        _clean(gpu_ctx)


@pytest.mark.parametrize("name", list(FORMS))
def test_fused_buses(gpu_ctx, name):
    """groove_bank_render_mix, _deferred and _paced against the f64 sum of the reference values: the same sums as the block form within
    fp32 order of addition, bus RMS / V <= 1e-5 (tests/test_gpu_sampler_interp.py's statement of it)."""
    with _form(gpu_ctx, name) as (n, says):
        blocks = _reference(n)[0]
        for channels in (2, 1):
            bank = _make(gpu_ctx, n, channels)
            for mode in (NEAREST, LINEAR, CUBIC):
                want = np.concatenate([b.astype(np.float64).sum(axis=2).T for b in blocks[mode]])    # [TOTAL][2]
                if channels == 1:
                    want = np.stack([want[:, 0], want[:, 0]], axis=1)
                bank.sample_interpolation = mode
                form = bank.kernel_form(64, True)
                assert says in form and form.endswith(", looped)"), form
                for entry in ("mix", "deferred", "paced"):
                    bank.reset()
                    got = _walk(gpu_ctx, bank, n, entry).astype(np.float64)
                    rms = np.sqrt(np.mean((got - want) ** 2, axis=0)) / n
                    sig = np.sqrt(np.mean(want[-SIZES[-1]:] ** 2, axis=0)) / n               # (the last block: only loops still sound there)
                    print(f"{name} {MODE_NAME[mode]} {channels}ch {entry}: bus RMS error / V = {rms[0]:.3e}, {rms[1]:.3e} (signal {sig[0]:.3e}, {sig[1]:.3e})")
                    assert (sig > 1e-4).all() and (rms <= 1e-5).all(), (name, mode, channels, entry, rms, sig)
            bank.destroy()
        _clean(gpu_ctx)


@pytest.mark.parametrize("name", ["tp-70", "serial-70"])
def test_loops_set_and_cleared_mid_walk(gpu_ctx, name):
    """Loops set before block 4 onto playing voices — block 3 re-triggered them, so the drumkit sample's sampler voices sit at frame 256,
    past its loop's end 200, and are folded at their next frame; the step-8 voices of the 5,000-frame sample sit at 2,048, inside
    [1000, 3000) — and cleared before
    block 10: each block is the reference's under the loops then in force, state included."""
    with _form(gpu_ctx, name) as (n, _):
        want, bounds, final, looping = _reference(n, "mid")
        smp = _sample_of(n)
        before4 = np.uint64(sum(SIZES[3:4])) * _note_step(n) >> np.uint64(44)     # the cursor before block 4: block 3 re-triggered
        assert (looping[4] & (smp == DRUM) & (before4 >= 200)).any() and (looping[4] & (smp == 4) & (before4 >= 1000) & (before4 < 3000)).any()
        assert not np.any(looping[:4]) and not np.any(looping[10:]) and looping[9].any()
        for channels in (2, 1):
            for mode in (NEAREST, LINEAR, CUBIC):
                bank = _make(gpu_ctx, n, channels, mode, loops=None)

                def before(k, bank=bank):
                    if k == 4:
                        bank.sample_loops = LOOPS
                    if k == 10:
                        bank.sample_loops = None
                got = _walk(gpu_ctx, bank, n, before_block=before)
                _check_walk(got, mode, want, bounds, (name, MODE_NAME[mode], channels), channels)
                assert np.array_equal(bank.download_state()[:5], _state_words(*final))
                bank.destroy()
        _clean(gpu_ctx)


def test_mixed_launch_takes_the_bank_by_bank_path(gpu_ctx):
    """groove_banks_render_mix_deferred over {a small Welsh bank, a looped sampler bank} against the two banks rendered one by one with
    groove_bank_render_mix_deferred: bus RMS / V <= 1e-5; and the sampler bank in it is the looped one (the last block still sounds)."""
    from groove_amd import entities as E
    nw, ns = 64, 300

    def run(together, loops):
        welsh, sampler = E.WelshSynth(gpu_ctx, P.welsh_voices(nw)), _make(gpu_ctx, ns, 1, NEAREST, loops)
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

    blocks = _reference(ns)[0]
    plain = _reference(ns, "never")[0]
    a, b, never = run(True, LOOPS), run(False, LOOPS), run(True, None)
    rms = np.sqrt(np.mean((a - b) ** 2, axis=0)) / (nw + ns)
    print(f"mixed call, looped: bus RMS difference / V = {rms[0]:.3e}, {rms[1]:.3e}")
    assert (rms <= 1e-5).all(), rms
    moved = np.concatenate([(x.astype(np.float64) - y.astype(np.float64)).sum(axis=2).T for x, y in zip(blocks[NEAREST], plain[NEAREST])])[:, 0]
    got = (a - never)[:, 0]                                                      # what the loops changed on the bus: the reference's difference
    assert np.abs(moved[-SIZES[-1]:]).max() > 1e-1 and np.sqrt(np.mean((got - moved) ** 2)) / (nw + ns) <= 1e-5
    _clean(gpu_ctx)


def test_controls_reset_and_sample_rate_keep_the_loops(gpu_ctx):
    """groove_bank_set_param, groove_bank_reset and a sample-rate change leave the loops where they are, and the walk after them is the walk."""
    n = 70
    want, bounds, final, _ = _reference(n)
    bank = _make(gpu_ctx, n, 2, LINEAR)
    loops = [tuple(x) for x in LOOPS]
    bank.control_set_param_by_index(T.CTL_SAMPLER_GAIN, 0.6)
    assert bank.sample_loops == loops
    rate = gpu_ctx.sample_rate
    try:
        gpu_ctx.update_sample_rate(48000)
        assert bank.sample_loops == loops
        gpu_ctx.update_sample_rate(rate)
    finally:
        if gpu_ctx.sample_rate != rate:
            gpu_ctx.update_sample_rate(rate)
    bank.reset()
    assert bank.sample_loops == loops and "looped" in bank.kernel_form(64, True)
    got = _walk(gpu_ctx, bank, n)
    g = float(np.float32(0.6))
    gains = _gains(n).astype(np.float64)[None, None, :]
    for k in range(len(SIZES)):                                                  # (the reference at gain 0.6: its values and bounds scale with the gain)
        _within(got[k], want[LINEAR][k] / gains * g, bounds[LINEAR][k] / gains * g, ("gain 0.6", k))
    assert np.array_equal(bank.download_state()[:5], _state_words(*final))
    bank.destroy()
    _clean(gpu_ctx)


def test_refusals_by_message(gpu_ctx):
    """The setter on a Welsh bank, a wrong sample count, start >= end and end beyond the sample fail with a message that names the
    function and change nothing; (0, 0) beside real loops is accepted."""
    from groove_amd import entities as E
    L, h = gpu_ctx.L, gpu_ctx.h
    welsh = E.WelshSynth(gpu_ctx, P.welsh_voices(4))
    one = (T.SampleLoop * 1)(T.SampleLoop(0, 1))
    assert L.groove_bank_set_sample_loops(welsh.h, one, 1) != 0
    assert L.groove_last_error(h).decode() == "groove_bank_set_sample_loops: only sampler and drumkit banks play samples"
    assert L.groove_bank_sample_loops(welsh.h, None, 0) == 0
    bank = _make(gpu_ctx, 5, 1, LINEAR)
    loops = [tuple(x) for x in LOOPS]
    for bad, says in (([(0, 1)] * 3, "n_samples is not the bank's sample count (7)"),
                      ([(0, 1), (2, 2)] + loops[2:], "start >= end (sample 1)"),
                      ([(0, 1), (1, 0)] + loops[2:], "start >= end (sample 1)"),
                      ([(0, 1), (0, 3)] + loops[2:], "end beyond the sample's length (sample 1)"),
                      (loops[:6] + [(4999, 5001)], "end beyond the sample's length (sample 6)")):
        with pytest.raises(_lib.GrooveError) as err:
            bank.sample_loops = bad
        assert str(err.value).endswith("groove_bank_set_sample_loops: " + says) or ("groove_bank_set_sample_loops: " + says) in str(err.value), str(err.value)
        assert bank.sample_loops == loops and bank.kernel_form(64, True).endswith(", looped)")
    assert L.groove_bank_sample_loops(bank.h, None, 0) == sum(1 for s, e in LOOPS if e) == 6
    assert L.groove_bank_set_sample_loops(None, one, 1) != 0
    bank.sample_loops = [(0, 0)] * 6 + [(0, 5000)]
    assert bank.sample_loops == [(0, 0)] * 6 + [(0, 5000)] and "looped" in bank.kernel_form(64, True)
    bank.sample_loops = [(0, 0)] * 7
    assert "looped" not in bank.kernel_form(64, True) and L.groove_bank_sample_loops(bank.h, None, 0) == 0
    for x in (welsh, bank):
        x.destroy()
    _clean(gpu_ctx)


@pytest.mark.parametrize("form", ["tp", "serial"])
def test_a_cursor_that_would_pass_2_to_the_64(gpu_ctx, form):
    """One sample of 2^20 - 1 frames, looped over its last five frames, key 127 on a root of 8.18 Hz (step ~1,534 frames): blocks of 256
    frames until the cursor has run past the sample's end, where idx + f * step exceeds 2^64 — the first block is a plain run-in, the
    third folds.  The reference replays the cursor in Python integers.  NEAREST bit for bit, LINEAR and CUBIC within the bound, state
    bit for bit."""
    from groove_amd import entities as E
    length, frames, n_blocks = (1 << 20) - 1, 256, 4
    start, end = length - 5, length
    rng = np.random.default_rng(7)
    pcm = (rng.standard_normal(length) * 0.3).astype(np.float32)
    descs = (T.SampleDesc * 1)()
    descs[0].offset, descs[0].length, descs[0].root_hz = 0, length, 8.18
    params = (T.SamplerParams * 1)()
    params[0].sample_index, params[0].one_shot, params[0].gain = 0, 0, 0.8
    gain = np.float32(0.8)
    formula = int(np.float64(440.0 * np.exp2((127.0 - 69.0) / 12.0)) / np.float64(np.float32(8.18)) * 17592186044416.0)
    big_s, big_e = start << 44, end << 44

    def fold(x):
        return x if x < big_e else big_s + (x - big_s) % (big_e - big_s)

    old = gpu_ctx.time_parallel_max_voices
    try:
        if form == "serial":
            gpu_ctx.time_parallel_max_voices = 0
        bank = E.Sampler(gpu_ctx, pcm, descs, params)
        bank.sample_loops = [(start, end)]
        assert ("sampler_tp_kernel" if form == "tp" else "sampler_render_kernel") in bank.kernel_form(frames, False)
        blk = gpu_ctx.block(1, frames)
        passed = False
        for mode in (NEAREST, LINEAR, CUBIC):
            bank.sample_interpolation = mode
            bank.reset()
            bank.handle_midi_events(T.note_events_np(np.zeros(1, dtype=np.uint32), np.array([127], dtype=np.uint8), True))
            idx = 0
            for b in range(n_blocks):
                bank.generate_batch_values(blk, frames)
                got = blk.download(frames)
                if b == 0:                                                       # the step is note-on's (the note rules are not this test's subject: the
                    state = bank.download_state()[:, 0]                          # device's own exp2, within a unit in the last place of the formula's)
                    step = int(state[3]) << 32 | int(state[2])
                    assert abs(step - formula) <= formula * 2.0 ** -50 and step > 1500 << 44, (step, formula)
                assert _same(got[0], got[1])
                for f in range(frames):
                    passed = passed or idx + f * step >= 1 << 64
                    c = fold(idx + f * step)
                    i, t = c >> 44, ((c >> 20) & 0xFFFFFF) * 2.0 ** -24
                    assert i < end

                    def tap(d):
                        j = i + d
                        if j >= end:
                            j = start + (j - start) % (end - start)
                        return float(pcm[j]) if j >= 0 else 0.0
                    if mode == NEAREST:
                        assert _same(got[0][f, 0], pcm[i] * gain), (form, b, f)
                    else:
                        y, m = _interp(mode, lambda d: np.float64(tap(d)), t)
                        ref = float(y) * float(gain)
                        assert abs(float(got[0][f, 0]) - ref) <= 2.0 ** -18 * float(m) * float(gain) + 2.0 ** -24 * abs(ref), (form, MODE_NAME[mode], b, f)
                idx = fold(idx + frames * step)
                state = bank.download_state()[:, 0]
                assert (int(state[1]) << 32 | int(state[0])) == idx and (int(state[3]) << 32 | int(state[2])) == step and state[4] == 1, (form, MODE_NAME[mode], b)
        assert passed                                                            # (the case is the one it claims to be)
        for x in (blk, bank):
            x.destroy()
    finally:
        gpu_ctx.time_parallel_max_voices = old
    _clean(gpu_ctx)
