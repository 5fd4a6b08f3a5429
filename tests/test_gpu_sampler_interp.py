"""GPU tier: sampler and drumkit banks that read their samples BETWEEN frames (include/groove_hip.h
groove_bank_set_sample_interpolation; docs/DSP_SPEC.md section 7; csrc/dsp_core.h sample_interp, sampler_chunk_interp; csrc/kernels.h
sampler_render_kernel<FUSED, STEREO, MODE>; csrc/welsh_tp.h sampler_tp_body<FUSED, WAVES, STEREO, MODE>).

The reference is numpy, section 7 restated: per voice the events are replayed on (idx, step, playing) in exact 64-bit integers; frame f
of a block has pos = idx + f * step, i = pos >> 44, t = ((pos >> 20) & 0xFFFFFF) * 2^-24; the taps are the bank's float32 values (0 for
a tap before the sample's first or past its last frame) and the formula — linear, or Catmull-Rom — is evaluated in float64, times the
gain.  NEAREST is float32(pcm) * float32(gain), exact.

The bound on a block-writing form's value: |gpu - ref| <= 2^-18 * M * gain + 2^-24 * |ref|, M the largest |tap| of the frame.  At most
~12 rounded fp32 operations on intermediates of magnitude <= 4 M, each off by at most half a unit in the last place, come to
<= 1.5e-6 * M; 2^-18 ~ 3.8e-6 leaves a factor of about 2.6; the second term is the rounding of the reference itself to fp32.  The
samples lie adjacent in the bank, their first and last frames and their neighbours' of magnitude >= 0.2: a tap read across a sample's
boundary, a wrong fraction or a wrong end rule is an error of 1e-2 or more.  No value is exempted.

Forms and shapes are tests/test_gpu_sampler_stereo.py's: the time-parallel kernel at 5, 70, 300, 1,100 and 4,100 voices, the serial
one at 70 and 300; block lengths 64, 37, 17, 256 in one walk; keys below, on and above the root; note-on, note-off, re-trigger; one-shots;
mono and stereo banks of independent noise; samples of 1, 2, 3, 100 and 5,000 frames and a drumkit sample.

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
LENGTHS = (1, 2, 3, 100, 5000, 5000)                               # the last one is the drumkit sample (root_hz 0: step 1 whatever the key)
ROOTS = (440.0, 440.0, 440.0, 440.0, 440.0, 0.0)
DRUM = len(LENGTHS) - 1
NEAREST, LINEAR, CUBIC = T.SAMPLE_NEAREST, T.SAMPLE_LINEAR, T.SAMPLE_CUBIC
MODE_NAME = {NEAREST: "nearest", LINEAR: "linear", CUBIC: "cubic"}
FORMS = {                                                          # name: (voices, time_parallel_max_voices or None, what kernel_form says)
    "tp-5": (5, None, "sampler_tp_kernel"), "tp-70": (70, None, "sampler_tp_kernel"), "tp-300": (300, None, "sampler_tp_kernel"),
    "tp-1100": (1100, None, "sampler_tp_kernel"), "tp-4100": (4100, None, "sampler_tp_kernel"),
    "serial-70": (70, 0, "sampler_render_kernel (serial"), "serial-300": (300, 0, "sampler_render_kernel (serial"),
}
_CACHE = {}


def _bank():
    """(pcm [frames, 2] float32, descs): left and right independent noise; every sample's first and last frame at least 0.2 in magnitude."""
    if "bank" not in _CACHE:
        rng = np.random.default_rng(20241020)
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
    return (57 + (12 * np.arange(n)) % 25).astype(np.uint8)         # voice 0: 57 (step 1/2), 1: 69 (step 1), 2: 81 (step 2), 3: 68, ...


def _sample_of(n):
    return (np.arange(n) + np.arange(n) // 25) % len(LENGTHS)        # (25 keys, 6 samples: the shift pairs every sample with every key)


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


def _note_step(n):
    root = np.array([ROOTS[s] for s in _sample_of(n)], dtype=np.float64)
    freq = 440.0 * np.exp2((_keys(n).astype(np.float64) - 69.0) / 12.0)
    ratio = np.where(root > 0.0, freq / np.where(root > 0.0, root, 1.0), 1.0)
    return (ratio * 17592186044416.0).astype(np.uint64)               # truncation, 2^44


def _integer_step(n):
    return (_note_step(n) & np.uint64((1 << 44) - 1)) == 0


def _interp(mode, tap, t):
    """The mode's formula in float64.  tap(k): the frame's tap i + k as float64 (0 outside the sample)."""
    if mode == LINEAR:
        p0, p1 = tap(0), tap(1)
        return p0 + t * (p1 - p0), np.maximum(np.abs(p0), np.abs(p1))
    pm, p0, p1, p2 = tap(-1), tap(0), tap(1), tap(2)
    c1 = 0.5 * (p1 - pm)
    c2 = pm - 2.5 * p0 + 2.0 * p1 - 0.5 * p2
    c3 = 0.5 * (p2 - pm) + 1.5 * (p0 - p1)
    return ((c3 * t + c2) * t + c1) * t + p0, np.max(np.abs([pm, p0, p1, p2]), axis=0)


def _reference(n, gain_from=None):
    """The walk in numpy.  {mode: blocks}, bounds, final state: blocks[k] is [2][frames][n] — float32 and exact for NEAREST, float64 for
    LINEAR and CUBIC; bounds[mode][k] is the allowed |gpu - ref| of the same shape (float64).  gain_from = (block, value): every voice's gain
    is float32(value) from that block on."""
    key = (n, gain_from)
    if key in _CACHE:
        return _CACHE[key]
    pcm, descs = _bank()
    smp = _sample_of(n)
    offset = np.array([descs[s].offset for s in smp], dtype=np.int64)
    length = np.array([descs[s].length for s in smp], dtype=np.int64)
    one_shot, gain = _one_shot(n).astype(bool), _gains(n)
    note_step = _note_step(n)
    idx, step, playing = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=bool)
    blocks, bounds = {m: [] for m in MODE_NAME}, {LINEAR: [], CUBIC: []}
    for k, frames in enumerate(SIZES):
        if k in ON_BLOCKS:
            idx[:], step[:], playing[:] = 0, note_step, True
        if k == OFF_BLOCK:
            playing &= one_shot
        if gain_from is not None and k == gain_from[0]:
            gain = np.full(n, np.float32(gain_from[1]), dtype=np.float32)
        f = np.arange(frames, dtype=np.uint64)
        pos = idx[None, :] + f[:, None] * step[None, :]                          # [frames][n], exact in 64 bits (idx < 2^57, f * step < 2^54)
        i = (pos >> np.uint64(44)).astype(np.int64)
        t = ((pos >> np.uint64(20)) & np.uint64(0xFFFFFF)).astype(np.float64) * 2.0 ** -24
        ok = playing[None, :] & (i < length[None, :])
        near = np.zeros((2, frames, n), dtype=np.float32)
        out = {LINEAR: np.zeros((2, frames, n)), CUBIC: np.zeros((2, frames, n))}
        bnd = {LINEAR: np.zeros((2, frames, n)), CUBIC: np.zeros((2, frames, n))}
        g64 = gain.astype(np.float64)[None, :]
        for ch in range(2):
            def tap(d, ch=ch):
                j = i + d
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
        valid = ok.sum(axis=0).astype(np.uint64)                                 # a prefix: the index only moves forward
        idx = idx + valid * step
        playing = playing & (valid == np.uint64(frames))
    for m in blocks:
        for b in blocks[m]:
            b.setflags(write=False)
    _CACHE[key] = (blocks, bounds, (idx.copy(), step.copy(), playing.copy()))
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


def _make(ctx, n, channels=2, mode=None):
    from groove_amd import entities as E
    pcm, descs = _bank()
    s = E.Sampler(ctx, pcm if channels == 2 else np.ascontiguousarray(pcm[:, 0]), descs, _params(n))
    if mode is not None:
        s.sample_interpolation = mode
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


def _clean(ctx):
    info = ctx.debug_info()
    assert info["zero_segments"] == 0 and info["fast_table_misses"] == 0, info


def _state_words(idx, step, playing):
    """SamplerState as groove_bank_download_state gives it: [6][n] words (idx lo, hi; step lo, hi; playing; pad)."""
    return np.stack([(idx & np.uint64(0xFFFFFFFF)).astype(np.uint32), (idx >> np.uint64(32)).astype(np.uint32),
                     (step & np.uint64(0xFFFFFFFF)).astype(np.uint32), (step >> np.uint64(32)).astype(np.uint32), playing.astype(np.uint32)])


def test_the_walk_has_every_case():
    """Not a GPU check: the numpy walk itself holds the cases the tests below rely on."""
    n = 70
    blocks, bounds, (idx, step, playing) = _reference(n)
    pcm, descs = _bank()
    steps = step.astype(np.float64) / 2.0 ** 44
    smp = _sample_of(n)
    pitched = smp != DRUM
    assert (steps[pitched] < 1).any() and (steps[pitched] == 1).any() and (steps[pitched] > 1).any() and (steps[~pitched] == 1).all()
    assert set(SIZES) == {64, 37, 17, 256} and set(LENGTHS) == {1, 2, 3, 100, 5000}
    for ln in set(LENGTHS):                                                      # every length below the root (fractions), and with an integer step
        assert ((np.array(LENGTHS)[smp] == ln) & (steps < 1)).any() and ((np.array(LENGTHS)[smp] == ln) & _integer_step(n)).any(), ln
    for k in range(len(LENGTHS)):                                                # adjacent samples, loud at both ends: a tap across a boundary shows
        o, ln = descs[k].offset, descs[k].length
        assert np.abs(pcm[o]).min() >= 0.2 and np.abs(pcm[o + ln - 1]).min() >= 0.2
        assert k == 0 or o == descs[k - 1].offset + descs[k - 1].length
    sounding = [np.any(b != 0, axis=(0, 1)) for b in blocks[NEAREST]]
    one_shot = _one_shot(n).astype(bool)
    long = smp >= 4
    assert (long & sounding[1] & ~sounding[2] & ~one_shot).any()                 # a note-off obeyed ...
    assert (sounding[2] & one_shot).any()                                        # ... and ignored by a one-shot, which the next note-on re-triggers
    frac = ~_integer_step(n)
    for mode in (LINEAR, CUBIC):                                                 # interpolation is audible where the step is fractional, and only there
        d = np.abs(blocks[mode][0][0] - blocks[NEAREST][0][0].astype(np.float64)).max(axis=0)
        assert (d[frac & (np.array(LENGTHS)[smp] >= 100)] > 1e-2).all() and (d[~frac] <= 2.0 ** -24).all(), mode   # (NEAREST's one fp32 rounding)
    assert np.abs(blocks[CUBIC][0] - blocks[LINEAR][0]).max() > 1e-2
    assert max(b.max() for b in bounds[CUBIC]) < 2e-5                            # the bound is rounding, orders below any of the above


@pytest.mark.parametrize("name", list(FORMS))
def test_blocks_and_state_in_every_mode(gpu_ctx, name):
    """Assertions 1, 2, 3: the block-writing forms against the f64 reference, both modes, mono and stereo; integer steps play NEAREST's
    bits; the state after the walk is the same words in the three modes (and the numpy walk's)."""
    with _form(gpu_ctx, name) as (n, says):
        want, bounds, final = _reference(n)
        whole = _integer_step(n)
        assert whole.any() and (~whole).any()
        for channels in (2, 1):
            bank = _make(gpu_ctx, n, channels)
            assert bank.sample_interpolation == NEAREST
            got, state = {}, {}
            for mode in (NEAREST, LINEAR, CUBIC):
                bank.sample_interpolation = mode
                assert bank.sample_interpolation == mode
                form = bank.kernel_form(64, False)
                assert says in form and (MODE_NAME[mode] in form) == (mode != NEAREST), form
                bank.reset()
                got[mode] = _walk(gpu_ctx, bank, n)
                state[mode] = bank.download_state()
            for k in range(len(SIZES)):
                for ch in range(2):
                    assert _same(got[NEAREST][k][ch], want[NEAREST][k][ch if channels == 2 else 0]), (name, channels, k, ch)
                for mode in (LINEAR, CUBIC):
                    _within(got[mode][k], want[mode][k], bounds[mode][k], (name, MODE_NAME[mode], channels, k), channels)
                    assert _same(got[mode][k][:, :, whole], got[NEAREST][k][:, :, whole]), (name, MODE_NAME[mode], channels, k)
            assert state[NEAREST].shape[0] == 6 and np.array_equal(state[NEAREST][:5], _state_words(*final)), (name, channels)
            assert np.array_equal(state[LINEAR], state[NEAREST]) and np.array_equal(state[CUBIC], state[NEAREST]), (name, channels)
            bank.destroy()
        _clean(gpu_ctx)


@pytest.mark.parametrize("name", list(FORMS))
def test_fused_buses(gpu_ctx, name):
    """Assertion 4: groove_bank_render_mix, _deferred and _paced against the f64 sum of the reference values: bus RMS / V <= 1e-5."""
    with _form(gpu_ctx, name) as (n, says):
        blocks = _reference(n)[0]
        for channels in (2, 1):
            bank = _make(gpu_ctx, n, channels)
            for mode in (LINEAR, CUBIC):
                want = np.concatenate([b.sum(axis=2).T for b in blocks[mode]])                       # [TOTAL][2]
                if channels == 1:
                    want = np.stack([want[:, 0], want[:, 0]], axis=1)
                bank.sample_interpolation = mode
                form = bank.kernel_form(64, True)
                assert says in form and MODE_NAME[mode] in form, form
                for entry in ("mix", "deferred", "paced"):
                    bank.reset()
                    got = _walk(gpu_ctx, bank, n, entry).astype(np.float64)
                    rms = np.sqrt(np.mean((got - want) ** 2, axis=0)) / n
                    sig = np.sqrt(np.mean(want ** 2, axis=0)) / n
                    print(f"{name} {MODE_NAME[mode]} {channels}ch {entry}: bus RMS error / V = {rms[0]:.3e}, {rms[1]:.3e} (signal {sig[0]:.3e}, {sig[1]:.3e})")
                    assert (sig > 1e-4).all() and (rms <= 1e-5).all(), (name, mode, channels, entry, rms, sig)
            bank.destroy()
        _clean(gpu_ctx)


@pytest.mark.parametrize("name", ["tp-70", "serial-70"])
def test_a_mode_set_mid_walk_takes_effect_at_the_next_block(gpu_ctx, name):
    """Assertion 5: LINEAR before block 2, CUBIC before block 4, NEAREST again before block 6 — each block is its own mode's reference
    (the state does not depend on the mode), the nearest blocks bit for bit."""
    with _form(gpu_ctx, name) as (n, _):
        want, bounds, final = _reference(n)
        plan = {2: LINEAR, 4: CUBIC, 6: NEAREST}
        for channels in (2, 1):
            bank = _make(gpu_ctx, n, channels)

            def before(k, bank=bank):
                if k in plan:
                    bank.sample_interpolation = plan[k]
            got = _walk(gpu_ctx, bank, n, before_block=before)
            for k, mode in enumerate([NEAREST, NEAREST, LINEAR, LINEAR, CUBIC, CUBIC, NEAREST, NEAREST]):
                if mode == NEAREST:
                    for ch in range(2):
                        assert _same(got[k][ch], want[NEAREST][k][ch if channels == 2 else 0]), (name, channels, k)
                else:
                    _within(got[k], want[mode][k], bounds[mode][k], (name, channels, k), channels)
            for k in (1, 2, 5, 6):                                                # the neighbours differ: a mode taken a block early or late shows
                assert np.abs(want[LINEAR][k] - want[NEAREST][k]).max() > 1e-2 and np.abs(want[CUBIC][k] - want[LINEAR][k]).max() > 1e-2
            assert np.array_equal(bank.download_state()[:5], _state_words(*final))
            bank.destroy()
        _clean(gpu_ctx)


def test_mixed_launch_takes_the_bank_by_bank_path(gpu_ctx):
    """Assertion 6: groove_banks_render_mix_deferred over {a small Welsh bank, an interpolated sampler bank} against the two banks rendered
    one by one with groove_bank_render_mix_deferred: bus RMS / V <= 1e-5; and the sampler bank in it is the interpolated one."""
    from groove_amd import entities as E
    nw, ns = 64, 300

    def run(together, mode):
        welsh, sampler = E.WelshSynth(gpu_ctx, P.welsh_voices(nw)), _make(gpu_ctx, ns, 1, mode)
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
    nearest = run(True, NEAREST)
    for mode in (LINEAR, CUBIC):
        a, b = run(True, mode), run(False, mode)
        rms = np.sqrt(np.mean((a - b) ** 2, axis=0)) / (nw + ns)
        print(f"mixed call, {MODE_NAME[mode]}: bus RMS difference / V = {rms[0]:.3e}, {rms[1]:.3e}")
        assert (rms <= 1e-5).all(), (mode, rms)
        moved = np.concatenate([(x - y.astype(np.float64)).sum(axis=2).T for x, y in zip(blocks[mode], blocks[NEAREST])])[:, 0]
        got = (a - nearest)[:, 0]                                                # what interpolation changed on the bus: the reference's difference
        assert np.abs(moved).max() > 1e-1 and np.sqrt(np.mean((got - moved) ** 2)) / (nw + ns) <= 1e-5, mode
    _clean(gpu_ctx)


def test_controls_reset_and_sample_rate_on_an_interpolated_bank(gpu_ctx):
    """Everything that takes a sampler bank takes an interpolated one: groove_bank_set_param on the gain before block 4 (the reference with
    the new gain), groove_bank_reset (the same walk again, bit for bit), and a sample-rate change, which leaves the mode where it is."""
    n = 70
    want, bounds, final = _reference(n, gain_from=(4, 0.6))
    bank = _make(gpu_ctx, n, 2, CUBIC)
    got = _walk(gpu_ctx, bank, n, before_block=lambda k: k == 4 and bank.control_set_param_by_index(T.CTL_SAMPLER_GAIN, 0.6))
    for k in range(len(SIZES)):
        _within(got[k], want[CUBIC][k], bounds[CUBIC][k], ("gain", k))
    assert np.array_equal(bank.download_state()[:5], _state_words(*final)) and bank.sample_interpolation == CUBIC
    rate = gpu_ctx.sample_rate
    try:
        gpu_ctx.update_sample_rate(48000)
        assert bank.sample_interpolation == CUBIC
        gpu_ctx.update_sample_rate(rate)
    finally:
        if gpu_ctx.sample_rate != rate:
            gpu_ctx.update_sample_rate(rate)
    assert bank.sample_interpolation == CUBIC
    bank.reset()                                                                 # (the state; the gain stays 0.6)
    again = _walk(gpu_ctx, bank, n)
    want, bounds, _ = _reference(n, gain_from=(0, 0.6))
    for k in range(len(SIZES)):
        _within(again[k], want[CUBIC][k], bounds[CUBIC][k], ("after reset", k))
        assert k < 4 or _same(again[k], got[k]), k                               # the same state and gain: the same bits
    _clean(gpu_ctx)
    bank.destroy()


def test_refusals_by_message(gpu_ctx):
    """Assertion 7: the setter on a Welsh bank and an unknown mode fail with a message and change nothing."""
    from groove_amd import entities as E
    L, h = gpu_ctx.L, gpu_ctx.h
    welsh = E.WelshSynth(gpu_ctx, P.welsh_voices(4))
    form = welsh.kernel_form(64, True)
    assert L.groove_bank_set_sample_interpolation(welsh.h, LINEAR) != 0
    assert L.groove_last_error(h).decode() == "groove_bank_set_sample_interpolation: only sampler and drumkit banks play samples"
    assert L.groove_bank_sample_interpolation(welsh.h) == NEAREST and welsh.kernel_form(64, True) == form
    bank = _make(gpu_ctx, 5, 1, LINEAR)
    assert L.groove_bank_set_sample_interpolation(bank.h, 3) != 0
    assert L.groove_last_error(h).decode() == "groove_bank_set_sample_interpolation: unknown mode (0 nearest, 1 linear, 2 cubic)"
    assert bank.sample_interpolation == LINEAR
    with pytest.raises(_lib.GrooveError, match="unknown mode"):
        bank.sample_interpolation = 0xFFFFFFFF
    assert bank.sample_interpolation == LINEAR and "linear" in bank.kernel_form(64, True)
    assert L.groove_bank_set_sample_interpolation(None, LINEAR) != 0 and L.groove_bank_sample_interpolation(None) == NEAREST
    for x in (welsh, bank):
        x.destroy()
    _clean(gpu_ctx)


def test_what_interpolation_is_for(gpu_ctx):
    """Assertion 8: one sample of sin(2 pi 440 n / 44100), root 440 Hz, played at key 57 (step 1/2) for one 256-frame block against the
    ideal sin(2 pi 220 n / 44100) * gain: the RMS error falls strictly from NEAREST to LINEAR to CUBIC.  In numpy the three are 1.24e-2,
    1.99e-4 and 1.96e-4; all but 1.5e-7 of CUBIC's is frame 1, whose tap before the sample's first frame is silence by definition where
    the ideal sine goes on.  Only the ordering is asserted."""
    from groove_amd import entities as E
    frames, length = 256, 600
    pcm = np.sin(2.0 * np.pi * 440.0 * np.arange(length) / 44100.0).astype(np.float32)
    descs = (T.SampleDesc * 1)()
    descs[0].offset, descs[0].length, descs[0].root_hz = 0, length, 440.0
    params = (T.SamplerParams * 1)()
    params[0].sample_index, params[0].one_shot, params[0].gain = 0, 0, 0.8
    ideal = np.sin(2.0 * np.pi * 220.0 * np.arange(frames) / 44100.0) * float(np.float32(0.8))
    bank = E.Sampler(gpu_ctx, pcm, descs, params)
    blk, rms = gpu_ctx.block(1, frames), {}
    for mode in (NEAREST, LINEAR, CUBIC):
        bank.sample_interpolation = mode
        bank.reset()
        bank.handle_midi_events(T.note_events_np(np.zeros(1, dtype=np.uint32), np.array([57], dtype=np.uint8), True))
        bank.generate_batch_values(blk, frames)
        got = blk.download(frames)
        assert _same(got[0], got[1])
        rms[mode] = float(np.sqrt(np.mean((got[0][:, 0].astype(np.float64) - ideal) ** 2)))
    print("RMS error against the ideal half-speed sine: " + ", ".join(f"{MODE_NAME[m]} {rms[m]:.3e}" for m in rms))
    assert rms[NEAREST] > rms[LINEAR] > rms[CUBIC], rms
    for x in (blk, bank):
        x.destroy()
    _clean(gpu_ctx)
