"""GPU tier: sampler banks whose samples carry amplitude envelopes (include/groove_hip.h groove_bank_set_sample_envelopes;
docs/DSP_SPEC.md section 7; csrc/dsp_core.h sampler_frame_env, sampler_chunk_env; csrc/derive.h sampler_note_env; csrc/kernels.h
sampler_render_kernel<FUSED, STEREO, MODE, LOOP, ENV>; csrc/welsh_tp.h sampler_tp_body<..., ENV>, sampler_env_valid / _lane / _block_end).

The reference is numpy and plain Python, section 7 restated per (sample, key) pair: the cursor in exact integers as in
tests/test_gpu_sampler_loops.py, the envelope of section 3 in float64 from the float32 `len` words of derive_env and its stage counts
(ceil(len (1 - 2^-16)), env_frames restated).  An enveloped voice (its sample has an envelope, it is no one-shot): note-on starts the
cursor and attacks from the current value, note-off releases and leaves the cursor alone; per frame tick, stop if idle, read the
frame, stop and initialise the envelope if the sample has ended, else frame * envelope.  Every other voice: the loop test's walk.

Bounds.  The envelope's fp32 value: at most about sixteen half-ulp errors on terms of size <= |D| <= 1, so within 2^-20, doubled:
2^-19.  NEAREST: |gpu - ref| <= 2^-19 |pcm gain| + 2^-24 |ref|.  LINEAR and CUBIC: (2^-18 + 2^-19) M gain + 2^-24 |ref|, M the largest
|tap| of the frame (the loop test's bound plus the envelope's term).  No value is exempt.  For every stage the reference enters it
asserts that len (1 - 2^-16) lies at least 0.01 frames from an integer, so that an fp32 rounding of a release's or retrigger's start
value cannot move a stage count; the envelope times are chosen so that this holds.

Shapes: the time-parallel kernel at 5, 70 and 1,100 voices, the serial one at 70; block lengths 64, 37, 17, 256 three times over
(1,122 frames); keys an octave below the root, on it, an octave and three octaves above; mono and stereo; three modes.  Samples, adjacent
in the bank with first and last frames of magnitude >= 0.2: 300 frames; 5,000 looped [1000, 3000) (loops through its release); 7 with
a loop of one frame, sustain 0; 100 looped without an envelope; the drumkit sample, enveloped (its one-shot voices ignore that); 420
frames (ends during its release); 2,000 looped whose release outlasts the timeline.  Events: on at frame 0, off at 101, on again at 118
(inside the release: an attack from a non-zero value), off at 475 — block starts of both splits used.

Every test ends on zero_segments == 0 and fast_table_misses == 0."""
import contextlib
import ctypes as C
import math

import numpy as np
import pytest

from groove_amd import abi_types as T, lib as _lib, patches as P

pytestmark = pytest.mark.gpu

SR = 44100.0
SIZES = [64, 37, 17, 256] * 3
SIZES_B = [101, 17, 256] * 3
TOTAL = sum(SIZES)
EVENTS = {0: True, 101: False, 118: True, 475: False}              # frame: note-on / note-off, every voice
LENGTHS = (300, 5000, 7, 100, 5000, 420, 2000)
LOOPS = ((0, 0), (1000, 3000), (3, 4), (90, 100), (0, 0), (0, 0), (500, 1500))
ROOTS = (440.0, 440.0, 440.0, 440.0, 0.0, 440.0, 440.0)
ENV_A, ENV_ZERO, ENV_LONG, GATE = (0.002, 0.003, 0.6, 0.005), (0.0, 0.0, 0.0, 0.001), (0.001, 0.0, 1.0, 1.0), (0.0, 0.0, 1.0, 0.0)
ENVS = (ENV_A, ENV_A, ENV_ZERO, None, ENV_A, ENV_A, ENV_LONG)
NO_ENV, DRUM = 3, 4
KEYS = (57, 69, 81, 105)
NEAREST, LINEAR, CUBIC = T.SAMPLE_NEAREST, T.SAMPLE_LINEAR, T.SAMPLE_CUBIC
MODE_NAME = {NEAREST: "nearest", LINEAR: "linear", CUBIC: "cubic"}
FORMS = {"tp-5": (5, None, "sampler_tp_kernel"), "tp-70": (70, None, "sampler_tp_kernel"), "tp-1100": (1100, None, "sampler_tp_kernel"),
         "serial-70": (70, 0, "sampler_render_kernel (serial")}
IDLE, ATTACK, DECAY, SUSTAIN, RELEASE = range(5)
_CACHE = {}


def _bank():
    if "bank" not in _CACHE:
        rng = np.random.default_rng(20261021)
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
    return (np.arange(n) + np.arange(n) // 4) % len(LENGTHS)         # 4 keys, 7 samples: every sample meets every key


def _one_shot(n):
    return (np.arange(n) // 28) % 2


def _gains(n):
    return (0.25 + 0.5 * ((np.arange(n) * 7) % 11) / 11.0).astype(np.float32)


def _params(n):
    arr = (T.SamplerParams * n)()
    raw = np.zeros(n, dtype=np.dtype([("sample_index", "<u4"), ("one_shot", "<u4"), ("gain", "<f4")]))
    raw["sample_index"], raw["one_shot"], raw["gain"] = _sample_of(n), _one_shot(n), _gains(n)
    C.memmove(arr, raw.tobytes(), n * C.sizeof(T.SamplerParams))
    return arr


def _events_at(n, frame):
    if frame not in EVENTS:
        return []
    return [T.note_events_np(np.arange(n, dtype=np.uint32), _keys(n), EVENTS[frame])]


def _note_step(key, root):
    if not root > 0.0:
        return 1 << 44
    return int(np.float64(440.0 * np.exp2((np.float64(key) - 69.0) / 12.0)) / np.float64(root) * 17592186044416.0)


class _Env:
    """Section 3's envelope in float64 from derive_env's float32 words; stage counts ceil(len (1 - 2^-16)) with the margin asserted."""

    def __init__(self, a, d, s, r):
        sus = min(max(s, 0.0), 1.0)
        self.attack_len, self.decay_len = float(np.float32(a * SR)), float(np.float32(d * SR * (1.0 - sus)))
        self.attack_n, self.decay_n = self._count(a * SR, True), self._count(d * SR * (1.0 - sus), True)
        self.sustain, self.release_len = float(np.float32(sus)), float(np.float32(r * SR))
        self.init()

    @staticmethod
    def _count(length, derived=False):
        if not length > 0.0:
            return 0
        x = length * (1.0 - 2.0 ** -16)
        assert abs(x - round(x)) >= 0.01, ("a stage of %r frames: an fp32 rounding could move its count" % length, derived)
        return int(math.ceil(x))

    def _plateau(self, stage, level):
        self.stage, self.n, self.N, self.A, self.D, self.len = stage, 0, 0xFFFFFFFF, level, 0.0, 0.0

    def _enter(self, stage, frm, to, length, count):
        self.stage, self.n, self.N, self.A, self.D, self.len = stage, 0, count, frm, to - frm, length

    def init(self):
        self._plateau(IDLE, 0.0)
        self.value = 0.0

    def attack(self):
        if self.value == 0.0:
            self._enter(ATTACK, 0.0, 1.0, self.attack_len, self.attack_n)
        else:
            length = self.attack_len * (1.0 - self.value)
            self._enter(ATTACK, self.value, 1.0, length, self._count(length))

    def release(self):
        if self.stage == IDLE:
            return
        length = self.release_len * self.value
        self._enter(RELEASE, self.value, 0.0, length, self._count(length))

    def tick(self):
        for _ in range(2):
            if self.n >= self.N:
                if self.stage == ATTACK:
                    self._enter(DECAY, 1.0, self.sustain, self.decay_len, self.decay_n)
                elif self.stage == DECAY:
                    self._plateau(SUSTAIN, self.sustain)
                elif self.stage == RELEASE:
                    self._plateau(IDLE, 0.0)
        t = self.n / self.len if self.len > 0.0 else 0.0
        self.value = self.A + self.D * (2.0 * t - t * t)
        self.n += 1


def _pair_walk(sample, key, one_shot, envs):
    """One (sample, key, one-shot) voice through the timeline: per frame the cursor it reads at (folded), whether it sounds, its loop
    in force (start, end; 0, 0 none) and the envelope's factor; the state before every frame (and its events); the stages entered."""
    length, (ls0, le0), env_p = LENGTHS[sample], LOOPS[sample], envs[sample]
    enveloped = env_p is not None and not one_shot
    env = _Env(*env_p) if enveloped else None
    step_on = _note_step(key, ROOTS[sample])
    idx, step, playing = 0, 0, False
    pos, ok, fac, lp = np.zeros(TOTAL, dtype=np.uint64), np.zeros(TOTAL, dtype=bool), np.ones(TOTAL), np.zeros((TOTAL, 2), dtype=np.int64)
    states, stages = {}, set()
    for f in range(TOTAL + 1):
        states[f] = (idx, step, playing, None if env is None else (env.stage, env.n, env.N))
        if f == TOTAL:
            break
        if f in EVENTS:
            if EVENTS[f]:
                idx, step, playing = 0, step_on, True
                if enveloped:
                    env.attack()
            elif enveloped:
                env.release()
            elif not one_shot:
                playing = False
        if not playing:
            continue
        if enveloped:
            env.tick()
            stages.add(env.stage)
            if env.stage == IDLE:
                playing = False
                continue
        loops = le0 > 0 and not one_shot
        c = idx
        if loops and c >= le0 << 44:
            c = (ls0 << 44) + (c - (ls0 << 44)) % ((le0 - ls0) << 44)
        if (c >> 44) >= length:
            playing = False
            if enveloped:
                env.init()
            continue
        pos[f], ok[f], lp[f] = c, True, ((ls0, le0) if loops else (0, 0))
        if enveloped:
            fac[f] = env.value
        idx = c + step
        if loops and idx >= le0 << 44:
            idx = (ls0 << 44) + (idx - (ls0 << 44)) % ((le0 - ls0) << 44)
    return pos, ok, fac, lp, states, stages


def _interp(mode, tap, t):
    if mode == LINEAR:
        p0, p1 = tap(0), tap(1)
        return p0 + t * (p1 - p0), np.maximum(np.abs(p0), np.abs(p1))
    pm, p0, p1, p2 = tap(-1), tap(0), tap(1), tap(2)
    c1 = 0.5 * (p1 - pm)
    c2 = pm - 2.5 * p0 + 2.0 * p1 - 0.5 * p2
    c3 = 0.5 * (p2 - pm) + 1.5 * (p0 - p1)
    return ((c3 * t + c2) * t + c1) * t + p0, np.max(np.abs([pm, p0, p1, p2]), axis=0)


def _reference(n, envs=ENVS):
    """{mode: [2][TOTAL][n] float64}, {mode: bounds}, states {frame: (idx, step, playing) arrays}, stages seen per pair."""
    key = (n, envs)
    if key in _CACHE:
        return _CACHE[key]
    pcm, descs = _bank()
    smp, keys, one_shot, gain = _sample_of(n), _keys(n), _one_shot(n).astype(bool), _gains(n).astype(np.float64)
    out = {m: np.zeros((2, TOTAL, n)) for m in MODE_NAME}
    bnd = {m: np.zeros((2, TOTAL, n)) for m in MODE_NAME}
    st_frames = sorted(set(np.cumsum(SIZES).tolist() + np.cumsum(SIZES_B).tolist()))
    states = {f: (np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=bool)) for f in st_frames}
    all_stages, pairs = {}, {}
    for v in range(n):
        pk = (int(smp[v]), int(keys[v]), bool(one_shot[v]))
        if pk not in pairs:
            pairs[pk] = _pair_walk(*pk, envs)
            all_stages[pk] = pairs[pk][5]
        pos, ok, fac, lp, sts, _ = pairs[pk]
        for f in st_frames:
            states[f][0][v], states[f][1][v], states[f][2][v] = sts[f][0], sts[f][1], sts[f][2]
        s = pk[0]
        offset, length = descs[s].offset, LENGTHS[s]
        i = (pos >> np.uint64(44)).astype(np.int64)
        t = ((pos >> np.uint64(20)) & np.uint64(0xFFFFFF)).astype(np.float64) * 2.0 ** -24
        ls, le = lp[:, 0], lp[:, 1]
        lam = np.where(le > 0, le - ls, 1)
        for ch in range(2):
            def tap(d, ch=ch):
                j = i + d
                j = np.where((le > 0) & (j >= le), ls + (j - ls) % lam, j)
                inside = ok & (j >= 0) & (j < length)
                return np.where(inside, pcm[offset + np.clip(j, 0, length - 1), ch].astype(np.float64), 0.0)
            raw = np.where(ok, pcm[offset + np.minimum(i, length - 1), ch].astype(np.float64), 0.0)
            g32 = np.float64(np.float32(gain[v]))
            out[NEAREST][ch][:, v] = raw * g32 * fac
            bnd[NEAREST][ch][:, v] = 2.0 ** -19 * np.abs(raw * g32) + 2.0 ** -24 * np.abs(out[NEAREST][ch][:, v])
            for mode in (LINEAR, CUBIC):
                y, m = _interp(mode, tap, t)
                out[mode][ch][:, v] = np.where(ok, y * g32 * fac, 0.0)
                bnd[mode][ch][:, v] = (2.0 ** -18 + 2.0 ** -19) * m * g32 + 2.0 ** -24 * np.abs(out[mode][ch][:, v])
    for m in out:
        out[m].setflags(write=False)
    _CACHE[key] = (out, bnd, states, all_stages)
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


def _make(ctx, n, channels=2, mode=None, envs=ENVS, loops=LOOPS):
    from groove_amd import entities as E
    pcm, descs = _bank()
    s = E.Sampler(ctx, pcm if channels == 2 else np.ascontiguousarray(pcm[:, 0]), descs, _params(n))
    if mode is not None:
        s.sample_interpolation = mode
    if loops is not None:
        s.sample_loops = loops
    if envs is not None:
        s.sample_envelopes = list(envs)
    return s


def _walk(ctx, synth, n, sizes=SIZES, entry="blocks", each=None):
    """The timeline through one render entry.  "blocks": [2][TOTAL][n]; otherwise the bus [TOTAL][2]."""
    at = 0
    if entry == "blocks":
        blk, out = ctx.block(n, 256), []
        for frames in sizes:
            for ev in _events_at(n, at):
                synth.handle_midi_events(ev)
            synth.generate_batch_values(blk, frames)
            out.append(blk.download(frames))
            at += frames
            if each:
                each(at)
        blk.destroy()
        return np.concatenate(out, axis=1)
    bus = ctx.bus(TOTAL)
    render = getattr(synth, {"mix": "render_mix", "deferred": "render_mix_deferred", "paced": "render_mix_paced"}[entry])
    for frames in sizes:
        for ev in _events_at(n, at):
            synth.handle_midi_events(ev)
        render(bus, frames, at_frame=at)
        at += frames
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
    return np.stack([(idx & np.uint64(0xFFFFFFFF)).astype(np.uint32), (idx >> np.uint64(32)).astype(np.uint32),
                     (step & np.uint64(0xFFFFFFFF)).astype(np.uint32), (step >> np.uint64(32)).astype(np.uint32), playing.astype(np.uint32)])


def _the_walk_has_every_case():
    """The reference itself holds the cases the tests rely on (70 voices: every (sample, key) pair as a sampler voice and a one-shot)."""
    out, bnd, states, stages = _reference(70)
    smp, one_shot = _sample_of(70), _one_shot(70).astype(bool)
    for s in range(len(LENGTHS)):
        for key in KEYS:
            for os_ in (False, True):
                assert ((smp == s) & (_keys(70) == key) & (one_shot == os_)).any(), (s, key, os_)
    a = _Env(*ENV_A)
    assert (a.attack_n, a.decay_n) == (89, 53) and 132 <= _Env._count(a.release_len * a.sustain) <= 133       # every boundary inside a block, the release across blocks
    assert {ATTACK, DECAY, SUSTAIN, RELEASE, IDLE} <= stages[(1, 69, False)]                                    # the looped pad: all stages, idle after its second release
    snd = np.abs(out[NEAREST][0]) > 0
    pad = int(np.flatnonzero((smp == 1) & (_keys(70) == 69) & ~one_shot)[0])
    assert snd[101:118, pad].all() and snd[476:600, pad].all() and not snd[620:, pad].any()                     # it loops through both releases, then stops
    fast = int(np.flatnonzero((smp == 1) & (_keys(70) == 105) & ~one_shot)[0])                                  # step 8: 3,900 frames of cursor by then
    assert snd[476:600, fast].all() and 1000 <= int(states[TOTAL][0][fast] >> np.uint64(44)) < 3000             # ... inside its loop, where the cursor stays
    end = int(np.flatnonzero((smp == 5) & (_keys(70) == 69) & ~one_shot)[0])
    assert snd[476:537, end].all() and not snd[538:, end].any() and RELEASE in stages[(5, 69, False)]           # 420 frames from 118: ends in its release
    long_ = (smp == 6) & ~one_shot
    assert snd[-1][long_].all() and states[TOTAL][2][long_].all()                                               # the long release outlasts the timeline
    zero = (smp == 2) & ~one_shot
    assert not snd[:, zero].any() and states[64][2][zero].all() and not states[TOTAL][2][zero].any()          # sustain 0: silent while held on its plateau at 0, idle after the note-off
    drums = (smp == DRUM) & one_shot
    assert snd[101:118][:, drums].all() and (np.abs(out[NEAREST][0][0][drums]) >= 0.2 * 0.25 - 1e-6).all()      # one-shots ignore note-off and the envelope (full level on frame 0)
    retrig = int(np.flatnonzero((smp == 1) & (_keys(70) == 57) & ~one_shot)[0])
    assert abs(out[NEAREST][0][118, retrig]) > 0 and RELEASE in stages[(1, 57, False)]                          # the retrigger attacks from a non-zero value
    assert max(b.max() for b in bnd[CUBIC]) < 2e-5


@pytest.mark.parametrize("name", list(FORMS))
def test_blocks_and_state_against_the_reference(gpu_ctx, name):
    """1. Every form against the numpy restatement, three modes, mono and stereo, within the bounds of the docstring, no value exempt;
    the SamplerState words are the reference's exact integers; groove_bank_kernel_form says "enveloped"."""
    with _form(gpu_ctx, name) as (n, says):
        want, bounds, states, _ = _reference(n)
        if n == 70:
            _the_walk_has_every_case()
        for channels in (2, 1):
            bank = _make(gpu_ctx, n, channels)
            for mode in (NEAREST, LINEAR, CUBIC):
                bank.sample_interpolation = mode
                form = bank.kernel_form(64, False)
                assert says in form and form.endswith(", looped, enveloped)"), form
                bank.reset()
                got = _walk(gpu_ctx, bank, n).astype(np.float64)
                for ch in range(2):
                    rc = ch if channels == 2 else 0
                    err = np.abs(got[ch] - want[mode][rc])
                    worst = np.unravel_index(np.argmax(err / np.maximum(bounds[mode][rc], 1e-300)), err.shape)
                    print(f"{name} {MODE_NAME[mode]} {channels}ch ch{ch}: |gpu - ref| {err[worst]:.3e} of bound {bounds[mode][rc][worst]:.3e} at its worst (frame, voice) {tuple(int(x) for x in worst)}")
                    assert (err <= bounds[mode][rc]).all(), (name, MODE_NAME[mode], channels, ch, worst, float(err[worst]), float(bounds[mode][rc][worst]), float(want[mode][rc][worst]))
                assert np.array_equal(bank.download_state()[:5], _state_words(*states[TOTAL])), (name, MODE_NAME[mode], channels)
            bank.destroy()
        _clean(gpu_ctx)


def _record(gpu_ctx, name, channels, mode, sizes=SIZES, envs=ENVS, entry="blocks"):
    """(output, [SamplerState words at every block end], [envelope state words at every block end]) of one form."""
    with _form(gpu_ctx, name) as (n, says):
        bank = _make(gpu_ctx, n, channels, mode, envs)
        assert says in bank.kernel_form(64, entry != "blocks")
        st, es = [], []
        if entry == "blocks":
            def each(at):
                st.append(bank.download_state())
                if envs is not None:
                    es.append(bank.sample_envelope_state())
            out = _walk(gpu_ctx, bank, n, sizes, each=each)
        else:
            out = _walk(gpu_ctx, bank, n, sizes, entry)
            st.append(bank.download_state())
            es.append(bank.sample_envelope_state())
        bank.destroy()
    return out, st, es


@pytest.mark.parametrize("channels", [2, 1])
def test_the_two_forms_agree_bit_for_bit(gpu_ctx, channels):
    """2. Time-parallel against serial at 70 voices: the output block, the SamplerState words and the envelope state words after every
    block, every mode; and the fused groove_bank_render_mix entries leave the state and envelope words of the plain render, their bus the
    plain render's sum (RMS / V <= 1e-5, fp32 order of addition)."""
    for mode in (NEAREST, LINEAR, CUBIC):
        tp, serial = _record(gpu_ctx, "tp-70", channels, mode), _record(gpu_ctx, "serial-70", channels, mode)
        assert _same(tp[0], serial[0]), (MODE_NAME[mode], channels)
        for k, (a, b) in enumerate(zip(tp[1], serial[1])):
            assert np.array_equal(a, b), (MODE_NAME[mode], channels, k)
        for k, (a, b) in enumerate(zip(tp[2], serial[2])):
            assert np.array_equal(a, b), (MODE_NAME[mode], channels, k, np.flatnonzero((a != b).any(axis=0))[:8])
        want = tp[0].astype(np.float64).sum(axis=2).T
        for name in ("tp-70", "serial-70"):
            for entry in ("mix", "deferred", "paced") if mode == CUBIC else ("mix",):
                bus, st, es = _record(gpu_ctx, name, channels, mode, entry=entry)
                assert np.array_equal(st[0], tp[1][-1]) and np.array_equal(es[0], tp[2][-1]), (name, entry, MODE_NAME[mode])
                rms = np.sqrt(np.mean((bus.astype(np.float64) - want) ** 2, axis=0)) / 70
                assert (rms <= 1e-5).all(), (name, entry, rms)
    _clean(gpu_ctx)


@pytest.mark.parametrize("name", ["tp-70", "serial-70"])
def test_the_split_into_blocks_changes_nothing(gpu_ctx, name):
    """3. The same events at the same frames under blocks (64, 37, 17, 256) and (101, 17, 256): identical output, and identical state
    and envelope records wherever both splits have a block end."""
    ends_a, ends_b = np.cumsum(SIZES).tolist(), np.cumsum(SIZES_B).tolist()
    common = [f for f in ends_a if f in ends_b]
    assert len(common) >= 6
    for channels, mode in ((2, CUBIC), (1, NEAREST), (1, LINEAR)):
        a, b = _record(gpu_ctx, name, channels, mode, SIZES), _record(gpu_ctx, name, channels, mode, SIZES_B)
        assert _same(a[0], b[0]), (name, channels, MODE_NAME[mode])
        for f in common:
            ia, ib = ends_a.index(f), ends_b.index(f)
            assert np.array_equal(a[1][ia], b[1][ib]) and np.array_equal(a[2][ia], b[2][ib]), (name, channels, MODE_NAME[mode], f)
    _clean(gpu_ctx)


@pytest.mark.parametrize("name", ["tp-70", "serial-70", "tp-1100"])
def test_the_gate_envelope_is_no_envelope(gpu_ctx, name):
    """4. Attack 0, decay 0, sustain 1, release 0 on every sample against the same bank without envelopes: output and
    groove_bank_download_state identical after every block of the event script."""
    for channels, mode in ((2, CUBIC), (1, NEAREST), (2, LINEAR)):
        gate = _record(gpu_ctx, name, channels, mode, envs=(GATE,) * len(LENGTHS))
        plain = _record(gpu_ctx, name, channels, mode, envs=None)
        assert _same(gate[0], plain[0]), (name, channels, MODE_NAME[mode])
        for k, (a, b) in enumerate(zip(gate[1], plain[1])):
            assert np.array_equal(a, b), (name, channels, MODE_NAME[mode], k)
    _clean(gpu_ctx)


def test_refusals_round_trip_and_what_keeps_the_envelopes(gpu_ctx):
    """5. The setter's refusals by message; the getter's round trip; reset silences the envelopes and keeps them; set_param on the gain
    keeps them, and so does a sample-rate change; clearing stops releasing voices and leaves held ones playing."""
    from groove_amd import entities as E
    L, h = gpu_ctx.L, gpu_ctx.h
    welsh = E.WelshSynth(gpu_ctx, P.welsh_voices(4))
    one = (T.EnvelopeParams * 1)(T.EnvelopeParams(*GATE))
    assert L.groove_bank_set_sample_envelopes(welsh.h, one, None, 1) != 0
    assert L.groove_last_error(h).decode() == "groove_bank_set_sample_envelopes: only sampler and drumkit banks play samples"
    assert L.groove_bank_sample_envelopes(welsh.h, None, None, 0) == 0
    n = 70
    bank = _make(gpu_ctx, n, 1, LINEAR)
    envs = [None if e is None else tuple(e) for e in ENVS]
    assert bank.sample_envelopes == envs and L.groove_bank_sample_envelopes(bank.h, None, None, 0) == 6
    for bad, says in (([ENV_A] * 3, "n_samples is not the bank's sample count (7)"),
                      ([ENV_A, (-0.1, 0, 1, 0)] + [ENV_A] * 5, "a negative or non-finite time (sample 1)"),
                      ([ENV_A, (0, float("inf"), 1, 0)] + [ENV_A] * 5, "a negative or non-finite time (sample 1)"),
                      ([ENV_A, (0, 0, 1, float("nan"))] + [ENV_A] * 5, "a negative or non-finite time (sample 1)"),
                      ([ENV_A] * 6 + [(0, 0, 1.5, 0)], "sustain outside [0, 1] (sample 6)"),
                      ([ENV_A] * 6 + [(0, 0, -0.5, 0)], "sustain outside [0, 1] (sample 6)")):
        with pytest.raises(_lib.GrooveError) as err:
            bank.sample_envelopes = bad
        assert ("groove_bank_set_sample_envelopes: " + says) in str(err.value), str(err.value)
        assert bank.sample_envelopes == envs and bank.kernel_form(64, True).endswith(", enveloped)")
    welsh.destroy()
    plain = _make(gpu_ctx, n, 1, LINEAR, envs=None)
    with pytest.raises(_lib.GrooveError, match="the bank has no sample envelopes"):
        plain.sample_envelope_state()
    plain.destroy()
    # set_param on the gain and a reset keep the envelopes; the reset leaves every record idle
    blk = gpu_ctx.block(n, 256)
    keys, lanes = _keys(n), np.arange(n, dtype=np.uint32)
    bank.handle_midi_events(T.note_events_np(lanes, keys, True))
    bank.generate_batch_values(blk, 64)
    assert (bank.sample_envelope_state()[0] != IDLE).any()
    bank.control_set_param_by_index(T.CTL_SAMPLER_GAIN, 0.6)
    assert bank.sample_envelopes == envs and (bank.sample_envelope_state()[0] != IDLE).any()
    bank.reset()
    es = bank.sample_envelope_state()
    assert bank.sample_envelopes == envs and (es[0] == IDLE).all() and (es[6] == 0).all() and "enveloped" in bank.kernel_form(64, False)
    # a sample-rate change keeps them, derives the parameters again (an attack of 0.002 s is 96 frames at 48 kHz, 89 at 44.1) and leaves the records idle
    rate, first = gpu_ctx.sample_rate, int(np.flatnonzero((_sample_of(n) == 1) & (_one_shot(n) == 0))[0])
    try:
        gpu_ctx.update_sample_rate(48000)
        assert bank.sample_envelopes == envs and (bank.sample_envelope_state()[0] == IDLE).all()
        bank.handle_midi_events(T.note_events_np(lanes, keys, True))
        bank.generate_batch_values(blk, 64)
        es = bank.sample_envelope_state()
        assert es[0][first] == ATTACK and es[1][first] == 64 and es[2][first] == 96, es[:3, first]
    finally:
        gpu_ctx.update_sample_rate(rate)
    es = bank.sample_envelope_state()
    assert bank.sample_envelopes == envs and (es[0] == IDLE).all()
    # clearing: releasing voices stop, held ones play on
    smp, one_shot = _sample_of(n), _one_shot(n).astype(bool)
    pads = np.flatnonzero((smp == 1) & ~one_shot)
    bank.handle_midi_events(T.note_events_np(lanes, keys, True))
    bank.generate_batch_values(blk, 256)
    bank.handle_midi_events(T.note_events_np(pads[:2].astype(np.uint32), keys[pads[:2]], False))
    bank.generate_batch_values(blk, 17)
    es, st = bank.sample_envelope_state(), bank.download_state()
    assert (es[0][pads[:2]] == RELEASE).all() and (es[0][pads[2:]] == SUSTAIN).all() and (st[4][pads] == 1).all()
    bank.sample_envelopes = None
    assert "enveloped" not in bank.kernel_form(64, False) and bank.sample_envelopes == [None] * len(LENGTHS)
    st = bank.download_state()
    assert (st[4][pads[:2]] == 0).all() and (st[4][pads[2:]] == 1).all()
    bank.generate_batch_values(blk, 64)
    got = blk.download(64)
    assert not got[:, :, pads[:2]].any() and np.abs(got[0][:, pads[2:]]).max() > 0
    # set again onto playing voices: a plateau at the sustain level for a voice that plays, idle for the others
    bank.sample_envelopes = envs
    es, st = bank.sample_envelope_state(), bank.download_state()
    enveloped = np.array([ENVS[s] is not None for s in smp]) & ~one_shot
    assert (es[0][enveloped & (st[4] == 1)] == SUSTAIN).all() and (es[0][~(enveloped & (st[4] == 1))] == IDLE).all() and (enveloped & (st[4] == 1)).any()
    assert np.array_equal(es[6][pads[2:]].view(np.float32), np.full(len(pads) - 2, np.float32(0.6)))
    for x in (blk, bank):
        x.destroy()
    _clean(gpu_ctx)


def test_mixed_launch_takes_the_bank_by_bank_path(gpu_ctx):
    """groove_banks_render_mix_deferred over {a small Welsh bank, an enveloped sampler bank without loops} against the two banks rendered
    one by one: bus RMS / V <= 1e-5, and the sampler in it is the enveloped one (its tail sounds after the note-off)."""
    from groove_amd import entities as E
    nw, ns = 64, 300

    def run(together, envs):
        welsh, sampler = E.WelshSynth(gpu_ctx, P.welsh_voices(nw)), _make(gpu_ctx, ns, 1, NEAREST, envs, loops=None)
        welsh.handle_midi_events(P.note_on_all(nw))
        bus, at = gpu_ctx.bus(TOTAL), 0
        for frames in SIZES:
            for ev in _events_at(ns, at):
                sampler.handle_midi_events(ev)
            if together:
                gpu_ctx.render_mix_banks_deferred([welsh, sampler], bus, frames, at_frame=at)
            else:
                welsh.render_mix_deferred(bus, frames, at_frame=at)
                sampler.render_mix_deferred(bus, frames, accumulate=True, at_frame=at)
            at += frames
        gpu_ctx.flush_bus()
        got = bus.download().astype(np.float64)
        for x in (bus, welsh, sampler):
            x.destroy()
        return got

    a, b, never = run(True, ENVS), run(False, ENVS), run(True, None)
    rms = np.sqrt(np.mean((a - b) ** 2, axis=0)) / (nw + ns)
    print(f"mixed call, enveloped: bus RMS difference / V = {rms[0]:.3e}, {rms[1]:.3e}")
    assert (rms <= 1e-5).all(), rms
    assert np.abs((a - never)[102:118]).max() > 1e-2                              # the release tail is on the bus
    _clean(gpu_ctx)
