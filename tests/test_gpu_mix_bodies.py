"""GPU tier: every reachable block body of the Welsh MIX kernel (kernels.h welsh_render_uniform_mix_kernel) and of the exact-f64 per-kind
kernels beside it, one representative patch each (tests/mix_bodies.py: 1,125 keys), against the f64 oracle and against each other.

Each representative plays 128 voices (two waves) on 64 keys over 14 ragged blocks (mix_bodies.SIZES): wave A struck in block 0 (its voices
agree: the FAST copy), wave B half in block 0 and half in block 1 (the shared body and the per-lane retune), part of A struck again in its
release, an idle tail.  pipeline_min_waves = 1 puts even these small banks in the MIX kernel.

(a) the block-writing MIX kernel (generate_batch_values_async), all representatives in one bank: every voice within 1e-5 RMS of
    max(1, level) of the oracle at look-ahead 3; at look-ahead 1 the same bits (F32 and exact-f64 kinds) or 2e-6 x max(1, peak) (smooth);
(b) the fused kernel, each representative sounding alone in that bank (groove_bank_reset between them), look-ahead 7 / 1 / 0 (FAST copy,
    shared body, per-lane retune): the same bits, or 1 == 0 and 7 within 2e-6 x 128 per sample of 1 (smooth); the bus against the
    oracle's within the voices' allowances summed; in a bank of its own, fast_waves grows block by block exactly as the voices' state
    says it must (mix_bodies.fast_waves_expected: empty and idle waves count too), and wave A takes its FAST copy with live voices in
    every block before its re-trigger;
(c) fused bus against the float64 sum of the block-writing voices (f64-filter bodies): rounding of an fp32 sum only, 16 x 2^-24 sum |voice|;
(d) fp32-filter bodies: against the same representative with GROOVE_F32_FILTER=0 (bits differ, 128 x 2e-6 RMS), and lanes 0, 31, 32, 63
    struck alone against the oracle (1e-5 RMS);
(e) each representative's bus from the shared bank is its bus from a bank of its own, value for value."""
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from groove_amd import abi_types as T
from tests import mix_bodies as M

pytestmark = pytest.mark.gpu

V = M.VOICES
FRAMES = sum(M.SIZES)
STARTS = np.cumsum([0] + M.SIZES[:-1])
LONE_LANES = (0, 31, 32, 63)


@pytest.fixture()
def mix_knobs(gpu_ctx):
    old = gpu_ctx.time_parallel_max_voices, gpu_ctx.split_max_waves, gpu_ctx.pipeline_min_waves, gpu_ctx.look_ahead
    assert old[3] == 3
    gpu_ctx.time_parallel_max_voices, gpu_ctx.split_max_waves, gpu_ctx.pipeline_min_waves = 0, 0, 1
    yield gpu_ctx
    gpu_ctx.time_parallel_max_voices, gpu_ctx.split_max_waves, gpu_ctx.pipeline_min_waves, gpu_ctx.look_ahead = old


def _table(patches):
    return (T.WelshParams * (V * len(patches)))(*[p for p in patches for _ in range(V)])


def _play_bus(ctx, synth, first=0, lanes=None):
    """The timeline on `synth` (its voices from `first`), fused onto a fresh bus; returns bus [frames][2] float64."""
    bus = ctx.bus(FRAMES)
    for b, fr in enumerate(M.SIZES):
        for ev in M.timeline_events(b, lanes, first=first):
            synth.handle_midi_events(ev)
        synth.render_mix(bus, fr, at_frame=int(STARTS[b]))
    out = bus.download().astype(np.float64)
    bus.destroy()
    return out


def _play_counted(ctx, synth, groups):
    """_play_bus on a representative's own bank at look-ahead 7, block by block: what the kernel counted in fast_waves against what
    welsh_wave_tables_up must count from the voices' state when the block starts (mix_bodies.fast_waves_expected).  Returns the bus and,
    per block, (counted, expected, the first voices of the live waves that took the FAST copy)."""
    bus = ctx.bus(FRAMES)
    per_block = []
    for b, fr in enumerate(M.SIZES):
        for ev in M.timeline_events(b):
            synth.handle_midi_events(ev)
        state = synth.download_state()   # (waits for the blocks before; the events land first, as they would in the render)
        before = ctx.debug_info()["fast_waves"]
        expected, live_fast = M.fast_waves_expected(state, groups)
        synth.render_mix(bus, fr, at_frame=int(STARTS[b]))
        synth.download_state()
        per_block.append((ctx.debug_info()["fast_waves"] - before, expected, live_fast))
    out = bus.download().astype(np.float64)
    bus.destroy()
    return out, per_block


def test_every_mix_body_against_the_oracle_and_itself(mix_knobs, oracle):
    from groove_amd import entities as E
    ctx = mix_knobs
    t0 = time.time()
    reps = M.representatives()
    keys = sorted(reps)
    R = len(keys)
    assert R == 1125 and all(reps[k] is not None for k in keys)
    patches = [reps[k] for k in keys]
    params = _table(patches)
    worst = {}

    def note(name, value):
        worst[name] = max(worst.get(name, 0.0), float(value))

    # ---- (a) block-writing MIX kernel, every voice, look-ahead 3 and 1; the oracle block by block (threads: one bank per representative)
    s3, s1 = E.WelshSynth(ctx, params), E.WelshSynth(ctx, params)
    assert "mix_kernel" in s3.kernel_form(256, True), s3.kernel_form(256, True)
    b3, b1 = ctx.block(V * R, 256), ctx.block(V * R, 256)
    obs = [oracle.Bank.welsh(_table([p])) for p in patches]
    err2, sig2, peak = np.zeros((R, V)), np.zeros((R, V)), np.zeros(R)   # M.voice_error_sums, block by block
    la_diff = np.zeros(R)
    la_bits = np.ones(R, dtype=bool)
    bus_want = np.zeros((R, FRAMES, 2))
    blk_sum = np.zeros((R, FRAMES, 2))
    blk_abs = np.zeros((R, FRAMES, 2))
    lone_want = np.zeros((R, len(LONE_LANES), FRAMES, 2))
    with ThreadPoolExecutor(16) as pool:
        for b, fr in enumerate(M.SIZES):
            for ev in M.timeline_events(b, copies=R):
                s3.handle_midi_events(ev); s1.handle_midi_events(ev)
            for ev in M.timeline_events(b):
                for ob in obs:
                    ob.note_events(ev)
            ctx.look_ahead = 3
            s3.generate_batch_values_async(b3, fr)
            ctx.look_ahead = 1
            s1.generate_batch_values_async(b1, fr)
            g3, g1 = b3.download(fr), b1.download(fr)
            f0 = int(STARTS[b])

            def check(r):
                want = obs[r].render(fr)
                x3 = g3[:, :, r * V:(r + 1) * V]
                x1 = g1[:, :, r * V:(r + 1) * V]
                e, w = M.voice_error_sums(x3, want)
                err2[r] += e
                sig2[r] += w
                peak[r] = max(peak[r], float(np.abs(want).max()) if fr else 0.0)
                la_bits[r] &= np.array_equal(x3.view(np.uint32), x1.view(np.uint32))
                la_diff[r] = max(la_diff[r], float(np.abs(x3.astype(np.float64) - x1).max()))
                bus_want[r, f0:f0 + fr] = want.sum(axis=2).T
                blk_sum[r, f0:f0 + fr] = x3.astype(np.float64).sum(axis=2).T
                blk_abs[r, f0:f0 + fr] = np.abs(x3.astype(np.float64)).sum(axis=2).T
                for i, lane in enumerate(LONE_LANES):
                    lone_want[r, i, f0:f0 + fr] = want[:, :, lane].T
                return bool(np.isfinite(x3).all()), float(np.abs(want).max()) if fr else 0.0

            res = list(pool.map(check, range(R)))
            assert all(ok for ok, _ in res), (b, [keys[r] for r, (ok, _) in enumerate(res) if not ok][:10])
            assert all(pk <= M.BOUND for _, pk in res), (b, [(keys[r], pk) for r, (_, pk) in enumerate(res) if pk > M.BOUND][:10])
    s3.destroy(); s1.destroy(); b3.destroy(); b1.destroy()
    del obs
    voice_err = M.voice_errors_of(err2, sig2, 2 * FRAMES)
    # the fused bus against the oracle's: if every voice keeps its bar, the bus's RMS error is at most the sum of their allowances
    bus_allow = M.VOICE_BAR * np.maximum(1.0, np.sqrt(sig2 / (2 * FRAMES))).sum(axis=1)
    smooth = np.array([k[0] in (2, 3) for k in keys])
    f32 = np.array([k[4] == 1 for k in keys])
    note("(a) voice RMS / max(1, level), look-ahead 3", voice_err.max())
    note("(a) smooth kinds, |look-ahead 1 - 3| / max(1, peak)", (la_diff / np.maximum(1.0, peak))[smooth].max())
    print(f"(a) done in {time.time() - t0:.1f} s")
    bad = np.flatnonzero(voice_err.max(axis=1) > M.VOICE_BAR)
    assert len(bad) == 0, [(keys[r], float(voice_err[r].max()), int(voice_err[r].argmax())) for r in bad[:10]]
    bad = np.flatnonzero(~la_bits & ~smooth)
    assert len(bad) == 0, [(keys[r], float(la_diff[r])) for r in bad[:10]]
    bad = np.flatnonzero(smooth & (la_diff > M.SMOOTH_BAR * np.maximum(1.0, peak)))
    assert len(bad) == 0, [(keys[r], float(la_diff[r])) for r in bad[:10]]
    assert np.sqrt(np.mean(bus_want ** 2)) > 1e-2

    # ---- (b) fused, each representative alone in the shared bank; (c) against the block-writing sum; (e) against a bank of its own;
    # (d) fp32-filter bodies: lanes alone, and against a context without the fp32 filter
    t1 = time.time()
    shared = E.WelshSynth(ctx, params)
    assert "mix_kernel" in shared.kernel_form(256, True)
    fused7 = {}
    for r, k in enumerate(keys):
        buses = {}
        for look in (7, 1, 0):
            ctx.look_ahead = look
            shared.reset()
            buses[look] = _play_bus(ctx, shared, first=r * V)
        fused7[r] = buses[7]
        bus_err = float(np.sqrt(np.mean((buses[7] - bus_want[r]) ** 2)))
        note("(b) fused bus RMS against the oracle, of the voices' allowances summed", bus_err / bus_allow[r])
        assert bus_err <= bus_allow[r], (k, bus_err, float(bus_allow[r]))
        if smooth[r]:
            assert np.array_equal(buses[1], buses[0]), k
            note("(b) smooth kinds, |look-ahead 7 - 1| per sample", np.abs(buses[7] - buses[1]).max())
            assert M.smooth_bus_ok(buses[7], buses[1]), (k, float(np.abs(buses[7] - buses[1]).max()))
        else:
            assert np.array_equal(buses[7], buses[1]) and np.array_equal(buses[1], buses[0]), (k, float(np.abs(buses[7] - buses[0]).max()))
        if not f32[r]:
            note("(c) fused bus against the block-writing sum, c", M.sum_rounding_c(buses[7], blk_sum[r], blk_abs[r]))
            assert M.sum_rounding_ok(buses[7], blk_sum[r], blk_abs[r]), (k, M.sum_rounding_c(buses[7], blk_sum[r], blk_abs[r]))
    shared.destroy()
    print(f"(b), (c) done in {time.time() - t1:.1f} s")

    t2 = time.time()
    miscounted, fast_short = [], []
    for r, k in enumerate(keys):
        ctx.look_ahead = 7
        own = E.WelshSynth(ctx, _table([patches[r]]))
        got = _play_bus(ctx, own)
        assert np.array_equal(got, fused7[r]), (k, float(np.abs(got - fused7[r]).max()))
        if k[0] < 4:   # (b) the FAST copies ran: counted exactly where the voices' state says, wave A in every block before its re-trigger
            own.reset()
            table = _table([patches[r]])
            groups = M.workgroups(table)
            assert [[n for _, n, _ in w] for _, w in groups] == [[64, 64, 0, 0]], groups   # waves A, B and two empty waves
            got, per_block = _play_counted(ctx, own, groups)
            assert np.array_equal(got, fused7[r]), (k, "counted run", float(np.abs(got - fused7[r]).max()))
            if any(c != e for c, e, _ in per_block):
                miscounted.append((k, per_block))
            # ... and the exact count requires wave A's (voices 0 - 63, struck together) in every block before the re-trigger
            if M.has_fast(k) and not all(0 in lf for _, _, lf in per_block[:M.RETRIGGER_BLOCK]):
                fast_short.append((k, per_block))
        if f32[r]:
            ctx.look_ahead = 3
            for i, lane in enumerate(LONE_LANES):
                own.reset()
                lone = _play_bus(ctx, own, lanes=np.array([lane], dtype=np.uint32))
                level = max(1.0, float(np.sqrt(np.mean(lone_want[r, i] ** 2))))
                note("(d) lane alone, RMS / max(1, level)", np.sqrt(np.mean((lone - lone_want[r, i]) ** 2)) / level)
                assert M.bus_ok(lone, lone_want[r, i]), (k, lane, float(np.sqrt(np.mean((lone - lone_want[r, i]) ** 2))))
        own.destroy()
    ctx.look_ahead = 3
    assert not miscounted, miscounted[:3]
    assert not fast_short, fast_short[:3]
    print(f"(e), FAST counts, (d) lanes done in {time.time() - t2:.1f} s")

    t3 = time.time()
    mp = pytest.MonkeyPatch()
    mp.setenv("GROOVE_F32_FILTER", "0")
    ctx0 = E.Context(0)
    mp.undo()
    try:
        ctx0.time_parallel_max_voices, ctx0.split_max_waves, ctx0.pipeline_min_waves = 0, 0, 1
        for r in np.flatnonzero(f32):
            s = E.WelshSynth(ctx0, _table([patches[r]]))
            got = _play_bus(ctx0, s)
            s.destroy()
            assert not np.array_equal(got, fused7[r]), f"{keys[r]}: the fp32-filter body gave the f64 body's bits"
            note("(d) fp32 against f64 body, bus RMS", np.sqrt(np.mean((got - fused7[r]) ** 2)))
            assert M.fp32_bus_ok(fused7[r], got), (keys[r], float(np.sqrt(np.mean((got - fused7[r]) ** 2))))
        ctx0.synchronize()
        info = ctx0.debug_info()
        assert info["zero_segments"] == 0 and info["fast_table_misses"] == 0, info
    finally:
        ctx0.close()
    print(f"(d) fp32 against f64 done in {time.time() - t3:.1f} s")
    info = ctx.debug_info()
    assert info["fast_table_misses"] == 0 and info["zero_segments"] == 0, info
    print(f"{R} representatives ({int(f32.sum())} fp32-filter, {sum(M.has_fast(k) for k in keys)} with a FAST copy) in {time.time() - t0:.1f} s; worst values:")
    for name, value in worst.items():
        print(f"  {name}: {value:.3e}")
