"""CPU tier: which Welsh block bodies a legal patch reaches (tests/mix_bodies.py), one bounded representative for each, and a negative
control for the bars tests/test_gpu_mix_bodies.py holds them to."""
import numpy as np

from groove_amd import abi_types as T
from tests import mix_bodies as M

REACHABLE = 1125   # of the 1,200 keys in the switches: 300 + 300 (F32 kinds) + 150 + 150 (smooth-f64) + 100 + 125 (exact-f64)


def test_the_grid_reaches_every_body_but_the_listed_ones():
    reach = M.reachable_keys()
    switch = M.switch_keys()
    print(f"reachable body keys: {len(reach)} of {len(switch)} in the switches ({len(switch - reach)} unreachable)")
    assert len(switch) == 1200
    assert reach <= switch
    assert len(reach) == REACHABLE
    by_kind = {b: sum(1 for k in reach if k[0] == b) for b in range(6)}
    assert by_kind == {0: 300, 1: 300, 2: 150, 3: 150, 4: 100, 5: 125}, by_kind
    # every key no legal patch reaches is a (kind, LFO class) plane with a reason: the list a pruning of the switches may drop
    missing = switch - reach
    planes = {(k[0], k[1]) for k in missing}
    assert planes == set(M.UNREACHABLE_REASONS), sorted(planes)
    assert missing == {k for k in switch if (k[0], k[1]) in M.UNREACHABLE_REASONS}
    for (base, cl), why in sorted(M.UNREACHABLE_REASONS.items()):
        print(f"  unreachable: {M.KIND_NAMES[base]} x LFO class {M.CLASS_NAMES[cl]} (25 oscillator pairs): {why}")
    # both widths of every body of kinds 0 - 3, and FAST copies for all of them but the static F32 kind's LFO-less bodies
    assert sum(1 for k in reach if k[0] < 4 and k[4] == 1) == 450
    assert sum(1 for k in reach if M.has_fast(k)) == 850


def test_the_grid_covers_every_field_the_classifier_reads():
    sc, oc = M.grid()
    assert {s[0] for s in sc} == set(range(11)) and {s[1] for s in sc} == set(M.ROUTINGS)
    assert {w for pair in oc for w in pair} == set(M.OSC_WAVES)
    # the filter descriptions sit on the intended side of the fp32 criterion (derive.h kFilterF32MaxError = 2e-6)
    for (mode, safe), _ in M.FILTERS.items():
        e = M.filter_f32_error(M.make_patch((T.WAVE_SINE, T.LFO_AMPLITUDE, 0, mode, safe), T.WAVE_SAWTOOTH, T.WAVE_SINE))
        assert (e <= 2e-6) == safe, (mode, safe, e)
    # an LFO-swept filter (cutoff routing) is flagged in both ways too
    swept = {sc[s][2] for s in sc if s[1] in M.CUTOFF_ROUTINGS and s[3] == "static" and sc[s][0] < 4}
    assert swept == {0, 1}
    # the unclassed, non-noise LFO waveforms reach the F32 kinds' `any` class, whose FAST copies a noise LFO never takes
    unclassed = [w for w in range(11) if w not in (T.WAVE_SINE, T.WAVE_SQUARE, T.WAVE_PULSE_WIDTH, T.WAVE_TRIANGLE, T.WAVE_SAWTOOTH, T.WAVE_NOISE)]
    for base in (0, 1):
        assert any(v[:2] == (base, M.OSC_ANY) and s[0] in unclassed for s, v in sc.items()), base


def test_every_reachable_key_has_a_bounded_representative():
    reps = M.representatives()
    assert set(reps) == M.reachable_keys()
    assert all(p is not None for p in reps.values()), [k for k, p in reps.items() if p is None]
    for k, p in reps.items():
        assert M.key(p) == k, (k, M.key(p))
    # every body with a FAST copy has a representative that can take it: no noise LFO (kernels.h welsh_wave_tables_up), the F32 kinds'
    # `any` LFO class included (its non-noise members: none, the debug constants, triangle-sine)
    noisy = [k for k, p in reps.items() if M.has_fast(k) and p.lfo_waveform == T.WAVE_NOISE]
    assert not noisy, noisy
    assert {p.lfo_waveform for k, p in reps.items() if M.has_fast(k) and k[0] in (0, 1) and k[1] == M.OSC_ANY} >= {
        T.WAVE_NONE, T.WAVE_DEBUG_ZERO, T.WAVE_DEBUG_MAX, T.WAVE_DEBUG_MIN, T.WAVE_TRIANGLE_SINE}
    # (representatives() keeps only patches bounded on all 128 voices of the timeline: M.bounded)


def _voices(seed=0):
    """Synthetic per-voice output [2][frames][128] with the level of a sounding representative."""
    rng = np.random.default_rng(seed)
    frames = sum(M.SIZES)
    t = np.arange(frames) / M.SR
    f = 110.0 * 2.0 ** (np.arange(M.VOICES) / 24.0)
    x = 0.3 * np.sin(2 * np.pi * f[None, :] * t[:, None]) + 0.05 * rng.standard_normal((frames, M.VOICES))
    return np.stack([x, 0.8 * x])


def test_the_checkers_reject_one_voice_perturbed_by_3e_5():
    want = _voices()
    rng = np.random.default_rng(1)
    for v in (0, 31, 64, 127):
        got = want.copy()
        d = rng.standard_normal(got[:, :, v].shape)
        got[:, :, v] += 3e-5 * d / np.sqrt(np.mean(d ** 2))   # 3e-5 RMS in one voice of 128
        assert M.voice_errors(want, want.astype(np.float32)).max() <= 1e-7
        # (the GPU test accumulates the same figure block by block: M.voice_error_sums over the ragged blocks, then M.voice_errors_of)
        cuts = np.cumsum([0] + M.SIZES)
        sums = [M.voice_error_sums(got[:, a:b], want[:, a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
        by_block = M.voice_errors_of(sum(e for e, _ in sums), sum(w for _, w in sums), 2 * cuts[-1])
        assert np.allclose(by_block, M.voice_errors(got, want), rtol=1e-12, atol=0)
        assert not M.voices_ok(got.astype(np.float32), want), v
        # ... and the same perturbation on a bus: one lane struck alone (the bus is that voice), and a representative's 128 voices
        # against the float64 sum of the block-writing kernel's voices — neither bar is divided by the voice count
        lone_want, lone_got = want[:, :, v].T, got[:, :, v].T
        assert M.bus_ok(lone_want.astype(np.float32), lone_want)
        assert not M.bus_ok(lone_got, lone_want), v
        bus_want, bus_got, abs_sum = want.sum(axis=2).T, got.sum(axis=2).T, np.abs(want).sum(axis=2).T
        assert M.sum_rounding_ok(bus_want.astype(np.float32), bus_want, abs_sum)
        assert not M.sum_rounding_ok(bus_got, bus_want, abs_sum), v
        # (the two bars that are per-voice allowances summed over 128 voices — fp32 body against f64 body, 2.56e-4 RMS; FAST copy against
        # the shared body in the smooth kinds, 2.56e-4 per sample — cannot see 3e-5 in one voice; the single lanes and the per-voice
        # block-writing checks are there for that)
        assert M.fp32_bus_ok(bus_got, bus_want) and M.smooth_bus_ok(bus_got, bus_want)
