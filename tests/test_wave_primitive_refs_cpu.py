"""CPU tier: the references and case tables of the cross-lane probes (tests/wave_primitive_cases.py), not the library.
tests/test_gpu_wave_primitives.py demands "bit for bit" of the device on the exact and integer families; that is a fair demand only if
every exact result is representable, if the f64 model of the device's bracketing (T) and the serial fold (S) land on it without a
rounding, and if every order of an integer sum is exact.  And the tables must hold the lane positions and sizes the probes are for.
Also here: the workgroup-to-voice-group mapping of the time-parallel kernels (tp_group_of_block, welsh_tp_grid; host code)."""
from fractions import Fraction as Fr

import numpy as np

from tests import dsp_primitive_cases as K
from tests import wave_primitive_cases as W
from tests.probe import wave_probe as WP


def test_fma_and_the_rounding_helper_are_what_they_claim():
    r = np.random.default_rng(5)
    a, b = r.standard_normal(4000), r.standard_normal(4000)
    c = np.where(r.random(4000) < 0.5, -a * b * (1.0 + r.standard_normal(4000) * 2.0 ** -40), r.standard_normal(4000))   # half of them cancel
    for x, y, z in zip(a.tolist(), b.tolist(), c.tolist()):
        exact = Fr(x) * Fr(y) + Fr(z)
        assert W.fma(x, y, z) == W.round_frac(exact, 53) == float(exact), (x, y, z)
        assert np.float32(W.round_frac(Fr(x) * Fr(y), 24)) == np.float32(x * y) or abs(x * y) < 1e-30   # (x y carries 106 bits: f64 first is exact enough here)
    assert W.round_frac(Fr(3, 2) + Fr(1, 1 << 24), 24) == 1.5 and W.round_frac(Fr(1) + Fr(3, 1 << 24), 24) == 1.0 + 2.0 ** -22   # ties to even
    assert W.round_frac(Fr((1 << 24) - 1, 1) + Fr(1, 2), 24) == float(1 << 24) and W.round_frac(Fr(-5, 8), 24) == -0.625


def test_scan_tables_hold_every_lane_position_and_the_edges():
    x, names = W.scan_add_inputs()
    for k in range(64):
        one = x[names.index(f"one lane {k}")]
        assert np.count_nonzero(one[:, 0]) == 1 and one[k, 0] != 0 and one[k, 0] >> np.uint64(32) != one[k, 0] & np.uint64(0xFFFFFFFF)
    assert (x[names.index("all 2^64 - 1")] == np.uint64(W.TWO64 - 1)).all() and not x[names.index("zeros")].any()
    assert sum(n.startswith("random") for n in names) >= 4
    for lpv in W.LPVS:   # the reference keeps the groups apart
        out = W.scan_add_exact(lpv)
        assert (out[:, ::lpv] == x[:, ::lpv]).all()
    m, names = W.scan_max_inputs()
    assert (m[names.index("all -1")] == -1).all() and m.min() >= -1 and m.max() <= 255
    for k in range(64):
        one = m[names.index(f"one lane {k}")]
        assert one[k] >= 0 and (np.delete(one, k) == -1).all()
    assert (np.diff(m[names.index("descending")]) < 0).all()
    assert (W.scan_max_exact(32)[:, 32] == np.maximum(m[:, 32], -1)).all()


def test_affine_exact_family_is_exact_in_every_bracketing():
    maps, s0, names = W.affine_exact_inputs()
    for k in range(64):
        c = names.index(f"identity but lane {k}")
        assert all((tuple(maps[c, l]) == W.IDENTITY) == (l != k) for l in range(64))
    a, b = W.PAIR_A, W.PAIR_B
    assert W.affine_compose(a, b) != W.affine_compose(b, a)
    for lpv in W.LPVS:
        rec, st = W.affine_exact_refs(lpv)
        for c in range(len(maps)):
            ms = [tuple(m) for m in maps[c].tolist()]
            T = W.scan_affine_model(lpv, ms)
            start = s0[c].tolist()
            for g in W.groups(lpv):
                s = list(start)
                for l in g:
                    assert all(Fr(t) == x for t, x in zip(T[l], rec[c, l])), (lpv, names[c], l)       # T == X, so X is representable
                    s = W.affine_mul(ms[l], s, True)                                                   # S: the maps applied one after the other
                    assert all(Fr(v) == x for v, x in zip(s, st[c, l])), (lpv, names[c], l)
                    assert all(Fr(v) == x for v, x in zip(W.affine_mul(T[l], start, True), st[c, l]))
        if lpv == 32:   # nothing of lanes 0 - 31 in lanes 32 - 63: lane 32 holds its own map
            assert all(tuple(Fr(v) for v in maps[c, 32]) == tuple(rec[c, 32]) for c in range(len(maps)))


def test_affine_real_family_references_agree_to_f64_rounding():
    cutoffs = {n.split(" fc ")[1].split()[0] for n, *_ in W.affine_real_voices() if " fc " in n}
    assert {"25", "40", "2500", f"{W.FC_MAX:.0f}"} <= cutoffs
    for lpv in W.LPVS:
        names, maps, s0, X, S, T = W.affine_real_refs(lpv)
        y = W.yardstick(X, S, T)
        mag = np.array([max(float(abs(v)) for v in rx.reshape(-1)) for rx in X])
        print(f"affine real, LPV {lpv}: yardstick / max|X| at most {np.max(y / mag):.3e}")
        assert (y / mag < 1e-9).all(), [n for n, ok in zip(names, y / mag < 1e-9) if not ok]


def test_bq_exact_family_is_exact_in_every_bracketing():
    voices = W.bq_exact_voices()
    assert {v[1] for v in voices} == set(W.BQ_FRAMES) and {v[2] for v in voices} == {1.0, float(np.float32(0.3))}
    assert any(any(s != 0 for s in v[5]) for v in voices)
    for v in voices:
        o, ys, ns = W.bq_exact_ref(v)
        assert all(W.representable(y, 24) for y in ys) and all(W.representable(x, 53) for x in ns), v[0]
        sy, sns = W.bq_serial(v)
        assert [Fr(float(a)) for a in sy] == ys and [Fr(a) for a in sns] == ns, v[0]
        for lpv in W.LPVS:
            ty, tns = W.bq_model(lpv, v)
            assert [Fr(float(a)) for a in ty] == ys and [Fr(a) for a in tns] == ns, (v[0], lpv)
        assert len(o) == v[1] and all(float(np.float32(a)) == a for a in o)


def test_bq_real_family_covers_the_modes_and_its_references_agree():
    designs = W.bq_real_designs()
    assert len({n.split()[1] for n, _ in designs if n.startswith("kind")}) == 8 and any(n.startswith("24 dB") for n, _ in designs)
    voices = W.bq_real_voices()
    assert {v[1] for v in voices} == set(W.BQ_FRAMES)
    for v in voices[::7]:
        _, ys, _ = W.bq_exact_ref(v)
        sy, _ = W.bq_serial(v)
        ty, _ = W.bq_model(64, v)
        mag = max(1.0, max(abs(float(y)) for y in ys))
        assert max(abs(float(Fr(float(a)) - y)) for a, y in zip(sy, ys)) < 1e-8 * mag and max(abs(float(Fr(float(a)) - y)) for a, y in zip(ty, ys)) < 1e-8 * mag, v[0]


def test_integer_families_are_exact_in_every_order_of_summation():
    x = W.sum_integer_inputs().astype(np.float64)
    assert (x == np.rint(x)).all() and (np.abs(x) < 2 ** 15).all() and (np.abs(x).sum(axis=1) < 2 ** 24).all()
    assert all(any(np.count_nonzero(c) == 1 and c[k] != 0 for c in x) for k in range(64))
    tile, par = W.fused_cases()
    t = tile.astype(np.float64)
    assert (t == np.rint(t)).all() and (np.abs(t).sum(axis=2) < 2 ** 24).all()
    rows, desc, combos, size = W.reduce_cases()
    assert (rows == np.rint(rows)).all() and max(W.REDUCE_ROWS) * np.abs(rows).max() + W.REDUCE_PREFILL < 2 ** 24 and W.REDUCE_SENTINEL > 2 * max(W.REDUCE_ROWS) * np.abs(rows).max()


def test_tables_hold_the_positions_and_sizes_the_probes_are_for():
    d, v32, v64 = W.shfl_inputs()
    assert set(range(1, 33)) <= set(d.tolist()) and ((v64 >> np.uint64(32)) != (v64 & np.uint64(0xFFFFFFFF))).all()
    ok, src = W.shfl_judged(d)
    assert ok[list(d).index(32)].sum() == 32 and ok[list(d).index(1)].sum() == 63
    m = W.min_inputs()
    assert {int(np.argmin(c)) for c in m} == set(range(64)) and (m >= 2 ** 31).all(axis=1).any() and (m == 0).all(axis=1).any() and (m == 0xFFFFFFFF).all(axis=1).any()
    assert any((c == c.min()).sum() > 1 and c.min() > 0 and c.max() > c.min() for c in m)   # ties
    # FusedAcc: the 2,048 positions, every count, a row pair other than 0
    tile, par = W.fused_cases()
    pos = {(int(s), int(t)) for s, t in zip(*np.nonzero(tile[:2048, :, :, 0])[1:])}
    assert len(pos) == 2048 and (np.count_nonzero(tile[:2048].reshape(2048, -1), axis=1) == 2).all()
    assert set(par[2048:, 0].tolist()) == set(range(1, 9)) and (par[:, 2] != 0).any() and (par[:, 1] != 0).any() and (par[:, 3] < W.FUSED_FRAMES).any()
    assert (W.fused_exact() == W.FUSED_SENTINEL).any(axis=1).all()
    # tp_reduce_prev: the sizes, all four columns-per-pass cases, grids with idle workgroups
    rows, desc, combos, size = W.reduce_cases()
    assert {c[0] for c in combos} == set(W.REDUCE_ROWS) and {c[1] for c in combos} == set(W.REDUCE_FRAMES) and {c[3] for c in combos} == {0, 1}
    assert set(W.REDUCE_GRIDS) <= {c[2] for c in combos} and all(any(c[1] == f and c[2] > 2 * f for c in combos) for f in W.REDUCE_FRAMES)
    seen = {W.reduce_cp(c[1], c[2]) for c in combos}
    assert {cp for cp, _ in seen} == {1, 2, 4, 8} and any(idle for _, idle in seen)
    assert len(desc) == sum(c[2] for c in combos)
    # the noise generator: the chained starts are the rows of dsp_primitive_cases.noise_exact, 64 ticks apart
    starts, chain = W.noise_starts()
    vals, end = W.noise_exact(starts)
    ref = K.noise_exact()
    assert chain >= 8 and (starts[0] == (0x70F4F854, 0xE1E9F0A7)).all()
    for k in range(chain):
        assert (end[k] == ref[64 * (k + 1), 1:3]).all()
        bits = (vals[k].astype(np.float32) * np.float32(2.0 ** -31)).view(np.uint32)
        assert (bits == ref[64 * k + 1:64 * k + 65, 0]).all()


def test_every_grid_maps_its_workgroups_onto_the_voice_groups_one_to_one():
    """For every bank size 1 .. 20,000 and both voices-per-wavefront: tp_group_of_block is a permutation of the grid welsh_tp_grid gives,
    and the groups at or beyond ceil(n / voices per workgroup) — the padding — are exactly the ones without a voice."""
    perms = {}
    for vpw in (1, 2):
        per = WP.voices_per_workgroup(vpw)
        assert per == 4 * vpw
        for n in range(1, 20001):
            grid = WP.welsh_tp_grid(n, vpw)
            real = -(-n // per)
            assert real <= grid < real + 8 and (grid == real or (real >= 16 and grid % 8 == 0)), (n, vpw, grid)
            if grid not in perms:
                g = WP.groups_of_blocks(grid)
                assert (np.sort(g) == np.arange(grid)).all(), grid
                perms[grid] = g
            g = perms[grid]
            with_voice = g.astype(np.int64) * per < n
            assert with_voice.sum() == real and set(g[~with_voice].tolist()) == set(range(real, grid)), (n, vpw)
