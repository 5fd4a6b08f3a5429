"""The Welsh block bodies the kernels hold, which of them a legal patch reaches, and one representative patch per reachable body
(tests/test_mix_body_coverage.py, tests/test_gpu_mix_bodies.py).

A BODY KEY is (base kind, LFO class, oscillator-1 class, oscillator-2 class, fp32-filter flag), read from the library's own rule
(dsp_core.h welsh_base_kind / welsh_body_classes, derive.h welsh_filter_f32_ok) through tests/emul (emul_welsh_classify).  The flag
names the fp32-filter copy of a body, which only the fused mix kernel carries (kinds 0 - 3); the exact-f64 kinds 4 and 5 ignore it
(kernels.h welsh_render_uniform_kernel), so their keys carry 0.

The classifier reads the two oscillators' waveforms for the oscillator classes and nothing else of them; it reads the LFO (waveform,
routing, depth, frequency) and the filter (cutoff, sweep, ripple) for the base kind, the LFO class and the flag, and no oscillator.  The
grid below is the product of every value of each such field, and its reachable set is the product of the two parts' classes.  Every
representative is classified again as the whole patch it is."""
import ctypes as C
import itertools
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from groove_amd import patches as P, abi_types as T

SR = T.DEFAULT_SAMPLE_RATE
KIND_NAMES = ("F32 static", "F32 retune", "smooth-f64 static", "smooth-f64 retune", "exact-f64 static", "exact-f64 retune")
OSC_ANY, OSC_PULSE, OSC_SAW, OSC_TRIANGLE, OSC_SINE = range(5)   # dsp_core.h "Oscillator CLASSES"
LFO_UNUSED = 5
CLASS_NAMES = ("any", "pulse", "saw", "triangle", "sine", "unused")

OSC_WAVES = [T.WAVE_NONE, T.WAVE_SINE, T.WAVE_SQUARE, T.WAVE_PULSE_WIDTH, T.WAVE_TRIANGLE, T.WAVE_SAWTOOTH,
             T.WAVE_NOISE, T.WAVE_TRIANGLE_SINE, T.WAVE_DEBUG_MAX]
LFO_WAVES = list(range(11))   # every groove_waveform, the debug constants and triangle-sine included
ROUTINGS = [T.LFO_NONE, T.LFO_AMPLITUDE, T.LFO_PITCH, T.LFO_PULSE_WIDTH, T.LFO_FILTER_CUTOFF,
            T.LFO_PITCH_OSC2, T.LFO_PW_OSC1, T.LFO_PW_OSC2, T.LFO_RESONANCE, T.LFO_CUTOFF_AMP]
CUTOFF_ROUTINGS = (T.LFO_FILTER_CUTOFF, T.LFO_CUTOFF_AMP)
# (depth, frequency Hz): a gentle LFO (a pitch LFO stays under the smooth promise, derive.h WF_LFO_SMOOTH) and a strong one (over it)
LFO_STRENGTHS = [(0.2, 5.13), (1.0, 61.7)]
# Filter descriptions, one the host's fp32 criterion accepts and one it refuses (derive.h welsh_filter_f32_error, checked by
# test_mix_body_coverage.py): (cutoff Hz, cutoff start, cutoff end, ripple).  A cutoff routing sweeps the `static` ones with the LFO.
FILTERS = {
    ("static", True): (2500.0, 0.75, 0.0, 0.707),
    ("static", False): (40.0, 0.03, 0.0, 0.707),
    ("env", True): (2500.0, 0.55, 0.3, 0.707),
    ("env", False): (40.0, 0.02, 0.3, 0.707),
}

# The timeline every representative plays (tests/test_gpu_mix_bodies.py): ragged blocks, 128 voices on 64 keys.  Wave A (voices 0 - 63)
# is struck in block 0 and its voices agree until part of it is struck again during its release (block RETRIGGER_BLOCK); wave B has half
# its voices struck in block 0 and half in block 1; A and B are released in different blocks; the run ends in an idle tail.
VOICES = 128
SIZES = [256, 1, 37, 256, 100, 64, 255, 1, 7, 37, 256, 129, 200, 64]
RETRIGGER_BLOCK = 5
# 64 keys, no A: 55 and 110 Hz are rational in 44,100 and put a square's edge exactly on a frame (docs/DSP_SPEC.md section 2)
KEYS = np.array([k for k in range(30, 120) if k % 12 != 9][:64], dtype=np.uint8)
LANES = np.arange(VOICES, dtype=np.uint32)
WAVE_A, B_LO, B_HI, RETRIG = LANES[:64], LANES[64:96], LANES[96:], LANES[:16]
BOUND = 4.0   # a representative's oracle output stays within this (test_gpu_welsh_classes.py's bar for "numerically meaningful")
SOUNDING = 0.05   # ... and reaches this: a silent representative (an amplitude LFO at depth 1 on a debug-minimum wave) proves nothing


def voice_key(v):
    return int(KEYS[int(v) % 64])


def timeline_events(block, lanes=None, first=0, copies=1):
    """The note events (groove_note_event arrays) that land before `block`, restricted to `lanes` when given; for the voices of a
    representative from voice `first` on, or for `copies` representatives side by side."""
    script = {0: [(WAVE_A, True), (B_LO, True)], 1: [(B_HI, True)], 4: [(WAVE_A, False)], RETRIGGER_BLOCK: [(RETRIG, True)],
              7: [(LANES[64:], False)], 9: [(RETRIG, False)]}
    out = []
    for voices, on in script.get(block, []):
        if lanes is not None:
            voices = np.intersect1d(voices, lanes).astype(np.uint32)
        if len(voices):
            keys = np.tile(KEYS[voices % 64], copies)
            voices = (np.arange(copies, dtype=np.uint32)[:, None] * VOICES + voices[None, :]).ravel() + np.uint32(first)
            out.append(T.note_events_np(voices.astype(np.uint32), keys, on))
    return out


_LIB = None


def _lib():
    global _LIB
    if _LIB is None:
        from tests.emul import emul as E
        _LIB = E.lib()
        _LIB.emul_welsh_classify.argtypes = [C.POINTER(T.WelshParams), C.c_uint32, C.POINTER(C.c_uint32)]
    return _LIB


def classify(p):
    """emul_welsh_classify: (base kind, LFO class, oscillator-1 class, oscillator-2 class, WF_FILTER_F32 promise, flags)."""
    out = (C.c_uint32 * 6)()
    _lib().emul_welsh_classify(C.byref(p), SR, out)
    return tuple(int(x) for x in out)


def key(p):
    base, cl, c1, c2, f32 = classify(p)[:5]
    return (base, cl, c1, c2, f32 if base < 4 else 0)


def filter_f32_error(p):
    return float(_lib().emul_filter_f32_error(C.byref(p), SR))


def has_fast(k):
    """The body has a FAST copy in the fused mix kernel (kernels.h welsh_dispatch_class): kinds 0 - 3 only; the retuned kinds 1 and 3
    carry the coefficient table, every LFO class but LFO_UNUSED the LFO table."""
    base, cl = k[0], k[1]
    return base < 4 and (base in (1, 3) or cl != LFO_UNUSED)


def switch_keys():
    """Every body key the kernels' class switches hold (kernels.h welsh_dispatch_class): six LFO classes in kinds 0, 1, 4, 5, three (any,
    triangle, sine) in the smooth-f64 kinds 2, 3; the fp32-filter copies in kinds 0 - 3 only."""
    out = set()
    for base in range(6):
        cls = range(6) if base not in (2, 3) else (OSC_ANY, OSC_TRIANGLE, OSC_SINE)
        for cl, c1, c2, f in itertools.product(cls, range(5), range(5), (0, 1) if base < 4 else (0,)):
            out.add((base, cl, c1, c2, f))
    return out


# Keys of the switches no legal patch reaches, and why (the bodies a pruning may drop).
UNREACHABLE_REASONS = {
    (4, OSC_PULSE): "a square or pulse LFO is always smooth (no slope between its edges): on the pitch or pulse width it takes the "
                    "smooth-f64 kinds, and only the resonance routing, which retunes, takes it to the exact-f64 kinds",
    (4, LFO_UNUSED): "an exact-f64 kind needs an LFO routed to the pitch, the pulse width or the resonance",
    (5, LFO_UNUSED): "an exact-f64 kind needs an LFO routed to the pitch, the pulse width or the resonance",
}


def base_patch(k=0):
    """The grid's fixed part: short envelopes, so that the timeline reaches every stage, the release and the idle tail."""
    p = P.welsh_patch(k)
    p.amp_envelope = T.EnvelopeParams(0.003, 0.01, 0.7, 0.004)
    p.filter_envelope = T.EnvelopeParams(0.002, 0.008, 0.5, 0.005)
    p.oscillator_mix = 0.6
    p.oscillator_2_sync = 0
    p.dca_gain = 1.0
    return p


def control_setups():
    """The grid's LFO x filter part: (LFO waveform, routing, strength index, filter mode, fp32-safe description)."""
    return list(itertools.product(LFO_WAVES, ROUTINGS, range(len(LFO_STRENGTHS)), ("static", "env"), (True, False)))


def osc_pairs():
    return list(itertools.product(OSC_WAVES, OSC_WAVES))


def make_patch(setup, w1, w2, depth_scale=1.0, freq_scale=1.0, k=0):
    wl, routing, si, mode, safe = setup
    p = base_patch(k)
    p.oscillator_1.waveform, p.oscillator_1.duty = w1, (0.3 if w1 == T.WAVE_PULSE_WIDTH else 0.5)
    p.oscillator_2.waveform, p.oscillator_2.duty = w2, (0.15 if w2 == T.WAVE_PULSE_WIDTH else 0.5)
    depth, freq = LFO_STRENGTHS[si]
    p.lfo_waveform, p.lfo_routing = wl, routing
    p.lfo_depth, p.lfo_frequency = depth * depth_scale, freq * freq_scale
    hz, start, end, ripple = FILTERS[(mode, safe)]
    p.filter_cutoff_hz, p.filter_cutoff_start, p.filter_cutoff_end, p.filter_passband_ripple = hz, start, end, ripple
    return p


_GRID = None


def grid():
    """(setup classes, oscillator classes): {setup: (base, LFO class, flag)} and {(w1, w2): (c1, c2)}, each from the classifier."""
    global _GRID
    if _GRID is None:
        w0 = (T.WAVE_SAWTOOTH, T.WAVE_SAWTOOTH)
        sc = {}
        for s in control_setups():
            base, cl, _, _, f32 = key(make_patch(s, *w0))
            sc[s] = (base, cl, f32)
        oc = {}
        s0 = (T.WAVE_SINE, T.LFO_AMPLITUDE, 0, "static", True)
        for w in osc_pairs():
            oc[w] = key(make_patch(s0, *w))[2:4]
        _GRID = (sc, oc)
    return _GRID


def reachable_keys():
    sc, oc = grid()
    return {(b, cl, c1, c2, f) for (b, cl, f) in set(sc.values()) for (c1, c2) in set(oc.values())}


def _candidates(k):
    """Grid points of key k, spread over the setups and waveform pairs that share it (rotated by the key, so that the representatives
    between them use every LFO waveform, routing and oscillator waveform of the class)."""
    sc, oc = grid()
    base, cl, c1, c2, f = k
    setups = [s for s, v in sc.items() if v == (base, cl, f)]
    if has_fast(k):   # a noise LFO never takes the FAST copy (kernels.h welsh_wave_tables_up): such keys get a representative without one
        setups = [s for s in setups if s[0] != T.WAVE_NOISE]
    if not setups:
        return
    pairs = [w for w, v in oc.items() if v == (c1, c2) and not (w[0] == T.WAVE_NONE and w[1] == T.WAVE_NONE)]
    h = c1 * 5 + c2 + 7 * cl
    setups = setups[h % len(setups):] + setups[:h % len(setups)]
    pairs = pairs[h % len(pairs):] + pairs[:h % len(pairs)]
    # a grid point that is unbounded (or silent) is replaced by another of the same key: the next setup, then other depths and
    # frequencies, then another waveform pair of the same classes
    for w in pairs:
        for ds, fs in ((1.0, 1.0), (0.5, 1.0), (1.0, 0.6), (0.25, 0.4)):
            for s in setups:
                yield make_patch(s, *w, depth_scale=ds, freq_scale=fs, k=(h % P.N_PATCHES))


def bounded(p, voices=None):
    """The patch's oracle output over the timeline stays finite and within BOUND, and sounds (peak >= SOUNDING) (voices: the lanes to
    play; default all of them)."""
    from oracle import oracle as O
    lanes = LANES if voices is None else voices
    params = (T.WelshParams * VOICES)(*[p] * VOICES)
    ob = O.Bank.welsh(params)
    peak = 0.0
    for b, fr in enumerate(SIZES):
        for ev in timeline_events(b, lanes):
            ob.note_events(ev)
        x = ob.render(fr)[:, :, lanes]
        if not np.isfinite(x).all():
            return False
        peak = max(peak, float(np.abs(x).max()))
    return SOUNDING <= peak <= BOUND


_REPS = None


def representative(k):
    """The representative of key k: its first grid point that is classified as k, bounded and sounding in the oracle over the timeline
    (None: the key has none)."""
    if _REPS is not None:
        return _REPS.get(k)
    for p in _candidates(k):
        if key(p) == k and bounded(p):
            return p
    return None


def representatives():
    """{key: patch}: representative(k) of every reachable key."""
    global _REPS
    if _REPS is None:
        keys = sorted(reachable_keys())
        _lib()
        with ThreadPoolExecutor(16) as pool:
            _REPS = dict(zip(keys, pool.map(representative, keys)))
    return _REPS


# ------------------------------------------------------------------ the bars of tests/test_gpu_mix_bodies.py (negative control: test_mix_body_coverage.py)
VOICE_BAR = 1e-5          # RMS per voice, of max(1, the voice's RMS level) — the path's bar (tests/test_gpu_random_inputs.py)
SMOOTH_BAR = 2e-6         # per voice and sample, of max(1, peak): the exact LFO look-ahead against the lanes' recurrences
F32_BAR = 2e-6            # RMS per voice: the fp32-filter criterion (derive.h kFilterF32MaxError)
SUM_C = 16                # fused bus against the f64 sum of the block-writing voices: c 2^-24 sum |voice| per frame


def voice_error_sums(got, want):
    """Per voice of [2][frames][voices]: (sum of squared errors, sum of squared oracle samples) — block by block these add up."""
    d = np.asarray(got, dtype=np.float64) - want
    return np.sum(d ** 2, axis=(0, 1)), np.sum(np.asarray(want, dtype=np.float64) ** 2, axis=(0, 1))


def voice_errors_of(err2, sig2, samples):
    """RMS error over the larger of full scale and the voice's RMS level, from voice_error_sums over `samples` samples per voice."""
    return np.sqrt(err2 / samples) / np.maximum(1.0, np.sqrt(sig2 / samples))


def voice_errors(got, want):
    """Per voice of [2][frames][voices]: RMS of got - want over the larger of full scale and the voice's RMS level."""
    return voice_errors_of(*voice_error_sums(got, want), 2 * np.shape(want)[1])


def voices_ok(got, want):
    return bool(np.isfinite(got).all() and voice_errors(got, want).max() <= VOICE_BAR)


def bus_ok(got, want):
    """A bus that holds ONE voice (a lane struck alone) against the oracle's: the per-voice bar, on [frames][2]."""
    got = np.asarray(got, dtype=np.float64)
    level = max(1.0, float(np.sqrt(np.mean(want ** 2))))
    return bool(np.isfinite(got).all() and np.sqrt(np.mean((got - want) ** 2)) <= VOICE_BAR * level)


def sum_rounding_ok(got, want, abs_sum, c=SUM_C):
    """Fused bus against the float64 sum of the same voices from the block-writing kernel: rounding of an fp32 sum and nothing else."""
    return bool(np.all(np.abs(np.asarray(got, dtype=np.float64) - want) <= c * 2.0 ** -24 * abs_sum))


def sum_rounding_c(got, want, abs_sum):
    """The smallest c for which sum_rounding_ok holds (what a run measured)."""
    d = np.abs(np.asarray(got, dtype=np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d > 0, d / (2.0 ** -24 * abs_sum), 0.0)
    return float(r.max())


def smooth_bus_ok(got, want, voices=VOICES):
    """Smooth-f64 kinds, FAST copy against the shared body of one representative: 2e-6 per voice and sample, summed over its voices."""
    return bool(np.abs(np.asarray(got, dtype=np.float64) - want).max() <= SMOOTH_BAR * voices)


def fp32_bus_ok(got, want, voices=VOICES):
    """fp32-filter body against the f64 one, one representative's bus: the criterion's 2e-6 RMS per voice, summed over its voices."""
    return bool(np.sqrt(np.mean((np.asarray(got, dtype=np.float64) - want) ** 2)) <= F32_BAR * voices)


# ------------------------------------------------------------------ the FAST-copy count (kernels.h welsh_wave_tables_up, diag.h fast_waves)
ENV_IDLE = 0


def state_words():
    """Word offsets of amp, fil, lfo, vflags in the voice record, the words of an envelope record and of the whole record (tests/emul)."""
    out = (C.c_uint32 * 6)()
    _lib().emul_welsh_state_words(out)
    return tuple(int(x) for x in out)


def workgroups(params):
    """The fused kernels' workgroups of a bank (csrc/welsh_plan.h welsh_plan, restated): virtual waves — runs of voices with the same
    patch, cut at 64 — ordered by (body key, WF_FILTER_F32) and cut into fours, a group's last workgroup filled up with empty waves that
    carry its first wave's patch.  Returns [(base kind, [(first voice, count, patch)] x 4)]; kinds 0 - 3 are the mix kernel's."""
    raw = [bytes(p) for p in params]
    memo, waves = {}, []
    v = 0
    while v < len(raw):
        e = v + 1
        while e < len(raw) and e - v < 64 and raw[e] == raw[v]:
            e += 1
        if raw[v] not in memo:
            c = classify(params[v])
            memo[raw[v]] = (((c[0] * 6 + c[1]) * 5 + c[2]) * 5 + c[3]) * 2 + c[4], c[0]
        waves.append((memo[raw[v]], v, e - v, params[v]))
        v = e
    waves.sort(key=lambda w: w[0][0])   # (stable: run order within a key)
    out = []
    i = 0
    while i < len(waves):
        j = i
        while j < len(waves) and waves[j][0][0] == waves[i][0][0]:
            j += 1
        group = [(w[1], w[2], w[3]) for w in waves[i:j]]
        group += [(waves[i][1], 0, waves[i][3])] * (-len(group) % 4)
        out += [(waves[i][0][1], group[g:g + 4]) for g in range(0, len(group), 4)]
        i = j
    return out


def fast_waves_expected(state, groups):
    """What the fused mix kernel counts in fast_waves at look-ahead 7 in a block that starts from `state` ([words][voices],
    groove_bank_download_state, the block's events applied), for the workgroups of `workgroups()`: (count, the first voices of the
    waves with live voices that took the FAST copy).  welsh_wave_tables_up, restated: a noise LFO never; a wave with no live voice (an empty wave, an idle one)
    always; otherwise its live voices must agree on the filter envelope's record, the LFO's phase and the first-tick flag.  Nothing is
    counted for a workgroup that is idle (welsh_idle_workgroup returns first) or that the per-kind kernels of kinds 4 and 5 run."""
    amp, fil, lfo, vflags, env, _ = state_words()
    rows = list(range(fil, fil + env)) + [lfo, lfo + 1, vflags]
    count, live_fast = 0, []
    for base, waves in groups:
        lanes = [slice(v0, v0 + n) for v0, n, _ in waves]
        if base >= 4 or not any(np.any((state[amp, ln] != ENV_IDLE) | (state[fil, ln] != ENV_IDLE)) for ln in lanes):
            continue
        for ln, (v0, _, p) in zip(lanes, waves):
            if (p.lfo_waveform & 15) == T.WAVE_NOISE:
                continue
            live = state[amp, ln] != ENV_IDLE
            words = state[rows, ln][:, live]
            if words.shape[1] == 0 or np.all(words == words[:, :1]):
                count += 1
                if words.shape[1] > 0:
                    live_fast.append(v0)
    return count, live_fast
