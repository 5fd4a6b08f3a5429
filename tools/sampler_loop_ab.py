#!/usr/bin/env python3
"""What LOOPED sample playback costs: config #4's shape (sampler-16384: 16,384 voices over the shared 60-buffer bank, staggered starts,
344 blocks of 256 frames) without loops, and with a forward loop on every sample (groove_bank_set_sample_loops: the second half of
each buffer) and every voice a sampler voice that is held — so that, once its cursor has reached the loop, every voice sounds in every
block — in each interpolation mode, through the fused walk bench.py uses for that row: a lone bank taking turns with itself on the ctx
stream, groove_bank_render_mix_deferred, one launch per block.

Both banks — the workload's own one-shot bank without loops, and the held, looped one — live in ONE process; per mode the two arms
alternate after a warm-up of each; seven regions (one pass over the 344-block timeline each) per arm; median and spread (max - min) of
the ms per block per arm, and the looped median over the loop-free one.  The looped arm does more than fold: its voices never end, so
it also gathers for voices the loop-free arm has dropped.  "held_no_loops" separates the two: the held bank with its loops cleared.
A record, not a bar.  Host wall clock: no kernel durations.

    python tools/sampler_loop_ab.py [--regions 7] [--stereo] [--out profiles/sampler_loop_ab.json]

The two committed records:

    python tools/sampler_loop_ab.py                   -> profiles/sampler_loop_ab.json
    python tools/sampler_loop_ab.py --stereo          -> profiles/sampler_loop_ab_stereo.json  (--stereo's default --out)
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from groove_amd import abi_types as T, entities as E, projects as PJ  # noqa: E402

FRAMES = 256
MODES = {"nearest": T.SAMPLE_NEAREST, "linear": T.SAMPLE_LINEAR, "cubic": T.SAMPLE_CUBIC}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--stereo", action="store_true", help="stereo banks (the mono bank's content on both channels)")
    ap.add_argument("--out", default=None, help="default: profiles/sampler_loop_ab.json, with --stereo profiles/sampler_loop_ab_stereo.json")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(REPO, "profiles", "sampler_loop_ab_stereo.json" if args.stereo else "sampler_loop_ab.json")
    wl = PJ.WORKLOADS["sampler-16384"]
    voices, blocks = wl["voices"], wl["blocks"]
    spec = PJ.plan("sampler-16384", np.arange(voices))[0]
    pcm = spec["pcm"]
    if args.stereo:
        pcm = np.ascontiguousarray(np.stack([pcm, pcm], axis=1))
    descs = spec["descs"]
    loops = [(int(d.length) // 2, int(d.length)) for d in descs]
    held = (T.SamplerParams * voices)()
    C.memmove(held, spec["params"], C.sizeof(held))
    for v in range(voices):
        held[v].one_shot = 0

    ctx = E.Context(0)
    banks = {"no_loops": E.Sampler(ctx, pcm, descs, spec["params"]), "held": E.Sampler(ctx, pcm, descs, held)}
    bus = ctx.bus(blocks * FRAMES)

    def region(arm, mode):
        bank = banks["no_loops" if arm == "no_loops" else "held"]
        bank.sample_interpolation = MODES[mode]
        if arm != "no_loops":
            bank.sample_loops = loops if arm == "looped" else None
        bank.reset()
        ctx.synchronize()
        t0 = time.perf_counter()
        for b in range(blocks):
            ev = spec["events"].get(b)
            if ev is not None:
                bank.handle_midi_events(ev)
            bank.render_mix_deferred(bus, FRAMES, at_frame=b * FRAMES)
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3 / blocks, bank

    arms = ("no_loops", "held_no_loops", "looped")
    forms, level, ms = {}, {}, {}
    for mode in MODES:
        for arm in arms:                                      # a warm-up of each
            _, bank = region(arm, mode)
            forms[f"{mode}/{arm}"] = bank.kernel_form(FRAMES, True)
            level[f"{mode}/{arm}"] = float(np.abs(bus.download()).sum())
        ms[mode] = {arm: [] for arm in arms}
        for _ in range(args.regions):
            for arm in arms:
                ms[mode][arm].append(region(arm, mode)[0])
    info = ctx.debug_info()
    out = {
        "tool": "tools/sampler_loop_ab.py", "workload": "sampler-16384", "voices": voices, "blocks_per_region": blocks, "frames": FRAMES,
        "bank_channels": banks["held"].sample_channels, "loops": "the second half of every buffer",
        "walk": "groove_bank_render_mix_deferred, one bank on the ctx stream (bench.py's walk for this row)",
        "kernel_form": forms, "bus_abs_sum": level,
        "timer": "host wall clock around a region, synchronised at both ends; no kernel trace", "regions": args.regions,
        "source_hash": info.get("source_hash"),
        "modes": {mode: {arm: {"ms_per_block": [round(x, 6) for x in v], "median": round(statistics.median(v), 6), "spread": round(max(v) - min(v), 6)}
                         for arm, v in ms[mode].items()} for mode in MODES},
    }
    for mode in MODES:
        m = out["modes"][mode]
        m["looped_over_no_loops_median"] = round(m["looped"]["median"] / m["no_loops"]["median"], 4)
        m["looped_over_held_no_loops_median"] = round(m["looped"]["median"] / m["held_no_loops"]["median"], 4)
    zeros, misses = info["zero_segments"], info["fast_table_misses"]
    for x in (*banks.values(), bus):
        x.destroy()
    ctx.close()
    assert zeros == 0 and misses == 0, info
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
