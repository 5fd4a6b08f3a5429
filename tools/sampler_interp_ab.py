#!/usr/bin/env python3
"""What INTERPOLATED sample playback costs: config #4's shape (sampler-16384: 16,384 one-shot voices over the shared 60-buffer bank,
staggered starts, 344 blocks of 256 frames) with the bank's sample interpolation NEAREST, LINEAR and CUBIC
(groove_bank_set_sample_interpolation), through the fused walk bench.py uses for that row — a lone bank taking turns with itself on
the ctx stream, groove_bank_render_mix_deferred, one launch per block.

The three modes on ONE bank in ONE process, alternating after a warm-up of each; seven regions (one pass over the 344-block timeline
each) per arm; median and spread (max - min) of the ms per block per arm.  A record, not a bar.  Host wall clock: no kernel durations.

    python tools/sampler_interp_ab.py [--regions 7] [--stereo] [--out profiles/sampler_interp_ab.json]
"""
import argparse
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
    ap.add_argument("--stereo", action="store_true", help="a stereo bank (the mono bank's content on both channels)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sampler_interp_ab.json"))
    args = ap.parse_args()
    wl = PJ.WORKLOADS["sampler-16384"]
    voices, blocks = wl["voices"], wl["blocks"]
    spec = PJ.plan("sampler-16384", np.arange(voices))[0]
    pcm = spec["pcm"]
    if args.stereo:
        pcm = np.ascontiguousarray(np.stack([pcm, pcm], axis=1))
    steps = sorted({float(d.root_hz) for d in spec["descs"]})

    ctx = E.Context(0)
    bank = E.Sampler(ctx, pcm, spec["descs"], spec["params"])
    bus = ctx.bus(blocks * FRAMES)

    def region(mode):
        bank.sample_interpolation = MODES[mode]
        bank.reset()
        ctx.synchronize()
        t0 = time.perf_counter()
        for b in range(blocks):
            ev = spec["events"].get(b)
            if ev is not None:
                bank.handle_midi_events(ev)
            bank.render_mix_deferred(bus, FRAMES, at_frame=b * FRAMES)
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3 / blocks

    forms, level = {}, {}
    for mode in MODES:                                        # a warm-up of each
        region(mode)
        forms[mode] = bank.kernel_form(FRAMES, True)
        level[mode] = float(np.abs(bus.download()).sum())
    ms = {mode: [] for mode in MODES}
    for _ in range(args.regions):
        for mode in MODES:
            ms[mode].append(region(mode))
    info = ctx.debug_info()
    out = {
        "tool": "tools/sampler_interp_ab.py", "workload": "sampler-16384", "voices": voices, "blocks_per_region": blocks, "frames": FRAMES,
        "bank_channels": bank.sample_channels, "sample_root_hz": steps,
        "walk": "groove_bank_render_mix_deferred, one bank on the ctx stream (bench.py's walk for this row)",
        "kernel_form": forms, "bus_abs_sum": level,
        "timer": "host wall clock around a region, synchronised at both ends; no kernel trace", "regions": args.regions,
        "source_hash": info.get("source_hash"),
        "arms": {mode: {"ms_per_block": [round(x, 6) for x in v], "median": round(statistics.median(v), 6), "spread": round(max(v) - min(v), 6)}
                 for mode, v in ms.items()},
    }
    for mode in ("linear", "cubic"):
        out[f"{mode}_over_nearest_median"] = round(out["arms"][mode]["median"] / out["arms"]["nearest"]["median"], 4)
    zeros, misses = info["zero_segments"], info["fast_table_misses"]
    for x in (bank, bus):
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
