#!/usr/bin/env python3
"""What a STEREO sample bank costs: config #4's shape (sampler-16384: 16,384 one-shot voices over the shared 60-buffer bank, staggered
starts, 344 blocks of 256 frames) as a mono bank (groove_sampler_create) and as a stereo bank with independent channels
(groove_sampler_create_stereo), through the fused walk bench.py uses for that row — a lone bank taking turns with itself on the ctx
stream, groove_bank_render_mix_deferred, one launch per block.

Both arms in ONE process, alternating after a warm-up of each; seven regions (one pass over the 344-block timeline each) per arm;
median and spread (max - min) of the ms per block per arm.  A record, not a bar.

    python tools/sampler_stereo_ab.py [--regions 7] [--out profiles/sampler_stereo_ab.json]
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

from groove_amd import entities as E, projects as PJ  # noqa: E402

FRAMES = 256


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sampler_stereo_ab.json"))
    args = ap.parse_args()
    wl = PJ.WORKLOADS["sampler-16384"]
    voices, blocks = wl["voices"], wl["blocks"]
    spec = PJ.plan("sampler-16384", np.arange(voices))[0]
    mono_pcm = spec["pcm"]
    rng = np.random.default_rng(7)
    # independent channels: the bank's own content on the left, the same buffers time-reversed and rescaled on the right
    right = np.concatenate([mono_pcm[d.offset:d.offset + d.length][::-1] for d in spec["descs"]]) * np.float32(0.8)
    right = right + (rng.standard_normal(len(right)) * 0.01).astype(np.float32)
    stereo_pcm = np.ascontiguousarray(np.stack([mono_pcm, right.astype(np.float32)], axis=1))

    ctx = E.Context(0)
    arms = {"mono": E.Sampler(ctx, mono_pcm, spec["descs"], spec["params"]), "stereo": E.Sampler(ctx, stereo_pcm, spec["descs"], spec["params"])}
    assert arms["mono"].sample_channels == 1 and arms["stereo"].sample_channels == 2
    bus = ctx.bus(blocks * FRAMES)

    def region(bank):
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

    crc = {}
    for name, bank in arms.items():                           # a warm-up of each; the buses differ between the arms on the right channel only
        region(bank)
        got = bus.download()
        crc[name] = [float(np.abs(got[:, 0]).sum()), float(np.abs(got[:, 1]).sum())]
    assert crc["mono"][0] == crc["stereo"][0] and crc["mono"][1] != crc["stereo"][1], crc
    ms = {name: [] for name in arms}
    for _ in range(args.regions):
        for name, bank in arms.items():
            ms[name].append(region(bank))
    info = ctx.debug_info()
    out = {
        "tool": "tools/sampler_stereo_ab.py", "workload": "sampler-16384", "voices": voices, "blocks_per_region": blocks, "frames": FRAMES,
        "walk": "groove_bank_render_mix_deferred, one bank on the ctx stream (bench.py's walk for this row)",
        "kernel_form": {name: bank.kernel_form(FRAMES, True) for name, bank in arms.items()},
        "timer": "host wall clock around a region, synchronised at both ends", "regions": args.regions,
        "source_hash": info.get("source_hash"),
        "arms": {name: {"ms_per_block": [round(x, 6) for x in v], "median": round(statistics.median(v), 6), "spread": round(max(v) - min(v), 6)}
                 for name, v in ms.items()},
    }
    out["stereo_over_mono_median"] = round(out["arms"]["stereo"]["median"] / out["arms"]["mono"]["median"], 4)
    zeros, misses = info["zero_segments"], info["fast_table_misses"]
    for x in list(arms.values()) + [bus]:
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
