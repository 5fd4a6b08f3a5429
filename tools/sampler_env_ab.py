#!/usr/bin/env python3
"""What sample ENVELOPES cost: config #4's shape (sampler-16384: 16,384 voices over the shared 60-buffer bank, staggered starts, 344
blocks of 256 frames), every voice a held sampler voice on a looped sample (the second half of each buffer: once its cursor has reached
the loop every voice sounds in every block), without envelopes and with the envelope (0.01, 0.1, 0.7, 0.3) on every sample
(groove_bank_set_sample_envelopes) — in both kernel forms, the time-parallel one the bank takes by itself and the serial one
(time_parallel_max_voices = 0), for a mono bank read nearest and a stereo bank read cubic, through the fused walk bench.py uses for
that row: groove_bank_render_mix_deferred, one launch per block.

One process; per (form, bank) the two arms alternate after a warm-up of each; seven regions (one pass over the 344-block timeline each)
per arm; median and spread (max - min) of the ms per block per arm, and the enveloped median over the other.  Both arms run the LOOP
text — the enveloped kernels are built on it — so the ratio is the envelope's own cost: the record's load and store, the ticks, one
multiply per frame and channel.  A record, not a bar.  Host wall clock: no kernel durations.

    python tools/sampler_env_ab.py [--regions 7] [--out profiles/sampler_env_ab.json]
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
ENVELOPE = (0.01, 0.1, 0.7, 0.3)
BANKS = {"nearest-mono": (T.SAMPLE_NEAREST, False), "cubic-stereo": (T.SAMPLE_CUBIC, True)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sampler_env_ab.json"))
    args = ap.parse_args()
    wl = PJ.WORKLOADS["sampler-16384"]
    voices, blocks = wl["voices"], wl["blocks"]
    spec = PJ.plan("sampler-16384", np.arange(voices))[0]
    descs = spec["descs"]
    loops = [(int(d.length) // 2, int(d.length)) for d in descs]
    held = (T.SamplerParams * voices)()
    C.memmove(held, spec["params"], C.sizeof(held))
    for v in range(voices):
        held[v].one_shot = 0

    ctx = E.Context(0)
    bus = ctx.bus(blocks * FRAMES)
    tp_default = ctx.time_parallel_max_voices
    out = {"tool": "tools/sampler_env_ab.py", "workload": "sampler-16384", "voices": voices, "blocks_per_region": blocks, "frames": FRAMES,
           "envelope": ENVELOPE, "loops": "the second half of every buffer, both arms",
           "walk": "groove_bank_render_mix_deferred, one bank on the ctx stream (bench.py's walk for this row)",
           "timer": "host wall clock around a region, synchronised at both ends; no kernel trace", "regions": args.regions, "forms": {}}
    for form, tp in (("time-parallel", tp_default), ("serial", 0)):
        ctx.time_parallel_max_voices = tp
        for name, (mode, stereo) in BANKS.items():
            pcm = spec["pcm"]
            if stereo:
                pcm = np.ascontiguousarray(np.stack([pcm, pcm], axis=1))
            bank = E.Sampler(ctx, pcm, descs, held)
            bank.sample_interpolation = mode
            bank.sample_loops = loops

            def region(arm, bank=bank):
                bank.sample_envelopes = [ENVELOPE] * len(descs) if arm == "enveloped" else None
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

            arms = ("no_envelopes", "enveloped")
            rec = {"kernel_form": {}, "bus_abs_sum": {}}
            for arm in arms:                                  # a warm-up of each
                region(arm)
                rec["kernel_form"][arm] = bank.kernel_form(FRAMES, True)
                rec["bus_abs_sum"][arm] = float(np.abs(bus.download()).sum())
            ms = {arm: [] for arm in arms}
            for _ in range(args.regions):
                for arm in arms:
                    ms[arm].append(region(arm))
            for arm, v in ms.items():
                rec[arm] = {"ms_per_block": [round(x, 6) for x in v], "median": round(statistics.median(v), 6), "spread": round(max(v) - min(v), 6)}
            rec["enveloped_over_no_envelopes_median"] = round(rec["enveloped"]["median"] / rec["no_envelopes"]["median"], 4)
            assert ("enveloped" in rec["kernel_form"]["enveloped"]) and ("enveloped" not in rec["kernel_form"]["no_envelopes"]), rec["kernel_form"]
            out["forms"][f"{form}/{name}"] = rec
            bank.destroy()
    ctx.time_parallel_max_voices = tp_default
    info = ctx.debug_info()
    out["source_hash"] = info.get("source_hash")
    zeros, misses = info["zero_segments"], info["fast_table_misses"]
    bus.destroy()
    ctx.close()
    assert zeros == 0 and misses == 0, info
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
