"""What a partly wet reverb costs config #3's chain, with groove_set_fx_wet_reverb_run off (the reverb walks the frames serially, the
fused run is cut in front of it, the mix reads the block back) and on (the reverb keeps the fused run's forms).

The workload is bench.py's chain-4096 (patches.chain_fx_params, 4,096 lanes, the paced walk of groove_amd/projects.py) with the
reverb's wet-dry-mix at 0.5 on every lane, and again on lane 0 only.  Both arms run in ONE process on one project, alternating, a
region being the workload's own 172 blocks after 4 warm-up blocks from a reset state (bench.time_project); both arms are warmed up
first.  Reported per wet pattern and arm: ms per block of every region and their median, the spread (max - min) of the arm's own
regions, the reverb's kernel form, and the CRC-32s of the bus.  (The two arms give every BLOCK the same bits —
tests/test_gpu_fx_wet_reverb.py — but not necessarily the bus: with the knob off the mix sums the block's lanes itself, with it on it
reduces the row sums the last kernel left, in another order.)

    python3 tools/wet_reverb_ab.py [--regions 7] [--out profiles/wet_reverb_ab.json]
"""
import argparse
import json
import os
import sys
import zlib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--blocks", type=int, default=172)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "wet_reverb_ab.json"))
    args = ap.parse_args()
    import numpy as np
    import bench as B
    from groove_amd import abi_types as T, entities as E, projects as PJ
    ctx = E.Context(0)
    ctx.sync_timeout_ms = 30000
    assert not ctx.fx_wet_reverb_run
    voices = PJ.WORKLOADS["chain-4096"]["voices"]
    proj = PJ.Project(ctx, "chain-4096", np.arange(voices, dtype=np.int64))
    inst, _, fx, _ = proj.banks[0]
    reverb = fx[-1]
    assert reverb.kind == T.FX_REVERB
    bus = ctx.bus((args.warmup + args.blocks) * PJ.FRAMES)
    result = {"workload": "chain-4096", "lanes": voices, "blocks_per_region": args.blocks, "warmup_blocks": args.warmup, "regions_per_arm": args.regions,
              "walk": "paced" if proj.paced else "not paced", "allpass_stream": bool(proj.allpass_stream), "patterns": {}}

    def region(on):
        ctx.fx_wet_reverb_run = on
        walls, kerns, _ = B.time_project(ctx, proj, bus, args.blocks, args.warmup, 1, True)
        form = reverb.kernel_form(proj.ahead[inst][0], PJ.FRAMES)
        crc = zlib.crc32(bus.download().tobytes())
        return walls[0] / args.blocks * 1e3, kerns[0], form, crc

    try:
        for name, lane in (("wet 0.5 on every lane", T.ALL_VOICES), ("wet 0.5 on lane 0 only", 0), ("all wet (the knob changes nothing)", None)):
            reverb.control_set_param_by_index(T.CTL_FX_WET, 1.0)
            if lane is not None:
                reverb.control_set_param_by_index(T.CTL_FX_WET, 0.5, lane=lane)
            arms = {False: {"ms_per_block": [], "event_ms_per_block": []}, True: {"ms_per_block": [], "event_ms_per_block": []}}
            for on in (False, True):                      # warm both arms up
                region(on)
            for _ in range(args.regions):
                for on in (False, True):                  # alternating
                    ms, ev, form, crc = region(on)
                    a = arms[on]
                    a["ms_per_block"].append(round(ms, 5)); a["event_ms_per_block"].append(round(ev, 5))
                    assert a.setdefault("reverb_form", form) == form
                    a.setdefault("bus_crc32", [])
                    if f"{crc:08x}" not in a["bus_crc32"]:
                        a["bus_crc32"].append(f"{crc:08x}")
            for a in arms.values():
                ms = sorted(a["ms_per_block"])
                a["median_ms_per_block"] = ms[len(ms) // 2]
                a["spread_ms"] = round(ms[-1] - ms[0], 5)
            off, on_ = arms[False], arms[True]
            entry = {"knob_off": off, "knob_on": on_, "same_bus_bits": off["bus_crc32"] == on_["bus_crc32"],
                     "on_minus_off_ms": round(on_["median_ms_per_block"] - off["median_ms_per_block"], 5),
                     "accepted": on_["median_ms_per_block"] <= off["median_ms_per_block"] + off["spread_ms"]}
            result["patterns"][name] = entry
            print(f"{name}: off {off['median_ms_per_block']:.4f} ms per block (spread {off['spread_ms']:.4f}; {off['reverb_form']}), "
                  f"on {on_['median_ms_per_block']:.4f} (spread {on_['spread_ms']:.4f}; {on_['reverb_form']}); same bus bits: {entry['same_bus_bits']}", flush=True)
    finally:
        ctx.fx_wet_reverb_run = False
    result["debug_info"] = {k: v for k, v in ctx.debug_info().items() if k in ("source_hash", "zero_segments", "fast_table_misses")}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"written": args.out}))
    proj.destroy(); bus.destroy(); ctx.close()


if __name__ == "__main__":
    sys.exit(main())
