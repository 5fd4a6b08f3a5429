#!/usr/bin/env python3
"""What one control-link apply costs, per instantiation of csrc/ctl_link.h's ctl_apply_kernel<Source, Target>, in two BUILDS of the
library (GROOVE_LIB_PATH: groove_amd/lib.py): an apply is a few wavefronts and all launch latency, so its cost is the host's enqueue
time.  Per (source, target) — an LFO or a trip onto a Gain's ceiling (plain words), a 12 dB low-pass's cutoff (filter), a Welsh bank's
dca-gain and an FM bank's gain (voices), 65 lanes or voices each — 1,000 applies are enqueued and the context synchronised ONCE;
the microseconds per apply are the region's wall clock over 1,000.  Five runs per build, each a child process of its own, the two
builds taking turns.  A record, not a bar: `verdict` says whether B's median lies at or under A's slowest run.

    python tools/ctl_apply_ab.py --a PATH/TO/libgroove_hip.so [--b groove_amd/libgroove_hip.so] [--runs 5] [--out profiles/ctl_apply_ab.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

N, APPLIES = 65, 1000
STEPS = [(1, 0.2, 0.8, 4.0)]          # one slope step of four beats from beat 0: every apply below lies inside it


def child():
    """One run in this process's build: {instantiation: microseconds per apply}."""
    from groove_amd import abi_types as T, entities as E, patches as P
    ctx = E.Context(0)
    gain = E.Effect(ctx, T.FX_GAIN, (T.FxParams * N)(*[T.fx_params(ceiling=0.75) for _ in range(N)]))
    lp12 = E.Effect(ctx, T.FX_BIQUAD_LP12, (T.FxParams * N)(*[T.fx_params(cutoff_hz=1000.0, q=0.9) for _ in range(N)]))
    welsh, fm = E.WelshSynth(ctx, P.welsh_voices(N)), E.FmSynth(ctx, P.fm_voices(N))
    targets = {"plain": (gain, T.CTL_FX_CEILING, {}), "filter": (lp12, T.CTL_FX_CUTOFF, {"derived": True}),
               "welsh": (welsh, T.CTL_WELSH_DCA_GAIN, {}), "voices": (fm, T.CTL_FM_DCA_GAIN, {})}
    out, links = {}, []
    for name, (target, index, kw) in targets.items():
        lfo = E.ControlLink(ctx, T.ctl_sources(1, source=T.CTL_SRC_LFO, waveform=T.WAVE_TRIANGLE, frequency_hz=3.0), target, index, **kw)
        trip = E.ControlTripLink(ctx, [STEPS], 0.0, target, index)
        links += [lfo, trip]
        for source, link, step in (("live", lfo, 256), ("trip", trip, 200)):
            for k in range(50):                                 # warm-up: the kernel's code object is loaded, the queues are up
                link.work(k * step)
            ctx.synchronize()
            t0 = time.perf_counter()
            for k in range(APPLIES):
                link.work(k * step)
            ctx.synchronize()
            out[f"{source}/{name}"] = (time.perf_counter() - t0) * 1e6 / APPLIES
    info = ctx.debug_info()
    for x in links + [gain, lp12, welsh, fm]:
        x.destroy()
    ctx.close()
    print(json.dumps({"us_per_apply": out, "source_hash": info.get("source_hash")}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--a", help="build A (the baseline): path of its libgroove_hip.so")
    ap.add_argument("--b", default=os.path.join(REPO, "groove_amd", "libgroove_hip.so"), help="build B (default: this tree's)")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ctl_apply_ab.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child()
    if not args.a:
        ap.error("--a is required")
    builds = {"a": os.path.abspath(args.a), "b": os.path.abspath(args.b)}
    runs, hashes = {"a": [], "b": []}, {}
    for _ in range(args.runs):
        for which, path in builds.items():                       # the builds take turns; one process with the GPU open at a time
            env = dict(os.environ, GROOVE_LIB_PATH=path)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True, timeout=300)
            if p.returncode != 0:
                sys.exit(f"build {which} ({path}) failed with status {p.returncode}:\n{p.stdout}\n{p.stderr}")
            rec = json.loads(p.stdout.strip().splitlines()[-1])
            runs[which].append(rec["us_per_apply"])
            hashes[which] = rec["source_hash"]
    out = {"tool": "tools/ctl_apply_ab.py", "lanes": N, "applies_per_region": APPLIES, "runs": args.runs,
           "timer": "host wall clock around 1,000 enqueued applies and one synchronise; no kernel trace",
           "source_hash": hashes, "instantiations": {}}
    for key in runs["a"][0]:
        a, b = [r[key] for r in runs["a"]], [r[key] for r in runs["b"]]
        out["instantiations"][key] = {"a_us": [round(x, 3) for x in a], "b_us": [round(x, 3) for x in b], "a_median": round(statistics.median(a), 3),
                                      "a_slowest": round(max(a), 3), "b_median": round(statistics.median(b), 3),
                                      "b_median_at_or_under_a_slowest": statistics.median(b) <= max(a)}
    out["verdict"] = all(v["b_median_at_or_under_a_slowest"] for v in out["instantiations"].values())
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
