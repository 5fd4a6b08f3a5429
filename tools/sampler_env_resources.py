#!/usr/bin/env python3
"""The compiler's resource table of the two sampler kernels for gfx950 (no GPU needed): every instantiation of sampler_tp_kernel
(csrc/welsh_tp.hip) and sampler_render_kernel (csrc/groove_hip.hip) with its VGPRs, SGPRs, scratch, spills and occupancy, as
-Rpass-analysis=kernel-resource-usage prints them.  Fails if an ENV instantiation (the last template argument) uses scratch or
spills a vector register (SGPR spills are shown: they go to lanes of a vector register, not to memory), or if a time-parallel one
needs more than the 128 VGPRs a lane of a 1,024-thread workgroup has.

  tools/sampler_env_resources.py                   compile both units (device side only; several minutes) and print the table
  tools/sampler_env_resources.py --parent DIR      the same for a checkout of the parent commit in DIR too: every instantiation that
                                                   exists there must have the parent's figures
  tools/sampler_env_resources.py --logs A B [--parent-logs C D]   parse remark logs made earlier instead of compiling
"""
import argparse
import os
import re
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNITS = ("welsh_tp", "groove_hip")
FIELDS = (("vgpr", r" VGPRs: (\d+)"), ("sgpr", r"TotalSGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)"),
          ("sgpr_spill", r"SGPRs Spill: (\d+)"), ("vgpr_spill", r"VGPRs Spill: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)"))


def remarks(root, unit):
    cmd = ["hipcc", "--offload-arch=gfx950", "--cuda-device-only", "-O3", "-std=c++17", "-fPIC", "-fno-slp-vectorize", "-Rpass-analysis=kernel-resource-usage",
           "-c", "-o", os.devnull, os.path.join("csrc", unit + ".hip")]
    return subprocess.run(cmd, cwd=os.path.join(root, "groove_amd"), capture_output=True, text=True, check=True).stderr


def parse(text):
    table, name = {}, None
    for line in text.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            table[name] = {}
        for key, pat in FIELDS:
            m = re.search(pat, line)
            if m and name:
                table[name][key] = int(m.group(1))
    names = list(table)
    plain = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.split("\n")
    out = {}
    for mangled, text in zip(names, plain):
        m = re.match(r"void groove::(sampler_tp_kernel|sampler_render_kernel)<(.*?)>\(", text)
        if m:
            out[(m.group(1), tuple(m.group(2).split(", ")))] = table[mangled]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent")
    ap.add_argument("--logs", nargs="+")
    ap.add_argument("--parent-logs", nargs="+")
    a = ap.parse_args()
    new, old = {}, {}
    for text in ([open(p, errors="replace").read() for p in a.logs] if a.logs else [remarks(REPO, u) for u in UNITS]):
        new.update(parse(text))
    if a.parent_logs or a.parent:
        for text in ([open(p, errors="replace").read() for p in a.parent_logs] if a.parent_logs else [remarks(a.parent, u) for u in UNITS]):
            old.update(parse(text))
    bad = []
    print("%-24s %-6s %-6s %-7s %-5s %-4s | %5s %5s %7s %6s %4s  %s" % ("kernel", "FUSED", "STEREO", "MODE", "LOOP", "ENV", "VGPRs", "SGPRs", "scratch", "s+v sp", "occ", "parent"))
    for (kernel, args), r in sorted(new.items(), key=lambda kv: (kv[0][0], kv[0][1][-1], kv[0][1][2], kv[0][1][1], kv[0][1][0])):
        env = len(args) == 5 and args[4] == "true"
        mode = {"0": "nearest", "1": "linear", "2": "cubic"}.get(args[2], args[2])
        note = ""
        if not env and old:
            o = old.get((kernel, args[:4])) or old.get((kernel, args))
            if o is None:
                note = "not in the parent"
            elif all(o.get(k) == r.get(k) for k, _ in FIELDS):
                note = "same"
            else:
                note = "PARENT %s VGPRs %s SGPRs %s scratch" % (o.get("vgpr"), o.get("sgpr"), o.get("scratch"))
                bad.append("%s<%s> differs from the parent" % (kernel, ", ".join(args)))
        spills = "%d+%d" % (r.get("sgpr_spill", 0), r.get("vgpr_spill", 0)) # scalar + vector
        if env and (r.get("scratch") or r.get("vgpr_spill")):
            bad.append("%s<%s> uses scratch or spills a vector register" % (kernel, ", ".join(args)))
        if env and kernel == "sampler_tp_kernel" and r.get("vgpr", 0) > 128:
            bad.append("%s<%s> needs more than 128 VGPRs" % (kernel, ", ".join(args)))
        print("%-24s %-6s %-6s %-7s %-5s %-4s | %5s %5s %7s %6s %4s  %s" % (kernel, args[0], args[1], mode, args[3], args[4] if len(args) > 4 else "-",
                                                                             r.get("vgpr"), r.get("sgpr"), r.get("scratch"), spills, r.get("occupancy"), note))
    n_env = sum(1 for (_, args) in new if len(args) == 5 and args[4] == "true")
    if n_env != 24:
        bad.append("expected 24 ENV instantiations (12 per kernel), found %d" % n_env)
    for b in bad:
        print("FAIL:", b)
    print("ok: %d instantiations, %d of them ENV, none of those with scratch" % (len(new), n_env) if not bad else "FAILED")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
