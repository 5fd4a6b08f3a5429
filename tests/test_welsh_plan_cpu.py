"""CPU tier: the plan of a Welsh bank (groove_amd/csrc/welsh_plan.h) — lane order, virtual waves, workgroups, the kind-sorted lists
and the mix kernel's striped copy — made without a GPU by tests/welsh_plan_check.cpp, a program of its own built here with g++,
once plain and once under AddressSanitizer + UndefinedBehaviorSanitizer.

The program checks every plan's invariants itself (exit status 1 on a violation; the list is in its check_plan) and prints one
SHA-256 per bank over the plan's bytes (the order is documented at its top).  The banks below are the smallest shapes at which
each rule of the plan can go wrong; what each must look like is asserted from the counts the program prints, and every digest
must equal the one in tests/golden/welsh_plan_parent.json: the bytes the last commit before welsh_plan.h existed uploaded for the
same bank."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from groove_amd import abi_types as T, patches as P

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "welsh_plan_check.cpp")
GOLDEN = os.path.join(REPO, "tests", "golden", "welsh_plan_parent.json")
SR = T.DEFAULT_SAMPLE_RATE
SAN_ENV = {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0:exitcode=97", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1:exitcode=98"}
SIZE = C.sizeof(T.WelshParams)


def _raw(patch):
    return np.frombuffer(bytes(patch), dtype=np.uint8)


def _runs(patches, lengths, n=None):
    """Voices in runs: run j holds lengths[j] voices of patches[j mod len(patches)]; cut at n voices when given."""
    table = np.stack([_raw(p) for p in patches])
    which = np.repeat(np.arange(len(lengths)) % len(patches), lengths)
    return np.ascontiguousarray(table[which if n is None else which[:n]])


def _body_bank(extra_long_runs):
    """One run per reachable body key (tests/mix_bodies.py), 40 voices (one wave, three pad waves: no kind's wave count is a multiple of
    four), every seventh 70 (two waves); the first `extra_long_runs` keys of the class-specialised kinds get 264 voices — five waves, a
    second workgroup — so that the 900 workgroups of those kinds become 900 + extra_long_runs."""
    from tests import mix_bodies as M
    reps = M.representatives()
    keys = sorted(reps)
    assert keys[0][0] < 4 and keys[extra_long_runs - 1][0] < 4
    lengths = [264 if i < extra_long_runs else 70 if i % 7 == 3 else 40 for i in range(len(keys))]
    return _runs([reps[k] for k in keys], lengths)


def corpus():
    """{bank name: (flagged, records [n][record bytes], records after a control change or None)}"""
    one = [P.welsh_patch(2)]
    two = [P.welsh_patch(2), P.welsh_patch(11)]
    table = [P.welsh_patch(j) for j in range(P.N_PATCHES)]
    banks = {}
    for n in (1, 64, 65, 257):
        banks[f"one_patch_{n}"] = (True, _runs(one, [n]), None)
    for n in (2048, 2049):
        banks[f"alternating_{n}"] = (True, _runs(two, [1] * n), None)
    own = np.frombuffer(bytes(bytearray((T.WelshParams * 2049)(*[P.welsh_patch(2)] * 2049))), dtype=np.uint8).reshape(2049, SIZE).copy()
    gain = T.WelshParams.dca_gain.offset
    own[:, gain:gain + 4] = (0.25 + np.arange(2049, dtype=np.float32) / 4096.0).astype("<f4").view(np.uint8).reshape(2049, 4)
    banks["own_patch_each_2049"] = (True, own, None)
    for run in (48, 40):
        banks[f"runs_of_{run}_131072"] = (True, _runs(table, [run] * (131072 // run + 1), 131072), None)
    voices = np.frombuffer(bytes(bytearray(P.welsh_voices(8192))), dtype=np.uint8).reshape(8192, SIZE)
    banks["voices_8192"] = (True, voices, None)
    banks["bodies_3k_plus_1"] = (True, _body_bank(1), None)
    banks["bodies_3k_plus_2"] = (True, _body_bank(2), None)
    changed = voices.copy()
    cutoff = T.WelshParams.filter_cutoff_hz.offset
    changed[1000, cutoff:cutoff + 4] = np.frombuffer(np.float32(1234.5).tobytes(), dtype=np.uint8)
    banks["voices_8192_cutoff_of_voice_1000_changed"] = (True, voices, changed)
    banks["voices_8192_no_flags"] = (False, voices, None)
    return banks


def write_corpus(directory):
    """The corpus as files; returns the program's bank arguments."""
    args = []
    for name, (flagged, first, second) in corpus().items():
        spec = [name, "f" if flagged else "-"]
        for k, records in enumerate(r for r in (first, second) if r is not None):
            path = os.path.join(str(directory), f"{name}.{k}.bin")
            records.tofile(path)
            spec.append(path)
        args.append(":".join(spec))
    return args


def build(directory, sanitized):
    exe = os.path.join(str(directory), "welsh_plan_check" + ("_san" if sanitized else ""))
    flags = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-g"] if sanitized else []
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Werror"] + flags + ["-I", REPO, SRC, "-o", exe], check=True)   # (the unknown pragmas: dsp_core.h's `#pragma unroll`)
    return exe


def run(exe, args):
    r = subprocess.run([exe, repr(SR)] + args, capture_output=True, text=True, timeout=900, env=dict(os.environ, **SAN_ENV))
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    out = {}
    for line in r.stdout.splitlines():
        name, digest, *fields = line.split()
        out[name] = dict([f.split("=") for f in fields] + [("digest", digest)])
    return out


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    d = tmp_path_factory.mktemp("welsh_plan")
    args = write_corpus(d)
    plain, sanitized = run(build(d, False), args), run(build(d, True), args)
    assert len(plain) == len(args)
    return plain, sanitized


def _ints(fields, *names):
    return [int(fields[k]) for k in names]


def test_the_header_is_host_only():
    text = open(os.path.join(REPO, "groove_amd", "csrc", "welsh_plan.h")).read()
    includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
    assert includes == ['"derive.h"', "<algorithm>", "<cstring>", "<utility>", "<vector>"]
    for word in ("groove_ctx", "groove_bank", "GHIP", "hipMalloc", "hipMemcpy"):
        assert word not in text, word


def test_the_sanitized_build_plans_the_same_bytes(plans):
    plain, sanitized = plans
    assert plain == sanitized


def test_every_plan_has_the_bytes_the_parent_uploaded(plans):
    golden = json.load(open(GOLDEN))
    assert golden["sample_rate"] == SR
    got = {name: f["digest"] for name, f in plans[0].items()}
    assert got == golden["digests"]


def test_one_patch_is_cut_at_64_and_padded_to_fours(plans):
    for n, waves, pads in ((1, 1, 3), (64, 1, 3), (65, 2, 2), (257, 5, 3)):
        f = plans[0][f"one_patch_{n}"]
        assert _ints(f, "n", "regrouped", "waves", "pads", "wgs", "kinds", "tp_pairs") == [n, 0, waves, pads, (waves + 3) // 4, 1, 1], (n, f)


def test_2048_waves_are_not_more_than_2048(plans):
    f = plans[0]["alternating_2048"]
    assert _ints(f, "regrouped", "waves", "tp_pairs") == [0, 2048, 0], f
    f = plans[0]["alternating_2049"]
    assert _ints(f, "regrouped", "waves") == [1, 17 + 16], f   # 1,025 voices of one patch, 1,024 of the other


def test_a_bank_regrouping_does_not_help_takes_the_per_lane_form(plans):
    f = plans[0]["own_patch_each_2049"]
    assert _ints(f, "regrouped", "waves", "pads", "wgs", "n_spec", "tp_pairs") == [0, 0, 0, 0, 0, 0], f
    assert f["mix"] == "0,0,0"


def test_the_one_and_a_half_rule_on_both_sides(plans):
    kept, regrouped = plans[0]["runs_of_48_131072"], plans[0]["runs_of_40_131072"]
    assert _ints(kept, "regrouped", "waves") == [0, 2731], kept            # 2,731 <= 2,048 + 1,024 + 8
    assert int(regrouped["regrouped"]) == 1, regrouped                     # 3,277 > 3,080
    voices_of_patch = np.bincount((np.arange(131072) // 40) % 32)
    assert int(regrouped["waves"]) == int(np.sum((voices_of_patch + 63) // 64)) == 2061   # patch-major: every patch's voices in one stretch


def test_the_benchmark_voices_regroup_into_four_waves_a_patch(plans):
    f = plans[0]["voices_8192"]
    assert _ints(f, "regrouped", "waves", "pads", "wgs", "tp_pairs") == [1, 128, 0, 32, 1], f
    assert 0 < int(f["flagged"]) < 8192
    bare = plans[0]["voices_8192_no_flags"]
    assert _ints(bare, "regrouped", "waves", "wgs", "flagged", "f32_wgs") == [1, 128, 32, 0, 0], bare
    assert bare["base"] == f["base"] and bare["digest"] != f["digest"]


def test_a_control_change_splits_a_run_and_keeps_the_order(plans):
    f = plans[0]["voices_8192_cutoff_of_voice_1000_changed"]
    # voice 1,000 is the 32nd of patch 8's 256: runs of 31, 1 and 224 voices — 1 + 1 + 4 waves where there were 4
    assert _ints(f, "regrouped", "order_kept", "waves", "tp_pairs") == [1, 1, 130, 0], f


@pytest.mark.parametrize("rest", [1, 2])
def test_every_body_in_one_bank(plans, rest):
    f = plans[0][f"bodies_3k_plus_{rest}"]
    base = [int(x) for x in f["base"].split(",")]
    n_spec, wgs = _ints(f, "n_spec", "wgs")
    assert n_spec == 900 + rest and n_spec % 3 == rest and sum(base[:4]) == n_spec, f
    assert base[4] > 0 and base[5] > 0 and sum(base) == wgs, f
    assert 0 < int(f["f32_wgs"]) < n_spec                       # both values of the fp32 flag
    assert int(f["padded_groups"]) == 1125                       # every body's wave count is 1, 2 or 5: no multiple of four
    assert [int(x) for x in f["mix"].split(",")] == [(n_spec + 2 - s) // 3 for s in range(3)]
    assert int(f["kinds"]) >= 200 and int(f["regrouped"]) == 0, f
