"""CPU tier: no cross-lane code without a test that reads its result.  The sources of the library (groove_amd/csrc/*.h, *.hip) are
searched for every function whose body moves data between lanes — __builtin_amdgcn_update_dpp, __shfl and its kin, v_writelane, or a
call of one of the library's single-move helpers (MOVES) — and each must be

  * a row of the probe table (PROBED: tests/probe/wave_probe.hip calls it, tests/test_gpu_wave_primitives.py judges it), or
  * a single-move helper whose every use is inside such functions (MOVES: judged through the probed routine named), or
  * an entry of INLINE_IN_KERNEL: cross-lane code written into a kernel body, with the whole-kernel test that covers it and why that
    test would notice.

New cross-lane code then cannot arrive untested without someone writing down why.  readfirstlane / readlane and __ballot are
uniformity plumbing (one value for the whole wavefront, no pattern to get wrong) and stay outside."""
import glob
import os
import re

from tests import wave_primitive_cases as W

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAW = re.compile(r"__builtin_amdgcn_update_dpp|__shfl\w*|v_writelane")

# function -> the row of tests/wave_primitive_cases.py PRIMITIVES it is
PROBED = {name: name for name in W.PRIMITIVES}
# single cross-lane moves -> a probed routine that is built from them
MOVES = {
    "tp_dpp_f64": "tp_scan_affine", "tp_dpp_compose": "tp_scan_affine",
    "tp_dpp_u64": "tp_scan_add_u64", "tp_dpp_add2": "tp_scan_add_u64", "tp_dpp_max": "tp_scan_max_i32",
    "dpp_add": "wave_sum_lane63",
    "tp_shfl": "tp_shfl", "tp_shfl_affine": "tp_shfl",
}
# function -> (test file, test function or None for the whole file, what the kernel does across lanes and why that test sees it)
INLINE_IN_KERNEL = {
    "welsh_tp_body": ("tests/test_gpu_time_parallel.py", "test_time_parallel_matches_serial_kernels_and_oracle",
                      "hard sync reads the previous lane's running wrap position (__shfl), every lane its start state and the noise generators' "
                      "end states from other lanes (tp_shfl): the hard-sync, noise and filter patches of the table, blocks and states voice by voice"),
    "fm_tp_body": ("tests/test_gpu_instruments.py", "test_fm_four_voices_per_wavefront_parity",
                   "the 16-lane row scan of the carrier increments at four voices per wavefront (tp_dpp_u64, row_shr only): the carrier phase is compared exactly"),
    "fx_lp24_tp_kernel": ("tests/test_gpu_fx_forms.py", None,
                          "the shuffle scan of the 24 dB effect's affine maps (tp_shfl_affine, lanes at or above d compose with lane - d): the form is asserted and played against the oracle"),
    "split_turn_tile": ("tests/test_gpu_split.py", "test_split_kernel_equals_the_serial_kernels_bit_for_bit",
                        "FusedAcc::flush's dpp_add chain written out for the role-split kernel's tile: its fused rows are compared with the serial kernels' bit for bit"),
}
SKIP_BEFORE_PAREN = {"__launch_bounds__", "__attribute__", "alignas", "decltype", "sizeof", "static_assert", "if", "for", "while", "switch", "return", "defined"}


def _strip(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    out, cont = [], False
    for line in text.split("\n"):   # preprocessor lines (with their continuations) hold no function
        if cont or line.lstrip().startswith("#"):
            cont = line.rstrip().endswith("\\")
            out.append("")
        else:
            out.append(line)
    return "\n".join(out)


def _function_name(header):
    """The identifier in front of the first parameter list of a declarator, or None when the header is no function's."""
    if not re.search(r"\)\s*(const|noexcept|mutable)?\s*$", header) and not re.search(r"\)\s*:\s*\w+\s*\(.*\)\s*$", header, flags=re.S):
        return None
    for m in re.finditer(r"([A-Za-z_]\w*)\s*\(", header):
        if m.group(1) not in SKIP_BEFORE_PAREN:
            return m.group(1)
    return None


def functions(text):
    """{qualified name: [bodies]} of the function definitions at namespace or class scope of a C++ text (comments stripped)."""
    found = {}
    stack = []        # (kind, name, start): 'scope' (namespace / class) | 'fn' | 'block'
    last = 0          # the end of the previous declaration at this point
    for i, ch in enumerate(text):
        if ch == ";" and not any(k == "fn" for k, _, _ in stack):
            last = i + 1
        elif ch == "{":
            header = text[last:i].strip()
            if any(k == "fn" for k, _, _ in stack):
                stack.append(("block", None, i))
            else:
                scope = re.search(r"\b(namespace|struct|class|union)\b\s*([A-Za-z_]\w*)?[^()]*$", header) or re.match(r'extern\s+"C"\s*$', header)
                name = None if scope else _function_name(header)
                if scope:
                    stack.append(("scope", scope.group(2) if scope.lastindex and scope.group(1) != "namespace" else None, i))
                elif name:
                    stack.append(("fn", "::".join([n for k, n, _ in stack if k == "scope" and n] + [name]), i))
                else:
                    stack.append(("block", None, i))
            last = i + 1
        elif ch == "}":
            kind, name, start = stack.pop()
            if kind == "fn":
                found.setdefault(name, []).append(text[start:i + 1])
            last = i + 1
    assert not stack
    return found


def library_functions():
    found = {}
    for path in sorted(glob.glob(os.path.join(REPO, "groove_amd", "csrc", "*.h")) + glob.glob(os.path.join(REPO, "groove_amd", "csrc", "*.hip"))):
        with open(path) as f:
            for name, bodies in functions(_strip(f.read())).items():
                found.setdefault(name, []).extend(bodies)
    return found


def _calls(body, name):
    return re.search(r"(?<![\w:])" + re.escape(name.split("::")[-1]) + r"\s*[<(]", body) is not None


def cross_lane_users(found):
    users = {}
    for name, bodies in found.items():
        body = "\n".join(bodies)
        why = sorted(set(RAW.findall(body))) + [m for m in MOVES if m != name and _calls(body, m)]
        if why:
            users[name] = why
    return users


def test_the_parser_finds_the_functions_it_is_for():
    found = library_functions()
    for name in list(PROBED) + list(MOVES) + list(INLINE_IN_KERNEL) + ["welsh_tp_kernel", "lp24_affine_compose", "FusedAcc::add", "run_frames"]:
        assert name in found, name
    assert len(found) > 300
    text = _strip("// v_writelane in a comment\n#define M { \\\n __shfl }\nstruct S { int f(int x) const { return g<1>(x); } };\n"
                  "template <int N = (3)> __global__ __launch_bounds__(64) void k(int* p) { auto l = [](int v) { return v; }; p[0] = l(1); }\nint t[] = {1, 2};\n")
    assert sorted(functions(text)) == ["S::f", "k"] and not RAW.search(text)


def test_every_cross_lane_function_is_probed_or_accounted_for():
    found = library_functions()
    users = cross_lane_users(found)
    for name, why in sorted(users.items()):
        print(f"  {name}: {', '.join(why)} -> " + ("probe row" if name in PROBED else f"through {MOVES[name]}" if name in MOVES else "inline, " + INLINE_IN_KERNEL.get(name, ("UNTESTED",))[0]))
    unaccounted = sorted(set(users) - set(PROBED) - set(MOVES) - set(INLINE_IN_KERNEL))
    assert not unaccounted, f"cross-lane code without a probe row or an INLINE_IN_KERNEL entry: {[(n, users[n]) for n in unaccounted]}"
    # nothing stale: every entry of the three tables is still cross-lane code of the library
    for name in list(PROBED) + list(MOVES) + list(INLINE_IN_KERNEL):
        assert name in users, f"{name} is in a table of this file and no cross-lane function of the library any more"
    assert not set(PROBED) & set(INLINE_IN_KERNEL) and not set(MOVES) & set(INLINE_IN_KERNEL)


def test_every_probe_row_is_called_by_the_probe_and_every_move_reaches_its_row():
    with open(os.path.join(REPO, "tests", "probe", "wave_probe.hip")) as f:
        probe = _strip(f.read())
    assert sorted(PROBED.values()) == sorted(W.PRIMITIVES)
    for name in PROBED:
        call = "flush" if name == "FusedAcc::flush" else name
        assert re.search(r"\b" + re.escape(call) + r"\s*[<(]", probe), f"{name}: no kernel of tests/probe/wave_probe.hip calls it"
    found = library_functions()
    for move, row in MOVES.items():
        assert row in PROBED
        reach, grew = {row}, True
        while grew:   # the helpers the probed routine is built from, transitively
            new = {m for m in MOVES if m not in reach and any(_calls("\n".join(found[r]), m) for r in reach)}
            grew = bool(new)
            reach |= new
        body = "\n".join(found[move])   # ... or the helper is itself nothing but calls of the probed routine (tp_shfl_affine: tp_shfl per word)
        assert move in reach or (_calls(body, row) and not RAW.search(body)), f"{move} is not reached from {row}"


def test_every_inline_entry_names_a_test_that_exists():
    for name, (path, test, why) in INLINE_IN_KERNEL.items():
        full = os.path.join(REPO, path)
        assert os.path.exists(full) and len(why) > 40, name
        with open(full) as f:
            text = f.read()
        assert "pytest.mark.gpu" in text, path
        if test is not None:
            assert re.search(r"^def " + re.escape(test) + r"\(", text, flags=re.M), (name, test)
