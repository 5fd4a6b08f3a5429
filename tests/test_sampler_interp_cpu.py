"""CPU tier: the interpolated sampler arithmetic of csrc/dsp_core.h (docs/DSP_SPEC.md section 7), compiled for the host as a program of
its own (tests/sampler_interp_check.cpp) and run."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_interpolated_chunks_are_count_calls_of_the_frame_form_on_the_cpu(tmp_path):
    """sampler_chunk_interp<MODE, 16> and its stereo sibling equal `count` calls of sampler_frame_interp<MODE> (values, idx, playing) in
    the three modes, mono and stereo, over count < C, samples that end inside the chunk, step 0, lengths 1 to 3 and 20,000 random
    (idx, step, length, count); NEAREST is sampler_frame's and sampler_chunk's bits, and so is every frame whose fraction is 0; at both
    ends of a sample between neighbours of 1e6 the per-frame form is the formula with the outside taps 0.  Built with the address and
    undefined-behaviour sanitizers: with a sample at either end of the allocation, no tap is read from outside it."""
    src = os.path.join(REPO, "tests", "sampler_interp_check.cpp")
    exe = str(tmp_path / "sampler_interp_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, src], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok:"), run.stdout + run.stderr


def test_the_bindings_name_the_modes_as_the_header_does():
    """groove_types.h groove_sample_interpolation and abi_types agree, and the library exports the two calls."""
    import ctypes
    import re
    from groove_amd import abi_types as T, lib
    text = open(os.path.join(REPO, "include", "groove_types.h")).read()
    enum = dict((k, int(v)) for k, v in re.findall(r"GROOVE_SAMPLE_(NEAREST|LINEAR|CUBIC) = (\d+)", text))
    assert enum == {"NEAREST": T.SAMPLE_NEAREST, "LINEAR": T.SAMPLE_LINEAR, "CUBIC": T.SAMPLE_CUBIC} == {"NEAREST": 0, "LINEAR": 1, "CUBIC": 2}
    so = ctypes.CDLL(lib.LIB_PATH)
    assert hasattr(so, "groove_bank_set_sample_interpolation") and hasattr(so, "groove_bank_sample_interpolation")
    host = ctypes.CDLL(os.path.join(REPO, "groove_amd", "host", "libgroove_host.so"))
    assert hasattr(host, "gh_set_sample_interpolation") and hasattr(host, "gh_sample_interpolation")
    cli = os.path.join(REPO, "groove_amd", "host", "groove-cli-hip")
    usage = subprocess.run([cli, "--help"], capture_output=True, text=True)
    assert usage.returncode == 0 and "--sample-interpolation nearest|linear|cubic" in usage.stdout, usage.stdout
    bad = subprocess.run([cli, "--sample-interpolation", "sinc", "x.json"], capture_output=True, text=True)
    assert bad.returncode == 2 and "nearest, linear or cubic" in bad.stderr, bad.stderr
