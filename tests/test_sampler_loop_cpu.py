"""CPU tier: the looped sampler arithmetic of csrc/dsp_core.h (docs/DSP_SPEC.md section 7) and the host layer's read_wav_loop, compiled
for the host as a program of its own (tests/sampler_loop_check.cpp) and run."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_looped_forms_are_the_fold_in_exact_integers_on_the_cpu(tmp_path):
    """sample_loop_fold against repeated subtraction and F(F(x) + y) == F(x + y) in 128-bit integers; sampler_chunk_loop<MODE, 16> and
    its stereo sibling equal `count` calls of sampler_frame_loop<MODE> (values, idx, playing) in the three modes for voices that loop
    and voices that do not, and a voice that does not loop is sampler_frame_interp's bits; the tap rule at loops of 1, 2 and 3 frames,
    start == 0 and end == length against the modulo formula in double, each sample ending where its allocation ends; length 2^20 - 1
    looped at its end with step 2^51; read_wav_loop on a forward, a ping-pong and a reverse loop, truncated chunks, dwEnd at and past
    the frame count and a file without the chunk.  Built with the address and undefined-behaviour sanitizers: no tap is read from
    outside [offset, offset + end)."""
    src = [os.path.join(REPO, "tests", "sampler_loop_check.cpp"), os.path.join(REPO, "groove_amd", "host", "project.cpp")]
    exe = str(tmp_path / "sampler_loop_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-DGROOVE_HOST_PARSER_ONLY", "-o", exe] + src, check=True)
    run = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok:"), run.stdout + run.stderr


def test_the_bindings_carry_the_loop_calls():
    """groove_types.h groove_sample_loop and abi_types.SampleLoop agree, the libraries export the calls, and the CLI knows the switch."""
    import ctypes
    from groove_amd import abi_types as T, lib
    text = open(os.path.join(REPO, "include", "groove_types.h")).read()
    assert "typedef struct { uint32_t start, end; } groove_sample_loop;" in text
    assert ctypes.sizeof(T.SampleLoop) == 8 and [f[0] for f in T.SampleLoop._fields_] == ["start", "end"]
    so = ctypes.CDLL(lib.LIB_PATH)
    assert hasattr(so, "groove_bank_set_sample_loops") and hasattr(so, "groove_bank_sample_loops")
    assert "groove_bank_set_sample_loops" in lib.SYMBOLS and "groove_bank_sample_loops" in lib.SYMBOLS
    host = ctypes.CDLL(os.path.join(REPO, "groove_amd", "host", "libgroove_host.so"))
    for name in ("gh_set_sample_loops", "gh_sample_loops", "gh_set_sample_loop", "gh_read_wav_loop"):
        assert hasattr(host, name), name
    cli = os.path.join(REPO, "groove_amd", "host", "groove-cli-hip")
    usage = subprocess.run([cli, "--help"], capture_output=True, text=True)
    assert usage.returncode == 0 and "--sample-loops" in usage.stdout, usage.stdout
