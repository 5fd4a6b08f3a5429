"""CPU tier: the enveloped sampler arithmetic of csrc/dsp_core.h, derive.h and welsh_tp.h (docs/DSP_SPEC.md section 7), compiled for
the host as a program of its own (tests/sampler_env_check.cpp) and run; and the bindings of the new calls."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_enveloped_forms_are_the_per_frame_definition_on_the_cpu(tmp_path):
    """One voice at a time through a timeline of note events in three forms — sampler_frame_env<MODE> per frame (the definition),
    sampler_chunk_env<MODE, 16> and its stereo sibling (the serial kernel's), and the time-parallel body's closed form (sampler_env_valid
    from env_idle_at, sampler_env_lane: env_seek to a lane's frame and its ticks, sampler_env_block_end) — equal bit for bit at every
    frame and in SamplerState and all EnvState words at every block end, three modes, two splits into blocks; the sample's end and the
    release's end on the same frame, one and two apart, the idle frame on every position of a block; the gate envelope plays
    sampler_frame_loop's bits and leaves its state.  Built with the address and undefined-behaviour sanitizers, every sample an
    allocation of exactly its length: no tap is read outside the voice's sample."""
    src = os.path.join(REPO, "tests", "sampler_env_check.cpp")
    exe = str(tmp_path / "sampler_env_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(REPO, "include"), "-o", exe, src], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok:"), run.stdout + run.stderr


def test_the_bindings_carry_the_envelope_calls():
    """The libraries export the calls, the binding tables name them, the record is 6 + 7 words, and the CLI knows the switch."""
    import ctypes
    from groove_amd import abi_types as T, lib
    so = ctypes.CDLL(lib.LIB_PATH)
    for name in ("groove_bank_set_sample_envelopes", "groove_bank_sample_envelopes", "groove_bank_download_sample_envelope_state"):
        assert hasattr(so, name) and name in lib.SYMBOLS, name
    assert len(T.SAMPLE_ENV_STATE_WORDS) == 7 and ctypes.sizeof(T.EnvelopeParams) == 32
    text = open(os.path.join(REPO, "groove_amd", "csrc", "dsp_core.h")).read()
    assert "kSampleEnvParamWords = 6, kSampleEnvStateWords = 7" in text
    host = ctypes.CDLL(os.path.join(REPO, "groove_amd", "host", "libgroove_host.so"))
    for name in ("gh_set_sample_envelope", "gh_sample_envelope"):
        assert hasattr(host, name), name
    cli = os.path.join(REPO, "groove_amd", "host", "groove-cli-hip")
    usage = subprocess.run([cli, "--help"], capture_output=True, text=True)
    assert usage.returncode == 0 and "--sample-envelope A,D,S,R" in usage.stdout, usage.stdout
    bad = subprocess.run([cli, "--sample-envelope", "0.1,0.2"], capture_output=True, text=True)
    assert bad.returncode == 2 and "--sample-envelope takes four numbers" in bad.stderr, bad.stderr
