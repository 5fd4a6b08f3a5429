"""CPU tier: the WAV reader that keeps channels (groove_amd/host/project.cpp read_wav_stereo, beside read_wav_mono: one parser), what a
project's samplers are described as with Orchestrator::set_stereo_samples on and off, and the host build of the stereo sampler text
of csrc/dsp_core.h (tests/sampler_stereo_check.cpp).  No GPU calls."""
import ctypes as C
import json
import os
import struct
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(REPO, "tests", "golden", "reference")   # the reference checkout's data files (tests/golden/make_reference_data.py)
_fp = C.POINTER(C.c_float)
FRAMES = 53


@pytest.fixture(scope="module")
def host():
    from groove_amd import host_binding
    if not os.path.exists(host_binding.HOST_LIB):
        import __graft_entry__ as g
        g.build()
    L = C.CDLL(host_binding.HOST_LIB)
    L.gh_read_wav_mono.restype = C.c_int64
    L.gh_read_wav_mono.argtypes = [C.c_char_p, _fp, C.c_uint64, C.POINTER(C.c_uint32), C.c_char_p, C.c_size_t]
    L.gh_read_wav_stereo.restype = C.c_int64
    L.gh_read_wav_stereo.argtypes = [C.c_char_p, _fp, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_char_p, C.c_size_t]
    L.gh_project_describe_samples.restype = C.c_void_p
    L.gh_project_describe_samples.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, C.c_size_t]
    L.gh_project_describe.restype = C.c_void_p
    L.gh_project_describe.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t]
    L.gh_free.argtypes = [C.c_void_p]
    return L


def _samples(fmt, channels, seed):
    """Raw samples [FRAMES][channels] (ints, or float32 for "f32"), extremes included."""
    rng = np.random.default_rng(seed)
    if fmt == "f32":
        x = (rng.standard_normal((FRAMES, channels)) * 0.4).astype(np.float32)
        x[0, 0], x[1, -1] = 1.0, -1.0
        return x
    bits = int(fmt)
    lo, hi = (0, 255) if bits == 8 else (-(1 << (bits - 1)), (1 << (bits - 1)) - 1)
    x = rng.integers(lo, hi + 1, size=(FRAMES, channels), dtype=np.int64)
    x[0, 0], x[1, -1], x[2, 0] = lo, hi, (128 if bits == 8 else 0)
    return x


def _payload(fmt, x):
    if fmt == "f32":
        return x.astype("<f4").tobytes()
    bits = int(fmt)
    if bits == 8:
        return x.astype(np.uint8).tobytes()
    if bits == 16:
        return x.astype("<i2").tobytes()
    if bits == 32:
        return x.astype("<i4").tobytes()
    u = (x.reshape(-1) & 0xFFFFFF).astype(np.uint32)
    return np.stack([u & 0xFF, (u >> 8) & 0xFF, (u >> 16) & 0xFF], axis=1).astype(np.uint8).tobytes()


def _decoded(fmt, x):
    """The decoded values in f64, as the reader computes them: ints scaled by 2^(bits-1), 8-bit offset by 128."""
    if fmt == "f32":
        return x.astype(np.float64)
    bits = int(fmt)
    return (x - 128) / 128.0 if bits == 8 else x / float(1 << (bits - 1))


def _wav(fmt, x):
    """RIFF/WAVE with an odd-length LIST chunk and a smpl chunk before `data`, and an acid chunk after it."""
    channels = x.shape[1]
    bits = 32 if fmt == "f32" else int(fmt)
    payload = _payload(fmt, x)
    hdr = struct.pack("<HHIIHH", 3 if fmt == "f32" else 1, channels, 44100, 44100 * channels * bits // 8, channels * bits // 8, bits)
    smpl = struct.pack("<9I", 0, 0, 22675, 62, 0, 0, 0, 0, 0)
    acid = struct.pack("<IHHfIHHf", 2, 57, 0x8000, 0.0, 4, 4, 4, 109.7)
    body = (b"WAVE" + b"fmt " + struct.pack("<I", len(hdr)) + hdr + b"LIST\x03\x00\x00\x00abc\x00" + b"smpl" + struct.pack("<I", len(smpl)) + smpl +
            b"data" + struct.pack("<I", len(payload)) + payload + (b"\x00" if len(payload) & 1 else b"") + b"acid" + struct.pack("<I", len(acid)) + acid)
    return b"RIFF" + struct.pack("<I", len(body)) + body


def _read(host, path, stereo):
    out = np.full(FRAMES * 2 + 8, np.float32(7.0))
    sr, ch, err = C.c_uint32(0), C.c_uint32(0), C.create_string_buffer(256)
    if stereo:
        n = host.gh_read_wav_stereo(str(path).encode(), out.ctypes.data_as(_fp), len(out), C.byref(ch), C.byref(sr), err, 256)
    else:
        n = host.gh_read_wav_mono(str(path).encode(), out.ctypes.data_as(_fp), len(out), C.byref(sr), err, 256)
    assert n == FRAMES and sr.value == 44100, (n, err.value)
    return out, ch.value


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("fmt", ["8", "16", "24", "32", "f32"])
@pytest.mark.parametrize("channels", [1, 2, 3])
def test_the_stereo_reader_keeps_two_channels_and_the_mono_reader_is_unchanged(host, tmp_path, fmt, channels):
    x = _samples(fmt, channels, seed=100 * channels + len(fmt) + (int(fmt) if fmt != "f32" else 7))
    path = tmp_path / "t.wav"
    path.write_bytes(_wav(fmt, x))
    v = _decoded(fmt, x)                                            # f64 [FRAMES][channels]
    acc = np.zeros(FRAMES)
    for c in range(channels):                                       # the mean as the reader computes it: an f64 sum in channel order, one division,
        acc = acc + v[:, c]                                         # one rounding to fp32 — for two channels (float)(((double)L + (double)R) / 2)
    mean = (acc / channels).astype(np.float32)
    got, ch = _read(host, path, stereo=True)
    if channels == 2:
        assert ch == 2
        assert np.array_equal(_bits(got[:2 * FRAMES].reshape(FRAMES, 2)), _bits(v.astype(np.float32)))     # (float) of each decoded value, no averaging
        assert np.all(got[2 * FRAMES:] == 7.0)
        assert not np.array_equal(got[0:2 * FRAMES:2], got[1:2 * FRAMES:2])
    else:
        assert ch == 1                                              # one channel; more than two: the mono reader's mean
        assert np.array_equal(_bits(got[:FRAMES]), _bits(mean)) and np.all(got[FRAMES:] == 7.0)
    mono, _ = _read(host, path, stereo=False)
    assert np.array_equal(_bits(mono[:FRAMES]), _bits(mean)) and np.all(mono[FRAMES:] == 7.0)


def test_the_stereo_reader_on_the_reference_assets_is_the_standard_library(host):
    """The reference's own stereo sampler file and a mono one through `wave`: channels kept, every value bit for bit."""
    import wave
    for name, want_ch in (("stereo-pluck.wav", 2), ("spoken_stereo-from-elevenlabs.io.wav", 2), ("spoken_mono-from-elevenlabs.io.wav", 1)):
        f = f"{REF}/assets/samples/{name}"
        with wave.open(f, "rb") as w:
            ch, width, frames = w.getnchannels(), w.getsampwidth(), w.getnframes()
            raw = w.readframes(frames)
        assert ch == want_ch and width in (2, 3)
        if width == 2:
            ints = np.frombuffer(raw, dtype="<i2").astype(np.int64)
        else:
            b = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 3).astype(np.int64)
            ints = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
            ints = np.where(ints & 0x800000, ints - (1 << 24), ints)
        want = (ints.reshape(-1, ch) / float(1 << (8 * width - 1))).astype(np.float32)
        out = np.zeros(want.size + 8, dtype=np.float32)
        sr, got_ch, err = C.c_uint32(0), C.c_uint32(0), C.create_string_buffer(256)
        n = host.gh_read_wav_stereo(f.encode(), out.ctypes.data_as(_fp), len(out), C.byref(got_ch), C.byref(sr), err, 256)
        assert n == frames and got_ch.value == ch, (name, n, err.value)
        assert np.array_equal(_bits(out[:want.size]), _bits(want.reshape(-1))), name


def test_a_missing_file_is_an_error_with_a_message(host, tmp_path):
    err, ch, sr = C.create_string_buffer(256), C.c_uint32(0), C.c_uint32(0)
    assert host.gh_read_wav_stereo(str(tmp_path / "missing.wav").encode(), None, 0, C.byref(ch), C.byref(sr), err, 256) == -1 and err.value
    (tmp_path / "junk.wav").write_bytes(b"RIFF\x00\x00\x00\x00WAVEjunk")
    assert host.gh_read_wav_stereo(str(tmp_path / "junk.wav").encode(), None, 0, C.byref(ch), C.byref(sr), err, 256) == -1
    assert b"fmt/data" in err.value


def _describe(host, path, stereo):
    err = C.create_string_buffer(512)
    p = host.gh_project_describe_samples(path.encode(), f"{REF}/assets".encode(), 1 if stereo else 0, err, 512)
    assert p, err.value
    try:
        return json.loads(C.string_at(p).decode())
    finally:
        host.gh_free(p)


@pytest.mark.parametrize("project, on", [("projects/tests/load-stereo-wav.json", 2), ("projects/demos/instruments/sampler.json", 2),
                                         ("projects/tests/load-mono-wav.json", 1)])
def test_the_reference_sampler_projects_describe_their_channels(host, project, on):
    """The switch on: a sampler on a two-channel file is a stereo bank; off (the default), and on a mono file, one channel."""
    for stereo, want in ((True, on), (False, 1)):
        samplers = [d for d in _describe(host, f"{REF}/{project}", stereo)["devices"] if d["kind"] == "sampler"]
        assert samplers and all(d["channels"] == want for d in samplers), (project, stereo, samplers)
    err = C.create_string_buffer(512)                               # the entry without the switch: one channel
    p = host.gh_project_describe(f"{REF}/{project}".encode(), f"{REF}/assets".encode(), err, 512)
    assert p, err.value
    plain = json.loads(C.string_at(p).decode())
    host.gh_free(p)
    assert all(d["channels"] == 1 for d in plain["devices"] if d["kind"] == "sampler")


def test_the_stereo_chunk_is_count_calls_of_the_frame_form_on_the_cpu(tmp_path):
    """csrc/dsp_core.h compiles for the host with the stereo sampler text in it, and sampler_chunk_stereo equals `count` calls of
    sampler_frame_stereo (values, idx, playing) over count < C, samples that end inside the chunk, step 0, length 1 and 20,000 random
    (idx, step, length, count); the mono forms on the left channel give the left channel's bits.  Built with the address and
    undefined-behaviour sanitizers as a program of its own: the clamped fetches stay inside the bank."""
    src = os.path.join(REPO, "tests", "sampler_stereo_check.cpp")
    exe = str(tmp_path / "sampler_stereo_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, src], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok:"), run.stdout + run.stderr


def test_the_emulation_tier_still_builds():
    from tests.emul import emul
    assert os.path.exists(emul.build())
