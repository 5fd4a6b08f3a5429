"""Regenerate tests/golden/reference/: the reference checkout's DATA files that the CPU tests read, so that the suite runs from a clean
checkout of this repository alone.

    python tests/golden/make_reference_data.py <reference checkout>

Copied as they are: every project file (projects/**/*.json*) and every Welsh patch (assets/patches/welsh/*.json).  Shortened: every WAV
file of assets/samples/ and of test-data/samples/ keeps its format and every chunk but the first WAV_FRAMES frames of its `data` chunk
(the RIFF and data sizes rewritten to match), so the decoders still meet every format, rate and chunk layout the reference ships.  Also
written: filters004_vectors.npz, what the reference's C filter text (oracle/_ref/libfilters004.so, `make -C oracle ref`) computes for
tests/test_oracle_ref.py's cases, for a checkout where that library cannot be built.  No source text of the reference is copied."""
import glob
import math
import os
import shutil
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "reference")
WAV_FRAMES = 300


def shorten_wav(blob, frames=WAV_FRAMES):
    """The same RIFF/WAVE file with its data chunk cut to `frames` frames; every other chunk kept in place."""
    assert blob[:4] == b"RIFF" and blob[8:12] == b"WAVE", "not a RIFF/WAVE file"
    pos, chunks, block_align = 12, [], None
    while pos + 8 <= len(blob):
        cid, size = blob[pos:pos + 4], struct.unpack("<I", blob[pos + 4:pos + 8])[0]
        body = blob[pos + 8:pos + 8 + size]
        if cid == b"fmt ":
            block_align = struct.unpack("<H", body[12:14])[0]
        chunks.append((cid, body))
        pos += 8 + size + (size & 1)
    out = b""
    for cid, body in chunks:
        if cid == b"data":
            body = body[:frames * block_align]
        out += cid + struct.pack("<I", len(body)) + body + (b"\x00" if len(body) & 1 else b"")
    return b"RIFF" + struct.pack("<I", 4 + len(out)) + b"WAVE" + out


def copy_data(ref):
    if os.path.isdir(OUT):
        shutil.rmtree(OUT)
    n = {"projects": 0, "patches": 0, "wavs": 0}
    for f in sorted(glob.glob(os.path.join(ref, "projects", "**", "*.json*"), recursive=True)):
        dst = os.path.join(OUT, os.path.relpath(f, ref))
        os.makedirs(os.path.dirname(dst), exist_ok=True)
        shutil.copyfile(f, dst)
        n["projects"] += 1
    for f in sorted(glob.glob(os.path.join(ref, "assets", "patches", "welsh", "*.json"))):
        dst = os.path.join(OUT, os.path.relpath(f, ref))
        os.makedirs(os.path.dirname(dst), exist_ok=True)
        shutil.copyfile(f, dst)
        n["patches"] += 1
    wavs = glob.glob(os.path.join(ref, "assets", "samples", "**", "*.wav"), recursive=True) + \
        glob.glob(os.path.join(ref, "test-data", "samples", "*.wav"))
    for f in sorted(wavs):
        dst = os.path.join(OUT, os.path.relpath(f, ref))
        os.makedirs(os.path.dirname(dst), exist_ok=True)
        with open(f, "rb") as src, open(dst, "wb") as o:
            o.write(shorten_wav(src.read()))
        n["wavs"] += 1
    return n


# tests/test_oracle_ref.py's cases: (fc, ripple) of the 24 dB sections, (f0, Q) of the RBJ low-pass, and the recurrence run
LP24_CASES = [(1000.0, 0.8), (40.0, 0.707), (12000.0, 2.0), (5000.0, 1.3), (19000.0, 0.9)]
RBJ_CASES = [(1000.0, 0.707), (250.0, 2.0), (8000.0, 0.5)]
IIR_CASE = {"fs": 44100.0, "fc": 1800.0, "ripple": 0.9, "n": 4096}


def lp24_sections(ripple):
    """(d, c) of the two sections of the 24 dB low-pass prototype, as tests/test_oracle_ref.py states them."""
    sg, cg = math.sinh(ripple), math.cosh(ripple) ** 2
    c0, c2 = 1 / (cg - 0.85355339059327376220), 1 / (cg - 0.14644660940672623780)
    return ((c0 * sg * 1.84775906502257351226, c0), (c2 * sg * 0.76536686473017954346, c2))


def szx_inputs():
    """Every (b1, b2, fc, fs) szxform() is called with by the tests."""
    rows = []
    for fc, ripple in LP24_CASES:
        rows += [(d, c, fc, 44100.0) for d, c in lp24_sections(ripple)]
    rows += [(1.0 / q, 1.0, f0, 44100.0) for f0, q in RBJ_CASES]
    rows += [(d, c, IIR_CASE["fc"], IIR_CASE["fs"]) for d, c in lp24_sections(IIR_CASE["ripple"])]
    return np.array(rows, dtype=np.float64)


def sawtooth(fs, n):
    t = np.arange(n)
    return (2.0 * ((t * 220.0 / fs) % 1.0) - 1.0).astype(np.float32)


def write_filter_vectors():
    import ctypes as C
    sys.path.insert(0, REPO)
    from oracle import oracle as O
    ref = O.ref_lib()
    if ref is None:
        raise SystemExit("oracle/_ref/libfilters004.so is not built (make -C oracle ref)")
    ins = szx_inputs()
    ks, coefs = np.zeros(len(ins)), np.zeros((len(ins), 4), dtype=np.float32)
    for i, (b1, b2, fc, fs) in enumerate(ins):
        k, sec = C.c_double(1.0), (C.c_float * 4)()
        ref.ref_szxform(1.0, 0.0, 0.0, 1.0, b1, b2, fc, fs, C.byref(k), sec)
        ks[i], coefs[i] = k.value, list(sec)
    # the recurrence: the two sections' coefficients as the reference computes them, gain first (its cascaded layout)
    coef = (C.c_float * 9)()
    gain = C.c_double(1.0)
    for i, (d, c) in enumerate(lp24_sections(IIR_CASE["ripple"])):
        sec = (C.c_float * 4)()
        ref.ref_szxform(1.0, 0.0, 0.0, 1.0, d, c, IIR_CASE["fc"], IIR_CASE["fs"], C.byref(gain), sec)
        for j in range(4):
            coef[1 + 4 * i + j] = sec[j]
    coef[0] = gain.value
    x = sawtooth(IIR_CASE["fs"], IIR_CASE["n"])
    y = np.zeros(IIR_CASE["n"], dtype=np.float32)
    fp = C.POINTER(C.c_float)
    ref.ref_iir_run(coef, 2, x.ctypes.data_as(fp), y.ctypes.data_as(fp), IIR_CASE["n"])
    np.savez_compressed(os.path.join(HERE, "filters004_vectors.npz"), szx_in=ins, szx_k=ks, szx_coef=coefs, iir_y=y)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    print(copy_data(sys.argv[1]))
    write_filter_vectors()
