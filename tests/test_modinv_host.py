"""The divstep inversion as compiled: mina_bridge_amd/csrc/fe_modinv.cuh -- the text the gfx950 kernels are built from -- compiled for the host
(tests/fuzz/modinv_twin.cpp, through tests/fuzz/hip_stub) on the corner set of tests/modinv_model.py, values of 31 .. 129 bits and random values, both fields:

    fe_inv_gcd == fe_inv (the Fermat routine of groupmap.cuh), word for word;       both == pow(x, p - 2, p) in the Montgomery domain, 0 -> 0;
    delta and the limbs of f, g, d, e at the end of every batch == the model's trace, for the corner set.

The same program is built a second time with -fsanitize=address,undefined -fno-sanitize-recover=all and run on the same rows: a stand-alone program with its own
main, nothing is loaded into the interpreter."""
import os
import re
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

import modinv_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACE_WORDS = 1 + M.BATCHES * 37


def _cxx():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import code_object as CO
    cxx = shutil.which("g++") or shutil.which("clang++") or os.path.join(CO.LLVM_BIN, "clang++")
    if not (cxx and os.path.exists(cxx)):
        pytest.skip("no C++ compiler")
    return cxx


def _build(d, extra):
    fz = os.path.join(ROOT, "tests", "fuzz")
    exe = str(d / "modinv_twin")
    done = subprocess.run([_cxx(), "-std=c++17", "-O1", "-w", *extra, "-I", os.path.join(fz, "hip_stub"), os.path.join(fz, "modinv_twin.cpp"), "-o", exe], capture_output=True, text=True)
    return exe, done


def words(x):
    return [(x >> (32 * i)) & M.M32 for i in range(8)]


@pytest.fixture(scope="module")
def rows():
    """per field: plain values (the corner set first) and their Montgomery words"""
    out = {}
    for F in (0, 1):
        p = M.P[F]
        plain = M.corners(F) + M.sized(F, 20, "modinv/host") + M.randoms(F, 400, "modinv/host")
        out[F] = (plain, [x * M.R % p for x in plain])
    return out


def _run(exe, d, rows):
    n, ntrace = len(rows[0][0]), len(M.corners(0))
    fin, fout = str(d / "in.bin"), str(d / "out.bin")
    with open(fin, "wb") as fh:
        fh.write(struct.pack("<2I", n, ntrace))
        for F in (0, 1):
            p = M.P[F]
            fh.write(np.array([words(c) for c in (M.R % p, M.R * M.R % p, p - 2)], np.uint32).tobytes())
            fh.write(np.array([words(a) for a in rows[F][1]], np.uint32).tobytes())
    done = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert done.returncode == 0, (done.returncode, done.stderr[-4000:])
    out = np.fromfile(fout, np.uint32)
    per = n * 16 + ntrace * TRACE_WORDS
    assert out.size == 2 * per
    for F in (0, 1):
        p = M.P[F]
        plain, mont = rows[F]
        res = out[F * per:F * per + n * 16].reshape(n, 16)
        trace = out[F * per + n * 16:(F + 1) * per].view(np.int32).reshape(ntrace, TRACE_WORDS)
        value = lambda w: sum(int(x) << (32 * i) for i, x in enumerate(w))
        for i, (x, a) in enumerate(zip(plain, mont)):
            gcd, fermat = value(res[i, :8]), value(res[i, 8:])
            assert gcd == fermat, (F, hex(x))
            assert gcd == pow(x, p - 2, p) * M.R % p and gcd < p, (F, hex(x))
        assert value(res[0, :8]) == 0 and plain[0] == 0                # 0 -> 0
        for i in range(ntrace):
            _, want = M.inverse_words(F, mont[i])                       # the routine's integer is the Montgomery word string
            assert int(trace[i, 0]) == len(want) <= M.BATCHES, (F, hex(plain[i]))
            for b, (delta, f, g, dd, e) in enumerate(want):
                got = [int(v) for v in trace[i, 1 + 37 * b:1 + 37 * (b + 1)]]
                assert got == [delta] + f + g + dd + e, (F, hex(plain[i]), b)
            assert not trace[i, 1 + 37 * len(want):].any()


def test_the_compiled_header_equals_fe_inv_pow_and_the_models_limbs(tmp_path, rows):
    exe, done = _build(tmp_path, [])
    assert done.returncode == 0, done.stderr[-4000:]
    _run(exe, tmp_path, rows)


def test_it_runs_clean_under_the_address_and_undefined_behaviour_sanitizers(tmp_path, rows):
    exe, done = _build(tmp_path, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if done.returncode != 0:
        assert re.search(r"asan|ubsan|sanitize", done.stderr, re.I), done.stderr[-4000:]
        pytest.skip("the compiler has no AddressSanitizer / UBSan runtime")
    _run(exe, tmp_path, rows)
