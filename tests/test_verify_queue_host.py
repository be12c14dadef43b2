"""CPU tier of the boundary's completion queue (`mina_verify_queue_*`): tests/fuzz/tsan_queue.cpp -- the product's api_verify.hip, host_core.hip, api_wire.hip and
api_consensus.hip against the stand-in runtime of tests/fuzz/hip_stub, the device layer stubbed by tsan_boundary.cpp -- built here with the compiler and flags
of the Makefile's `tsan` target, once under ThreadSanitizer for the stress run and once under AddressSanitizer + UBSan for the fixed single-thread script.  Stand-alone
programs that link their sanitizer themselves; nothing is preloaded."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUZZ = os.path.join(ROOT, "tests", "fuzz")
CSRC = os.path.join(ROOT, "mina_bridge_amd", "csrc")
CLANGXX = os.environ.get("CLANGXX", "/opt/rocm/lib/llvm/bin/clang++")
BOUNDARY_FLAGS = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-I", os.path.join(FUZZ, "hip_stub"), "-pthread", "-Wno-everything"]
TSAN_SRC = ["host_core.hip", "api_wire.hip", "api_consensus.hip", "api_verify.hip"]
FIXTURES = [os.path.join(ROOT, "tests", "golden", "state_proofs_k15_bytes.json"), os.path.join(ROOT, "tests", "golden", "account_proofs_bytes.json")]


def build(out_dir, name, sanitize):
    """the Makefile's build_boundary recipe with tsan_queue.cpp in tsan_boundary.cpp's place; the four sources compile side by side"""
    objs, procs = [], []
    for f in TSAN_SRC:
        o = os.path.join(out_dir, f"{name}_{f[:-4]}.o")
        objs.append(o)
        procs.append(subprocess.Popen([CLANGXX] + BOUNDARY_FLAGS + sanitize + ["-x", "c++", "-c", os.path.join(CSRC, f), "-o", o], stderr=subprocess.PIPE, text=True))
    for p in procs:
        err = p.communicate()[1]
        assert p.returncode == 0, err[-3000:]
    exe = os.path.join(out_dir, name)
    subprocess.run([CLANGXX] + BOUNDARY_FLAGS + sanitize + [os.path.join(FUZZ, "tsan_queue.cpp")] + objs + ["-o", exe], check=True, capture_output=True, text=True)
    return exe


def sanitizer_env():
    env = dict(os.environ)
    env["TSAN_OPTIONS"] = "halt_on_error=0 exitcode=66"
    return env


def test_queue_under_thread_sanitizer(tmp_path):
    """10 s of 3 submitters (mixed kinds, random MINA_SUBMIT_MORE, occasional flush), a consumer on `wait`, a consumer on `poll` + the descriptor, 4 synchronous
    callers and a thread flipping merge / max_jobs / linger_us: every accepted tag completed exactly once with the stub's verdict for its bytes, MINA_ERR_FULL was
    seen and never while slots could have been free, a destroy with entries in flight returned, nothing stays allocated, and ThreadSanitizer reported nothing"""
    if not os.path.exists(CLANGXX):
        pytest.fail(f"{CLANGXX} not found: the ThreadSanitizer tier needs ROCm's clang (tests/fuzz/Makefile says why not g++)")
    exe = build(str(tmp_path), "tsan_queue", ["-fsanitize=thread"])
    r = subprocess.run([exe] + FIXTURES + ["10"], capture_output=True, text=True, timeout=600, env=sanitizer_env())
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-4000:])
    assert "ThreadSanitizer" not in r.stderr, r.stderr[-4000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(out)
    assert out["accepted"] == out["taken"] > 0 and out["missing"] == out["twice"] == out["stray"] == out["wrong"] == 0
    assert out["full"] > 0 and out["full_with_free_slots"] == 0 and out["live_allocs"] == 0


def test_queue_script_under_address_and_ub_sanitizers(tmp_path):
    """the fixed single-thread script: MINA_ERR_FULL exactly while 4 of 4 slots are held, caller buffers freed right after `submit`, zero lengths, the
    descriptor's level, `wait`'s timeout, argument errors, destroy with entries held back, shutdown on an idle queue -- no report, no leak"""
    if not os.path.exists(CLANGXX):
        pytest.fail(f"{CLANGXX} not found")
    exe = build(str(tmp_path), "asan_queue", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    # One suppression, by function: the stand-in device layer (tsan_boundary.cpp, reused unchanged) gives a view context four streams of its own, where the real
    # mb_ctx_create_view creates lane 0's only (ctx.h `is_view`): the first culprit search replaces lanes 1 .. 3 by the failed chunk's borrowed streams and the
    # stand-in's three are lost -- 3 x 4 bytes of the stub's, not of the product.  Every other leak still fails the run.
    supp = tmp_path / "lsan.supp"
    supp.write_text("leak:mb_ctx_create_view\n")
    env = sanitizer_env()
    env["LSAN_OPTIONS"] = f"suppressions={supp}:print_suppressions=0"
    r = subprocess.run([exe] + FIXTURES + ["script"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-4000:])
    assert json.loads(r.stdout.strip().splitlines()[-1]) == {"script": "ok"}
