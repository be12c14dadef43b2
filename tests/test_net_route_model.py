"""The rule that routes a Proof-of-State proof to an index set by the network flag of its public input (mina_bridge_amd/csrc/net_route.h: one host function,
the boundary's and this test's), compiled for the host by tests/fuzz/net_route_twin.cpp and compared with a restatement of the rule as include/mina_verify.h
states it, over its WHOLE domain: 2 modes x 3 declared networks x 4 readiness pairs x 2 flags (48 lines)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGACY, NETWORK = 0, 1


def route_rule(mode, declared, ready, flag):
    """-> (set, reject).  ready: (set 0 ready, set 1 ready)"""
    if mode == NETWORK:                       # the proof's network is its flag; its set must hold a full configuration
        return (flag, 0) if ready[flag] else (0, 1)
    if declared == -1:                        # one pair, no network declared: the flag is not looked at
        return 0, 0
    return (0, 0) if flag == declared else (0, 1)


def _cxx():
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    if not (cxx and os.path.exists(cxx)):
        pytest.skip("no C++ compiler")
    return cxx


def _table(d, extra, name):
    exe = str(d / name)
    done = subprocess.run([_cxx(), "-std=c++17", "-O1", "-Wall", "-Werror", *extra, os.path.join(ROOT, "tests", "fuzz", "net_route_twin.cpp"), "-o", exe], capture_output=True, text=True)
    if done.returncode != 0:
        return None, done.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-4000:]
    return [tuple(int(x) for x in line.split()) for line in run.stdout.splitlines()], ""


def check(rows):
    assert len(rows) == 2 * 3 * 4 * 2
    assert {r[:4] for r in rows} == {(m, d, r, f) for m in (0, 1) for d in (-1, 0, 1) for r in range(4) for f in (0, 1)}
    for mode, declared, r, flag, got_set, reject in rows:
        want = route_rule(mode, declared, (r & 1, r & 2), flag)
        assert (got_set, reject) == want, (mode, declared, r, flag, got_set, reject, want)
        assert got_set in (0, 1) and (not reject or got_set == 0)


def test_the_rule_equals_its_restatement_on_its_whole_domain(tmp_path):
    rows, err = _table(tmp_path, [], "net_route_twin")
    assert rows is not None, err
    check(rows)
    legacy = [r for r in rows if r[0] == LEGACY]
    # the legacy rows are the single-pair library's rule: set 0 always; the flag matters only under a declared network, readiness never
    assert all(s == 0 for *_, s, _ in legacy)
    assert all(rej == 0 for _, d, _, _, _, rej in legacy if d == -1)
    assert all(rej == (1 if f != d else 0) for _, d, _, f, _, rej in legacy if d != -1)
    # network mode: a proof reaches the set of its own network or none
    assert all(rej or s == f for m, _, _, f, s, rej in rows if m == NETWORK)
    assert all(rej == (0 if (r >> f) & 1 else 1) for m, _, r, f, _, rej in rows if m == NETWORK)


def test_the_rule_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    rows, err = _table(tmp_path, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "net_route_twin_asan")
    if rows is None:
        pytest.skip("this compiler links no sanitizer runtime: " + err[-200:])
    check(rows)
