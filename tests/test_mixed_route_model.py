"""When ONE pass of the boundary may serve the proofs of both networks (MINA_VERIFY_MIXED_NETWORK_JOB; mina_bridge_amd/csrc/net_route.h mixed_pass_allowed: one host
function, the boundary's and this test's), compiled for the host by tests/fuzz/mixed_route_twin.cpp and compared with a restatement of the rule as
include/mina_verify.h states it, over its whole domain: 2 modes x 4 readiness pairs x 3 x 3 wrap domains x 4 feature pairs x the flag (576 lines)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NETWORK = 1


def allowed_rule(mode, ready, k, aware, flag):
    """network mode, both networks ready, equal kimchi_log2, equal feature_aware, the flag set"""
    return int(bool(flag) and mode == NETWORK and all(ready) and k[0] == k[1] and bool(aware[0]) == bool(aware[1]))


def test_the_rule_equals_its_restatement_on_its_whole_domain(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    if not (cxx and os.path.exists(cxx)):
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "mixed_route_twin")
    done = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "fuzz", "mixed_route_twin.cpp"), "-o", exe], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-4000:]
    rows = [tuple(int(x) for x in line.split()) for line in run.stdout.splitlines()]
    assert len(rows) == 2 * 4 * 3 * 3 * 4 * 2 and len({r[:6] for r in rows}) == len(rows)
    for mode, r, k0, k1, fa, flag, got in rows:
        assert got == allowed_rule(mode, (r & 1, r & 2), (k0, k1), (fa & 1, fa & 2), flag), (mode, r, k0, k1, fa, flag, got)
    yes = [r for r in rows if r[6]]
    assert len(yes) == 3 * 2 and all(r[0] == NETWORK and r[1] == 3 and r[2] == r[3] and r[4] in (0, 3) and r[5] == 1 for r in yes)
    assert not any(r[6] for r in rows if r[5] == 0), "without the flag nothing differs"
