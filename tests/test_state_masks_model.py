"""The rule that composes a Proof-of-State proof's `passed` / `ran` masks (mina_bridge_amd/csrc/state_masks.h: one host/device function, the masks kernel's and
this test's), compiled for the host by tests/fuzz/state_masks_twin.cpp and compared with a restatement of the rule as include/mina_verify.h states it, over
EVERY combination of its inputs: front absent or each of its 8 values, 4 deny words, 8 section settings, the 4 per-proof bits (4608 lines)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMAT, LEDGER, CHAIN, CONSENSUS, ACCUMULATOR, KIMCHI = 1, 2, 4, 8, 16, 32


def masks_rule(front, deny, with_states, with_accumulator, with_ipa, chain, stmt, ipa_each, acc_each):
    """front: None = absent.  -> (passed, ran)"""
    ran = FORMAT
    if (front is not None and not front & FORMAT) or deny & FORMAT:
        return 0, ran
    passed = FORMAT
    if front is not None:
        ran |= LEDGER | CONSENSUS
        passed |= front & (LEDGER | CONSENSUS)
    if with_states:
        ran |= CHAIN
        passed |= CHAIN if chain else 0
    if with_accumulator:
        ran |= ACCUMULATOR
        passed |= ACCUMULATOR if acc_each else 0
    if with_ipa:
        ran |= KIMCHI
        passed |= KIMCHI if (stmt and ipa_each) else 0
    return passed & ~deny, ran


def _cxx():
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    if not (cxx and os.path.exists(cxx)):
        pytest.skip("no C++ compiler")
    return cxx


def _table(d, extra, name):
    exe = str(d / name)
    done = subprocess.run([_cxx(), "-std=c++17", "-O1", "-Wall", "-Werror", *extra, os.path.join(ROOT, "tests", "fuzz", "state_masks_twin.cpp"), "-o", exe], capture_output=True, text=True)
    if done.returncode != 0:
        return None, done.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-4000:]
    return [tuple(int(x) for x in line.split()) for line in run.stdout.splitlines()], ""


def check(rows):
    assert len(rows) == 9 * 4 * 8 * 16
    seen = set()
    for front, deny, sec, bits, passed, ran in rows:
        seen.add((front, deny, sec, bits))
        want = masks_rule(None if front < 0 else front, deny, sec & 1, sec & 2, sec & 4, bits & 1, bits & 2, bits & 4, bits & 8)
        assert (passed, ran) == want, (front, deny, sec, bits, passed, ran, want)
        assert passed & ~ran == 0                                                    # nothing passes that did not run
    assert len(seen) == len(rows)
    assert {r[0] for r in rows} == {-1, 0, 1, 2, 3, 8, 9, 10, 11} and {r[1] for r in rows} == {0, FORMAT, KIMCHI, ACCUMULATOR | CHAIN}


def test_the_rule_equals_its_restatement_on_every_input(tmp_path):
    rows, err = _table(tmp_path, [], "state_masks_twin")
    assert rows is not None, err
    check(rows)
    # what the single-proof form pins: a proof that fails FORMAT answers (0, FORMAT) whatever else is known about it
    assert all((p, r) == (0, FORMAT) for f, d, _, _, p, r in rows if (f >= 0 and not f & FORMAT) or d & FORMAT)


def test_the_rule_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    rows, err = _table(tmp_path, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "state_masks_twin_asan")
    if rows is None:
        pytest.skip("this compiler links no sanitizer runtime: " + err[-200:])
    check(rows)
