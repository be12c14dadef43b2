"""The rows tests/test_gpu_fe29.py runs the compiled 29-bit routines on (tests/fe29_model.py `site_rows`) are ADVERSARIAL and LEGAL -- shown here without a GPU.

For every product site the proofs recorded (tools/fe29_bounds.py `Prover.calls`: the mixed add, the general add, the Poseidon lane forms; both fields):
  * every operand of every row lies inside its recorded interval -- limb by limb, and the value at most vmax;
  * the model's result lies inside the site's result interval, limbs 0..7 normalised, and is the textbook field element;
  * the largest column the model sees over the site's rows is at least HALF the prover's worst column for that site -- a condition that stops easy values passing
    for corners, not a measurement (the bound row and the all-ones row alone give 0.51 at "16-lane product + rc" in Fp, ~0.73 at the single signed products,
    0.98 - 1.00 at the strict dot products).
Every bound comes from the recorded call sites; none is restated."""
import os
import re

import pytest

import fe29_model as M

ROOT = M.ROOT
SITES = {F: M.recorded_sites(F) for F in (0, 1)}
CASES = [(F, i) for F in (0, 1) for i in range(len(SITES[F]))]


@pytest.mark.parametrize("F,i", CASES, ids=[f"F{F}-{SITES[F][i][1]['site']}" for F, i in CASES])
def test_a_sites_rows_are_inside_its_intervals_and_reach_half_its_worst_column(F, i):
    p = M.P[F]
    _, call = SITES[F][i]
    routine, ops, out = M.routine_of(call), M.site_operands(call), call["out"]
    rows = M.site_rows(F, call)
    assert 2 <= len(rows) <= M.ROWS_PER_SITE
    seen = 0
    for r in rows:
        for slot, v in ops.items():
            assert all(0 <= x <= m for x, m in zip(r[slot], v.limb)), (call["site"], slot)
            assert M.value(r[slot]) <= v.vmax, (call["site"], slot)
            if v.normal:
                assert all(x <= M.M29 for x in r[slot][:-1])
        got, peak = M.model_row(p, routine, r)
        assert M.value(got) <= out.vmax and got[8] <= out.limb[8] and all(x <= M.M29 for x in got[:-1]), call["site"]
        assert M.value(got) * M.R % p == M.textbook_row(p, routine, r)
        seen = max(seen, peak)
    assert 2 * seen >= call["worst"], (call["site"], seen / call["worst"])
    assert seen <= call["worst"]                                  # ... and the prover's worst case IS an upper bound of what a legal row reaches


def test_every_generated_routine_has_rows_and_the_uncalled_ones_are_legal_for_the_model():
    """the routines no recorded site calls run on the operand generators of test_fe29_lazy_model.py: the model's own assertions (columns, top limb) hold on every row"""
    gen = M._load("gen_fe29").generated()
    emitted = set(re.findall(r"fe29_t fe29_(\w+)\(", gen))
    assert emitted == {n.lower() for n in M.ROUTINES}, "a generated routine has no row shape in tests/fe29_model.py ROUTINES"
    called = {M.routine_of(c) for F in (0, 1) for _, c in SITES[F]}
    free = sorted(set(M.ROUTINES) - called)
    assert free and called
    for F in (0, 1):
        for routine in free:
            rows = M.free_rows(F, routine)
            assert len(rows) <= M.ROWS_PER_SITE
            for r in rows:
                got, _ = M.model_row(M.P[F], routine, r)
                assert M.value(got) * M.R % M.P[F] == M.textbook_row(M.P[F], routine, r) and all(x <= M.M29 for x in got[:-1])


def test_the_op_codes_of_the_header_are_mirrored_in_python_and_cover_every_routine():
    import mina_bridge_amd.lib as lib
    hdr = open(os.path.join(ROOT, "include", "mina_verify.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define\s+MINA_FE29_(\w+)\s+(\d+)\b", hdr)}
    consts = {"IN_OPERANDS": lib.FE29_IN_OPERANDS, "OUT_RESULTS": lib.FE29_OUT_RESULTS, "FLAG_NEG": lib.FE29_FLAG_NEG, "FLAG_OK": lib.FE29_FLAG_OK, "FLAG_INF": lib.FE29_FLAG_INF}
    assert defs == dict(lib.FE29_OPS, **consts)
    assert len(set(lib.FE29_OPS.values())) == len(lib.FE29_OPS) and set(M.ROUTINES) <= set(lib.FE29_OPS)
    assert lib.FE29_IN_OPERANDS == M.SLOTS and lib.FE29_IN_WORDS == M.SLOTS * M.L + 1
    src = open(os.path.join(ROOT, "mina_bridge_amd", "csrc", "api_selftest.hip")).read()
    assert all(f"X(MINA_FE29_{name})" in src for name in lib.FE29_OPS)


def test_the_comments_the_rows_are_specified_by_quote_the_proven_constants():
    """ec29.cuh's header and the 16-lane form of sponge.cuh state their bounds in words: they must be the constants the proofs ran with"""
    e = M.B.EC29
    ec = open(os.path.join(ROOT, "mina_bridge_amd", "csrc", "ec29.cuh")).read()
    head = ec[:ec.index("#pragma once")]
    assert f"({e['INV_X']}, {e['INV_Y']}, {e['INV_ZZ']}, {e['INV_ZZZ']}:" in head and "LAZY" not in head
    assert f"{len(M.B.EC29_SIGNED)} of the nine".replace("8 of", "eight of") in head
    sp = open(os.path.join(ROOT, "mina_bridge_amd", "csrc", "sponge.cuh")).read()
    milli = M.B.SPONGE["LANES16_STATE_MILLI_P"]
    assert f"SPONGE29::LANES16_STATE_MILLI_P / 1000 = {milli / 1000:g} p" in sp and f"x < {milli / 1000:g}," in sp
