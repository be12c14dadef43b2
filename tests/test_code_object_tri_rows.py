"""The 3-lane permutation on the diagonal-normalised rows (sponge.cuh poseidon_rounds_tri_norm), CPU tier.

1. The lane schedule, restated on Python integers against `permute_plain` for both fields: lane e of a triple holds element e times 2^261, runs row[r][e] with
   a[0] against the NEXT lane's x^7 and a[1] against the PREVIOUS lane's, the round constant (times 2^522) inside the reduction, and round 54 on the full matrix.
   `rows1` is the model of api_sponge.hip poseidon_rows1 that tests/test_sponge_one_lane.py proves.
2. The proof (tools/fe29_bounds.py prove_sponge_rounds, "3-lane normalised") closes for both fields from the bound it states, the state enters through the strict
   `enter` product, a bound the row does not close is refused, and the generator regenerates fp29.cuh exactly with the per-lane variant of the row in it.
3. The code objects of the five transcript kernels: the round loops that run when the rows are installed hold 702 .. 704 multiply-accumulates, exactly 18
   ds_bpermute, no scratch and no matrix-core instruction, in no more VALU instructions and s_nop than the build in the tree shows plus 1 % (profiles/r09_tri_rows.md)
   -- below the 923 of the plain rounds, or the form is pointless.  The plain rounds stay beside them, one loop per permutation site, as the fallback."""
import os
import random
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mina_bridge_amd.poseidon_params as PP  # noqa: E402
import fe29_model as M  # noqa: E402
from test_sponge_one_lane import P_FP, P_FQ, permute_plain, rows1  # noqa: E402

R261 = 1 << 261


# ------------------------------------------------------------------------------------------------ 1. the lane schedule
def permute_tri_norm(s, mds, rc, p):
    """poseidon_permute_tri with the rows installed, lane by lane, on the values the lanes hold (x 2^261 mod p)"""
    rows, last, last_rc = rows1(mds, rc, p)
    rinv = pow(R261, p - 2, p)
    red = lambda t: t * rinv % p                                    # a reduction: T / 2^261
    # the tables as the device holds them: a = A 2^261, rc = d' rc 2^522
    a_dev = [[(rows[r][e][0] * R261 % p, rows[r][e][1] * R261 % p, rows[r][e][2] * R261 * R261 % p) for e in range(3)] for r in range(54)]
    last_dev = [[last[i][j] * R261 % p for j in range(3)] for i in range(3)]
    last_rc_dev = [x * R261 * R261 % p for x in last_rc]
    x = [v * R261 % p for v in s]                                   # `enter`
    for r in range(54):
        t = [red(red(red(red(v * v) ** 2) * red(v * v)) * v) for v in x]            # x^2, x^4, x^6, x^7
        nxt = []
        for e in range(3):
            en, ep = (0 if e == 2 else e + 1), (2 if e == 0 else e - 1)
            an, ap, c = a_dev[r][e]
            nxt.append((t[e] + red(an * t[en] + ap * t[ep] + c)) % p)               # fe29_row1_sg<F, true>(t, an, tn, ap, tq, rc)
        x = nxt
    t = [red(red(red(red(v * v) ** 2) * red(v * v)) * v) for v in x]
    out = []
    for e in range(3):
        en, ep = (0 if e == 2 else e + 1), (2 if e == 0 else e - 1)
        out.append(red(last_dev[e][e] * t[e] + last_dev[e][en] * t[en] + last_dev[e][ep] * t[ep] + last_rc_dev[e]))     # fe29_dot3rc_sg
    return [v * rinv % p for v in out]                             # `leave`


@pytest.mark.parametrize("field", [0, 1])
def test_the_lane_schedule_is_the_plain_permutation(field):
    p = P_FP if field == 0 else P_FQ
    rng = random.Random(31 + field)
    sets = [PP.default_params_ints(field),
            ([[rng.randrange(1, p) for _ in range(3)] for _ in range(3)], [[rng.randrange(p) for _ in range(3)] for _ in range(55)])]
    for mds, rc in sets:
        states = [[0, 0, 0], [p - 1, p - 1, p - 1], [1, 0, 0], [0, 0, 1]] + [[rng.randrange(p) for _ in range(3)] for _ in range(4)]
        for s in states:
            assert permute_tri_norm(s, mds, rc, p) == permute_plain(s, mds, rc, p)


def test_a_swapped_neighbour_order_is_not_the_permutation():
    """the falsification of the above: a[0] against the PREVIOUS lane's x^7 gives another function"""
    p = P_FP
    mds, rc = PP.default_params_ints(0)
    rows, last, last_rc = rows1(mds, rc, p)
    s = [1, 2, 3]
    for r in range(54):
        t = [pow(v, 7, p) for v in s]
        s = [(t[e] + rows[r][e][0] * t[(e + 2) % 3] + rows[r][e][1] * t[(e + 1) % 3] + rows[r][e][2]) % p for e in range(3)]
    t = [pow(v, 7, p) for v in s]
    s = [(sum(last[i][j] * t[j] for j in range(3)) + last_rc[i]) % p for i in range(3)]
    assert s != permute_plain([1, 2, 3], mds, rc, p)


# ------------------------------------------------------------------------------------------------ 2. the proof and the generator
@pytest.mark.parametrize("field", [0, 1])
def test_the_normalised_three_lane_round_is_proven(field):
    B = M.B
    p = B.P[field]
    pr, out = B.prove_sponge_rounds(field)
    n = out["lanes3n"]
    bound = B.SPONGE["LANES3N_STATE_MILLI_P"] * p // 1000
    assert n["row"].vmax <= bound and n["last_row"].vmax <= bound and n["entered"].vmax <= bound
    assert n["entered"].vmax < 1.01 * p, "the state enters through the strict product by 2^266 mod p"
    sites = {c["site"]: c for c in pr.calls}
    row = sites["3-lane normalised row + rc"]
    assert M.routine_of(row) == "ROW1_SG" and row["hi"] is sites["3-lane normalised x^7"]["out"]
    assert M.routine_of(sites["3-lane normalised last row + rc"]) == "DOT3RC_SG"
    assert sites["3-lane normalised enter: Montgomery-2^256 words x 2^266"]["mode"] is False
    assert row["worst"] < 1 << 63
    with pytest.raises(B.BoundError):
        B.prove_sponge_rounds(field, {"LANES3N_STATE_MILLI_P": 4000})      # x^7 < 2.07 p and the signed quotient's (1 p, 2 p]: a row reaches 4.1 p


def test_the_generator_round_trip_holds_and_the_per_lane_row_reads_no_scalar_constant():
    gen = M._load("gen_fe29")
    path = os.path.join(ROOT, "mina_bridge_amd", "csrc", "fp29.cuh")
    text = open(path).read()
    assert gen.rewrite(text) == text, "fp29.cuh is not what tools/gen_fe29.py --write makes"
    assert f"LANES3N_STATE_MILLI_P = {M.B.SPONGE['LANES3N_STATE_MILLI_P']};" in text
    body = text[text.index("fe29_t fe29_row1_sg("):]
    body = body[:body.index("\n}\n")]
    per_lane, uniform = body[body.index("if constexpr (PER_LANE) {"):body.index("} else {")], body[body.index("} else {"):]
    mac = lambda s: len(re.findall(r"v_mad_u64_u32", s))
    assert mac(per_lane) == mac(uniform) == 2 * 81 + 9 + 8           # two products, the round constant, x^7 into columns 9 .. 16 (its top limb is added to the last carry)
    assert not re.search(r'"s"\((a0|a1|c)\.', per_lane) and len(re.findall(r'"s"\((a0|a1|c)\.', uniform)) == 2 * 81 + 9
    sp = open(os.path.join(ROOT, "mina_bridge_amd", "csrc", "sponge.cuh")).read()
    assert "fe29_row1_sg<F, true>(t, an, tn, ap, tq, rc)" in sp
    milli = M.B.SPONGE["LANES3N_STATE_MILLI_P"]
    assert f"SPONGE29::LANES3N_STATE_MILLI_P / 1000 = {milli / 1000:g}" in sp


# ------------------------------------------------------------------------------------------------ 3. the code objects
import code_object as CO  # noqa: E402

_have_tools = os.path.exists(os.path.join(CO.LLVM_BIN, "llvm-objdump"))
# kernel -> (VALU, s_nop) of its costliest normalised round loop in the build in the tree (profiles/r09_tri_rows.md); the test allows 1 % more
BUILD = {
    "pickles_digest_kernel<3>": (852, 51),
    "pickles_tick_kernel<3>": (852, 50),
    "kimchi_fq_kernel<3>": (852, 65),
    "kimchi_fr_kernel<3>": (852, 50),
    "ipa_prepare_kernel<0, 3, 2>": (857, 50),
}
PLAIN_VALU = 923


@pytest.fixture(scope="module")
def co():
    if not _have_tools:
        pytest.skip("LLVM binutils of the ROCm toolchain not present")
    c = CO.CodeObjects()
    yield c
    c.close()


def _round_loops(co, kernel):
    """the innermost loops of a kernel that move x^7 across lanes: the 3-lane round loops"""
    loops = co.loops(kernel)
    out = []
    for (s, e) in loops:
        if any(s <= s2 and e2 <= e and (s2, e2) != (s, e) for (s2, e2) in loops):
            continue
        summ = CO.summarize(co.histogram(kernel, (s, e)))
        if summ["mac64"] >= 600 and summ["ds_bpermute"]:
            out.append(((s, e), summ))
    return out


@pytest.mark.parametrize("kernel", sorted(BUILD))
def test_transcript_kernels_run_the_normalised_round_loops(co, kernel):
    valu, nops = BUILD[kernel]
    assert valu < PLAIN_VALU
    loops = _round_loops(co, kernel)
    norm = [(sp, s) for sp, s in loops if s["mac64"] < 740]
    plain = [(sp, s) for sp, s in loops if s["mac64"] >= 740]
    print(kernel, "normalised:", sorted((s["mac64"], s["valu"], s["s_nop"]) for _, s in norm), "plain:", sorted((s["mac64"], s["valu"], s["s_nop"]) for _, s in plain))
    assert norm and len(norm) == len(plain), f"{kernel}: {len(norm)} normalised round loops beside {len(plain)} plain ones"
    for span, s in norm:
        assert 702 <= s["mac64"] <= 704, (span, s)
        assert s["ds_bpermute"] == 18 and s["scratch"] == 0 and s["mfma"] == 0, (span, s)
        assert s["valu"] <= valu * 101 // 100, (span, s)
        assert s["s_nop"] <= nops * 101 // 100, (span, s)
    for span, s in plain:
        assert 774 <= s["mac64"] <= 776 and s["ds_bpermute"] == 18 and s["scratch"] == 0, (span, s)


def test_the_kernels_left_on_the_plain_rounds_hold_no_normalised_loop(co):
    """api_ipa.hip: the first phase of the opening check (96 VGPRs beside the state hashes) and the test-facing tape interpreter keep the plain rounds alone"""
    for kernel in ("ipa_prepare_kernel<0, 3, 1>", "ipa_prepare_kernel<1, 3, 1>", "sponge_tape_kernel<0, 3>", "sponge_tape_kernel<1, 3>", "pstate_hash_kernel<0, 3>"):
        loops = _round_loops(co, kernel)
        assert loops and all(774 <= s["mac64"] <= 776 for _, s in loops), (kernel, [s["mac64"] for _, s in loops])
