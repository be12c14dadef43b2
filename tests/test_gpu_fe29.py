"""The COMPILED 29-bit routines (fp29.cuh, ec29.cuh) on the corner inputs of their proofs, through mina_selftest_fe29 -- one routine per kernel, raw limbs back.

tools/fe29_bounds.py proves on intervals that no column leaves its accumulator; tests/test_fe29_lazy_model.py runs a Python restatement of the column loops on the worst
cases.  Neither is the code.  Here the device's limbs must EQUAL the model's (tests/fe29_model.py), limb for limb -- integer arithmetic, no tolerance -- on the rows
tests/test_fe29_rows.py shows to be legal and adversarial: a wrong operand index in one multiply-accumulate, a dropped reduction term, a raw "K p - b" limb that
underflows near its bound, a multiple of p the zero test misses -- each changes a limb on some row.  On top: the textbook congruence for every product, `kp_redundant`
arithmetic for the limb-wise forms, and for the group laws the oracle's point addition on SRS points of both curves, with every coordinate lifted to the edge of its
invariant.  Every bound is read from fe29_bounds (EC29, SPONGE, the recorded call sites); none is restated.

What this does NOT cover: each routine is compiled into a kernel of its own, so a register-allocation-dependent defect of an asm constraint inside
msm_accumulate29_kernel or pstate_hash_kernel is still seen only by the parity tests, on the values those kernels meet."""
import functools
import random

import numpy as np
import pytest

import fe29_model as M

pytestmark = pytest.mark.gpu

B, L, W, M29, R, P = M.B, M.L, M.W, M.M29, M.R, M.P
E = dict(B.EC29, **B.EC29_GENERAL)
COORDS = ("x", "y", "zz", "zzz")
INV = {"x": E["INV_X"], "y": E["INV_Y"], "zz": E["INV_ZZ"], "zzz": E["INV_ZZZ"]}
ZERO = [0] * L


def run(ctx, F, op, rows, flags=None):
    """rows: lists of up to 8 operands of 9 limbs -> (results [n][4][9] as Python integers, flag words)"""
    import mina_bridge_amd.lib as lib
    a = np.zeros((len(rows), lib.FE29_IN_WORDS), np.uint32)
    for i, r in enumerate(rows):
        r = list(r) + [ZERO] * (lib.FE29_IN_OPERANDS - len(r))
        a[i, :-1] = np.array(r, dtype=np.uint64).reshape(-1).astype(np.uint32)
    if flags is not None:
        a[:, -1] = flags
    out = ctx.selftest_fe29(F, lib.FE29_OPS[op], a)
    return out[:, :-1].reshape(len(rows), lib.FE29_OUT_RESULTS, L).tolist(), out[:, -1].tolist()


def words_value(v):
    """a result of eight 32-bit words (limbs 0..7 of its slot, limb 8 zero)"""
    assert v[8] == 0
    return sum(x << (32 * i) for i, x in enumerate(v[:8]))


@functools.lru_cache(maxsize=None)
def sites(F):
    return M.recorded_sites(F)


def site(F, prove, name):
    hit = [c for c in prove(F)[0].calls if c["site"] == name]
    assert len(hit) == 1, name
    return hit[0]


def corners(p, v, rng, count=40):
    """concrete values of a normalised recorded operand: its bound, all ones, zero, the named values that fit, random ones"""
    out = [M.at_bound(v), M.all_ones(v), M.zero(v)] + [M.limbs(x) for x in M.named_values(p) if M.within(v, x)]
    return out + [M.limbs(rng.randrange(v.vmax + 1)) for _ in range(count)] + [M.limbs(rng.randrange(min(p, v.vmax + 1))) for _ in range(count)]


# ------------------------------------------------------------------------------------------------ the generated products
@pytest.mark.parametrize("routine", sorted(M.ROUTINES))
@pytest.mark.parametrize("F", (0, 1))
def test_a_generated_product_equals_the_model_limb_for_limb_on_the_corner_rows_of_every_site_that_calls_it(ctx, F, routine):
    p = P[F]
    rows = [r for _, c in sites(F) if M.routine_of(c) == routine for r in M.site_rows(F, c)] or M.free_rows(F, routine)
    got, _ = run(ctx, F, routine, rows)
    bad = []
    for i, r in enumerate(rows):                                   # every row: none skipped
        want, _ = M.model_row(p, routine, r)
        if got[i][0] != want or M.value(got[i][0]) * R % p != M.textbook_row(p, routine, r):
            bad.append(i)
        assert got[i][1:] == [ZERO] * 3
    assert not bad, f"{routine} F={F}: {len(bad)} of {len(rows)} rows differ from the model, first {bad[0]}: device {got[bad[0]][0]}, model {M.model_row(p, routine, rows[bad[0]])[0]}"


# ------------------------------------------------------------------------------------------------ the limb-wise forms of ec29.cuh
LIMBWISE = {  # op -> (proof, recorded site): the instantiations the laws use, by the multiple's EC29:: name
    "SUB_KP_ONE": (B.prove_group_law, "p - py (first point)"), "KP_MINUS_NEG_Y": (B.prove_group_law, "-py = K p - py"), "KP_MINUS_SUB_X1": (B.prove_group_law, "K p - x1"),
    "KP_MINUS_SUB_Y1": (B.prove_group_law, "K p - y1"), "KP_MINUS_G_U1": (B.prove_group_add, "K p - u1"), "KP_MINUS_G_S1": (B.prove_group_add, "K p - s1"),
    "KP_MINUS_A_2B_X3_SUB": (B.prove_group_law, "K p - ppp - 2 q"), "KP_MINUS_A_2B_G_X3_SUB": (B.prove_group_add, "K p - ppp - 2 q (general)"),
    "ADD_KP_MINUS_SUB_X3": (B.prove_group_law, "q + K p - x3"), "ADD_KP_MINUS_G_SUB_X3": (B.prove_group_add, "q + K p - x3 (general)"),
}
MULT_NAME = {"SUB_KP_ONE": None, "KP_MINUS_NEG_Y": "NEG_Y_MULT", "KP_MINUS_SUB_X1": "SUB_X1_MULT", "KP_MINUS_SUB_Y1": "SUB_Y1_MULT", "KP_MINUS_G_U1": "G_U1_MULT", "KP_MINUS_G_S1": "G_S1_MULT",
             "KP_MINUS_A_2B_X3_SUB": "X3_SUB_MULT", "KP_MINUS_A_2B_G_X3_SUB": "G_X3_SUB_MULT", "ADD_KP_MINUS_SUB_X3": "SUB_X3_MULT", "ADD_KP_MINUS_G_SUB_X3": "G_SUB_X3_MULT"}


@pytest.mark.parametrize("op", sorted(LIMBWISE))
@pytest.mark.parametrize("F", (0, 1))
def test_a_limb_wise_difference_is_kp_redundant_arithmetic_on_the_corners_of_its_operands(ctx, F, op):
    p = P[F]
    call = site(F, *LIMBWISE[op])
    mult = call["mult"]
    assert mult == (E[MULT_NAME[op]] if MULT_NAME[op] else 1)
    rng = random.Random(f"{op}/{F}")
    cs = [corners(p, v, rng) for v in call["operands"]]
    rows = [[a] for a in cs[0]] if len(cs) == 1 else [[a, b] for a in cs[0] for b in cs[1][:3] + rng.sample(cs[1][3:], 6)] + [[a, b] for a in cs[0][:3] for b in cs[1]]
    got, _ = run(ctx, F, op, rows)
    for r, g in zip(rows, got):
        if call["kind"] == "kp_minus":
            want = M.kp_minus(p, mult, r[0])
        elif call["kind"] == "add_kp_minus":
            want = [a + k for a, k in zip(r[0], M.kp_minus(p, mult, r[1]))]
        elif call["kind"] == "kp_minus_a_minus_2b":
            want = [k - a - 2 * b for k, a, b in zip(B.kp_redundant(p, mult, 31), r[0], r[1])]
        else:
            assert call["kind"] == "sub_kp"
            want = M.limbs(M.value(r[0]) + mult * p - M.value(r[1]))                     # WITH the carry pass: normalised
        assert all(0 <= x < 1 << 32 for x in want)
        assert g[0] == want, (op, F, r)
        if call["kind"] != "sub_kp":
            assert M.value(g[0]) == M.value(want) and all(x <= m for x, m in zip(g[0], call["out"].limb))


@pytest.mark.parametrize("F", (0, 1))
def test_the_normalised_sums_and_the_word_forms(ctx, F):
    p = P[F]
    rng = random.Random(f"sums/{F}")
    # fe29_add / fe29_add3: the lane forms add rows, absorbed fields and entered salts that TOGETHER fit the state bound; every operand below the largest of them
    v = B.norm(max(B.SPONGE.values()) * p // 1000 + 1)
    cs = corners(p, v, rng, 12)
    rows = [[a, b, c] for a in cs for b in cs[:3] + rng.sample(cs, 3) for c in cs[:3] + rng.sample(cs, 2)]
    for op, n in (("ADD", 2), ("ADD3", 3)):
        got, _ = run(ctx, F, op, rows)
        for r, g in zip(rows, got):
            assert g[0] == M.limbs(sum(M.value(x) for x in r[:n])), (op, r)
    # fe29_from_words / fe29_to_words: every 256-bit word string, at the limb and the word boundaries
    xs = [0, 1, p - 1, p, p + 1, (1 << 256) - 1, 1 << 255] + [rng.getrandbits(256) for _ in range(40)]
    xs += [y for i in range(1, L) for y in ((1 << (W * i)) - 1, 1 << (W * i))] + [y for j in range(1, 8) for y in ((1 << (32 * j)) - 1, 1 << (32 * j), ((1 << 256) - 1) ^ (0xFFFFFFFF << (32 * j)))]
    rows = [[[(x >> (32 * i)) & 0xFFFFFFFF for i in range(8)] + [0]] for x in xs]
    got, _ = run(ctx, F, "WORDS", rows)
    for x, g in zip(xs, got):
        assert g[0] == M.limbs(x) and words_value(g[1]) == x, hex(x)


@pytest.mark.parametrize("F", (0, 1))
def test_the_exact_zero_test_finds_every_multiple_of_p_below_its_bound_and_nothing_beside_them(ctx, F):
    p = P[F]
    ks = list(range(E["PD_MAX"] + 1))
    ds = [1, 1 << 29, 1 << 145, 1 << 232]                                              # the list of the model's own test ...
    ds += [y for i in range(L) for y in (1 << (W * i), M29 << (W * i))]                # ... and a perturbation of every single limb
    cases = [(k, 0) for k in ks] + [(k, d) for k in ks for d in ds]
    rows = [[M.limbs(k * p + d)] for k, d in cases]
    _, flags = run(ctx, F, "IS_MULTIPLE_OF_P", rows)
    for (k, d), r, f in zip(cases, rows, flags):
        assert f == (1 if d == 0 else 0) == int(M.is_multiple_of_p(p, r[0])), (k, hex(d))


@pytest.mark.parametrize("F", (0, 1))
def test_leaving_the_29_bit_form_gives_canonical_words_for_coordinates_at_their_invariants(ctx, F):
    """fe29_leave / xyzz29_leave: a coordinate v 2^261 (lazy, up to its invariant) -> the canonical Montgomery-2^256 words of v, i.e. the integer a 2^-5 mod p"""
    p = P[F]
    rng = random.Random(f"leave/{F}")
    i32 = pow(32, -1, p)
    cs = {name: corners(p, site(F, B.prove_group_law, f"leave {name}")["pairs"][0][0], rng, 20) for name in COORDS}
    for name in COORDS:
        got, _ = run(ctx, F, "LEAVE", [[a] for a in cs[name]])
        for a, g in zip(cs[name], got):
            assert words_value(g[0]) == M.value(a) * i32 % p, (name, a)
    n = min(len(v) for v in cs.values())
    rows = [[cs[name][i] for name in COORDS] for i in range(n)]
    import mina_bridge_amd.lib as lib
    got, flags = run(ctx, F, "XYZZ_LEAVE", rows + rows[:4], flags=[0] * n + [lib.FE29_FLAG_INF] * 4)
    for r, g in zip(rows, got[:n]):
        assert [words_value(x) for x in g] == [M.value(a) * i32 % p for a in r]
    assert all(g == [ZERO] * 4 for g in got[n:]) and set(flags[n:]) == {lib.FE29_FLAG_OK | lib.FE29_FLAG_INF} and set(flags[:n]) == {lib.FE29_FLAG_OK}   # infinity: zz = 0


# ------------------------------------------------------------------------------------------------ the laws whole, on SRS points
def curve_of(F):
    return 0 if F == 0 else 1                                      # Pallas lives over Fp (field 0), Vesta over Fq


def srs_points(oracle, srs_oracle, F, count):
    g = srs_oracle[curve_of(F)][0]
    return [(oracle.le_to_int(g[i, :32]), oracle.le_to_int(g[i, 32:])) for i in range(count)]


def chord(p, a, b):
    """the affine sum of two points with different x: the formula uses neither curve coefficient, so it also serves table entries with an edge y that lie on no curve"""
    lam = (b[1] - a[1]) * pow(b[0] - a[0], -1, p) % p
    x3 = (lam * lam - a[0] - b[0]) % p
    return x3, (lam * (a[0] - x3) - a[1]) % p


def lifted(p, pt, z, ks):
    """the XYZZ image of the affine point with z, in the 2^261 domain, coordinate c lifted to v + ks[c] p (still below its invariant)"""
    v = {"x": pt[0] * z * z * R % p, "y": pt[1] * z * z * z * R % p, "zz": z * z * R % p, "zzz": z * z * z * R % p}
    assert all(ks[c] < INV[c] for c in COORDS)
    return {c: M.limbs(v[c] + ks[c] * p) for c in COORDS}


def lifts(rng):
    """k = 0, invariant - 1 and random, per coordinate"""
    yield {c: 0 for c in COORDS}
    yield {c: INV[c] - 1 for c in COORDS}
    for _ in range(2):
        yield {c: rng.randrange(INV[c]) for c in COORDS}


def affine_of(p, acc):
    return M.value(acc[0]) * pow(M.value(acc[2]), -1, p) % p, M.value(acc[1]) * pow(M.value(acc[3]), -1, p) % p


def oracle_sum(oracle, F, a, b):
    return oracle.bytes_to_point(oracle.point_add(curve_of(F), oracle.point_to_bytes(a), oracle.point_to_bytes(b)))


EDGE_Y = lambda p: [p - 1, p - 2, 1 << 254, (1 << 254) - 1, (1 << 254) - (1 << 232), (1 << 254) - (1 << 233) - 1, 1]       # test_fe29_lazy_model.py edge_y


@pytest.mark.parametrize("F", (0, 1))
def test_the_mixed_add_equals_the_model_and_the_oracle_with_every_coordinate_lifted_to_its_invariant(ctx, oracle, srs_oracle, F):
    p = P[F]
    rng = random.Random(f"madd/{F}")
    pts = srs_points(oracle, srs_oracle, F, 16)
    cases = []                                                      # (accumulator point, z, lift, table x, table y IN THE DOMAIN, the affine point added or None)
    for i in range(8):
        a, q = pts[2 * i], pts[2 * i + 1]
        for ks in lifts(rng):
            cases.append((a, rng.randrange(1, p), ks, q[0] * R % p, q[1] * R % p, q))
    for i, y in enumerate(EDGE_Y(p)):                               # table entries whose y limbs sit where ONE p under them underflows: on no curve, the chord formula is the reference
        a, q = pts[i], pts[15 - i]
        for ks in lifts(rng):
            cases.append((a, rng.randrange(1, p), ks, q[0] * R % p, y, None))
    rinv = pow(R, -1, p)
    rows, flags, ops, want_pts = [], [], [], []
    for a, z, ks, qx, y, q in cases:
        acc = lifted(p, a, z, ks)
        accl = [acc[c] for c in COORDS]
        # the y of the point ADDED in all three forms: y as it is, the normalised p - y of the pre-split table, the twin overload with neg off and on
        for op, qy, flag, sign in (("ADD_AFFINE", M.limbs(y), 0, 1), ("ADD_AFFINE", M.limbs(p - y), 0, -1), ("ADD_AFFINE_TWIN", M.limbs(y), 0, 1), ("ADD_AFFINE_TWIN", M.limbs(y), 1, -1)):
            rows.append(accl + [M.limbs(qx), qy]); flags.append(flag); ops.append(op)
            law_qy = M.kp_minus(p, E["NEG_Y_MULT"], M.limbs(y)) if (op, flag) == ("ADD_AFFINE_TWIN", 1) else qy
            added = (qx * rinv % p, sign * y * rinv % p)
            if q is not None:
                assert added[0] == q[0] and added[1] == sign * q[1] % p
            want_pts.append((acc, law_qy, a, added, q is not None))
    got = {}
    for op in ("ADD_AFFINE", "ADD_AFFINE_TWIN"):
        idx = [i for i, o in enumerate(ops) if o == op]
        res, fl = run(ctx, F, op, [rows[i] for i in idx], [flags[i] for i in idx])
        got.update({i: (res[j], fl[j]) for j, i in enumerate(idx)})
    for i, (acc, law_qy, a, added, real) in enumerate(want_pts):
        out, fl = got[i]
        want, _ = M._law(p, acc, rows[i][4], law_qy, E)
        assert fl == 1, (i, "the add reported an exceptional case")
        assert out == [want["x3"], want["y3"], want["zz"], want["zzz"]], (i, ops[i], flags[i])
        assert all(M.value(out[j]) < INV[c] * p and max(out[j][:-1]) <= M29 for j, c in enumerate(COORDS)), i          # inside the invariants again
        assert affine_of(p, out) == chord(p, a, added), i
        if real:
            assert affine_of(p, out) == oracle_sum(oracle, F, a, added), i


@pytest.mark.parametrize("F", (0, 1))
def test_the_mixed_adds_first_point_and_exceptional_cases(ctx, oracle, srs_oracle, F):
    p = P[F]
    rng = random.Random(f"madd-edge/{F}")
    pts = srs_points(oracle, srs_oracle, F, 6)
    one = M.limbs(R % p)                                           # 1 in the 2^261 domain
    # first point of a bucket (`inf` true, both signs): the accumulator becomes the point itself, -y normalised
    ys = [q[1] * R % p for q in pts] + EDGE_Y(p)
    rows = [[ZERO] * 4 + [M.limbs(pts[i % 6][0] * R % p), M.limbs(y)] for i, y in enumerate(ys) for _ in (0, 1)]
    flags = [2 | neg for _ in ys for neg in (0, 1)]
    got, fl = run(ctx, F, "ADD_AFFINE_TWIN", rows, flags)
    for r, f, g, o in zip(rows, flags, got, fl):
        y = M.value(r[5])
        assert o == 1 and g == [r[4], M.limbs(p - y) if f & 1 else r[5], one, one], (f, y)
    # Q = P and Q = -P for EVERY lift of acc.x: pd = u2 + K p - x1 is a different multiple of p each time; the add returns false and leaves the accumulator alone
    for a in pts[:3]:
        z = rng.randrange(1, p)
        rows, flags, ops, multiples = [], [], [], set()
        rest = {c: rng.randrange(INV[c]) for c in COORDS}
        for k in range(E["INV_X"]):
            ks = dict(rest, x=k)
            acc = lifted(p, a, z, ks)
            pd, _ = M.model_product(p, [(M.limbs(a[0] * R % p), acc["zz"])], lazy="sg", hi=M.kp_minus(p, E["SUB_X1_MULT"], acc["x"]))
            assert M.is_multiple_of_p(p, pd) and M.value(pd) < E["PD_MAX"] * p
            multiples.add(M.value(pd) // p)
            y = a[1] * R % p
            for op, qy, flag in (("ADD_AFFINE", M.limbs(y), 0), ("ADD_AFFINE", M.limbs(p - y), 0), ("ADD_AFFINE_TWIN", M.limbs(y), 0), ("ADD_AFFINE_TWIN", M.limbs(y), 1)):
                rows.append([acc[c] for c in COORDS] + [M.limbs(a[0] * R % p), qy]); flags.append(flag); ops.append(op)
        assert len(multiples) == E["INV_X"]
        for op in ("ADD_AFFINE", "ADD_AFFINE_TWIN"):
            idx = [i for i, o in enumerate(ops) if o == op]
            got, fl = run(ctx, F, op, [rows[i] for i in idx], [flags[i] for i in idx])
            for j, i in enumerate(idx):
                assert fl[j] == 0 and got[j] == rows[i][:4], (op, i)                    # false, and bit-identical


@pytest.mark.parametrize("F", (0, 1))
def test_the_general_add_equals_the_model_and_the_oracle_and_hands_back_equal_and_opposite_points(ctx, oracle, srs_oracle, F):
    p = P[F]
    rng = random.Random(f"add/{F}")
    pts = srs_points(oracle, srs_oracle, F, 16)
    rows, want = [], []
    for i in range(8):
        a, b = pts[2 * i], pts[2 * i + 1]
        for ka in lifts(rng):
            for kb in list(lifts(rng))[1:3]:
                A, Bb = lifted(p, a, rng.randrange(1, p), ka), lifted(p, b, rng.randrange(1, p), kb)
                rows.append([A[c] for c in COORDS] + [Bb[c] for c in COORDS]); want.append((A, Bb, a, b))
    got, fl = run(ctx, F, "XYZZ_ADD", rows)
    for i, ((A, Bb, a, b), out) in enumerate(zip(want, got)):
        w = M._general_add(p, A, Bb, E)
        assert fl[i] == 1 and out == [w["x3"], w["y3"], w["zz"], w["zzz"]], i
        assert all(M.value(out[j]) < INV[c] * p and max(out[j][:-1]) <= M29 for j, c in enumerate(COORDS)), i
        assert affine_of(p, out) == oracle_sum(oracle, F, a, b) == chord(p, a, b), i
    # equal and opposite points that carry DIFFERENT z: false, and `a` comes back untouched
    rows = []
    for a in pts[:4]:
        for sign in (1, -1):
            for ka in lifts(rng):
                A, Bb = lifted(p, a, rng.randrange(1, p), ka), lifted(p, (a[0], sign * a[1] % p), rng.randrange(1, p), list(lifts(rng))[2])
                rows.append([A[c] for c in COORDS] + [Bb[c] for c in COORDS])
    got, fl = run(ctx, F, "XYZZ_ADD", rows)
    for r, g, f in zip(rows, got, fl):
        assert f == 0 and g == r[:4]
