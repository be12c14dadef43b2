"""The 9 x 29-bit-limb routines of fp29.cuh / ec29.cuh on Python integers, and the ROWS the compiled routines are run on.

Two halves:
  * the model: the generator's column loops (tools/gen_fe29.py `body`, `body_sg`) on a 64-bit accumulator, the limb-wise "K p - b", both group laws statement by
    statement.  tests/test_fe29_lazy_model.py checks it against the textbook formulas and against the prover's intervals; tests/test_gpu_fe29.py compares the device's
    limbs with it, limb for limb.
  * the row builder: for every call site the prover (tools/fe29_bounds.py `Prover.calls`) recorded -- the mixed add, the general add, the Poseidon lane forms, both
    fields -- concrete operands at the corners of the recorded intervals.  No bound is restated here: every maximum is read from the recorded `V`."""
import importlib.util
import os
import random

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    return mod


B = _load("fe29_bounds")
L, W, M29, R, P = B.L, B.W, B.M29, B.R, B.P


def limbs(x):
    return B.limbs_of(x)


def value(v):
    return sum(x << (W * i) for i, x in enumerate(v))


# ------------------------------------------------------------------------------------------------ the generated column loop on concrete integers
def model_product_signed(p, pairs, hi=None, c=None):
    """tools/gen_fe29.py `body_sg` on a 64-bit two's-complement accumulator: the digit of column k < 8 is the column's low word read as an int32 and SUBTRACTED against the
    prime limbs; digit 8 is (col & M29) - 2^30.  Returns (result limbs, largest |true column value| seen); asserts that the wrapped register and the true value agree
    whenever the column is shifted."""
    pl = limbs(p)
    MASK = (1 << 64) - 1
    s64 = lambda x: x - (1 << 64) if x >> 63 else x
    col, true, d, r, peak = 0, 0, [0] * L, [0] * L, 0
    for k in range(2 * L - 1):
        for a, b in pairs:
            for i in range(L):
                if 0 <= k - i < L:
                    col = (col + a[i] * b[k - i]) & MASK; true += a[i] * b[k - i]
        for j in (1, 2, 3, 4, 8):
            if 0 <= k - j < L and k - j < k:
                col = (col - d[k - j] * pl[j]) & MASK; true -= d[k - j] * pl[j]
        if hi is not None and k >= L:
            col = (col + hi[k - L]) & MASK; true += hi[k - L]
        if c is not None and k < L:
            col = (col + c[k]) & MASK; true += c[k]
        if k < L:
            lo = col & 0xFFFFFFFF
            d[k] = (lo - (1 << 32) if lo >> 31 else lo) if k < L - 1 else (lo & M29) - (1 << 30)
            col = (col - d[k]) & MASK; true -= d[k]
            assert s64(col) == true and true & M29 == 0, "the signed accumulator wrapped"
            peak = max(peak, abs(true))
            true >>= W; col = (s64(col) >> W) & MASK
        else:
            assert s64(col) == true, "the signed accumulator wrapped"
            peak = max(peak, abs(true))
            r[k - L] = true & M29
            true >>= W; col = (s64(col) >> W) & MASK
    assert true >= 0, "negative top limb"
    r[L - 1] = true + (hi[L - 1] if hi is not None else 0)
    assert peak < 1 << 63 and r[L - 1] < 1 << 32
    return r, peak


def model_product(p, pairs, lazy=False, hi=None, c=None):
    """tools/gen_fe29.py `body`: (result limbs, largest accumulator value seen); lazy = "sg": the signed-digit loop"""
    if lazy == "sg":
        return model_product_signed(p, pairs, hi=hi, c=c)
    pl = limbs(p)
    col, m, r, peak = 0, [0] * L, [0] * L, 0
    for k in range(2 * L - 1):
        for a, b in pairs:
            for i in range(L):
                if 0 <= k - i < L:
                    col += a[i] * b[k - i]
        for j in (1, 2, 3, 4, 8):
            if 0 <= k - j < L and k - j < k:
                col += m[k - j] * pl[j]
        if hi is not None and k >= L:
            col += hi[k - L]
        if c is not None and k < L:
            col += c[k]
        peak = max(peak, col)
        if k < L:
            m[k] = (-col) & (0xFFFFFFFF if lazy else M29)
            col += m[k]
            peak = max(peak, col)
            assert col & M29 == 0
            col >>= W
        else:
            r[k - L] = col & M29
            col >>= W
    r[L - 1] = col + (hi[L - 1] if hi is not None else 0)
    assert peak < 1 << 64, "a column left its 64-bit accumulator"
    assert r[L - 1] < 1 << 32
    return r, peak


def kp_minus(p, mult, b, lend=30):
    k = B.kp_redundant(p, mult, lend)
    out = [k[i] - b[i] for i in range(L)]
    assert all(0 <= x < 1 << 32 for x in out), "a limb of K p - b went negative"
    return out


def inside(v, iv):
    """concrete limbs `v` lie inside the interval the prover derived"""
    return value(v) <= iv["vmax"] and v[8] <= iv["top_limb"]


def is_multiple_of_p(p, a):
    """ec29.cuh fe29_is_multiple_of_p on concrete limbs"""
    pl = limbs(p)
    if a[5] | a[6] | a[7] | (a[8] & 0x3FFFFF): return False
    k = a[8] >> 22
    t, carry = [], 0
    for j in range(5):
        x = k * pl[j] + carry; t.append(x & M29); carry = x >> W
    return a[:5] == t and carry == 0


def _law(p, acc, qx, qy, c):
    """xyzz29_add_affine on concrete limbs (ec29.cuh, statement by statement); returns every intermediate"""
    md = lambda name: B.mode_of(name, B.EC29_LAZY, B.EC29_SIGNED)
    pd, _ = model_product(p, [(qx, acc["zz"])], lazy=md("pd"), hi=kp_minus(p, c["SUB_X1_MULT"], acc["x"]))
    r, _ = model_product(p, [(qy, acc["zzz"])], lazy=md("r"), hi=kp_minus(p, c["SUB_Y1_MULT"], acc["y"]))
    pp, _ = model_product(p, [(pd, pd)], lazy=md("pp"))
    ppp, _ = model_product(p, [(pd, pp)], lazy=md("ppp"))
    q, _ = model_product(p, [(acc["x"], pp)], lazy=md("q"))
    k = B.kp_redundant(p, c["X3_SUB_MULT"], 31)
    h = [k[i] - ppp[i] - 2 * q[i] for i in range(L)]
    assert all(0 <= x < 1 << 32 for x in h), "a limb of K p - ppp - 2 q went negative"
    x3, _ = model_product(p, [(r, r)], lazy=md("x3"), hi=h)
    k3 = kp_minus(p, c["SUB_X3_MULT"], x3)
    a = [q[i] + k3[i] for i in range(L)]
    assert all(x < 1 << 32 for x in a)
    y3, peak = model_product(p, [(r, a), (kp_minus(p, c["SUB_Y1_MULT"], acc["y"]), ppp)], lazy=md("y3"))
    zz, _ = model_product(p, [(acc["zz"], pp)], lazy=md("zz"))
    zzz, _ = model_product(p, [(acc["zzz"], ppp)], lazy=md("zzz"))
    return {"pd": pd, "r": r, "pp": pp, "ppp": ppp, "q": q, "x3": x3, "y3": y3, "zz": zz, "zzz": zzz}, peak


def _general_add(p, a, b, c):
    """xyzz29_add on concrete limbs (ec29.cuh, statement by statement): a, b accumulators {x, y, zz, zzz}; returns every intermediate"""
    md = lambda name: B.mode_of(name, B.EC29_GENERAL_LAZY, B.EC29_GENERAL_SIGNED)
    u1, _ = model_product(p, [(a["x"], b["zz"])], lazy=md("u1")); s1, _ = model_product(p, [(a["y"], b["zzz"])], lazy=md("s1"))
    pd, _ = model_product(p, [(b["x"], a["zz"])], lazy=md("pd"), hi=kp_minus(p, c["G_U1_MULT"], u1))
    r, _ = model_product(p, [(b["y"], a["zzz"])], lazy=md("r"), hi=kp_minus(p, c["G_S1_MULT"], s1))
    pp, _ = model_product(p, [(pd, pd)], lazy=md("pp")); ppp, _ = model_product(p, [(pd, pp)], lazy=md("ppp")); q, _ = model_product(p, [(u1, pp)], lazy=md("q"))
    k4 = B.kp_redundant(p, c["G_X3_SUB_MULT"], 31)
    h = [k4[i] - ppp[i] - 2 * q[i] for i in range(L)]
    assert all(0 <= x < 1 << 32 for x in h)
    x3, _ = model_product(p, [(r, r)], lazy=md("x3"), hi=h)
    k3 = kp_minus(p, c["G_SUB_X3_MULT"], x3)
    y3, _ = model_product(p, [(r, [q[i] + k3[i] for i in range(L)]), (kp_minus(p, c["G_S1_MULT"], s1), ppp)], lazy=md("y3"))
    zz12, _ = model_product(p, [(a["zz"], b["zz"])], lazy=md("zz12")); zz, _ = model_product(p, [(zz12, pp)], lazy=md("zz"))
    zzz12, _ = model_product(p, [(a["zzz"], b["zzz"])], lazy=md("zzz12")); zzz, _ = model_product(p, [(zzz12, ppp)], lazy=md("zzz"))
    return {"u1": u1, "s1": s1, "pd": pd, "r": r, "pp": pp, "ppp": ppp, "q": q, "x3": x3, "y3": y3, "zz": zz, "zzz": zzz}


# ------------------------------------------------------------------------------------------------ rows: concrete operands at the corners of the recorded intervals
# product routine -> (pairs, square, c, hi, mode): the shape mina_selftest_fe29 gives its rows (include/mina_verify.h): pair t in slots 2 t, 2 t + 1 (a square reads
# slot 0), c -- added before the reduction -- in slot 6, h / t -- added to the high half -- in slot 7
ROUTINES = {
    "MUL_ASM": (1, False, False, False, False), "SQR_ASM": (1, True, False, False, False), "DOT2_ASM": (2, False, False, False, False), "DOT3_ASM": (3, False, False, False, False),
    "SQR_HI_ASM": (1, True, False, True, False), "MUL_HI_ASM": (1, False, False, True, False),
    "MUL_LZ": (1, False, False, False, True), "SQR_LZ": (1, True, False, False, True), "MUL_HI_LZ": (1, False, False, True, True), "MULRC_LZ": (1, False, True, False, True),
    "DOT2RC_LZ": (2, False, True, False, True), "DOT3RC_LZ": (3, False, True, False, True),
    "MUL_SG": (1, False, False, False, "sg"), "SQR_SG": (1, True, False, False, "sg"), "MUL_HI_SG": (1, False, False, True, "sg"), "SQR_HI_SG": (1, True, False, True, "sg"),
    "MULRC_SG": (1, False, True, False, "sg"), "DOT2RC_SG": (2, False, True, False, "sg"), "DOT3RC_SG": (3, False, True, False, "sg"), "ROW1_SG": (2, False, True, True, "sg"),
}
SLOTS, C_SLOT, HI_SLOT = 8, 6, 7
ROWS_PER_SITE = 500


def routine_of(call):
    """the generated routine a recorded product site runs"""
    pairs = call["pairs"]
    shape = (len(pairs), len(pairs) == 1 and pairs[0][0] is pairs[0][1], call["c"] is not None, call["hi"] is not None, call["mode"])
    hit = [name for name, s in ROUTINES.items() if s == shape]
    assert len(hit) == 1, (call["site"], shape)
    return hit[0]


def model_row(p, routine, slots):
    """the model's (limbs, peak) for one row of `routine`"""
    n, sq, has_c, has_hi, mode = ROUTINES[routine]
    pairs = [(slots[2 * t], slots[2 * t] if sq else slots[2 * t + 1]) for t in range(n)]
    return model_product(p, pairs, lazy=mode, hi=slots[HI_SLOT] if has_hi else None, c=slots[C_SLOT] if has_c else None)


def textbook_row(p, routine, slots):
    """value R mod p of the result of one row: the sum of the products, plus c, plus h R"""
    n, sq, has_c, has_hi, _ = ROUTINES[routine]
    t = sum(value(slots[2 * k]) * value(slots[2 * k] if sq else slots[2 * k + 1]) for k in range(n))
    return (t + (value(slots[C_SLOT]) if has_c else 0) + (value(slots[HI_SLOT]) * R if has_hi else 0)) % p


def leaves(v):
    """the normalised operands a recorded operand is made of"""
    if v.src is None:
        return [v]
    return [x for part in v.src[1:] if isinstance(part, B.V) for x in leaves(part)]


def image(p, v, pick, raw=True, sub=False):
    """concrete limbs of the recorded operand `v`: `pick(leaf V, sub)` chooses every normalised value (sub: the leaf is a SUBTRAHEND of a raw form), the raw forms are
    their limb-wise images; a `select` (an operand that is either a normalised value or its raw negation) takes the raw side when `raw`"""
    if v.src is None:
        return pick(v, sub)
    kind = v.src[0]
    if kind == "select":
        a, b = v.src[1], v.src[2]
        side = (b if b.src is not None else a) if raw else (a if b.src is not None else b)
        return image(p, side, pick, raw, sub)
    mult = v.src[1]
    if kind == "kp_minus":
        k, b = B.kp_redundant(p, mult, v.src[2]), image(p, v.src[3], pick, raw, True)
        out = [k[i] - b[i] for i in range(L)]
    elif kind == "add_kp_minus":
        k, a, b = B.kp_redundant(p, mult, 30), image(p, v.src[2], pick, raw), image(p, v.src[3], pick, raw, True)
        out = [a[i] + k[i] - b[i] for i in range(L)]
    else:
        assert kind == "kp_minus_a_minus_2b", kind
        k, a, b = B.kp_redundant(p, mult, 31), image(p, v.src[2], pick, raw, True), image(p, v.src[3], pick, raw, True)
        out = [k[i] - a[i] - 2 * b[i] for i in range(L)]
    assert all(0 <= x < 1 << 32 for x in out), "a limb of a raw form left its register"
    return out


def within(v, x):
    """the integer x is a value the normalised operand `v` can hold"""
    return 0 <= x <= v.vmax and (x >> B.TOP) <= v.limb[8]


def at_bound(v):
    return limbs(v.vmax)


def all_ones(v):
    """limbs 0..7 all ones, limb 8 the operand's top-limb maximum -- one less where that would exceed vmax"""
    top = v.limb[8]
    if value([M29] * (L - 1) + [top]) > v.vmax:
        top -= 1
    return [M29] * (L - 1) + [top] if top >= 0 else limbs(v.vmax)


def zero(v):
    return [0] * L


def named_values(p):
    """0, 1, 2, p - 1, p, p + 1, the values around 2^254 where a canonical y meets the top limb of ONE p, and single-limb patterns with a limb at 0 or 2^29 - 1"""
    out = [0, 1, 2, p - 1, p, p + 1, 1 << 254, (1 << 254) - 1, (1 << 254) - (1 << 232), (1 << 254) - (1 << 233) - 1]
    for i in range(L):
        out.append(M29 << (W * i))                                            # one limb all ones, the others zero
        out.append(((1 << (W * L)) - 1) ^ (M29 << (W * i)))                   # one limb zero, the others all ones (clipped to the operand below)
    return out


def site_operands(call):
    """slot -> recorded operand of a product site (a square's operand once, in slot 0)"""
    n, sq, has_c, has_hi, _ = ROUTINES[routine_of(call)]
    ops = {}
    for t, (a, b) in enumerate(call["pairs"]):
        ops[2 * t] = a
        if not sq:
            ops[2 * t + 1] = b
    if has_c: ops[C_SLOT] = call["c"]
    if has_hi: ops[HI_SLOT] = call["hi"]
    return ops


def site_rows(F, call, seed=0):
    """the rows of one recorded product site: lists of SLOTS operands (9 limbs each; unused slots zero), at most ROWS_PER_SITE"""
    p = P[F]
    rng = random.Random(f"{F}/{call['site']}/{seed}")
    sq = ROUTINES[routine_of(call)][1]
    ops = site_operands(call)

    def below(v): return limbs(rng.randrange(v.vmax + 1))
    def canonical(v): return limbs(rng.randrange(min(p, v.vmax + 1)))

    def clipped(x):
        """a named value where it lies inside the operand; a pattern wider than the operand keeps its low limbs under the largest top limb that fits"""
        def pick(v):
            if within(v, x):
                return limbs(x)
            y = limbs(x)[:L - 1] + [min(x >> B.TOP, v.limb[8])]
            if value(y) > v.vmax and y[8] > 0:
                y[8] -= 1
            return y if value(y) <= v.vmax else below(v)
        return pick

    def row(picks, raw=True):
        """picks: slot -> picker, or (picker of the values, picker of the subtrahends of a raw form); a slot left out: random below vmax"""
        r = [[0] * L for _ in range(SLOTS)]
        for slot, v in ops.items():
            pk = picks.get(slot, below)
            val, subt = pk if isinstance(pk, tuple) else (pk, pk)
            r[slot] = image(p, v, lambda leaf, sub: (subt if sub else val)(leaf), raw)
        if sq:
            r[1] = list(r[0])
        return r

    # the bound row (every normalised operand at its vmax, every raw form the image of b = 0: the redundant K p limbs themselves) and the all-ones row
    rows = [row({s: (at_bound, zero) for s in ops}), row({s: (all_ones, zero) for s in ops})]
    # the raw forms: images of the subtrahend's corners, the normalised operands at the bound and all ones
    for s in [s for s, v in ops.items() if v.src is not None]:
        for corner in (at_bound, all_ones, zero):
            for rest in (at_bound, all_ones):
                for raw in (True, False):
                    rows.append(row({t: (rest, corner if t == s else zero) for t in ops}, raw))
    # the named values: in every slot in turn (the others random), and in all slots at once
    for x in named_values(p):
        rows.append(row({s: clipped(x) for s in ops}))
        for s in ops:
            rows.append(row({s: clipped(x)}, raw=rng.random() < 0.5))
    for i in range(100):
        rows.append(row({} if i % 2 else {s: canonical for s in ops}, raw=i % 4 < 2))
    assert len(rows) <= ROWS_PER_SITE
    return rows


def recorded_sites(F):
    """every product site the proofs of the mixed add, the general add and the lane forms recorded: [(prover, call)]"""
    out = []
    for prove in (B.prove_group_law, B.prove_group_add, B.prove_sponge_rounds):
        pr = prove(F)[0]
        out += [(pr, c) for c in pr.calls if c["kind"] == "product"]
    return out


def free_rows(F, routine, count=400, seed=0):
    """rows for a routine no recorded site calls: the operand generators of test_lazy_products_are_the_same_field_element_... (the largest state any lane form keeps) and of
    test_signed_digit_products_... (the high-half addend K p - x of the mixed add) -- the bounds under which the model's own assertions hold"""
    p = P[F]
    rng = random.Random(f"{F}/{routine}/{seed}")
    bound = B.SPONGE["LANES16_STATE_MILLI_P"] * p // 1000
    top = bound >> B.TOP
    extreme = [M29] * (L - 1) + [top]
    k = B.kp_redundant(p, B.EC29["SUB_X1_MULT"], 30)

    def operand():
        t = rng.random()
        if t < 0.25: return list(extreme)
        if t < 0.45: return limbs(rng.randrange(bound))
        if t < 0.55: return [rng.choice([0, M29]) for _ in range(L - 1)] + [rng.choice([0, top])]
        return limbs(rng.randrange(p))
    n, sq, has_c, has_hi, _ = ROUTINES[routine]
    rows = []
    for it in range(count):
        r = [[0] * L for _ in range(SLOTS)]
        for t in range(2 * n):
            r[t] = list(extreme) if it == 0 else operand()
        if sq: r[1] = list(r[0])
        if has_c: r[C_SLOT] = limbs(rng.randrange(p)) if rng.random() < 0.7 and it else [M29] * (L - 1) + [p >> B.TOP]
        if has_hi: r[HI_SLOT] = [k[i] - x for i, x in enumerate(limbs(rng.randrange(B.EC29["INV_X"] * p)) if it else [0] * L)]
        rows.append(r)
    return rows
