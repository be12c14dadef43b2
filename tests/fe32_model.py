"""The 8 x 32 layer (mina_bridge_amd/csrc/fp.cuh, ec.cuh, fe_inv / fe_sqrt of groupmap.cuh) as big-integer arithmetic, a column-level emulation of the generated
products, and the rows mina_selftest_fe32 is run on (tests/test_gpu_fe32.py on the device, tests/fuzz/fe32_twin.cpp on the portable forms, tests/test_fe32_rows.py).

CONTRACTS (words are 8 x u32 little-endian; p = 2^254 + t, t < 2^126; R = 2^256).  The hook checks none of them: the caller -- here, `in_contract` -- owns them.
    COND_SUB_P a            a < 2p                       -> a - p if a >= p else a
    ADD a b / DBL a         a, b < p                     -> a + b (- p if >= p): the sum is below 2p < 2^256, no carry leaves limb 7
    SUB a b / NEG b         a, b < p                     -> a - b (+ p if a < b)
    MUL / SQR / DOT2 / DOT3 / TO_MONT / FROM_MONT        sum a_i b_i < p R, operands any 256-bit words (NOT necessarily below p)
                                                         -> sum a_i b_i / R mod p, canonical: the value before the last subtraction is (sum + m p) / R < 2p
    INV a / SQRT a          a < p, Montgomery            -> a^(p-2); ark's Tonelli-Shanks root (the particular root fixes the y-sign of every SRS point) and the bool
    WORDS_CANONICAL a       any words                    -> a < p
    laws                    coordinates < p, Montgomery  -> the XYZZ words of ec.cuh's formulas (the quad forms: the same words on all four lanes)

THE GENERATED PRODUCTS, COLUMN BY COLUMN.  `product_trace` replays tools/gen_fe_mul.py's schedule -- `column_terms` and `MAX_TERMS_PER_ASM` are imported, not restated
-- on a 64-bit `acc` and a 32-bit `hi` that counts the carries out of `acc`, one asm chunk after the other, and records per column lo, mid, hi before the fold and
per chunk the value of hi at its start and the carries it added.  The EVENTS the rows must reach are read off that record (`events_of`); "routine" there means the
three generated device routines (MUL, DOT2, DOT3).  SQR, TO_MONT and FROM_MONT are fe_mul_device with a tied operand: they get the value-level families (named values,
a = 2^256 - 1, a in {p, 2p, 3p}, the pre-reduction targets the tie leaves a solution for -- SQR: a root of v 2^256 mod p, so p - 1, p + 1 and p + 2^128 always -- and
random words); their column events are not demanded.

WHERE UNCHECKED WORDS REACH A ROUTINE OTHER THAN A PRODUCT (every `load_fe` of csrc/ and the raw word loads beside them, read one by one):
    every host-supplied element goes through fe_to_mont (a product: any 256-bit value is legal) before any chain sees it -- pickles_tick_kernel (the digest),
    pickles_scalar_kernel (`EV` / `EVI`, pub_in, ft_eval1, the digest mod q), kimchi_scalar_kernel (`EV`, prev_chals, ft_eval1), load_point_mont, acct_hash_kernel,
    acct_fold_kernel and salted_hash_kernel, sponge_tape_kernel (ABSORB_FR shifts the raw words right by one -- plain integer code -- then converts),
    ipa_prepare_kernel's cip of phase 2 and its rand_base / sg_rand_base, field_mul / field_inv / field_sqrt_kernel; bpoly_colsum_reduce_kernel multiplies its
    256-bit t0, t1 by 1 and by R^2 first.  With the canonicity check beside the conversion: load_point_checked, ld_checked (kimchi_dev.cuh), ipa_prepare_kernel's
    sponge state and its `load_scalar_checked`, xyzz_eq_affine_kernel.
    Loads that reach fe_add / fe_sub / fe_is_zero WITHOUT a product in between, and why each is canonical already:
      ipa_shared_tail_kernel   fe_add over shared_sc -- written only by ipa_prepare_kernel, `store_fe` of an fe_from_mont output: below p;
      ipa_prepare_kernel, phase 2: the resumed sponge state, and ipa_to_group_kernel's t for bw_to_group -- the hand-over buffer of the split transcript, written by
                               phase 1 on the device from fe_t values of reduced routines: below p;
      the xyzz_t / affine_t buffers of the MSM, SRS and Lagrange kernels: device-produced Montgomery values (srs_create_kernel, load_point_*: product outputs).
    No host-supplied word reaches fe_add, fe_sub or fe_is_zero non-canonically; nothing to fix."""
import functools
import importlib.util
import os
import random
import re
from collections import namedtuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _load("gen_fe_mul")
P = {0: 0x40000000000000000000000000000000224698FC094CF91B992D30ED00000001, 1: 0x40000000000000000000000000000000224698FC0994A8DD8C46EB2100000001}
R, M32, M64, M128, M256 = 1 << 256, (1 << 32) - 1, (1 << 64) - 1, (1 << 128) - 1, (1 << 256) - 1
SLOTS, RESULTS, IN_WORDS, OUT_WORDS = 8, 4, 65, 33
FLAG_TRUE, FLAG_LANES_AGREE = 1, 2
FIELD_OPS = ("COND_SUB_P", "ADD", "SUB", "NEG", "DBL", "MUL", "SQR", "DOT2", "DOT3", "TO_MONT", "FROM_MONT", "INV", "SQRT", "WORDS_CANONICAL")
LAW_OPS = ("DBL_AFFINE", "XYZZ_DBL", "ADD_AFFINE", "XYZZ_ADD", "XYZZ_DBL_QUAD", "XYZZ_ADD_QUAD")
OPS = FIELD_OPS + LAW_OPS
CHAINS = ("COND_SUB_P", "ADD", "SUB", "NEG", "DBL")
PRODUCTS = ("MUL", "SQR", "DOT2", "DOT3", "TO_MONT", "FROM_MONT")
GENERATED = {"MUL": 1, "DOT2": 2, "DOT3": 3}                      # the generated device routines and their number of pairs
MAX_ROWS = 4000

Row = namedtuple("Row", "family ops")                            # ops: up to 8 integers below 2^256


def words(x):
    assert 0 <= x <= M256, hex(x)
    return [(x >> (32 * i)) & M32 for i in range(8)]


def value(w):
    return sum(int(x) << (32 * i) for i, x in enumerate(w))


def tee(p):
    """p = 2^254 + t: the four low limbs (1, p1, p2, p3)"""
    assert p >> 254 == 1 and words(p)[4:7] == [0, 0, 0]
    return p - (1 << 254)


# ------------------------------------------------------------------------------------------------ the chains, limb by limb
def chain_sub(a, b):
    """a - b over eight limbs: (difference mod 2^256, the borrow INTO each limb 0..8)"""
    aw, bw, br, out, brs = words(a), words(b), 0, [], [0]
    for i in range(8):
        t = aw[i] - bw[i] - br
        br = 1 if t < 0 else 0
        out.append(t & M32); brs.append(br)
    return value(out), brs


def chain_add(a, b):
    """a + b over eight limbs: (sum mod 2^256, the carry INTO each limb 0..8)"""
    aw, bw, c, out, cs = words(a), words(b), 0, [], [0]
    for i in range(8):
        t = aw[i] + bw[i] + c
        c = t >> 32
        out.append(t & M32); cs.append(c)
    return value(out), cs


def cond_sub_p(p, a):
    d, brs = chain_sub(a, p)
    return a if brs[8] else d


def fe_add(p, a, b):
    s, cs = chain_add(a, b)
    assert cs[8] == 0
    return cond_sub_p(p, s)


def fe_sub(p, a, b):
    d, brs = chain_sub(a, b)
    return chain_add(d, p)[0] if brs[8] else d


NAMED = lambda p: {"0": 0, "p-1": p - 1, "p": p, "p+1": p + 1, "2p-1": 2 * p - 1, "2^254": 1 << 254, "2^254-1": (1 << 254) - 1, "2^254+1": (1 << 254) + 1}


def chain_events(p, op, ops):
    """what a row of a chain reaches, named: the values of the issue's list at the operand, the intermediate sum / difference and the result, and whether the borrow
    / carry of the chain that has the literal 0 in limbs 4..6 entered limb 4 with those limbs at their transparent value (all 0 for the subtraction of p, all
    0xffffffff for the add-back of p) -- `through456` -- or found them transparent WITHOUT a borrow / carry coming -- `stops456`."""
    ev, named = set(), NAMED(p)
    a, b = ops[0], ops[1]
    if op in ("NEG",): a, b = 0, ops[0]
    if op in ("DBL",): b = a

    def csp(x):                                                   # the subtraction of p inside COND_SUB_P / ADD
        d, brs = chain_sub(x, p)
        mid = words(x)[4:7]
        for name, v in named.items():
            if x == v: ev.add(("pre", name))
        if mid == [0, 0, 0]: ev.add(("sub_p", "through456" if brs[4] else "stops456"))
        ev.add(("sub_p", "kept" if brs[8] else "subtracted"))
    if op == "COND_SUB_P":
        csp(a)
    elif op in ("ADD", "DBL"):
        s, cs = chain_add(a, b)
        for i in range(7):
            if cs[i + 1]: ev.add(("carry_out", i))
            if cs[i] and cs[i + 1] and (words(a)[i] + words(b)[i]) & M32 == M32: ev.add(("carry_propagates", i))
        csp(s)
    else:
        d, brs = chain_sub(a, b)
        for i in range(8):
            if brs[i + 1]: ev.add(("borrow_out", i))
            if brs[i] and brs[i + 1] and words(a)[i] == words(b)[i]: ev.add(("borrow_propagates", i))
        ev.add(("add_back", "yes" if brs[8] else "no"))
        if brs[8]:
            _, cs = chain_add(d, p)
            if words(d)[4:7] == [M32] * 3: ev.add(("add_back", "through456" if cs[4] else "stops456"))
            if b - a == 1: ev.add(("diff", "-1"))
        for name, v in named.items():
            if fe_sub(p, a, b) == v: ev.add(("result", name))
    if a == b: ev.add(("operands", "a==b"))
    if a == 0: ev.add(("operands", "a=0"))
    if b == 0: ev.add(("operands", "b=0"))
    x = a ^ b
    if x and x & (x - 1) == 0 or (x and sum(1 for u, v in zip(words(a), words(b)) if u != v) == 1):
        ev.add(("one_limb_differs", [u != v for u, v in zip(words(a), words(b))].index(True)))
    return ev


def chain_required(op):
    """the events every field's rows of a chain must reach"""
    pre = [("pre", n) for n in ("p-1", "p", "p+1", "0", "2p-1", "2^254", "2^254-1", "2^254+1")]
    subp = [("sub_p", x) for x in ("through456", "stops456", "kept", "subtracted")]
    if op == "COND_SUB_P":
        return pre + subp
    if op == "ADD":
        return ([e for e in pre if e[1] != "2p-1"] + subp + [("carry_out", i) for i in range(7)] + [("carry_propagates", i) for i in range(1, 7)] +
                [("operands", x) for x in ("a==b", "a=0", "b=0")] + [("one_limb_differs", i) for i in range(8)])
    if op == "DBL":                                               # 2a: the even ones of the list
        return [("pre", "0"), ("pre", "p-1"), ("pre", "p+1"), ("pre", "2^254"), ("sub_p", "kept"), ("sub_p", "subtracted"), ("sub_p", "through456"), ("sub_p", "stops456")]
    sub = [("add_back", x) for x in ("yes", "no", "through456", "stops456")] + [("result", n) for n in ("0", "p-1", "2^254", "2^254-1", "2^254+1")]
    if op == "NEG":
        return sub + [("operands", "a==b"), ("borrow_propagates", 5)]
    return (sub + [("diff", "-1")] + [("borrow_out", i) for i in range(8)] + [("borrow_propagates", i) for i in range(1, 8)] +
            [("operands", x) for x in ("a==b", "a=0", "b=0")] + [("one_limb_differs", i) for i in range(8)])


# (what `chain_required` leaves out cannot happen: 2p - 1 is no sum of two values below p -- the largest is 2p - 2 -- and p, p + 1, 2p - 1 are no results of a reduced
# routine; only COND_SUB_P meets them, as its operand)
def edge_values(p, rng):
    """values whose limbs 4..6 are all 0 or all 0xffffffff and whose low four limbs sit just below / at / just above t = (1, p1, p2, p3) and its complement, under
    every top limb that matters; the named values; single-limb values"""
    t = tee(p)
    lows = [0, 1, t - 1, t, t + 1, (1 << 128) - t - 1, (1 << 128) - t, (1 << 128) - t + 1, M128 - 1, M128, rng.getrandbits(128)]
    out = []
    for top in (0, 1, 0x3FFFFFFF, 0x40000000, 0x40000001, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xBFFFFFFF, 0xC0000000, 0xFFFFFFFF):
        for mid in (0, (1 << 96) - 1):
            out += [lo | (mid << 128) | (top << 224) for lo in lows]
    out += list(NAMED(p).values()) + [p - 2, 2 * p - 2, (p - 1) // 2, (p + 1) // 2, 1 << 253]
    out += [y for i in range(8) for y in (1 << (32 * i), M32 << (32 * i), M256 >> (32 * (7 - i)))]
    return sorted(set(out))


@functools.lru_cache(maxsize=None)
def chain_rows(F, op):
    p, rng = P[F], random.Random(f"fe32/{op}/{F}")
    ev = edge_values(p, rng)
    canon = [x for x in ev if x < p]
    rows = []
    if op == "COND_SUB_P":
        rows += [Row("edge values", [x]) for x in ev if x < 2 * p]
        rows += [Row("random", [rng.randrange(2 * p)]) for _ in range(200)]
    elif op in ("NEG", "DBL"):
        rows += [Row("edge values", [x]) for x in canon]
        rows += [Row("random", [rng.randrange(p)]) for _ in range(200)]
    elif op == "ADD":
        for s in [x for x in ev if x <= 2 * p - 2]:               # the SUM at every edge value, split in several ways
            lo, hi = max(0, s - (p - 1)), min(s, p - 1)
            for a in {lo, hi, (lo + hi) // 2, rng.randint(lo, hi)}:
                rows.append(Row("sum at an edge value", [a, s - a]))
        rows += [Row("operand edges", [a, b]) for a in (0, 1, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, 1 << 253) for b in (0, 1, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, 1 << 253)]
        for i in range(8):                                        # a pair that differs only in limb i; a carry born in limb 0 that runs up to limb i and no further
            a = rng.randrange(1 << 252) & ~(M32 << (32 * i))
            rows += [Row("one limb differs", [a, a | (1 << (32 * i))]), Row("one limb differs", [a | (M32 >> (2 if i == 7 else 0)) << (32 * i), a])]
            if i:
                rows.append(Row("carry runs to limb i", [(1 << (32 * i)) - 1, 1]))
        for i in range(1, 7):                                     # limb sums of 0xffffffff with a carry coming in: the carry propagates through limb i
            x = rng.getrandbits(32 * (i + 1)) | (1 << (32 * i - 1))
            a, b = x, (((1 << (32 * (i + 1))) - 1) ^ x) + (1 << (32 * i - 1)) + (1 << (32 * (i - 1)))
            rows.append(Row("carry propagates", [a % (1 << 250), b % (1 << 250)]))
        rows += [Row("random", [rng.randrange(p), rng.randrange(p)]) for _ in range(200)]
    else:
        assert op == "SUB"
        t = tee(p)
        for d in canon:                                           # the DIFFERENCE at every edge value, positive ...
            for b in {0, p - 1 - d, rng.randint(0, p - 1 - d)}:
                rows.append(Row("difference at an edge value", [b + d, b]))
        ks = [1, 2, t - 1, t, t + 1, M128 - 1, M128, M128 + 1, p - 1, p - 2] + [(1 << 254) - lo for lo in (0, 1, t - 1, t, t + 1)] + [1 << (32 * i) for i in range(8)]
        for k in [k for k in ks if 0 < k < p]:                    # ... and negative: a - b = -k, the add-back of p meets 2^256 - k
            for b in {k, p - 1, rng.randint(k, p - 1)}:
                rows.append(Row("negative difference", [b - k, b]))
        rows += [Row("operand edges", [a, b]) for a in (0, 1, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, 1 << 253) for b in (0, 1, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, 1 << 253)]
        for i in range(8):
            a = rng.randrange(1 << 252) & ~(M32 << (32 * i))
            rows += [Row("one limb differs", [a, a | (1 << (32 * i))]), Row("one limb differs", [a | (1 << (32 * i)), a]), Row("one limb differs", [a | (M32 >> (2 if i == 7 else 0)) << (32 * i), a])]
            if i:                                                 # equal limbs 1..i-1 under a borrow born in limb 0: it propagates, and stops at limb i
                hi_a, lo = rng.randrange(1, 1 << 20) << (32 * i), rng.getrandbits(32 * i) & ~M32
                rows.append(Row("borrow propagates", [hi_a | lo, lo | 1]))
            rows.append(Row("borrow propagates", [rng.getrandbits(224) & ~M32, rng.getrandbits(224) & ~M32 | 1]))      # a borrow born in limb 0 under random limbs
        x = rng.getrandbits(250) & ~M32
        rows.append(Row("borrow propagates", [x, x | 1]))        # every limb above 0 equal: the borrow runs to the top
        rows += [Row("random", [rng.randrange(p), rng.randrange(p)]) for _ in range(200)]
    assert all(in_contract(F, op, r.ops) for r in rows)
    return rows


# ------------------------------------------------------------------------------------------------ the generated products, column by column
_TERM = re.compile(r"^(?:([ab])(\d?)\.v\[(\d)\]|([mp])(\d))$")


def product_trace(p, pairs):
    """the schedule of tools/gen_fe_mul.py on concrete words.  -> dict(result, prered, m, cols); cols[k] = dict(lo, mid, hi, chunks=[(hi at its start, carries added)])"""
    n = len(pairs)
    aw, bw, pw, m = [words(a) for a, _ in pairs], [words(b) for _, b in pairs], words(p), [None] * 8

    def val(name):
        g = _TERM.match(name)
        assert g, name
        if g.group(1):
            return (aw if g.group(1) == "a" else bw)[int(g.group(2) or 0)][int(g.group(3))]
        return m[int(g.group(5))] if g.group(4) == "m" else pw[int(g.group(5))]
    acc, cols, r = 0, [], [0] * 8
    for k in range(15):
        terms, hi, chunks = G.column_terms(k, n), 0, []
        for c0 in range(0, len(terms), G.MAX_TERMS_PER_ASM):
            start = hi
            for x, y in terms[c0:c0 + G.MAX_TERMS_PER_ASM]:
                acc += val(x) * val(y)
                hi += acc >> 64; acc &= M64
            chunks.append((start, hi - start))
        assert hi <= M32
        lo, mid = acc & M32, acc >> 32
        cols.append(dict(lo=lo, mid=mid, hi=hi, chunks=chunks))
        if k < 8:                                                 # mb_fold_shift: + m_k p_0 clears the low word and carries iff it was not zero; then >> 32
            m[k] = -lo & M32
            nlo = mid + (1 if lo else 0)
            nhi = hi + (nlo >> 32)
            assert nhi <= M32
            acc = (nhi << 32) | (nlo & M32)
        else:
            r[k - 8] = lo
            acc = mid | (hi << 32)
    assert acc <= M32
    r[7] = acc
    pre = value(r)
    assert pre * R == sum(a * b for a, b in pairs) + value(m) * p and pre < 2 * p          # the emulation IS Montgomery's identity
    return dict(result=cond_sub_p(p, pre), prered=pre, m=value(m), cols=cols)


def mont(p, pairs):
    return sum(a * b for a, b in pairs) * pow(R, -1, p) % p


def op_pairs(F, op, ops):
    p = P[F]
    if op == "MUL": return [(ops[0], ops[1])]
    if op == "SQR": return [(ops[0], ops[0])]
    if op == "DOT2": return [(ops[0], ops[1]), (ops[2], ops[3])]
    if op == "DOT3": return [(ops[0], ops[1]), (ops[2], ops[3]), (ops[4], ops[5])]
    if op == "TO_MONT": return [(ops[0], R * R % p)]
    assert op == "FROM_MONT"
    return [(ops[0], 1)]


# p - 2^254 = t, factored (the test re-multiplies the primes and Miller-Rabin-tests each): what `mul_family_peak` enumerates divisors from
T_FACTORS = {0: {3: 2, 41956983792049: 1, 120653508039540541869833: 1}, 1: {3: 1, 29: 1, 140381: 1, 3730432093505987426119307858579: 1}}


@functools.lru_cache(maxsize=None)
def mul_family_peak(F):
    """THE LARGEST PRE-REDUCTION VALUE OF A SINGLE PRODUCT -- what is known, and the row that stands for it.  -> (v, a, b)
    r 2^256 = a b + m p with a b < p 2^256 and m <= 2^256 - 1 gives r <= 2p - 1; a dot product reaches 2p - 1 itself (see product_rows).  For ONE product, write
    v = 2p - 1 - d and m = 2^256 - j: v is reached iff (p - 1 - d) 2^256 + j p is a product of two words for some j >= 1 -- for a general pair (a, b) that asks for a
    divisor of a 510-bit number inside [p, 2^256), which no argument decides and no search here can (heuristically such pairs exist for almost every d: about 12 d of
    them), so the true supremum is not known.  What CAN be settled is the family with an operand next to the top, a = 2^256 - c, b = p - e with c e < 2^254: there
        (c + j) / 4 - s = (c e - (c + j) t) / 2^256     for the integer s = 1 + d - e,
    the left side is a multiple of 1/4 and the right side is smaller than 1/4, so both are 0: c + j = 4 s, c e = 4 s t and d = s - 1 + e with e | 4 s t, e > t.
    The smallest s for a given e is e / gcd(e, 4t); for g = gcd(e, 4t), q = 4t / g the smallest e above t is g (floor(q / 4) + 1).  The minimum of d over the
    divisors q of 4t is therefore the family's exact optimum -- d = t + about 2^75 (Fp), t + about 2^100 (Fq) -- and the value is ABOVE 2^255 = 2p - 2t: the recipe of
    `solve_prered` stops near 7p/4 only because its window for m gets narrower than b, not because nothing lies beyond.  The event ('prered', 'peak') of MUL is THIS
    value, exactly; the rows' largest pre-reduction value is asserted to be it (tests/test_fe32_rows.py)."""
    from math import gcd
    p = P[F]
    t, divs = tee(p), [1]
    for q, e in list(T_FACTORS[F].items()) + [(2, 2)]:
        divs = [d * q ** i for d in divs for i in range(e + 1)]
    best = None
    for q in sorted(divs):
        e = (4 * t // q) * (q // 4 + 1)
        s = e // gcd(e, 4 * t)
        if best is None or e - 1 + s < best[0]: best = (e - 1 + s, e, s)
    d, e, s = best
    c = 4 * s * t // e
    assert c * e == 4 * s * t and 1 <= c < 4 * s and t < d <= 2 * t and c * e < 1 << 254
    return 2 * p - 1 - d, R - c, p - e


PRERED = lambda p: {"p-1": p - 1, "p": p, "p+1": p + 1, "2^254": 1 << 254, "2^254+1": (1 << 254) + 1, "p+2^128": p + (1 << 128)}


@functools.lru_cache(maxsize=None)
def hi_floor(routine, F, k):
    """the carries the a.b terms ALONE cause in column k on the all-ones rows (`all_ones_operands`) -- the quotient terms and the carry from the column before only add
    to it.  NOT a proof of `the largest hi the contract allows`: in columns 0..6 the a.b part is the largest there is (every one of the column's word products is
    (2^32 - 1)^2, and the rows keep all seven low words of b at all ones), but the quotient terms m_i p_j depend on the operands and are not maximised, and in columns
    7..14 the contract ties the top words of a and b together.  The event is named for what it is: hi at the all-ones rows."""
    n = GENERATED[routine]
    best = 0
    for pairs in all_ones_operands(F, n):
        aw, bw = [words(a) for a, _ in pairs], [words(b) for _, b in pairs]
        s = sum(aw[t][i] * bw[t][k - i] for t in range(n) for i in range(8) if 0 <= k - i < 8)
        best = max(best, s >> 64)
    return best


def all_ones_operands(F, n):
    """a_i all ones; b_i the largest common b with n (2^256 - 1) b < p 2^256, and the same with its top limb one lower and every limb below it all ones (columns 0..6
    read only those)"""
    p = P[F]
    b = (p * R - 1) // (n * M256)
    b2 = ((b >> 224) - 1) << 224 | ((1 << 224) - 1)
    return [[(M256, b)] * n, [(M256, b2)] * n, [(b2, M256)] * n]


def events_of(routine, F, tr):
    """the events of the issue's table a product row reaches, from its trace"""
    p, ev = P[F], set()
    for k, c in enumerate(tr["cols"]):
        if k < 8:
            if c["lo"] == 0 and (c["mid"] or c["hi"]): ev.add(("lo0", k))
            if c["lo"] and c["mid"] == M32: ev.add(("mid_ones", k))
        for j, (start, carries) in enumerate(c["chunks"]):
            if carries: ev.add(("carry_in_chunk", k, j))
            if j and start: ev.add(("hi_set_at_chunk", k, j))
        if c["hi"] and c["hi"] >= hi_floor(routine, F, k): ev.add(("hi_at_all_ones", k))
    for name, v in PRERED(p).items():
        if tr["prered"] == v: ev.add(("prered", name))
    if tr["prered"] == (mul_family_peak(F)[0] if routine == "MUL" else 2 * p - 1): ev.add(("prered", "peak"))
    return ev


def required_events(routine):
    n = GENERATED[routine]
    ev = [("lo0", k) for k in range(8)] + [("mid_ones", k) for k in range(8)] + [("hi_at_all_ones", k) for k in range(15)]
    for k in range(15):
        nch = -(-len(G.column_terms(k, n)) // G.MAX_TERMS_PER_ASM)
        ev += [("carry_in_chunk", k, j) for j in range(nch)] + [("hi_set_at_chunk", k, j) for j in range(1, nch)]
    return ev + [("prered", name) for name in list(PRERED(P[0])) + ["peak"]]


# events NO legal row reaches, each with its argument.  FIXED: written down from the arithmetic, never computed from a run of anything.
UNREACHABLE = {
    ("MUL", ("mid_ones", 0)): "column 0 of a single product is a_0 b_0 <= (2^32 - 1)^2 = 0xfffffffe00000001 < 0xffffffff 2^32",
    ("MUL", ("carry_in_chunk", 0, 0)): "column 0 of a single product starts from acc = 0 and adds one term a_0 b_0 < 2^64: no carry leaves acc",
    ("MUL", ("hi_at_all_ones", 0)): "the same: hi is 0 in column 0 of a single product (the event needs hi != 0)",
    ("MUL", ("carry_in_chunk", 14, 0)): "column 14 holds r >> 192 with r <= 2p - 1 < 2^255 + 2^127: at most 2^63, no carry leaves acc",
    ("DOT2", ("carry_in_chunk", 14, 0)): "column 14 holds r >> 192 with r <= 2p - 1 < 2^255 + 2^127: at most 2^63, no carry leaves acc",
    ("DOT3", ("carry_in_chunk", 14, 0)): "column 14 holds r >> 192 with r <= 2p - 1 < 2^255 + 2^127: at most 2^63, no carry leaves acc",
    ("MUL", ("hi_at_all_ones", 14)): "the same: hi is 0 in column 14",
    ("DOT2", ("hi_at_all_ones", 14)): "the same: hi is 0 in column 14",
    ("DOT3", ("hi_at_all_ones", 14)): "the same: hi is 0 in column 14",
}


def solve_prered(p, v, b, extra=0):
    """the issue's recipe: a with (a b + extra + m p) = v 2^256 for the Montgomery quotient m of the row, or None.  m = (v 2^256 - extra) / p (mod b) inside
    [ceil((v 2^256 - extra - b (2^256 - 1)) / p), floor((v 2^256 - extra) / p)] and below 2^256 (then it IS the quotient: the sum is 0 mod 2^256)"""
    n = v * R - extra
    lo, hi = max(0, -(-(n - b * M256) // p)), min(n // p, M256)
    m0 = n * pow(p, -1, b) % b if b > 1 else 0
    m = lo + (m0 - lo) % b
    if m > hi:
        return None
    a = (n - m * p) // b
    assert a * b + extra + m * p == v * R and 0 <= a <= M256
    return a if a * b + extra < p * R else None


def _rand_words(rng, top=0x40000000):
    return rng.getrandbits(224) | (rng.randrange(top) << 224)


def _col_acc(p, pairs, k):
    c = product_trace(p, pairs)["cols"][k]
    return c["lo"] | (c["mid"] << 32)


def _set_word(x, i, w):
    return x & ~(M32 << (32 * i)) | (w << (32 * i))


@functools.lru_cache(maxsize=None)
def product_rows(F, op):
    p, rng = P[F], random.Random(f"fe32/{op}/{F}")
    n = {"MUL": 1, "SQR": 1, "DOT2": 2, "DOT3": 3, "TO_MONT": 1, "FROM_MONT": 1}[op]
    tied = op in ("SQR", "TO_MONT", "FROM_MONT")
    rows = []

    def add(family, pairs):
        if tied:
            ops = [pairs[0][0]]
        else:
            ops = [x for ab in pairs for x in ab]
        if in_contract(F, op, ops): rows.append(Row(family, ops))
        return in_contract(F, op, ops)
    fixed_b = {"TO_MONT": R * R % p, "FROM_MONT": 1}.get(op)
    rest = lambda: [(_rand_words(rng), _rand_words(rng)) for _ in range(n - 1)]
    zeros = [(0, 0)] * (n - 1)
    # -- value-level families
    for a in (M256, p, 2 * p, 3 * p, p - 1, p + 1, 0, 1, 1 << 255, M256 - p):
        for b in ([a] if op == "SQR" else [fixed_b] if fixed_b is not None else (p - 1, 1, 2, 0, rng.randrange(p), R % p, (p - 1) // 2)):
            fam = "a = 2^256 - 1" if a == M256 else "a in {p, 2p, 3p}" if a in (p, 2 * p, 3 * p) else "named operands"
            add(fam, [(a, b)] + zeros)
            if n > 1:
                add(fam, [(a, b // n)] + [(rng.randrange(p), rng.randrange(p) // n) for _ in range(n - 1)])
                add(fam, [(rng.randrange(p), rng.randrange(p) // n) for _ in range(n - 1)] + [(b // n, a)])
    if op == "SQR":                                               # the largest square inside the contract: a^2 < p 2^256
        import math
        top = math.isqrt(p * R - 1)
        for a in (top, top - 1, top >> 1, 1 << 254, p - 1, (1 << 255) - 1):
            add("named operands", [(a, a)])
    for pairs in all_ones_operands(F, n):
        add("hi at the all-ones rows", pairs)
        add("hi at the all-ones rows", [(b, a) for a, b in pairs])
    # -- pre-reduction values
    for name, v in PRERED(p).items():
        if op == "SQR":                                           # a^2 + m p = v 2^256: a is a square root of v 2^256 mod p (+ k p) whose quotient (v 2^256 - a^2) / p lies in [0, 2^256)
            K = field(F)
            root, ok, _ = K.sqrt(K.M(v * R % p))
            for a in ([(K.plain(root) * sg) % p + k * p for sg in (1, -1) for k in range(4)] if ok else []):
                if a <= M256 and 0 <= v * R - a * a < p * R: add("pre-reduction value", [(a, a)])
            continue
        done = 0
        for b in ([fixed_b] if fixed_b is not None else [3, 5, 64, 63, 17] if v <= (1 << 254) + 1 else [p - 1, p - 2, p - 4, p - 3]):
            for e in range(3 if n > 1 else 1):
                others = [(rng.getrandbits(120), rng.getrandbits(120)) for _ in range(n - 1)] if e else zeros
                a = solve_prered(p, v, b, sum(x * y for x, y in others))
                if a is not None and add("pre-reduction value", [(a, b)] + others): done += 1
            if done: break
    if op == "MUL":                                               # the exact optimum of the family a = 2^256 - c (`mul_family_peak`), both ways round, and its neighbours
        v, a, b = mul_family_peak(F)
        add("pre-reduction value", [(a, b)]); add("pre-reduction value", [(b, a)])
        add("pre-reduction value", [(a - 1, b)]); add("pre-reduction value", [(a + 1, b - 1)])
    if n > 1:                                                     # a dot product reaches 2p - 1 exactly: m = 2^256 - 1, the sum (2p - 1) 2^256 - m p split as a1 p + rho
        for v in (2 * p - 1, 2 * p - 2, 2 * p - 1 - rng.getrandbits(31)):
            s = v * R - M256 * p
            a1, rho = divmod(s, p)
            add("pre-reduction value", [(rho, 1), (a1, p)] + [(0, 0)] * (n - 2))
    # -- column events (the generated routines; the tied forms take what their tie leaves)
    if not tied:
        for k in range(8):
            for attempt in range(40):                             # lo == 0 with (mid, hi) != 0: a0_k from the column's low word, b0_0 odd
                pairs = [(_rand_words(rng), _rand_words(rng) | 1)] + rest()
                if n == 1 and k == 0:
                    pairs = [(_set_word(pairs[0][0], 0, rng.randrange(1, 1 << 16) << 16), _set_word(pairs[0][1], 0, (rng.randrange(1 << 15) << 17) | (1 << 16)))]
                else:
                    a0, b0 = pairs[0]
                    lo = _col_acc(p, pairs, k) & M32
                    ak = (words(a0)[k] - lo * pow(words(b0)[0], -1, 1 << 32)) & M32
                    pairs[0] = (_set_word(a0, k, ak), b0)
                if ("lo0", k) in events_of(op, F, product_trace(p, pairs)):
                    add("lo == 0 under a non-zero column", pairs)
                    break
            for attempt in range(600):                            # lo != 0 and mid == 0xffffffff: the column set to 0xffffffff80000000 with a0_k b0_0 + a0_0 b0_k, a0_0 small
                if k == 0:
                    if n == 1: break
                    pairs = [(_set_word(_rand_words(rng), 0, M32), _set_word(_rand_words(rng), 0, M32)), (_set_word(_rand_words(rng), 0, 1 << 16), _set_word(_rand_words(rng), 0, 1 << 16))] + [(_rand_words(rng) & ~M32, _rand_words(rng))] * (n - 2)
                else:
                    a00 = rng.randrange(1, 1 << 15) | 1
                    a0 = _set_word(_set_word(_rand_words(rng), 0, a00), k, 0)
                    b0 = _set_word(_set_word(_rand_words(rng), 0, rng.randrange(0xF0000000, 1 << 32) | 1), k, 0)
                    pairs = [(a0, b0)] + rest()
                    want = (0xFFFFFFFF80000000 - _col_acc(p, pairs, k)) & M64
                    if want >> 32 >= words(b0)[0]:
                        continue
                    ak = want // words(b0)[0]
                    bk = (want - ak * words(b0)[0]) // a00               # the column lands within a00 < 2^15 below 0xffffffff80000000
                    if k == 7 and (ak >= 0x40000000 or bk >= 0x40000000):      # limb 7 of an operand below p
                        continue
                    pairs[0] = (_set_word(a0, k, ak), _set_word(b0, k, bk))
                if ("mid_ones", k) in events_of(op, F, product_trace(p, pairs)):
                    add("mid == 0xffffffff over a non-zero lo", pairs)
                    break
        for _ in range(60):                                       # words near 2^32: a carry into hi at almost every term, in every chunk, and hi set when the next chunk begins
            big = lambda top: sum(rng.randrange(0xE0000000, 1 << 32) << (32 * i) for i in range(7)) | (rng.randrange(top >> 1, top) << 224)
            add("carries in every chunk", [(big(0x40000000), big(0x40000000)) for _ in range(n)])
        for _ in range(20):                                       # the carry of a late chunk ALONE: small a.b terms, so the first chunks of a multi-chunk column add none
            small = lambda: sum(rng.randrange(1 << 12) << (32 * i) for i in range(8))
            add("carry in a late chunk only", [(small(), small()) for _ in range(n)])
    for _ in range(300):
        add("random canonical", [(rng.randrange(p), fixed_b if fixed_b is not None else rng.randrange(p)) for _ in range(n)])
    for _ in range(300):                                          # any 256-bit words against what the contract leaves
        a = [rng.getrandbits(256) for _ in range(n)]
        add("random non-canonical", [(x, fixed_b if fixed_b is not None else rng.randrange((p * R - 1) // (n * x) + 1 if x else p) & M256) for x in a])
    assert len(rows) <= MAX_ROWS
    return rows


# ------------------------------------------------------------------------------------------------ inversion and ark's Tonelli-Shanks, in the Montgomery domain
class Field:
    def __init__(self, F):
        self.F, self.p = F, P[F]
        p = self.p
        self.rinv = pow(R, -1, p)
        self.one, self.r2 = R % p, R * R % p
        self.t = (p - 1) >> 32
        assert (p - 1) == self.t << 32 and self.t & 1
        self.root_plain = pow(5, self.t, p)                       # FieldK::root's plain value: a generator of the 2^32-th roots of unity
        self.root = self.root_plain * R % p
        self.consts = [self.one, self.r2, p - 2, (self.t - 1) // 2, self.root]           # what the host twin is handed: one, r2, pm2, tm1d2, root

    def mm(self, a, b):
        return a * b * self.rinv % self.p

    def M(self, x):
        return x * R % self.p

    def plain(self, x):
        return x * self.rinv % self.p

    def inv(self, a):
        return self.M(pow(self.plain(a), self.p - 2, self.p))

    def sqrt(self, a):
        """groupmap.cuh fe_sqrt == ark-ff 0.3 `SquareRootField::sqrt`, statement for statement -> (root or 0, is a square, [(kk, gap)] of the loop's passes)"""
        mm, one = self.mm, self.one
        if a == 0:
            return 0, True, []
        w = self.M(pow(self.plain(a), (self.t - 1) // 2, self.p))
        x = mm(w, a)
        b = mm(x, w)
        l = b
        for _ in range(31): l = mm(l, l)
        if l != one:
            return 0, False, []
        z, v, passes = self.root, 32, []
        while b != one:
            kk, b2k = 0, b
            while b2k != one: b2k = mm(b2k, b2k); kk += 1
            j = v - kk - 1
            passes.append((kk, j))
            w = z
            for _ in range(j): w = mm(w, w)
            z = mm(w, w)
            b = mm(b, z)
            x = mm(x, w)
            v = kk
        return x, True, passes


@functools.lru_cache(maxsize=None)
def field(F):
    return Field(F)


@functools.lru_cache(maxsize=None)
def sqrt_rows(F):
    """for every j = 0..31 squares a whose a^t has exact order 2^j -- a power of the root of unity of order 2^(j+1) times a 2^32-th-power residue -- and the
    non-residues beside them (order 2^32); 0 and 1"""
    K, rng = field(F), random.Random(f"fe32/SQRT/{F}")
    p = K.p
    rows = [Row("0 and 1", [0]), Row("0 and 1", [K.one])]
    for j in range(32):
        for rep in range(3):
            c = pow(rng.randrange(2, p), 1 << 32, p) if rep else 1                     # a 2^32-th-power residue: c^t = 1
            odd = rng.randrange(1 << 31) * 2 + 1 if rep else 1
            a = pow(K.root_plain, odd << (32 - j), p) * c % p if j else c             # root^(odd 2^(32-j)) has order 2^j and t is odd: a^t has exact order 2^j (j = 0: a^t = 1)
            assert pow(pow(a, K.t, p), 1 << j, p) == 1 and (j == 0 or pow(pow(a, K.t, p), 1 << (j - 1), p) != 1)
            rows.append(Row(f"order 2^{j}", [K.M(a)]))
        n = pow(K.root_plain, rng.randrange(1 << 31) * 2 + 1, p) * pow(rng.randrange(2, p), 1 << 32, p) % p
        assert pow(n, (p - 1) // 2, p) == p - 1
        rows.append(Row("non-residue", [K.M(n)]))
    rows += [Row("random", [rng.randrange(p)]) for _ in range(40)]
    return rows


@functools.lru_cache(maxsize=None)
def inv_rows(F):
    K, rng = field(F), random.Random(f"fe32/INV/{F}")
    p = K.p
    return [Row("named", [K.M(x)]) for x in (1, p - 1, 2, (p + 1) // 2, 0, 5)] + [Row("random", [rng.randrange(p)]) for _ in range(30)]


@functools.lru_cache(maxsize=None)
def canonical_rows(F):
    p, rng = P[F], random.Random(f"fe32/WORDS_CANONICAL/{F}")
    xs = [0, 1, p - 1, p, p + 1, M256, 2 * p, 1 << 254, (1 << 254) - 1]
    xs += [y for i in range(8) for y in (p + (1 << (32 * i)), p - (1 << (32 * i))) if 0 <= y <= M256] + [p ^ (M32 << (32 * i)) for i in range(8)]
    return [Row("around p", [x]) for x in xs] + [Row("random", [rng.getrandbits(256)]) for _ in range(60)]


# ------------------------------------------------------------------------------------------------ the group laws of ec.cuh, formula for formula
INF = (0, 0, 0, 0)


class Laws:
    def __init__(self, F):
        self.K = field(F)
        self.p = self.K.p

    def add(self, a, b): return fe_add(self.p, a, b)
    def sub(self, a, b): return fe_sub(self.p, a, b)
    def mul(self, a, b): return self.K.mm(a, b)
    def dot2(self, a, b, c, d): return mont(self.p, [(a, b), (c, d)])

    def dbl_affine(self, x, y):
        if y == 0: return INF
        A, S, M = self.add, self.sub, self.mul
        u = A(y, y); v = M(u, u); w = M(u, v); s = M(x, v); x2 = M(x, x); m = A(A(x2, x2), x2)
        x3 = S(S(M(m, m), s), s)
        return (x3, self.dot2(m, S(s, x3), w, S(0, y)), v, w)

    def dbl(self, P_):
        x, y, zz, zzz = P_
        if zz == 0 or y == 0: return INF
        x3, y3, v, w = self.dbl_affine(x, y)
        return (x3, y3, self.mul(v, zz), self.mul(w, zzz))

    def add_affine(self, acc, qx, qy):
        A, S, M = self.add, self.sub, self.mul
        x, y, zz, zzz = acc
        if zz == 0: return (qx, qy, self.K.one, self.K.one)
        pd, r = S(M(qx, zz), x), S(M(qy, zzz), y)
        if pd == 0:
            return self.dbl_affine(qx, qy) if r == 0 else INF
        pp = M(pd, pd); ppp = M(pd, pp); q = M(x, pp)
        x3 = S(S(S(M(r, r), ppp), q), q)
        return (x3, self.dot2(r, S(q, x3), S(0, y), ppp), M(zz, pp), M(zzz, ppp))

    def add_xyzz(self, acc, q):
        A, S, M = self.add, self.sub, self.mul
        if q[2] == 0: return tuple(acc)
        if acc[2] == 0: return tuple(q)
        u1, u2, s1, s2 = M(acc[0], q[2]), M(q[0], acc[2]), M(acc[1], q[3]), M(q[1], acc[3])
        pd, r = S(u2, u1), S(s2, s1)
        if pd == 0:
            return self.dbl(acc) if r == 0 else INF
        pp = M(pd, pd); ppp = M(pd, pp); qq = M(u1, pp)
        x3 = S(S(S(M(r, r), ppp), qq), qq)
        return (x3, self.dot2(r, S(qq, x3), S(0, s1), ppp), M(M(acc[2], q[2]), pp), M(M(acc[3], q[3]), ppp))

    def affine(self, P_):
        """the plain affine point of raw XYZZ words, None for infinity"""
        if P_[2] == 0: return None
        K = self.K
        x, y, zz, zzz = (K.plain(c) for c in P_)
        return x * pow(zz, -1, self.p) % self.p, y * pow(zzz, -1, self.p) % self.p


def scaled(F, pt, lam):
    """the XYZZ image (x l^2, y l^3, l^2, l^3) of a plain affine point, Montgomery words"""
    K = field(F)
    p = K.p
    return (K.M(pt[0] * lam * lam % p), K.M(pt[1] * pow(lam, 3, p) % p), K.M(lam * lam % p), K.M(pow(lam, 3, p)))


def x_zero_point(F):
    """(0, sqrt 5) where 5 is a square.  None for both fields (asserted in tests/test_fe32_rows.py): a point with x = 0 would have order 3 -- its tangent's slope
    3 x^2 / 2y is 0, so 2P = -P -- and both groups have prime order.  The issue's `doubling whose x is 0 where the curve has such a point` has no row to build."""
    K = field(F)
    y, ok, _ = K.sqrt(K.M(5))
    return (0, K.plain(y)) if ok else None


def law_rows(F, op, pts):
    """pts: plain affine SRS points of the curve over field F (at least 8).  Equal and opposite points in DIFFERENT representations, infinity on either side and on
    both, a mixed add onto a non-normalised accumulator equal or opposite to the affine point, doublings with y = 0 (no such point: the branch).  Neither curve has a point with x = 0
    (`x_zero_point`)"""
    K, rng = field(F), random.Random(f"fe32/{op}/{F}")
    p = K.p
    pts = [tuple(q) for q in pts[:8]]
    lams = lambda: (1, 2, p - 1, rng.randrange(3, p - 1))
    neg = lambda q: (q[0], (p - q[1]) % p)
    garbage_inf = lambda: (rng.randrange(p), rng.randrange(p), 0, rng.randrange(p))
    rows = []
    base = op.replace("_QUAD", "")
    if base == "DBL_AFFINE":
        rows += [Row("points", [K.M(q[0]), K.M(q[1])]) for q in pts]
        rows += [Row("y = 0", [K.M(pts[0][0]), 0]), Row("y = 0", [0, 0])]
    elif base == "XYZZ_DBL":
        rows += [Row("points", list(scaled(F, q, l))) for q in pts[:4] for l in lams()]
        rows += [Row("infinity", list(INF)), Row("infinity", list(garbage_inf())), Row("y = 0", list(scaled(F, (pts[0][0], 0), 2)))]
    elif base == "ADD_AFFINE":
        for i, a in enumerate(pts[:4]):
            q = pts[i + 4]
            for l in lams():
                rows.append(Row("different points", list(scaled(F, a, l)) + [K.M(q[0]), K.M(q[1])]))
                rows.append(Row("equal points", list(scaled(F, a, l)) + [K.M(a[0]), K.M(a[1])]))
                rows.append(Row("opposite points", list(scaled(F, a, l)) + [K.M(a[0]), K.M(p - a[1])]))
            rows.append(Row("infinity", list(INF) + [K.M(q[0]), K.M(q[1])]))
            rows.append(Row("infinity", list(garbage_inf()) + [K.M(q[0]), K.M(q[1])]))
    else:
        assert base == "XYZZ_ADD"
        for i, a in enumerate(pts[:4]):
            q = pts[i + 4]
            for l1 in lams():
                for l2 in lams():
                    rows.append(Row("different points", list(scaled(F, a, l1)) + list(scaled(F, q, l2))))
                    rows.append(Row("equal points", list(scaled(F, a, l1)) + list(scaled(F, a, l2))))
                    rows.append(Row("opposite points", list(scaled(F, a, l1)) + list(scaled(F, neg(a), l2))))
            rows.append(Row("infinity", list(INF) + list(scaled(F, q, 2))))
            rows.append(Row("infinity", list(scaled(F, a, 2)) + list(INF)))
            rows.append(Row("infinity", list(INF) + list(INF)))
            rows.append(Row("infinity", list(garbage_inf()) + list(scaled(F, q, p - 1))))
            rows.append(Row("infinity", list(scaled(F, a, p - 1)) + list(garbage_inf())))
            rows.append(Row("infinity", list(garbage_inf()) + list(garbage_inf())))
    return rows


LAW_FAMILIES = {"DBL_AFFINE": ["points", "y = 0"], "XYZZ_DBL": ["points", "infinity", "y = 0"], "ADD_AFFINE": ["different points", "equal points", "opposite points", "infinity"],
                "XYZZ_ADD": ["different points", "equal points", "opposite points", "infinity"]}
FAMILIES = {
    "COND_SUB_P": ["edge values", "random"], "NEG": ["edge values", "random"], "DBL": ["edge values", "random"],
    "ADD": ["sum at an edge value", "operand edges", "one limb differs", "carry runs to limb i", "carry propagates", "random"],
    "SUB": ["difference at an edge value", "negative difference", "operand edges", "one limb differs", "borrow propagates", "random"],
    "MUL": ["a = 2^256 - 1", "a in {p, 2p, 3p}", "named operands", "hi at the all-ones rows", "pre-reduction value", "lo == 0 under a non-zero column", "mid == 0xffffffff over a non-zero lo",
            "carries in every chunk", "carry in a late chunk only", "random canonical", "random non-canonical"],
    "SQR": ["a in {p, 2p, 3p}", "named operands", "hi at the all-ones rows", "pre-reduction value", "random canonical", "random non-canonical"],
    "TO_MONT": ["a = 2^256 - 1", "a in {p, 2p, 3p}", "named operands", "hi at the all-ones rows", "pre-reduction value", "random canonical", "random non-canonical"],
    "FROM_MONT": ["a = 2^256 - 1", "a in {p, 2p, 3p}", "named operands", "hi at the all-ones rows", "pre-reduction value", "random canonical", "random non-canonical"],
    "INV": ["named", "random"], "SQRT": ["0 and 1", "non-residue", "random"] + [f"order 2^{j}" for j in range(32)], "WORDS_CANONICAL": ["around p", "random"],
}
FAMILIES["DOT2"] = FAMILIES["DOT3"] = FAMILIES["MUL"]
for _op in LAW_OPS:
    FAMILIES[_op] = LAW_FAMILIES[_op.replace("_QUAD", "")]


def rows_of(F, op, pts=None):
    if op in CHAINS: return chain_rows(F, op)
    if op in PRODUCTS: return product_rows(F, op)
    if op == "INV": return inv_rows(F)
    if op == "SQRT": return sqrt_rows(F)
    if op == "WORDS_CANONICAL": return canonical_rows(F)
    assert pts is not None, "the laws run on SRS points"
    return law_rows(F, op, pts)


def in_contract(F, op, ops):
    p = P[F]
    if not all(0 <= x <= M256 for x in ops): return False
    if op == "COND_SUB_P": return ops[0] < 2 * p
    if op in ("ADD", "SUB"): return ops[0] < p and ops[1] < p
    if op in ("NEG", "DBL", "INV", "SQRT"): return ops[0] < p
    if op in PRODUCTS: return sum(a * b for a, b in op_pairs(F, op, ops)) < p * R
    if op == "WORDS_CANONICAL": return True
    return all(x < p for x in ops)


def expect(F, op, ops):
    """-> ([four results], out flag): the contract's answer for a row"""
    p, K = P[F], field(F)
    ops = list(ops) + [0] * (SLOTS - len(ops))
    z = [0, 0, 0]
    if op == "COND_SUB_P": return [cond_sub_p(p, ops[0])] + z, 0
    if op == "ADD": return [fe_add(p, ops[0], ops[1])] + z, 0
    if op == "SUB": return [fe_sub(p, ops[0], ops[1])] + z, 0
    if op == "NEG": return [fe_sub(p, 0, ops[0])] + z, 0
    if op == "DBL": return [fe_add(p, ops[0], ops[0])] + z, 0
    if op in PRODUCTS: return [product_trace(p, op_pairs(F, op, ops))["result"]] + z, 0
    if op == "INV": return [K.inv(ops[0])] + z, 0
    if op == "SQRT":
        x, ok, _ = K.sqrt(ops[0])
        return [x] + z, FLAG_TRUE if ok else 0
    if op == "WORDS_CANONICAL": return [0] + z, FLAG_TRUE if ops[0] < p else 0
    L = Laws(F)
    base, flag = op.replace("_QUAD", ""), FLAG_LANES_AGREE if op.endswith("_QUAD") else 0
    if base == "DBL_AFFINE": return list(L.dbl_affine(ops[0], ops[1])), flag
    if base == "XYZZ_DBL": return list(L.dbl(ops[:4])), flag
    if base == "ADD_AFFINE": return list(L.add_affine(ops[:4], ops[4], ops[5])), flag
    return list(L.add_xyzz(ops[:4], ops[4:8])), flag


def pack(rows):
    """rows -> the n x 65 word table of mina_selftest_fe32 (numpy is the caller's: a list of lists of words)"""
    out = []
    for r in rows:
        ops = list(r.ops) + [0] * (SLOTS - len(r.ops))
        out.append([w for x in ops for w in words(x)] + [0])
    return out


def unpack(table):
    """the n x 33 word table -> [([four results], flag)]"""
    return [([value(t[8 * k:8 * k + 8]) for k in range(RESULTS)], int(t[32])) for t in table]


# ------------------------------------------------------------------------------------------------ the independent references: the textbook congruence and the oracle
def srs_points(oracle, F, count=8):
    """the first SRS points of the curve over field F (Pallas over Fp, Vesta over Fq), plain affine integers, from the CPU oracle"""
    g, _ = oracle.srs_create(F, count, threads=1)
    return [(oracle.le_to_int(g[i, :32]), oracle.le_to_int(g[i, 32:])) for i in range(count)]


def check_against_references(oracle, F, op, rows, results):
    """`results` ([([four results], flag)], the model's or the device's) against what does not share the model's code: sum a_i b_i = r 2^256 (mod p) for the products,
    the oracle's (ark's) field_inv / field_sqrt, and for the laws the oracle's point_add on the normalised points"""
    p, K = P[F], field(F)
    if op in PRODUCTS:
        for r, (res, _) in zip(rows, results):
            assert res[0] < p and (res[0] * R - sum(a * b for a, b in op_pairs(F, op, r.ops))) % p == 0, (op, r)
    elif op == "INV":
        want = oracle.field_inv(F, oracle.ints_to_le([K.plain(r.ops[0]) or 1 for r in rows]))
        for r, (res, _), w in zip(rows, results, want):
            assert K.plain(res[0]) == (oracle.le_to_int(w) if r.ops[0] else 0), r
    elif op == "SQRT":
        want, ok = oracle.field_sqrt(F, oracle.ints_to_le([K.plain(r.ops[0]) for r in rows]))
        for r, (res, flag), w, o in zip(rows, results, want, ok):
            assert flag == (FLAG_TRUE if o else 0), r
            assert K.plain(res[0]) == (oracle.le_to_int(w) if o else 0), r               # ark's root, not merely a root
    elif op in LAW_OPS:
        L, base = Laws(F), op.replace("_QUAD", "")
        for r, (res, flag) in zip(rows, results):
            ops = list(r.ops) + [0] * (SLOTS - len(r.ops))
            assert flag == (FLAG_LANES_AGREE if op.endswith("_QUAD") else 0), (op, r.family, flag)
            got = L.affine(res)
            if r.family == "y = 0":                               # on no curve: the branch hands back infinity
                assert got is None
                continue
            if base == "DBL_AFFINE": a = b = (K.plain(ops[0]), K.plain(ops[1]))
            elif base == "XYZZ_DBL": a = b = L.affine(ops[:4])
            elif base == "ADD_AFFINE": a, b = L.affine(ops[:4]), (K.plain(ops[4]), K.plain(ops[5]))
            else: a, b = L.affine(ops[:4]), L.affine(ops[4:8])
            want = oracle.bytes_to_point(oracle.point_add(F, oracle.point_to_bytes(a), oracle.point_to_bytes(b)))
            assert got == want, (op, r.family)
            if r.family == "opposite points": assert got is None
            if r.family == "equal points": assert got is not None and got != a
