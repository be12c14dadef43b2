"""The digit path of the matrix-core b_poly fold (mina_bridge_amd/csrc/bpoly_mfma.cuh) restated on integers, and the inputs that put chosen digits into it.
TEST INFRASTRUCTURE ONLY.

The kernels turn every table entry into its Montgomery image (x * 2^256 mod p) BEFORE they cut it into balanced base-256 digits, so the digits of a plain value such
as 0, 1 or p - 1 are pseudo-random.  A case here therefore starts from the IMAGE it wants in a table entry and solves for the canonical challenge or weight that
produces it (`image_to_plain`; an entry that is a product of several factors is solved for its last factor).

What is restated, in the kernels' order:
  * `half_tables`:     L[e] = prod of the challenges of the set bits of e (index bits 0 .. lb - 1), H[e] = w * the same over index bits lb .. k - 1, as images;
  * `balanced_digits`: 32 digits in [-128, 127] with the carry d >= 128, as `bpoly_emit_digits`;
  * `fold_by_columns`: the int8 GEMM over the batch (one accumulator per digit pair of an (hi, lo) pair), the 63 anti-diagonal sums of every 32 x 32 tile, the
                       signed carry `v >> 8` into 17 limbs, T / 2^256 mod p from the three limb groups and the conversion out of Montgomery form.
Accumulators and column sums are int64 numpy arrays (they are bounded by 2^31 and 2^36, checked); everything after them is Python integers.

A batch is a handful of DISTINCT proofs tiled round-robin (column b holds distinct proof b % D), so a case of 2^17 - 1 proofs is D digit columns with
multiplicities, its reference is the closed form  sum_d count_d * w_d * b_poly_coefficients(chals_d)  (oracle/pasta_ref.py), and no loop runs over the batch.

`fold_by_columns` also takes deliberately wrong variants (WRONG_VARIANTS) and the stale pad columns a missing clear would leave: tests/test_bpoly_digits_model.py
shows that the named cases tell each of them from the reference, so that tests/test_gpu_bpoly_mfma_edges.py cannot pass on a kernel wrong in that way."""
import random

import numpy as np

from oracle import pasta_ref as R

MODS = {0: R.P, 1: R.Q}
MONT_R = 1 << 256
DIGITS, COLS, KALIGN = 32, 63, 128                      # BPM_DIGITS, the anti-diagonals of a tile, BPM_KALIGN
MFMA_MIN_BATCH, MFMA_END_BATCH = 256, 1 << 17          # run_bpoly_fold (api_sponge.hip): 256 <= batch < 2^17 and lb >= 1 go to the matrix cores

IMG_M128 = int.from_bytes(bytes([0x80] + [0x7F] * 30 + [0x3F]), "little")      # 0x3F7F..7F80: every raw digit 128 -> 31 digits of -128, top digit 64
IMG_P127 = int.from_bytes(bytes([0x7F] * 31 + [0x3F]), "little")               # 0x3F7F..7F7F: 31 digits of +127, top digit 63, no carry anywhere
IMG_FF = (1 << 254) - 1                                                          # 0x3FFF..FF: -1, then the carry runs through thirty 0 digits into a top digit of 64
IMG_2_254 = 1 << 254                                                             # top byte 0x40, every other digit 0
IMG_2_254_HIGH = (1 << 254) + (1 << 125)                                         # 2^254 + 2^253 is above p: the highest single extra bit that stays below it
IMG_2_254_CARRY = (1 << 254) + int.from_bytes(bytes([0x80] + [0x7F] * 14), "little")      # top byte 0x40 over a run of -128 in the low 15 digits

WRONG_VARIANTS = ("colsum_int32", "colsum_uint32", "carry_gt_128", "logical_shift", "stale_pad_columns")


def kpad_of(batch):
    return (batch + KALIGN - 1) // KALIGN * KALIGN


def takes_matrix_cores(k, batch):
    return MFMA_MIN_BATCH <= batch < MFMA_END_BATCH and k // 2 >= 1


def plain_to_image(field, x):
    return x * MONT_R % MODS[field]


def image_to_plain(field, m):
    """the canonical value whose Montgomery image is m:  m * R^-1 mod p,  R = 2^256"""
    p = MODS[field]
    assert 0 <= m < p
    return m * R.inv(MONT_R % p, p) % p


def balanced_digits(m, carry_gt_128=False):
    """the 32 digits `bpoly_emit_digits` stores for the image m: d = byte + carry (0 .. 256), carry = d >= 128, digit = (int8)(d - 256 carry).  The carry out of the
    top digit is dropped, as there: for m < p the top byte is <= 0x40 and there is none.  carry_gt_128: the wrong threshold d > 128."""
    out, carry = [], 0
    for i in range(DIGITS):
        d = ((m >> (8 * i)) & 0xFF) + carry
        carry = 1 if (d > 128 if carry_gt_128 else d >= 128) else 0
        out.append(((d - (carry << 8) + 128) & 0xFF) - 128)       # the store is an int8
    return out


def half_tables(field, k, chals, weight=None):
    """-> (L, H): the Montgomery images of the low-half and high-half product tables of one proof, as `bpoly_tables_digits_kernel` (and `bpoly_tables_kernel`)
    builds them; chals are the k canonical challenges, weight None = 1.  Index bit i of an output j = (hi << lb) + lo belongs to chals[k - 1 - i]."""
    p, lb = MODS[field], k // 2
    hb = k - lb

    def entry(acc, bits, base):
        q = 0
        while bits:
            if bits & 1:
                acc = acc * chals[k - 1 - (base + q)] % p
            bits >>= 1
            q += 1
        return plain_to_image(field, acc)

    w = 1 if weight is None else weight % p
    return [entry(1, e, 0) for e in range(1 << lb)], [entry(w, e, lb) for e in range(1 << hb)]


def digit_rows(field, k, chals, weights, carry_gt_128=False):
    """-> (Ld [D, nl * 32], Hd [D, nh * 32]) int64: row d = the digit column every batch column holding distinct proof d contributes (entry e, digit i at e * 32 + i)"""
    Ld, Hd = [], []
    for d, c in enumerate(chals):
        L, H = half_tables(field, k, c, None if weights is None else weights[d])
        Ld.append([x for m in L for x in balanced_digits(m, carry_gt_128)])
        Hd.append([x for m in H for x in balanced_digits(m, carry_gt_128)])
    return np.array(Ld, np.int64), np.array(Hd, np.int64)


def stale_pad_columns(k, batch, prev):
    """The digits a call WITHOUT the clear of the planes would find in its pad columns batch .. kpad - 1.  prev = (k, batch, Ld, Hd) of the call before it on the
    same buffers (Ld, Hd as `digit_rows`, that batch tiled round-robin): a plane buffer is flat, row r column b at byte r * kpad + b, so with another kpad the bytes
    under the new pad columns are digits of other rows and columns of the previous call.  Bytes past the previous call's planes count as zero.
    -> (Ls [kpad - batch, nl * 32], Hs [kpad - batch, nh * 32])"""
    pk, pbatch, pLd, pHd = prev
    kpad, pkpad = kpad_of(batch), kpad_of(pbatch)
    out = []
    for rows, prows, pd in ((DIGITS << (k // 2), DIGITS << (pk // 2), pLd), (DIGITS << (k - k // 2), DIGITS << (pk - pk // 2), pHd)):
        off = np.arange(rows, dtype=np.int64)[None, :] * kpad + np.arange(batch, kpad, dtype=np.int64)[:, None]
        pr, pb = off // pkpad, off % pkpad
        ok = (pr < prows) & (pb < pbatch)
        out.append(np.where(ok, pd[np.where(ok, pb, 0) % len(pd), np.where(ok, pr, 0)], 0))
    return out[0], out[1]


def fold_by_columns(field, k, chals, weights, counts=None, variant=None, prev=None):
    """The matrix-core fold of a batch in which distinct proof d (chals[d]: k canonical integers, weights[d] or None = 1) stands in counts[d] columns (None: one
    each) -> (out [2^k] canonical integers, largest |accumulator|, largest |column sum|).
    variant: None, or one of WRONG_VARIANTS; "stale_pad_columns" needs prev = (k, batch, chals, weights) of the call before it, both batches tiled round-robin."""
    assert variant is None or variant in WRONG_VARIANTS
    p, lb = MODS[field], k // 2
    nl, nh = 1 << lb, 1 << (k - lb)
    cnt = np.ones(len(chals), np.int64) if counts is None else np.array(counts, np.int64)
    Ld, Hd = digit_rows(field, k, chals, weights, variant == "carry_gt_128")
    if variant == "stale_pad_columns":
        pk, pbatch, pchals, pweights = prev
        Ls, Hs = stale_pad_columns(k, int(cnt.sum()), (pk, pbatch) + digit_rows(field, pk, pchals, pweights))
        Ld, Hd, cnt = np.concatenate([Ld, Ls]), np.concatenate([Hd, Hs]), np.concatenate([cnt, np.ones(len(Ls), np.int64)])
    assert int(cnt.sum()) <= 1 << 20 and np.abs(Ld).max() <= 128 and np.abs(Hd).max() <= 128        # |accumulator| <= 2^34: int64 is exact
    # the int8 GEMM: acc[(hi, a)][(lo, c)] = sum over the batch of Hd[(hi, a)] * Ld[(lo, c)]
    acc = (Hd * cnt[:, None]).T @ Ld
    max_acc = int(np.abs(acc).max())
    # the epilogue: 63 anti-diagonal sums a + c of every (hi, lo) tile
    acc4 = acc.reshape(nh, DIGITS, nl, DIGITS)
    cs = np.zeros((nh, nl, COLS), np.int64)
    for a in range(DIGITS):
        cs[:, :, a:a + DIGITS] += acc4[:, a, :, :]
    max_col = int(np.abs(cs).max())
    if variant == "colsum_int32":
        cs = ((cs + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)
    elif variant == "colsum_uint32":
        cs = cs & 0xFFFFFFFF
    # `bpoly_colsum_reduce_kernel`: signed columns -> 17 limbs -> T / R mod p = t0 / R + t1 + t2 R -> out of Montgomery form
    rinv, mask = R.inv(MONT_R % p, p), MONT_R - 1
    out = [0] * (1 << k)
    for hi in range(nh):
        for lo in range(nl):
            col = [int(x) for x in cs[hi, lo]]
            T, carry = 0, 0
            for i in range(68):
                v = (col[i] if i < COLS else 0) + carry
                T |= (v & 0xFF) << (8 * i)
                carry = (v & ((1 << 64) - 1)) >> 8 if variant == "logical_shift" else v >> 8
            if variant is None:
                assert carry == 0 and T == sum(c << (8 * i) for i, c in enumerate(col)), "the columns of a sum of products: T >= 0 and below 2^544"
            t0, t1, t2 = T & mask, (T >> 256) & mask, T >> 512
            out[(hi << lb) + lo] = (t0 * rinv + t1 + t2 * MONT_R) * rinv % p
    return out, max_acc, max_col


# ------------------------------------------------------------------------------------------------ references
def closed_form(field, k, chals, weights, counts=None):
    """sum_d counts[d] * weights[d] * b_poly_coefficients(chals[d]) mod p"""
    p = MODS[field]
    out = [0] * (1 << k)
    for d, c in enumerate(chals):
        f = (1 if counts is None else counts[d]) * (1 if weights is None else weights[d])
        for j, s in enumerate(R.b_poly_coefficients(c, p)):
            out[j] = (out[j] + f * s) % p
    return out


def tile_counts(batch, ndistinct):
    """how many of the columns 0 .. batch - 1 hold distinct proof d = column % ndistinct"""
    return [(batch - d + ndistinct - 1) // ndistinct for d in range(ndistinct)]


def to_le(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), np.uint8).reshape(-1, 32)


def tile_inputs(k, batch, chals, weights):
    """the byte arrays of the batch for `b_poly_fold`: chals [batch * k, 32], weights [batch, 32] or None -- numpy tiling of the distinct proofs"""
    D = len(chals)
    reps = (batch + D - 1) // D
    c = np.tile(to_le([x for c in chals for x in c]).reshape(D, k * 32), (reps, 1))[:batch]
    w = None if weights is None else np.ascontiguousarray(np.tile(to_le(weights), (reps, 1))[:batch])
    return np.ascontiguousarray(c).reshape(batch * k, 32), w


# ------------------------------------------------------------------------------------------------ the named cases
def _rand(rng, p):
    return rng.randrange(1, p)


def _random_proof(field, k, rng):
    p = MODS[field]
    return [_rand(rng, p) for _ in range(k)], _rand(rng, p)


def _pinned_proof(field, k, rng, img_l, img_h, how):
    """one proof whose tables hold the image img_l in L[nl - 1] and img_h in H[nh - 1] (and in more entries, by `how`):
      "direct":      w = plain(img_h) and every high challenge 1: ALL of H is img_h;  the challenge of index bit 0 = plain(img_l), the other low ones 1: every odd
                     entry of L is img_l (L[0] is the image of 1 whatever the input, and the even entries are products without that challenge);
      "last_chal":   random weight and challenges, the challenge of the top index bit of each half solved for;
      "weight":      random challenges, the top low challenge and the WEIGHT solved for."""
    p, lb = MODS[field], k // 2
    hb = k - lb
    chals = [None] * k
    lo_idx, hi_idx = [k - 1 - q for q in range(lb)], [k - 1 - (lb + q) for q in range(hb)]
    pl, ph = image_to_plain(field, img_l), image_to_plain(field, img_h)
    if how == "direct":
        for i in lo_idx[1:] + hi_idx:
            chals[i] = 1
        if lb:
            chals[lo_idx[0]] = pl
        return chals, ph
    for i in lo_idx[:-1] + hi_idx[:-1]:
        chals[i] = _rand(rng, p)
    if lb:
        prod = 1
        for i in lo_idx[:-1]:
            prod = prod * chals[i] % p
        chals[lo_idx[-1]] = pl * R.inv(prod, p) % p
    prod = 1
    for i in hi_idx[:-1]:
        prod = prod * chals[i] % p
    if how == "last_chal":
        w = _rand(rng, p)
        chals[hi_idx[-1]] = ph * R.inv(w * prod % p, p) % p
    else:
        chals[hi_idx[-1]] = _rand(rng, p)
        w = ph * R.inv(prod * chals[hi_idx[-1]] % p, p) % p
    return chals, w


HOWS = ("direct", "last_chal", "weight")


def _case_pinned(field, k, rng, img_l, img_h):
    return [_pinned_proof(field, k, rng, img_l, img_h, how) for how in HOWS]


def _case_top_byte(field, k, rng):
    imgs = [IMG_2_254, IMG_2_254_HIGH, MODS[field] - 1, IMG_2_254_CARRY]
    return [_pinned_proof(field, k, rng, imgs[i % 4], imgs[(i + 1 + i // 4) % 4], HOWS[i % 3]) for i in range(8)]


def _case_zero(field, k, rng):
    """a weight 0 (all of H is the image 0), a low and a high challenge 0 (half of that table is), both at once, and one proof without any"""
    out = []
    c, w = _random_proof(field, k, rng); out.append((c, 0))
    c, w = _random_proof(field, k, rng); c[k - 1] = 0; out.append((c, w))
    c, w = _random_proof(field, k, rng); c[0] = 0; out.append((c, w))
    c, w = _random_proof(field, k, rng); c[0] = 0; c[k - 1] = 0; out.append((c, 0))
    out.append(_random_proof(field, k, rng))
    return out


def _case_mixed(field, k, rng):
    """the images of the other cases in rotation with random proofs: 23 distinct proofs, so that a batch tiled from them has no two equal neighbours and the
    K tile of 128 columns never sees the same alignment twice"""
    imgs = [IMG_M128, IMG_P127, IMG_FF, IMG_2_254, IMG_2_254_HIGH, MODS[field] - 1, IMG_2_254_CARRY]
    out = []
    for i in range(23):
        if i % 2:
            out.append(_random_proof(field, k, rng))
        elif i == 22:
            out.append(_case_zero(field, k, rng)[1])
        else:
            out.append(_pinned_proof(field, k, rng, imgs[(i // 2) % 7], imgs[(i // 2 + 1 + i // 14) % 7], HOWS[(i // 2) % 3]))
    return out


CASES = {
    "all_minus_128": lambda f, k, rng: _case_pinned(f, k, rng, IMG_M128, IMG_M128),
    "plus_127_times_minus_128": lambda f, k, rng: _case_pinned(f, k, rng, IMG_M128, IMG_P127),       # L: -128, H: +127
    "ff_run": lambda f, k, rng: _case_pinned(f, k, rng, IMG_FF, IMG_FF),
    "top_byte_0x40": _case_top_byte,
    "zero_image": _case_zero,
    "mixed": _case_mixed,
}

# (k, batch) every named case runs at: the last batch of the matrix-core path for each tables kernel (k = 2: one entry per lane, k = 6: eight); the first batches at
# which a signed (31 B 2^14 >= 2^31) and an unsigned (>= 2^32) 32-bit column sum of all -128 digits would wrap; one column past two K tiles for every small k
CASE_RUNS = [(2, (1 << 17) - 1), (6, (1 << 17) - 1), (4, 4229), (4, 8457)] + [(k, 257) for k in (2, 3, 4, 5, 6)]


def named_case(name, field, k):
    """-> (chals [D][k], weights [D]): the distinct proofs of the case, canonical integers; the same for every call"""
    proofs, seen = [], set()
    for c, w in CASES[name](field, k, random.Random(f"{name}/{field}/{k}")):
        if (tuple(c), w) not in seen:                            # k = 1 has no low half: proofs that differ only there coincide
            seen.add((tuple(c), w))
            proofs.append((c, w))
    return [c for c, _ in proofs], [w for _, w in proofs]
