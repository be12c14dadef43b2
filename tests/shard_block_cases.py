"""Cases and references for the reduction operators of the multi-GPU exchange step (mina_field_sum_rows_dev, mina_points_sum_dev,
mina_point_records_equal_dev): seeded, deterministic, in Python integers plus the CPU oracle.  No GPU here: tests/test_shard_block_cases.py checks that
the cases are what their names say, tests/test_gpu_shard_blocks.py runs the kernels on them.

Point record: 68 bytes {x[32], y[32], u32 is_infinity}; a flag word != 0 means infinity and the coordinates are ignored."""
import random

import numpy as np

P = 0x40000000000000000000000000000000224698FC094CF91B992D30ED00000001
Q = 0x40000000000000000000000000000000224698FC0994A8DD8C46EB2100000001
FIELD_MOD = {0: P, 1: Q}
BASE_MOD = {0: P, 1: Q}              # curve 0 = Pallas over Fp, curve 1 = Vesta over Fq
SCALAR_MOD = {0: Q, 1: P}
RECORD = 68
NONUNIT_FLAG = 0x0100                # byte 65 of the record set: non-zero, not 1


def to_le(xs) -> np.ndarray:
    """integers -> [len, 32] little-endian bytes"""
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in xs), np.uint8).copy().reshape(-1, 32)


def from_le(rows) -> list:
    rows = np.ascontiguousarray(rows, np.uint8).reshape(-1, 32)
    return [int.from_bytes(r.tobytes(), "little") for r in rows]


# ------------------------------------------------------------------------------------------------ records
def rec(pt64, flag=None) -> np.ndarray:
    """64-byte affine point (zeros = infinity) -> 68-byte record"""
    pt64 = np.asarray(pt64, np.uint8).reshape(64)
    out = np.zeros(RECORD, np.uint8)
    out[:64] = pt64
    out[64:68] = np.frombuffer(int((0 if pt64.any() else 1) if flag is None else flag).to_bytes(4, "little"), np.uint8)
    return out


def garbage_coords(garbage: int) -> np.ndarray:
    """64 non-zero bytes that are canonical field elements but (x, y) on neither curve (test_shard_block_cases.py checks that)"""
    g = np.array([(garbage * 37 + i * 11) % 255 + 1 for i in range(64)], np.uint8)
    g[31] = (g[31] & 0x3F) | 1
    g[63] = (g[63] & 0x3F) | 1
    return g


def rec_inf(garbage=None, flag=1) -> np.ndarray:
    """an infinity record; `garbage` (an integer) fills the 64 coordinate bytes with a non-zero, off-curve pattern"""
    assert flag != 0
    return rec(np.zeros(64, np.uint8) if garbage is None else garbage_coords(garbage), flag=flag)


def rec_inf_nonunit(garbage=None) -> np.ndarray:
    """an infinity record whose flag word is NONUNIT_FLAG: the kernels test word != 0, not word == 1"""
    return rec_inf(garbage, flag=NONUNIT_FLAG)


def is_flagged(r) -> bool:
    return bool(np.asarray(r, np.uint8)[64:68].any())


def unrec(rec68) -> np.ndarray:
    """68-byte record -> 64-byte affine form (zeros at infinity, whatever the record's coordinates hold)"""
    rec68 = np.asarray(rec68, np.uint8).reshape(RECORD)
    return np.zeros(64, np.uint8) if is_flagged(rec68) else rec68[:64].copy()


def neg(curve, pt64) -> np.ndarray:
    pt64 = np.asarray(pt64, np.uint8).reshape(64)
    if not pt64.any():
        return pt64.copy()
    out = pt64.copy()
    out[32:] = to_le([BASE_MOD[curve] - from_le(pt64[32:])[0]])[0]
    return out


# ------------------------------------------------------------------------------------------------ references
def ref_points_sum(oracle, curve, recs) -> np.ndarray:
    """left-to-right fold with the oracle's group law, flagged records skipped -> 64-byte affine point"""
    recs = np.asarray(recs, np.uint8).reshape(-1, RECORD)
    acc = np.zeros(64, np.uint8)
    for i in np.flatnonzero(~recs[:, 64:68].any(axis=1)):
        acc = oracle.point_add(curve, acc, recs[i, :64])
    return acc


def ref_sum_rows(field, rows_of_ints) -> list:
    """column sums modulo p"""
    p = FIELD_MOD[field]
    return [sum(col) % p for col in zip(*rows_of_ints)]


def fold(oracle, curve, pts) -> np.ndarray:
    acc = np.zeros(64, np.uint8)
    for pt in pts:
        acc = oracle.point_add(curve, acc, pt)
    return acc


# ------------------------------------------------------------------------------------------------ point cases
def points_sum_cases(oracle, curve, g) -> dict:
    """name -> [n, 68] records, built from the points g[0 ..] (at least 24 distinct points of `curve`)"""
    Pt, Qt, Rt = g[0], g[1], g[2]
    add = lambda a, b: oracle.point_add(curve, a, b)
    pq = add(Pt, Qt)
    cases = {
        "single": [rec(Pt)],
        "pair": [rec(Pt), rec(Qt)],
        "double_at_once": [rec(Pt), rec(Pt)],
        "double_late": [rec(Pt), rec(Qt), rec(pq)],
        "cancel_late_then_go_on": [rec(Pt), rec(Qt), rec(neg(curve, pq)), rec(Rt)],
        "cancel_at_once": [rec(Pt), rec(neg(curve, Pt))],
        "all_infinite": [rec_inf(1), rec_inf(2), rec_inf(3)],
        "infinite_first_mid_last": [rec_inf(4), rec(Pt), rec_inf(), rec(Qt), rec_inf(5)],
        "nonunit_flag": [rec(Pt), rec_inf_nonunit(6), rec(Qt)],
    }
    # what ShardedStateJob hands the kernel at 8 ranks: 8 fixed-base partials, then 8 variable-base partials, 16 records that sum to infinity
    fifteen = [g[3 + i] for i in range(15)]
    cases["pallas_total_shape"] = [rec(x) for x in fifteen] + [rec(neg(curve, fold(oracle, curve, fifteen)))]
    # the documented maximum n; every record but the first and the last is infinity with garbage coordinates
    sparse = np.empty((65536, RECORD), np.uint8)
    sparse[:, :64] = np.stack([garbage_coords(i) for i in range(255)])[np.arange(65536) % 255]
    sparse[:, 64:] = 0
    sparse[:, 64] = 1
    sparse[1::3, 64], sparse[1::3, 65] = 0, 1                     # every third one with the non-unit flag word
    sparse[0], sparse[65535] = rec(Pt), rec(Qt)
    cases["long_sparse"] = sparse
    # 1 000 records from 6 points and their negatives, about 10 % infinity.  The running sum is sum_k coef[k] * pool[k]; half of the steps walk back towards the
    # origin, so it keeps coming through pool[k] itself (the next record equal to it: doubling with zz != 1; opposite to it: infinity, then a restart)
    rng = random.Random(0x5EED0 + curve)
    pool = [g[18 + i] for i in range(6)]
    pool += [neg(curve, x) for x in pool]
    dense, coef = [], [0] * 6
    for i in range(1000):
        if i == 999:                                                  # the last step leads away from the origin: the total is finite
            dense.append(rec(pool[0] if coef[0] >= 0 else pool[6]))
            break
        if rng.random() < 0.1:
            dense.append(rec_inf(rng.randrange(1, 200), flag=rng.choice([1, NONUNIT_FLAG, 0xFFFFFFFF])))
            continue
        away = [k for k in range(6) if coef[k]]
        if away and rng.random() < 0.5:
            k = rng.choice(away)
            sign = -1 if coef[k] > 0 else 1
        else:
            k, sign = rng.randrange(6), rng.choice([1, -1])
        coef[k] += sign
        dense.append(rec(pool[k] if sign > 0 else pool[6 + k]))
    cases["long_dense"] = dense
    return {name: np.stack(v) if isinstance(v, list) else v for name, v in cases.items()}


# ------------------------------------------------------------------------------------------------ row-sum cases
SUM_ROWS_SHAPES = [(1, 1), (2, 3), (3, 257), (8, 255), (8, 256), (16, 5), (4096, 3)]
N_FAMILIES = 7


def _family_value(fam, r, j, p, rng):
    """entry [r][j] of a column of value family `fam`; pairs sit in rows (2t, 2t + 1), so a running sum over the rows reaches p exactly after the odd row"""
    if fam == 0:
        return p - 1                                              # rows of them: the sum is p - rows mod p
    if fam == 1:                                                  # (a, p - a): a drawn per pair and column
        a = 1 + pow(0x9E3779B97F4A7C15 * (j + 1) + 0xBF58476D1CE4E5B9 * (r // 2 + 1), 5, p - 1)
        return a if r % 2 == 0 else p - a
    if fam == 2:                                                  # ((p + 1) / 2, (p - 1) / 2), the order by column
        return (p + 1) // 2 if (r + j // N_FAMILIES) % 2 == 0 else (p - 1) // 2
    if fam == 3:                                                  # (p - 1, 1) then (p - 1, 2): running sums p - 1, p, 2p - 1 -> p - 1, p + 1
        return p - 1 if r % 2 == 0 else 1 + (r // 2 + j // N_FAMILIES) % 2
    if fam == 4:
        return (1 << 254) + rng.randrange(p - (1 << 254))         # uniform over [2^254, p)
    if fam == 5:
        return 0
    return rng.randrange(p)                                       # uniform below p


def sum_rows_cases(field) -> dict:
    """name -> (rows, m, matrix [rows][m] of canonical integers); the value family of column j is (j + index of the shape) mod 7"""
    p = FIELD_MOD[field]
    cases = {}
    for si, (rows, m) in enumerate(SUM_ROWS_SHAPES):
        rng = random.Random(1000 * field + si)
        mat = [[_family_value((j + si) % N_FAMILIES, r, j, p, rng) for j in range(m)] for r in range(rows)]
        cases[f"{rows}x{m}"] = (rows, m, mat)
    return cases


def running_sums_hit_p(field, mat) -> int:
    """number of columns whose running sum (each step reduced as fe_add does: one conditional subtraction) equals p exactly before that subtraction"""
    p, hits = FIELD_MOD[field], 0
    for col in zip(*mat):
        acc, hit = 0, False
        for v in col:
            acc += v
            hit |= acc == p
            if acc >= p:
                acc -= p
        hits += hit
    return hits
