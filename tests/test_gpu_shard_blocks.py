"""GPU parity of the reduction operators of the multi-GPU exchange step (api_shard.hip: field_sum_rows_kernel, points_sum_kernel, records_equal_kernel, and the
entry points around them) with the CPU oracle and Python integers, at the shapes 1 to 8 ranks give them and on the branches honest partial sums never reach:
doubling with zz != 1, infinity in the middle of a sum, flagged records with garbage coordinates, a running sum equal to p, first = rank * m.  Every assertion
is a byte comparison; the cases and their references come from tests/shard_block_cases.py (checked on the CPU by tests/test_shard_block_cases.py)."""
import random

import numpy as np
import pytest

import shard_block_cases as S
from dev_helpers import Dev

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
INF_RECORD = S.rec(np.zeros(64, np.uint8))                    # 64 zero bytes, then the word 1


@pytest.fixture
def dev(ctx):
    d = Dev(ctx)
    yield d
    d.close()


def uniform_scalars(n, modulus, seed):
    """n canonical field elements drawn uniformly below the modulus (conftest.rand_scalars clears the top two bits)"""
    rng = random.Random(seed)
    return S.to_le([rng.randrange(modulus) for _ in range(n)])


def word(b) -> int:
    return int(np.ascontiguousarray(b, np.uint8).view(np.uint32)[0])


# ------------------------------------------------------------------------------------------------ field_sum_rows_kernel
@pytest.mark.parametrize("field", [0, 1])
def test_field_sum_rows_equals_the_column_sum_mod_p(ctx, dev, field):
    """only this test gives field_sum_rows_kernel a running sum equal to p (the equality edge of fe_add's conditional subtraction), values in [2^254, p),
    rows = 8 and 4096, and m on both sides of its 256-thread block"""
    for name, (rows, m, mat) in S.sum_rows_cases(field).items():
        d_in = dev.put(S.to_le([v for row in mat for v in row]))
        d_out = dev.put(np.full(m * 32 + 32, SENTINEL, np.uint8))
        ctx.field_sum_rows_dev(field, rows, m, d_in, d_out)
        got = dev.get(d_out, m * 32 + 32)
        exp = S.to_le(S.ref_sum_rows(field, mat)).reshape(-1)
        bad = np.flatnonzero((got[:m * 32] != exp).reshape(m, 32).any(axis=1))
        assert bad.size == 0, (name, "columns", bad[:8].tolist())
        assert (got[m * 32:] == SENTINEL).all(), (name, "bytes past the output were written")


# ------------------------------------------------------------------------------------------------ points_sum_kernel
@pytest.fixture(scope="module")
def point_cases(oracle, srs_oracle):
    """per curve: name -> (records, record of the oracle's fold); computed once"""
    out = {}
    for curve in (0, 1):
        cases = S.points_sum_cases(oracle, curve, srs_oracle[curve][0])
        out[curve] = {name: (recs, S.rec(S.ref_points_sum(oracle, curve, recs))) for name, recs in cases.items()}
    return out


@pytest.mark.parametrize("curve", [1, 0])
def test_points_sum_equals_the_oracle_fold(ctx, dev, point_cases, curve):
    """only this test takes points_sum_kernel through the doubling branch of xyzz_add_affine with zz != 1 (double_late, long_dense), through infinity in the
    middle of a sum (cancel_late_then_go_on), past flagged records whose coordinates are garbage and whose flag word is not 1, and to n = 65 536"""
    for name, (recs, exp) in point_cases[curve].items():
        d_recs = dev.put(recs)
        d_out = dev.put(np.full(72, SENTINEL, np.uint8))
        ctx.points_sum_dev(curve, len(recs), d_recs, d_out)
        got = dev.get(d_out, 72)
        assert got[:68].tobytes() == exp.tobytes(), (name, got[:68].tolist(), exp.tolist())
        assert word(got[64:68]) == (0 if exp[:64].any() else 1), name
        assert (got[68:] == SENTINEL).all(), (name, "bytes past the record were written")
    for name in ("cancel_at_once", "all_infinite", "pallas_total_shape"):                   # the generator is checked on the CPU; this pins which cases end at infinity
        assert point_cases[curve][name][1].tobytes() == INF_RECORD.tobytes(), name


# ------------------------------------------------------------------------------------------------ records_equal_kernel
def test_point_records_equal_truth_table(ctx, dev, srs_oracle):
    """only this test gives records_equal_kernel records that differ in one coordinate word, infinity records with different garbage and with flag words other
    than 1, and a verdict word that already holds something"""
    g = srs_oracle[1][0]
    a, b = S.rec(g[0]), S.rec(g[1])
    pairs = [("equal finite records", a, a.copy(), 1), ("different points", a, b, 0)]
    for i in range(16):
        c = a.copy()
        c[4 * i + ((5 * i + 3) % 32) // 8] ^= 1 << ((5 * i + 3) % 8)
        pairs.append((f"coordinate word {i} differs", a, c, 0))
        pairs.append((f"coordinate word {i} differs, swapped", c, a, 0))
    same_coords_flagged = S.rec(g[0], flag=1)
    for nm, inf in (("canonical infinity", S.rec_inf()), ("infinity with garbage", S.rec_inf(7)), ("infinity with the finite record's coordinates", same_coords_flagged),
                    ("infinity with flag word 0x0100", S.rec_inf_nonunit(8))):
        pairs.append((f"finite against {nm}", a, inf, 0))
        pairs.append((f"{nm} against finite", inf, a, 0))
    pairs.append(("infinity against infinity, different garbage", S.rec_inf(9), S.rec_inf(10), 1))
    pairs.append(("infinity against infinity, garbage against zeros", S.rec_inf(11), S.rec_inf(), 1))
    pairs.append(("infinity against infinity, flag words 1 and 0x0100", S.rec_inf(12), S.rec_inf_nonunit(13), 1))
    pairs.append(("infinity against infinity, flag words 0x0100 and 1", S.rec_inf_nonunit(13), S.rec_inf(12), 1))
    pairs.append(("infinity against infinity, flag words 0x0100 and 0xFFFFFFFF", S.rec_inf_nonunit(), S.rec_inf(14, flag=0xFFFFFFFF), 1))
    n = len(pairs)
    d_a, d_b = dev.put(np.stack([p[1] for p in pairs])), dev.put(np.stack([p[2] for p in pairs]))
    d_v = dev.put(np.full(4 * n + 4, 0xFF, np.uint8))                                       # every verdict word pre-filled with 0xFFFFFFFF
    for i in range(n):
        ctx.point_records_equal_dev(d_a + 68 * i, d_b + 68 * i, d_v + 4 * i)
    got = dev.get(d_v, 4 * n + 4).view(np.uint32)
    for i, (nm, _, _, exp) in enumerate(pairs):
        assert int(got[i]) == exp, (nm, hex(int(got[i])))
    assert int(got[n]) == 0xFFFFFFFF                                                         # the word after the last verdict is untouched


# ------------------------------------------------------------------------------------------------ mina_msm_srs_range_dev
RANK_SLICES = [(0, 1), (0, 31), (1, 32), (31, 33), (224, 32), (448, 64), (65535, 1), (65279, 257)]      # the last two end on the last base of the SRS


@pytest.mark.parametrize("curve", [1, 0])
def test_msm_srs_range_record_on_rank_slices(ctx_srs, dev, oracle, srs_oracle, curve):
    """the device record with first != 0 against the oracle (so far only the host form was, at 2^16 / world sizes): slice lengths on both sides of the 32-point
    switch between the two group laws, first not a multiple of anything, slices that end on the last base"""
    ctx, g, r = ctx_srs, srs_oracle[curve][0], S.SCALAR_MOD[curve]
    assert ctx.srs_depth(curve) == 65536 and RANK_SLICES[-1][0] + RANK_SLICES[-1][1] == 65536 and RANK_SLICES[-2][0] + RANK_SLICES[-2][1] == 65536
    for first, n in RANK_SLICES:
        last_only = np.zeros((n, 32), np.uint8)
        last_only[n - 1] = S.to_le([r - 1])[0]
        for kind, sc in (("uniform", uniform_scalars(n, r, seed=first * 1000 + n + curve)), ("r - 1 in the last row", last_only), ("zeros", np.zeros((n, 32), np.uint8))):
            d_sc, d_out = dev.put(sc), dev.put(np.full(72, SENTINEL, np.uint8))
            ctx.msm_srs_range_dev(curve, first, n, d_sc, d_out)
            got = dev.get(d_out, 72)
            exp = S.rec(oracle.msm_naive(curve, g[first:first + n], sc))
            assert got[:68].tobytes() == exp.tobytes(), ("oracle", first, n, kind)
            assert S.rec(ctx.msm_srs_range(curve, first, sc)).tobytes() == got[:68].tobytes(), ("host form", first, n, kind)
            assert (got[68:] == SENTINEL).all(), (first, n, kind)
            if kind == "zeros":
                assert got[:68].tobytes() == INF_RECORD.tobytes(), (first, n)
            if kind == "r - 1 in the last row":                                              # (r - 1) g = -g: the x of the slice's last base
                assert got[:68].tobytes() == S.rec(S.neg(curve, g[first + n - 1])).tobytes(), (first, n)


# ------------------------------------------------------------------------------------------------ mina_challenge_to_field_dev
@pytest.mark.parametrize("field", [0, 1])
def test_challenge_to_field_dev_equals_host_and_oracle(ctx, dev, oracle, field):
    """n on both sides of the kernel's 64-thread block; the all-zero and the all-ones challenge among the inputs"""
    _, endo_r = oracle.endo(1 if field == 0 else 0)           # the curve whose scalar field is `field`
    rng = np.random.Generator(np.random.PCG64(40 + field))
    for n in (1, 63, 64, 65):
        ch = rng.integers(0, 256, size=(n, 16), dtype=np.uint8)
        ch[0] = 0 if n != 63 else 255
        if n > 2:
            ch[n - 1], ch[n // 2] = 255, 0
        d_ch, d_out = dev.put(ch), dev.put(np.full(n * 32 + 32, SENTINEL, np.uint8))
        ctx.challenge_to_field_dev(field, n, d_ch, d_out)
        got = dev.get(d_out, n * 32 + 32)
        exp = np.stack([oracle.challenge_to_field(field, c.copy(), endo_r) for c in ch])
        assert got[:n * 32].tobytes() == exp.tobytes(), ("oracle", n)
        assert ctx.challenge_to_field(field, ch).tobytes() == got[:n * 32].tobytes(), ("host form", n)
        assert (got[n * 32:] == SENTINEL).all(), n


# ------------------------------------------------------------------------------------------------ the exchange step, transport replaced by slicing
EX_CURVE, EX_FIELD, EX_K, EX_B = 1, 0, 8, 11                  # Vesta, whose scalars live in Fp; 256 bases; 11 accumulators
PARTITION = {1: [11], 2: [4, 7], 4: [3, 0, 5, 3], 8: [2, 1, 0, 3, 1, 0, 2, 2]}      # instances per shard: ragged, with empty shards from 4 ranks on


@pytest.fixture(scope="module")
def exchange_batch(oracle, srs_oracle):
    """B accumulator instances at k = 8 with everything the oracle can say about their folded check: prechallenges, sg_b, rho_b, the folded scalar vector
    F[j] = sum_b rho_b s_b[j] and both sides of  <F, g> == sum_b rho_b sg_b"""
    p, n = S.FIELD_MOD[EX_FIELD], 1 << EX_K
    g = srs_oracle[EX_CURVE][0][:n]
    _, endo_r = oracle.endo(EX_CURVE)
    rng = np.random.Generator(np.random.PCG64(77))
    pre = rng.integers(0, 256, size=(EX_B, EX_K, 16), dtype=np.uint8)
    coeffs = [S.from_le(oracle.b_poly_coefficients(EX_FIELD, np.stack([oracle.challenge_to_field(EX_FIELD, c.copy(), endo_r) for c in pre[b]]))) for b in range(EX_B)]
    sg = np.stack([oracle.msm_naive(EX_CURVE, g, S.to_le(coeffs[b])) for b in range(EX_B)])
    rho = uniform_scalars(EX_B, p, seed=78)
    rho_i = S.from_le(rho)
    folded = [sum(rho_i[b] * coeffs[b][j] for b in range(EX_B)) % p for j in range(n)]
    left = oracle.msm_naive(EX_CURVE, g, S.to_le(folded))
    assert left.tobytes() == oracle.msm_naive(EX_CURVE, sg, rho).tobytes()                  # the batch is honest under the oracle
    return {"g": g, "pre": pre, "sg": sg, "rho": rho, "folded": folded, "left": left}


@pytest.mark.parametrize("G", [1, 2, 4, 8])
def test_exchange_step_arithmetic_for_1_2_4_8_ranks(ctx_srs, dev, oracle, exchange_batch, G):
    """The arithmetic of ShardedAccumulatorCheck.verify_base_sliced for G ranks in one process on one context, the transport replaced by slicing on the host.
    This pins the kernels at the shapes G ranks give them -- rows = G, m = 256 / G (32 at G = 8: the switch point between the two group laws), first = r * m,
    G and 2 G records per sum, empty shards -- with every intermediate result compared with the oracle.  It does not test the control flow of sharded.py (the
    2-rank tests run that), and it is the only test that gives field_sum_rows_kernel rows = 8 and mina_msm_srs_range_dev first = r * m at m = 32."""
    ctx, e = ctx_srs, exchange_batch
    curve, field, k, n, p = EX_CURVE, EX_FIELD, EX_K, 1 << EX_K, S.FIELD_MOD[EX_FIELD]
    m = n // G
    bounds = np.concatenate([[0], np.cumsum(PARTITION[G])])
    shards = [(int(bounds[s]), int(bounds[s + 1])) for s in range(G)]
    assert bounds[-1] == EX_B and (G < 4 or any(lo == hi for lo, hi in shards))
    d_rho = dev.put(e["rho"])

    # 1. every shard folds its challenge polynomials: S_s[j] = sum_{b in shard} rho_b s_b[j]  (an empty shard: zeros)
    d_pre, d_chals = dev.put(e["pre"]), dev.alloc(EX_B * k * 32)
    d_S = dev.put(np.zeros(G * n * 32, np.uint8))
    for lo, hi in shards:
        if hi > lo:
            ctx.challenge_to_field_dev(field, (hi - lo) * k, d_pre + 16 * k * lo, d_chals + 32 * k * lo)
    ctx.synchronize()                                                    # consecutive calls go to different lanes: the folds read what these wrote
    for s, (lo, hi) in enumerate(shards):
        if hi > lo:
            ctx.b_poly_fold_dev(field, k, hi - lo, d_chals + 32 * k * lo, d_rho + 32 * lo, d_S + 32 * n * s)
    vectors = dev.get(d_S, G * n * 32).reshape(G, n, 32)

    # 2. + 3. rank r receives slice r of every shard's vector (the all-to-all), folds the G slices and commits over its n / G bases
    d_mine, d_left = dev.alloc(n * 32), dev.put(np.full(G * 68 + 4, SENTINEL, np.uint8))
    for r in range(G):
        d_recv = dev.put(vectors[:, r * m:(r + 1) * m])                  # [G, m, 32]: what all_to_all_single leaves on rank r
        ctx.field_sum_rows_dev(field, G, m, d_recv, d_mine + 32 * m * r)
    mine = dev.get(d_mine, n * 32).reshape(G, m * 32)
    for r in range(G):
        assert mine[r].tobytes() == S.to_le(e["folded"][r * m:(r + 1) * m]).tobytes(), ("summed slice of rank", r)
        ctx.msm_srs_range_dev(curve, r * m, m, d_mine + 32 * m * r, d_left + 68 * r)
    left = dev.get(d_left, G * 68 + 4)
    assert (left[G * 68:] == SENTINEL).all()
    left = left[:G * 68].reshape(G, 68)
    for r in range(G):
        assert left[r].tobytes() == S.rec(oracle.msm_naive(curve, e["g"][r * m:(r + 1) * m], S.to_le(e["folded"][r * m:(r + 1) * m]))).tobytes(), ("left record of rank", r)

    # 4. + 5. the shards' shares of sum_b rho_b sg_b, then both totals and the comparison
    def right_records(sg):
        d_sg, d_right = dev.put(sg), dev.put(np.tile(INF_RECORD, G))      # an empty shard contributes the infinity record
        for s, (lo, hi) in enumerate(shards):
            if hi > lo:
                ctx.msm_dev(curve, hi - lo, d_sg + 64 * lo, d_rho + 32 * lo, d_right + 68 * s)
        right = dev.get(d_right, G * 68).reshape(G, 68)
        for s, (lo, hi) in enumerate(shards):
            assert right[s].tobytes() == S.rec(oracle.msm_naive(curve, sg[lo:hi], e["rho"][lo:hi]) if hi > lo else np.zeros(64, np.uint8)).tobytes(), ("right record of shard", s)
        return right

    def total(records):
        d_recs, d_out = dev.put(records), dev.put(np.full(72, SENTINEL, np.uint8))
        ctx.points_sum_dev(curve, len(records), d_recs, d_out)
        got = dev.get(d_out, 72)
        assert (got[68:] == SENTINEL).all()
        return got[:68], d_out

    def verdict(d_a, d_b):
        d_v = dev.put(np.full(4, 0xFF, np.uint8))
        ctx.point_records_equal_dev(d_a, d_b, d_v)
        return word(dev.get(d_v, 4))

    L, d_L = total(left)
    assert L.tobytes() == S.rec(e["left"]).tobytes(), "left total against the oracle's MSM of the folded vector"
    right = right_records(e["sg"])
    R, d_R = total(right)
    assert R.tobytes() == S.rec(oracle.msm_naive(curve, e["sg"], e["rho"])).tobytes(), "right total against the oracle's sum rho_b sg_b"
    assert verdict(d_L, d_R) == 1 and verdict(d_R, d_L) == 1

    # one sg of the last non-empty shard replaced
    last = max(s for s, (lo, hi) in enumerate(shards) if hi > lo)
    bad = e["sg"].copy()
    bad[shards[last][1] - 1] = e["g"][3]
    Rb, d_Rb = total(right_records(bad))
    assert Rb.tobytes() == S.rec(oracle.msm_naive(curve, bad, e["rho"])).tobytes() and Rb.tobytes() != R.tobytes()
    assert verdict(d_L, d_Rb) == 0

    # opposite discrepancies in two shards (in two proofs of the one shard at G = 1): sg + T here, sg - T there; the rho are independent, so they do not cancel
    first_shard = min(s for s, (lo, hi) in enumerate(shards) if hi > lo)
    ia, ib = shards[first_shard][0], shards[last][1] - 1
    assert ia != ib and (G == 1 or first_shard != last)
    T = e["g"][5]
    bad = e["sg"].copy()
    bad[ia], bad[ib] = oracle.point_add(curve, bad[ia], T), oracle.point_add(curve, bad[ib], S.neg(curve, T))
    Rc, d_Rc = total(right_records(bad))
    assert Rc.tobytes() == S.rec(oracle.msm_naive(curve, bad, e["rho"])).tobytes() and Rc.tobytes() != R.tobytes()
    assert verdict(d_L, d_Rc) == 0

    # the Pallas-shaped ending of ShardedStateJob: the left records and the NEGATED right partials, 2 G records that sum to infinity
    negated = np.stack([S.rec(S.neg(curve, S.unrec(x))) for x in right])
    Z, d_Z = total(np.concatenate([left, negated]))
    assert Z.tobytes() == INF_RECORD.tobytes()
    assert verdict(d_Z, dev.put(INF_RECORD)) == 1
    assert verdict(d_Z, d_L) == 0
