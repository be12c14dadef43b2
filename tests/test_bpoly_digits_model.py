"""tests/bpoly_digits_model.py under the plain big-integer fold: the restated digit path computes the fold, the named cases put the digits into the tables that
their names promise and reach the accumulator bound they claim, and each of five wrong variants of the path is told from the reference by at least one named case
-- so that tests/test_gpu_bpoly_mfma_edges.py cannot pass on a kernel that is wrong in one of those ways.  No GPU."""
import random

import numpy as np
import pytest

import bpoly_digits_model as B
from oracle import pasta_ref as R

FIELDS = (0, 1)
REDUCED = {2: 29, 3: 30, 4: 31, 5: 32, 6: 33}       # a batch per k that tiles every case unevenly (the distinct proofs number 3, 5, 8 and 23)


def per_proof_fold(field, k, chals, weights):
    """sum_b w_b * b_poly_coefficients(chals_b), one proof at a time"""
    p = B.MODS[field]
    acc = [0] * (1 << k)
    for c, w in zip(chals, weights):
        for j, s in enumerate(R.b_poly_coefficients(c, p)):
            acc[j] = (acc[j] + w * s) % p
    return acc


# ------------------------------------------------------------------------------------------------ digits
def edge_images(field):
    p = B.MODS[field]
    return [0, 1, 127, 128, 129, 255, 256, p - 1, p - 2, B.IMG_M128, B.IMG_M128 - 1, B.IMG_M128 + 1, B.IMG_P127, B.IMG_FF, B.IMG_FF - 1, B.IMG_2_254, B.IMG_2_254 + 1,
            B.IMG_2_254_HIGH, B.IMG_2_254_CARRY, (1 << 254) - (1 << 247), (1 << 254) - (1 << 247) - 1, (1 << 248) - 1, 1 << 248,
            int.from_bytes(bytes([0x80] * 31 + [0x3F]), "little"), int.from_bytes(bytes([0x7F, 0x80] * 15 + [0x7F, 0x3F]), "little")]


@pytest.mark.parametrize("field", FIELDS)
def test_balanced_digits_reconstruct_and_stay_in_range(field):
    """sum d_i 256^i is the image itself and every digit, the top one included, is an int8: the top byte of an image below p is at most 0x40, and 0x40 stands over a
    zero byte (p - 2^254 < 2^126), so the top digit is at most 64 and no carry leaves it"""
    p = B.MODS[field]
    assert (p - (1 << 254)).bit_length() <= 126
    rng = random.Random(11 + field)
    imgs = edge_images(field) + [rng.randrange(p) for _ in range(4000)] + [p - 1 - rng.randrange(1 << 120) for _ in range(500)]
    imgs += [int.from_bytes(bytes(rng.choice((0x7F, 0x80, 0xFF, 0x00, 0x7E, 0x81)) for _ in range(31)) + bytes([rng.randrange(0x40)]), "little") for _ in range(2000)]
    for m in imgs:
        assert m < p
        d = B.balanced_digits(m)
        assert len(d) == 32 and all(-128 <= x <= 127 for x in d) and 0 <= d[31] <= 64, hex(m)
        assert sum(x << (8 * i) for i, x in enumerate(d)) == m, hex(m)


def test_the_named_images_have_the_digits_they_are_named_after():
    assert B.IMG_M128 == int("3F" + "7F" * 30 + "80", 16) and B.balanced_digits(B.IMG_M128) == [-128] * 31 + [64]
    assert B.balanced_digits(B.IMG_P127) == [127] * 31 + [63]
    assert B.balanced_digits(B.IMG_FF) == [-1] + [0] * 30 + [64]
    assert B.balanced_digits(B.IMG_2_254) == [0] * 31 + [64]
    assert B.balanced_digits(B.IMG_2_254_CARRY) == [-128] * 15 + [1] + [0] * 15 + [64]
    assert B.balanced_digits(0) == [0] * 32
    for field in FIELDS:
        p = B.MODS[field]
        assert B.IMG_2_254 + (1 << 253) > p > B.IMG_2_254_HIGH > B.IMG_2_254_CARRY and B.IMG_2_254 + (1 << 126) > p
        assert B.balanced_digits(p - 1)[31] == 64
        for m in (B.IMG_M128, B.IMG_FF, p - 1, 0, 1):
            assert B.plain_to_image(field, B.image_to_plain(field, m)) == m and B.image_to_plain(field, m) < p


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6])
def test_cases_put_their_images_into_the_tables(field, k):
    p, lb = B.MODS[field], k // 2
    nl, nh = 1 << lb, 1 << (k - lb)
    for name in B.CASES:
        chals, weights = B.named_case(name, field, k)
        assert all(0 <= x < p for c in chals for x in c) and all(0 <= w < p for w in weights) and all(len(c) == k for c in chals), name
        assert len({(tuple(c), w) for c, w in zip(chals, weights)}) == len(chals) >= 3, name       # distinct: tiled round-robin, no two neighbouring columns are equal
        assert B.named_case(name, field, k) == (chals, weights)
    for name, img_l, img_h in (("all_minus_128", B.IMG_M128, B.IMG_M128), ("plus_127_times_minus_128", B.IMG_M128, B.IMG_P127), ("ff_run", B.IMG_FF, B.IMG_FF)):
        chals, weights = B.named_case(name, field, k)
        for d, (c, w) in enumerate(zip(chals, weights)):
            L, H = B.half_tables(field, k, c, w)
            assert H[nh - 1] == img_h and (lb == 0 or L[nl - 1] == img_l), (name, d)
            assert L[0] == B.MONT_R % p
            if d == 0:                                         # "direct": all of H, every odd entry of L
                assert set(H) == {img_h} and all(L[e] == img_l for e in range(1, nl, 2)), name
    seen = {m for c, w in zip(*B.named_case("top_byte_0x40", field, k)) for t in B.half_tables(field, k, c, w) for m in t}
    assert {B.IMG_2_254, B.IMG_2_254_HIGH, p - 1, B.IMG_2_254_CARRY} <= seen
    seen = [t for c, w in zip(*B.named_case("zero_image", field, k)) for t in B.half_tables(field, k, c, w)]
    assert any(set(t) == {0} for t in seen) and any(0 in t and set(t) != {0} for t in seen) and any(0 not in t for t in seen)
    seen = {m for c, w in zip(*B.named_case("mixed", field, k)) for t in B.half_tables(field, k, c, w) for m in t}
    assert {B.IMG_M128, B.IMG_P127, B.IMG_FF, B.IMG_2_254, B.IMG_2_254_HIGH, p - 1, B.IMG_2_254_CARRY, 0} <= seen


def test_case_runs_cover_what_the_dispatch_and_the_wrap_points_need():
    runs = set(B.CASE_RUNS)
    assert {(2, (1 << 17) - 1), (6, (1 << 17) - 1), (4, 4229), (4, 8457)} <= runs and {(k, 257) for k in range(2, 7)} <= runs
    assert all(B.takes_matrix_cores(k, b) for k, b in runs)
    assert not B.takes_matrix_cores(2, 1 << 17) and not B.takes_matrix_cores(2, 255) and not B.takes_matrix_cores(1, 300) and B.takes_matrix_cores(2, 256)
    assert B.kpad_of(257) == 384 and B.kpad_of(384) == 384 and B.kpad_of((1 << 17) - 1) == 1 << 17
    # 31 terms of B * 2^14 in the longest all -128 anti-diagonal: the first B at which that leaves an int32 / a uint32
    assert 31 * 4228 << 14 < 1 << 31 <= 31 * 4229 << 14 and 31 * 8456 << 14 < 1 << 32 <= 31 * 8457 << 14


# ------------------------------------------------------------------------------------------------ the model computes the fold
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("k", [2, 3, 4, 5, 6])
def test_model_equals_closed_form_and_per_proof_fold_on_the_named_cases(field, k):
    batch = REDUCED[k]
    for name in B.CASES:
        chals, weights = B.named_case(name, field, k)
        counts = B.tile_counts(batch, len(chals))
        assert sum(counts) == batch
        ref = B.closed_form(field, k, chals, weights, counts)
        cols = [b % len(chals) for b in range(batch)]
        assert ref == per_proof_fold(field, k, [chals[d] for d in cols], [weights[d] for d in cols]), name
        got, _, _ = B.fold_by_columns(field, k, chals, weights, counts)
        assert got == ref, name
        one_by_one, _, _ = B.fold_by_columns(field, k, [chals[d] for d in cols], [weights[d] for d in cols])
        assert one_by_one == ref, name
        # the byte arrays of the GPU test hold the same batch
        c8, w8 = B.tile_inputs(k, batch, chals, weights)
        assert c8.shape == (batch * k, 32) and w8.shape == (batch, 32)
        for b in (0, 1, len(chals), batch - 1):
            assert [int.from_bytes(c8[b * k + i].tobytes(), "little") for i in range(k)] == chals[cols[b]] and int.from_bytes(w8[b].tobytes(), "little") == weights[cols[b]]


def test_model_equals_per_proof_fold_on_random_inputs():
    rng = random.Random(2024)
    for i in range(200):
        field, k, batch = rng.randrange(2), rng.randrange(1, 7), rng.randrange(1, 41)
        p = B.MODS[field]
        chals = [[rng.randrange(p) for _ in range(k)] for _ in range(batch)]
        weights = None if i % 5 == 0 else [rng.randrange(p) for _ in range(batch)]
        got, max_acc, max_col = B.fold_by_columns(field, k, chals, weights)
        assert got == per_proof_fold(field, k, chals, weights or [1] * batch) == B.closed_form(field, k, chals, weights), (i, field, k, batch)
        assert max_acc <= batch << 14 and max_col <= 32 * max_acc


# ------------------------------------------------------------------------------------------------ the bound, as arithmetic
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("k", [2, 6])
def test_accumulator_bound_at_the_dispatch_limit(field, k):
    """all -128 digits on both sides of every column: the largest accumulator is B * 2^14 -- 2^31 - 2^14 at the last batch the matrix cores take, 2^31 (one past an
    int32) at the first batch they must not.  Computed from the digit columns and their multiplicities."""
    chals, weights = B.named_case("all_minus_128", field, k)
    ref_at = {}
    for batch, want in (((1 << 17) - 1, (1 << 31) - (1 << 14)), (1 << 17, 1 << 31)):
        counts = B.tile_counts(batch, len(chals))
        got, max_acc, max_col = B.fold_by_columns(field, k, chals, weights, counts)
        assert max_acc == want == batch << 14
        assert max_col >= 31 * max_acc - 2 * (batch << 13) and max_col < 1 << 36
        assert got == B.closed_form(field, k, chals, weights, counts)
        ref_at[batch] = got
    assert ref_at[(1 << 17) - 1] != ref_at[1 << 17]
    chals, weights = B.named_case("plus_127_times_minus_128", field, k)
    batch = (1 << 17) - 1
    _, max_acc, _ = B.fold_by_columns(field, k, chals, weights, B.tile_counts(batch, len(chals)))
    assert max_acc == 127 * 128 * batch < 1 << 31                # the most negative accumulator: inside an int32 at every batch the positive bound allows


@pytest.mark.parametrize("field", FIELDS)
def test_column_sums_cross_32_bits_where_the_runs_say(field):
    chals, weights = B.named_case("all_minus_128", field, 4)
    col = {b: B.fold_by_columns(field, 4, chals, weights, B.tile_counts(b, len(chals)))[2] for b in (4228, 4229, 8456, 8457)}
    assert col[4228] < 1 << 31 <= col[4229] and col[8456] < 1 << 32 <= col[8457]


def test_report_largest_accumulators_and_column_sums():
    """prints, for every named case at its listed batches, the largest |accumulator| and |column sum| of the model (field 0); asserts that they fit their registers"""
    lines = []
    for k, batch in B.CASE_RUNS:
        for name in B.CASES:
            chals, weights = B.named_case(name, 0, k)
            _, max_acc, max_col = B.fold_by_columns(0, k, chals, weights, B.tile_counts(batch, len(chals)))
            assert max_acc < 1 << 31 and max_col < 1 << 36
            lines.append(f"k={k} batch={batch} {name}: max|acc|={max_acc} (2^{np.log2(max(max_acc, 1)):.2f}) max|colsum|={max_col} (2^{np.log2(max(max_col, 1)):.2f})")
    print("\n" + "\n".join(lines))


# ------------------------------------------------------------------------------------------------ the cases are sharp
def _variant_differs(variant, field):
    """the named (case, k, batch) runs on which the wrong variant's output differs from the reference"""
    hits = []
    for k, batch in B.CASE_RUNS:
        if k == 6 and batch > 257:
            continue                                             # the same digits as k = 2 at that batch; keeps this test short
        for name in B.CASES:
            chals, weights = B.named_case(name, field, k)
            counts = B.tile_counts(batch, len(chals))
            if B.fold_by_columns(field, k, chals, weights, counts, variant=variant)[0] != B.closed_form(field, k, chals, weights, counts):
                hits.append((name, k, batch))
    return hits


@pytest.mark.parametrize("field", FIELDS)
def test_int32_column_sums_are_caught(field):
    hits = _variant_differs("colsum_int32", field)
    assert ("all_minus_128", 4, 4229) in hits and ("all_minus_128", 2, (1 << 17) - 1) in hits
    # and only by the cases built for it: below the wrap point that variant IS the reference, which is why random inputs never saw it
    chals, weights = B.named_case("all_minus_128", field, 4)
    counts = B.tile_counts(4228, len(chals))
    assert B.fold_by_columns(field, 4, chals, weights, counts, variant="colsum_int32")[0] == B.closed_form(field, 4, chals, weights, counts)
    assert not [h for h in hits if h[2] == 257]


@pytest.mark.parametrize("field", FIELDS)
def test_uint32_column_sums_are_caught(field):
    """bins of 32 bits read back without a sign: wrong as soon as a column sum is negative, and for the all-positive columns of -128 * -128 from batch 8457 on"""
    hits = _variant_differs("colsum_uint32", field)
    assert ("all_minus_128", 4, 8457) in hits and ("plus_127_times_minus_128", 4, 257) in hits and ("mixed", 2, 257) in hits


@pytest.mark.parametrize("field", FIELDS)
def test_carry_threshold_above_128_is_caught(field):
    hits = _variant_differs("carry_gt_128", field)
    assert {h[0] for h in hits} >= {"all_minus_128", "plus_127_times_minus_128", "mixed"}
    assert ("all_minus_128", 2, 257) in hits
    assert B.balanced_digits(B.IMG_M128, carry_gt_128=True) != B.balanced_digits(B.IMG_M128)
    assert B.balanced_digits(B.IMG_P127, carry_gt_128=True) == B.balanced_digits(B.IMG_P127)         # no raw digit 128 in it: the other side of that case has them


@pytest.mark.parametrize("field", FIELDS)
def test_logical_shift_in_the_column_carry_is_caught(field):
    hits = _variant_differs("logical_shift", field)
    assert {h[0] for h in hits} >= {"plus_127_times_minus_128", "mixed", "all_minus_128"}


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("k", [4, 6])
def test_stale_pad_columns_are_caught(field, k):
    """the sequence of the GPU test: all -128 digits at batch 512 dirty the planes, then `mixed` at batch 257 (127 pad columns) and at 384 (none)"""
    prev = (k, 512) + B.named_case("all_minus_128", field, k)
    chals, weights = B.named_case("mixed", field, k)
    counts = B.tile_counts(257, len(chals))
    ref = B.closed_form(field, k, chals, weights, counts)
    assert B.fold_by_columns(field, k, chals, weights, counts)[0] == ref
    assert B.fold_by_columns(field, k, chals, weights, counts, variant="stale_pad_columns", prev=prev)[0] != ref
    Ls, Hs = B.stale_pad_columns(k, 257, (k, 512) + B.digit_rows(field, k, *B.named_case("all_minus_128", field, k)))
    assert Ls.shape == (127, 32 << (k // 2)) and Hs.shape == (127, 32 << (k - k // 2)) and (Ls != 0).mean() > 0.5 and (Hs != 0).mean() > 0.5
    counts = B.tile_counts(384, len(chals))                      # no pad columns: nothing stale to read, with or without the clear
    Ls, Hs = B.stale_pad_columns(k, 384, (k, 512) + B.digit_rows(field, k, *B.named_case("all_minus_128", field, k)))
    assert len(Ls) == 0 and len(Hs) == 0
    assert B.fold_by_columns(field, k, chals, weights, counts, variant="stale_pad_columns", prev=prev)[0] == B.closed_form(field, k, chals, weights, counts)
