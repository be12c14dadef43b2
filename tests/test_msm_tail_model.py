"""The identity behind the fused MSM tail, on integers (tests/msm_tail_model.py): rows of 128 buckets reduced to (S_r, T_r), set totals from the row pairs alone,
Horner over the sets -- against the definition  sum_b (b + 1) B_b  and  sum_w 2^(c w) total_w."""
import random

import pytest

import msm_tail_model as M


def direct(buckets):
    return sum((b + 1) * v for b, v in enumerate(buckets)) % M.ORDER


def fill(nb, kind, rng):
    if kind == "random":
        return [rng.randrange(M.ORDER) for _ in range(nb)]
    if kind == "sparse":
        return [rng.randrange(M.ORDER) if rng.random() < 0.05 else 0 for _ in range(nb)]
    out = [0] * nb
    if kind == "first":
        out[0] = rng.randrange(1, M.ORDER)
    elif kind == "last":
        out[nb - 1] = rng.randrange(1, M.ORDER)
    return out


@pytest.mark.parametrize("nb", [128, 4096, 32768])
@pytest.mark.parametrize("kind", ["random", "sparse", "empty", "first", "last"])
def test_set_total_equals_the_weighted_bucket_sum(nb, kind):
    buckets = fill(nb, kind, random.Random(nb * 7 + len(kind)))
    assert M.set_total(buckets) == direct(buckets)
    if kind == "empty":
        assert M.set_total(buckets) == 0
    if kind == "last":
        assert M.set_total(buckets) == nb * buckets[-1] % M.ORDER


@pytest.mark.parametrize("n", [1, 2, 15, 16, 17, 32, 128, 255, 256])
def test_weighted_block_sum(n):
    rng = random.Random(n)
    v = [rng.randrange(M.ORDER) for _ in range(n)]
    assert M.weighted_block_sum(v) == (sum(v) % M.ORDER, sum(i * x for i, x in enumerate(v)) % M.ORDER)


def test_row_pair_of_two_cancelling_buckets():
    """P in bucket 0 and -P in bucket 1: the row's plain sum is zero, its weighted sum is -P"""
    p = 123456789
    row = [p, M.ORDER - p] + [0] * (M.C - 2)
    assert M.row_pair(row) == (0, M.ORDER - p)


@pytest.mark.parametrize("nb,c,nsets", [(128, 8, 32), (4096, 13, 20), (32768, 16, 1)])
def test_problem_total_is_horner_over_the_sets(nb, c, nsets):
    rng = random.Random(nb + nsets)
    sets = [fill(nb, "sparse" if nb > 128 else "random", rng) for _ in range(nsets)]
    want = sum(pow(2, c * w, M.ORDER) * direct(b) for w, b in enumerate(sets)) % M.ORDER
    assert M.problem_total(sets, c) == want
