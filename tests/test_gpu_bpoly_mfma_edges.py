"""The matrix-core b_poly fold (mina_bridge_amd/csrc/bpoly_mfma.cuh) at its digit, accumulator and tile edges, through `b_poly_fold` / `b_poly_fold_dev`.

The kernels cut the MONTGOMERY IMAGE of a table entry into balanced digits, so plain extremes give random digits; the inputs here come from
tests/bpoly_digits_model.py, which solves for the challenges and weights whose images are 0x3F7F..7F80 (31 digits of -128), 0x3F7F..7F7F (+127), 2^254 - 1 (a carry
through all 32 digits), 2^254 and above (top byte 0x40), p - 1 and 0, and tiles a few distinct proofs over the batch.  tests/test_bpoly_digits_model.py shows on the
CPU that these cases reach the accumulator bound 2^31 - 2^14 at batch 2^17 - 1 and tell 32-bit column sums, a wrong carry threshold, a logical shift in the column
carry and uncleared pad columns from the truth.

Every comparison is byte equality with the closed form  sum over distinct proofs of count * w * b_poly_coefficients(chals)  on Python integers."""
import numpy as np
import pytest

import bpoly_digits_model as B
from dev_helpers import Dev

pytestmark = pytest.mark.gpu

FIELDS = (0, 1)
GRID_K, GRID_BATCH = (1, 2, 3, 4, 5, 6), (255, 256, 257, 383, 384, 385)      # both sides of the first matrix-core batch and of a K tile boundary (kpad 256 / 384 / 512)


@pytest.fixture(scope="module")
def mlib():
    import mina_bridge_amd as m
    assert m.lib.verify_tuning_get().bpoly_mfma != 0, "the matrix-core fold is the default; these tests are about it"
    return m.lib


def inputs(name, field, k, batch, with_weights=True):
    """-> (chals [batch * k, 32], weights [batch, 32] or None, reference [2^k, 32]) of a named case tiled over the batch"""
    chals, weights = B.named_case(name, field, k)
    if not with_weights:
        weights = None
    c8, w8 = B.tile_inputs(k, batch, chals, weights)
    return c8, w8, B.to_le(B.closed_form(field, k, chals, weights, B.tile_counts(batch, len(chals))))


def fold_both_paths(ctx, mlib, field, k, c8, w8):
    """-> (the default result, the result of the VALU kernels)"""
    got = ctx.b_poly_fold(field, k, c8, w8)
    with mlib.tuning(bpoly_mfma=0):
        valu = ctx.b_poly_fold(field, k, c8, w8)
    return got, valu


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("k,batch", B.CASE_RUNS)
@pytest.mark.parametrize("name", list(B.CASES))
def test_named_cases(ctx, mlib, name, k, batch, field):
    """every named case at its listed batch -- 2^17 - 1 (the last batch of the path: accumulators up to 2^31 - 2^14) for both tables kernels, 4229 and 8457 (the
    first batches at which a signed / unsigned 32-bit column sum of all -128 digits would wrap), 257 for every small k -- equals the reference, and the VALU kernels
    give the same bytes"""
    assert B.takes_matrix_cores(k, batch)
    c8, w8, ref = inputs(name, field, k, batch)
    got, valu = fold_both_paths(ctx, mlib, field, k, c8, w8)
    assert (got == ref).all(), "matrix cores vs reference"
    assert (valu == got).all(), "VALU kernels vs matrix cores"


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("batch", GRID_BATCH)
@pytest.mark.parametrize("k", GRID_K)
def test_shape_grid(ctx, mlib, k, batch, field):
    """k = 1 (no low half: stays on the VALU kernels), 2 and 3 (one partial GEMM block, for k = 3 partial on the n side only), 4 and 5 (one table entry per lane,
    entries of several factors), 6 (the smallest shape of the eight-entries-per-lane tables kernel) at batches around 256 and around a K tile boundary"""
    c8, w8, ref = inputs("mixed", field, k, batch)
    got, valu = fold_both_paths(ctx, mlib, field, k, c8, w8)
    assert (got == ref).all(), "default path vs reference"
    assert (valu == got).all(), "VALU kernels vs default path"


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("k", [4, 6])
def test_pad_columns_are_cleared_of_the_previous_call(ctx, mlib, k, field):
    """all -128 digits at batch 512 fill the digit planes of the context; the next calls, at batch 257 (kpad 384: 127 pad columns that must be cleared) and at batch
    384 (no pad columns, no clear), must not see them"""
    c8, w8, ref = inputs("all_minus_128", field, k, 512)
    assert (ctx.b_poly_fold(field, k, c8, w8) == ref).all()
    for batch in (257, 384):
        c8, w8, ref = inputs("mixed", field, k, batch)
        assert (ctx.b_poly_fold(field, k, c8, w8) == ref).all(), batch
        c8, w8, ref = inputs("all_minus_128", field, k, 512)
        assert (ctx.b_poly_fold(field, k, c8, w8) == ref).all()


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("name", ["all_minus_128", "plus_127_times_minus_128", "mixed"])
def test_first_batch_past_the_matrix_cores(ctx, mlib, name, field):
    """batch 2^17, where an accumulator of all -128 digits would be 2^31: the dispatch must send it to the VALU kernels (64 slices), so it equals the reference and
    the result does not depend on the tuning field"""
    k, batch = 2, 1 << 17
    assert not B.takes_matrix_cores(k, batch) and B.takes_matrix_cores(k, batch - 1)
    c8, w8, ref = inputs(name, field, k, batch)
    got, valu = fold_both_paths(ctx, mlib, field, k, c8, w8)
    assert (got == ref).all(), "default path vs reference"
    assert (valu == got).all()


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("k", [5, 6])
def test_null_weights_on_the_matrix_cores(ctx, mlib, k, field):
    """weights = NULL is every weight 1: both tables kernels, host and device entry points, and a device call with explicit weights 1"""
    batch = 300
    c8, _, ref = inputs("mixed", field, k, batch, with_weights=False)
    got, valu = fold_both_paths(ctx, mlib, field, k, c8, None)
    assert (got == ref).all(), "matrix cores vs reference"
    assert (valu == got).all(), "VALU kernels vs matrix cores"
    dev = Dev(ctx)
    try:
        n = 32 << k
        ones = np.zeros((batch, 32), np.uint8)
        ones[:, 0] = 1
        d_c, d_w, d_out, d_out1 = dev.put(c8), dev.put(ones), dev.alloc(n), dev.alloc(n)
        ctx.b_poly_fold_dev(field, k, batch, d_c, 0, d_out)
        ctx.b_poly_fold_dev(field, k, batch, d_c, d_w, d_out1)
        assert (dev.get(d_out, n).reshape(-1, 32) == ref).all(), "b_poly_fold_dev, d_weights = 0"
        assert (dev.get(d_out1, n).reshape(-1, 32) == ref).all(), "b_poly_fold_dev, weights 1"
    finally:
        dev.close()
