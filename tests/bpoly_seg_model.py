"""The segmented matrix-core b_poly fold (mina_bridge_amd/csrc/bpoly_mfma_seg.cuh) restated on integers, on top of tests/bpoly_digits_model.py.
TEST INFRASTRUCTURE ONLY.

A segment [begin, end) is a range of the batch, the GEMM's K dimension.  `bpoly_field_gemm_seg_kernel` runs the K loop over the 128-column tiles that cover the
range -- from begin & ~127 to min(kpad, roundup(end, 128)) -- and clears, in the first and the last tile, the A-operand bytes of the columns outside the range.
`segment_columns` restates exactly that, tile by tile, and says which columns of the batch reach the accumulators; `seg_fold_by_tiles` then runs the digit path of
bpoly_digits_model over them.  Two deliberately wrong variants leave the first or the last tile unmasked (WRONG_VARIANTS): a neighbouring proof's digits inside the
same K tile then add to the sum.  tests/test_bpoly_seg_model.py shows that the FLANKED input tells each of them from the closed form, so that
tests/test_gpu_bpoly_seg_mfma.py cannot pass on a kernel without either mask.

A batch here is a column map: column b holds distinct proof colmap[b] (the closed form needs only the count of each distinct proof inside the range)."""
import numpy as np

import bpoly_digits_model as B

KT = B.KALIGN                                   # BPM_KT = BPM_KALIGN = 128
SEG_END = B.MFMA_END_BATCH                      # BPM_SEG_END: segments of 2^17 proofs or more stay on the VALU kernels
WRONG_VARIANTS = ("first_tile_unmasked", "last_tile_unmasked")


def takes_matrix_cores(k, length, min_len=256):
    """the host's rule (mb_bpoly_seg_plan) with mina_verify_tuning.bpoly_mfma on"""
    return k // 2 >= 1 and min_len != 0 and min_len <= length < SEG_END


def tile_range(batch, begin, end):
    """-> (kb, ke): the K loop of the segment runs over tiles kb, kb + 128, .. < ke"""
    if end <= begin:
        return begin & ~(KT - 1), begin & ~(KT - 1)
    return begin & ~(KT - 1), min(B.kpad_of(batch), (end + KT - 1) // KT * KT)


def segment_columns(batch, begin, end, variant=None):
    """the columns of the batch whose digits reach the accumulators of segment [begin, end), as the kernel's loop and mask decide (pad columns >= batch hold zero
    digits -- the planes are cleared -- and are left out)"""
    assert variant is None or variant in WRONG_VARIANTS
    assert 0 <= begin <= end <= batch
    kb, ke = tile_range(batch, begin, end)
    cols = []
    for k0 in range(kb, ke, KT):
        tile = np.arange(k0, k0 + KT)
        edge = k0 < begin or k0 + KT > end                  # uniform per tile: interior tiles are not masked at all
        unmasked = (variant == "first_tile_unmasked" and k0 == kb) or (variant == "last_tile_unmasked" and k0 + KT >= ke)
        if edge and not unmasked:
            tile = tile[(tile >= begin) & (tile < end)]
        cols.append(tile[tile < batch])
    return np.concatenate(cols) if cols else np.zeros(0, np.int64)


def counts_of(colmap, cols, ndistinct):
    return [int(x) for x in np.bincount(np.asarray(colmap)[cols], minlength=ndistinct)]


def seg_fold_by_tiles(field, k, chals, weights, colmap, begin, end, variant=None):
    """segment [begin, end) of the batch `colmap` through the kernel's tiles and mask and the digit path -> (out [2^k], largest |accumulator|)"""
    cnt = counts_of(colmap, segment_columns(len(colmap), begin, end, variant), len(chals))
    out, max_acc, _ = B.fold_by_columns(field, k, chals, weights, cnt)
    return out, max_acc


def seg_closed_form(field, k, chals, weights, colmap, begin, end):
    """sum over the proofs of the range of w * b_poly_coefficients(chals): what every kernel must give"""
    return B.closed_form(field, k, chals, weights, counts_of(colmap, np.arange(begin, end), len(chals)))


def tiled_colmap(batch, ndistinct, first=0):
    """column b holds distinct proof first + b % ndistinct"""
    return first + np.arange(batch) % ndistinct


def flanked_case(field, k):
    """512 columns: [0, 100) and [400, 512) hold the `all_minus_128` proofs (every digit of both operands -128: the loudest neighbour there is), [100, 400) the
    `mixed` case, each tiled round-robin.  -> (chals, weights, colmap); the segments under test are (100, 400), (100, 101) and (127, 129)."""
    mc, mw = B.named_case("mixed", field, k)
    fc, fw = B.named_case("all_minus_128", field, k)
    colmap = np.concatenate([tiled_colmap(100, len(fc), len(mc)), tiled_colmap(300, len(mc)), tiled_colmap(112, len(fc), len(mc))])
    return mc + fc, mw + fw, colmap


FLANKED_SEGMENTS = ((100, 400), (100, 101), (127, 129))


def colmap_inputs(k, chals, weights, colmap):
    """the byte arrays of the batch for `b_poly_fold`: chals [batch * k, 32], weights [batch, 32]"""
    c = B.to_le([x for c in chals for x in c]).reshape(len(chals), k * 32)[colmap]
    w = B.to_le(weights)[colmap]
    return np.ascontiguousarray(c).reshape(len(colmap) * k, 32), np.ascontiguousarray(w)
