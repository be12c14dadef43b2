"""tests/bpoly_seg_model.py against the closed form: the tiles-and-mask restatement of the segmented matrix-core fold is right, each of its two wrong variants
is told apart by the flanked input, and the bound case reaches the largest accumulator an int32 holds on this path, 2^31 - 2^14."""
import os
import re

import pytest

import bpoly_digits_model as B
import bpoly_seg_model as S

FIELDS = (0, 1)


def test_tile_range_and_mask():
    assert S.tile_range(700, 0, 700) == (0, 768) and S.tile_range(700, 129, 700) == (128, 768) and S.tile_range(700, 127, 383) == (0, 384)
    assert S.tile_range(700, 128, 384) == (128, 384) and S.tile_range(700, 5, 6) == (0, 128) and S.tile_range(768, 768, 768) == (768, 768)
    for begin, end in ((0, 700), (1, 257), (127, 383), (128, 384), (129, 700), (255, 511), (444, 700), (5, 6), (0, 0), (700, 700)):
        assert list(S.segment_columns(700, begin, end)) == list(range(begin, end)), (begin, end)
        kb, ke = S.tile_range(700, begin, end)
        assert kb % 128 == 0 and ke % 128 == 0 and ke <= 768 and (begin == end or (kb <= begin and end <= ke))
    # an aligned range has no edge tile: the wrong variants coincide with the right one
    for v in S.WRONG_VARIANTS:
        assert list(S.segment_columns(700, 128, 384, v)) == list(range(128, 384))
    assert list(S.segment_columns(512, 100, 400, "first_tile_unmasked")) == list(range(0, 400))
    assert list(S.segment_columns(512, 100, 400, "last_tile_unmasked")) == list(range(100, 512))


def test_model_constants_are_the_kernels():
    """the tile, the accumulator bound, the default shortest segment and the colsum budget as the sources state them"""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mina_bridge_amd", "csrc")
    seg = open(os.path.join(csrc, "bpoly_mfma_seg.cuh")).read()
    assert re.search(r"BPM_SEG_END\s*=\s*1u\s*<<\s*17\b", seg) and S.SEG_END == 1 << 17
    assert re.search(r"BPM_SEG_COLSUM_BUDGET\s*=\s*\(size_t\)256\s*<<\s*20\b", seg)
    assert re.search(r"BPM_KT\s*=\s*128\b", open(os.path.join(csrc, "bpoly_mfma.cuh")).read()) and S.KT == 128
    assert re.search(r"seg_fold_mfma_min\s*=\s*256\b", open(os.path.join(csrc, "ctx.h")).read())
    assert "k0 < first || k0 + BPM_KT > end" in seg, "the edge-tile test the model restates"


def test_the_rule():
    assert S.takes_matrix_cores(2, 256) and not S.takes_matrix_cores(2, 255) and not S.takes_matrix_cores(1, 300)
    assert S.takes_matrix_cores(2, (1 << 17) - 1) and not S.takes_matrix_cores(2, 1 << 17)
    assert S.takes_matrix_cores(3, 1, min_len=1) and not S.takes_matrix_cores(3, 0, min_len=1) and not S.takes_matrix_cores(3, 5000, min_len=0)


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("k", [4, 6])
def test_flanked_input_tells_each_missing_mask(k, field):
    chals, weights, colmap = S.flanked_case(field, k)
    assert len(colmap) == 512
    for begin, end in S.FLANKED_SEGMENTS:
        ref = S.seg_closed_form(field, k, chals, weights, colmap, begin, end)
        out, _ = S.seg_fold_by_tiles(field, k, chals, weights, colmap, begin, end)
        assert out == ref, (begin, end)
        for v in S.WRONG_VARIANTS:
            bad, _ = S.seg_fold_by_tiles(field, k, chals, weights, colmap, begin, end, v)
            assert bad != ref, (begin, end, v)


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("name", ["all_minus_128", "plus_127_times_minus_128"])
def test_bound_case_reaches_the_accumulator_bound(name, field):
    """k = 2, batch 2^17 + 200, segment (100, 100 + 2^17 - 1): the longest segment of the path, unaligned at both ends"""
    k, batch = 2, (1 << 17) + 200
    chals, weights = B.named_case(name, field, k)
    colmap = S.tiled_colmap(batch, len(chals))
    begin, end = 100, 100 + (1 << 17) - 1
    assert S.takes_matrix_cores(k, end - begin) and not S.takes_matrix_cores(k, end - begin + 1)
    out, max_acc = S.seg_fold_by_tiles(field, k, chals, weights, colmap, begin, end)
    assert out == S.seg_closed_form(field, k, chals, weights, colmap, begin, end)
    if name == "all_minus_128":
        assert max_acc == (1 << 31) - (1 << 14)
    else:
        assert max_acc == 127 * 128 * ((1 << 17) - 1) < 1 << 31
    # one tile more on either side and the largest accumulator no longer fits
    _, over = S.seg_fold_by_tiles(field, k, chals, weights, colmap, begin, end, "first_tile_unmasked")
    assert over > max_acc and (name != "all_minus_128" or over >= 1 << 31)
