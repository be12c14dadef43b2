"""The segmented b_poly fold on the matrix cores (mina_bridge_amd/csrc/bpoly_mfma_seg.cuh) through `b_poly_fold_segments_dev` and the grouped culprit search:
ranges that start and end anywhere in a K tile, a segment flanked by the loudest neighbours there are (tests/bpoly_seg_model.py shows on the CPU that this input
tells a missing mask of the first or the last tile from the truth), the longest segment an int32 accumulator holds and the first lengths past it, pad columns left
by an earlier call, more segments than one pass holds, and the search's rounds.  Every comparison is byte equality -- with the VALU kernels over the range alone,
or with the closed form on Python integers.  `mina_ctx_seg_fold_stats` says which kernels ran, so no case can pass on the other path."""
import ctypes

import numpy as np
import pytest

import bpoly_digits_model as B
import bpoly_seg_model as S
import test_grouped_search_gpu as GS
from dev_helpers import Dev

pytestmark = pytest.mark.gpu

FIELDS = (0, 1)
MINA_ERR_ARG = -1
COLSUM_BUDGET = 256 << 20                      # BPM_SEG_COLSUM_BUDGET


@pytest.fixture(scope="module")
def mlib():
    import mina_bridge_amd as m
    assert m.lib.verify_tuning_get().bpoly_mfma != 0, "the matrix-core fold is the default; these tests are about it"
    return m.lib


@pytest.fixture(scope="module")
def sctx():
    """a context of its own: the shortest matrix-core segment and the counters are context state"""
    c = GS.fresh_context()
    yield c
    c.close()


@pytest.fixture
def dev(sctx):
    d = Dev(sctx)
    yield d
    d.close()


class Folded:
    """one batch in HBM and segmented folds over it"""

    def __init__(self, ctx, dev, field, k, c8, w8):
        self.ctx, self.dev, self.field, self.k, self.batch, self.n = ctx, dev, field, k, len(c8) // k, 32 << k
        self.d_c, self.d_w = dev.put(c8), dev.put(w8)

    def segments(self, segs, min_len=None):
        """-> (out [nseg, 2^k * 32], the counters' rise); min_len None = the context's default"""
        nseg = len(segs)
        d_lo, d_hi = self.dev.put(np.array([s[0] for s in segs], np.uint32)), self.dev.put(np.array([s[1] for s in segs], np.uint32))
        d_out = self.dev.alloc(nseg * self.n)
        self.ctx.dev_upload(d_out, np.full(nseg * self.n, 0xEE, np.uint8))
        self.ctx.set_seg_fold_mfma_min(256 if min_len is None else min_len)
        try:
            before = self.ctx.seg_fold_stats()
            self.ctx.b_poly_fold_segments_dev(self.field, self.k, self.batch, nseg, d_lo, d_hi, self.d_c, self.d_w, d_out)
            after = self.ctx.seg_fold_stats()
        finally:
            self.ctx.set_seg_fold_mfma_min(256)
        return self.dev.get(d_out, nseg * self.n).reshape(nseg, self.n), {key: after[key] - before[key] for key in after}

    def single(self, lo, hi):
        """mina_b_poly_fold_dev over [lo, hi) alone"""
        d_ref = self.dev.alloc(self.n)
        self.ctx.b_poly_fold_dev(self.field, self.k, hi - lo, self.d_c + 32 * self.k * lo, self.d_w + 32 * lo, d_ref)
        return self.dev.get(d_ref, self.n)


def closed(field, k, chals, weights, colmap, seg):
    return B.to_le(S.seg_closed_form(field, k, chals, weights, colmap, *seg)).reshape(-1)


UNALIGNED = [(0, 700), (0, 256), (1, 257), (127, 383), (128, 384), (129, 700), (255, 511), (300, 556), (444, 700), (0, 0), (5, 6), (600, 700)]


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("k", [2, 3, 4, 6])
def test_unaligned_ranges(sctx, dev, mlib, k, field):
    """batch 700 (kpad 768): ranges that begin and end at, one before and one after a tile edge, overlapping, beside an empty, a single-proof and a short one"""
    batch = 700
    chals, weights = B.named_case("mixed", field, k)
    f = Folded(sctx, dev, field, k, *B.tile_inputs(k, batch, chals, weights))
    assert sum(S.takes_matrix_cores(k, e - b) for b, e in UNALIGNED) == 9
    with mlib.tuning(bpoly_mfma=0):
        refs = [f.single(b, e) if e > b else np.zeros(f.n, np.uint8) for b, e in UNALIGNED]      # the VALU kernels over each range alone
    got, rose = f.segments(UNALIGNED)
    assert rose == {"mfma_segments": 9, "valu_segments": 2, "mfma_passes": 1}, rose
    for i, seg in enumerate(UNALIGNED):
        assert (got[i] == refs[i]).all(), seg
    off, rose = f.segments(UNALIGNED, min_len=0)
    assert rose == {"mfma_segments": 0, "valu_segments": 11, "mfma_passes": 0}, rose
    assert (off == got).all()
    with mlib.tuning(bpoly_mfma=0):
        off, rose = f.segments(UNALIGNED)
    assert rose == {"mfma_segments": 0, "valu_segments": 11, "mfma_passes": 0}, rose
    assert (off == got).all()


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("k", [4, 6])
def test_flanked_segment(sctx, dev, k, field):
    """columns [0, 100) and [400, 512) hold proofs whose every digit is -128, [100, 400) the mixed case: a neighbour inside the same K tile must add nothing"""
    chals, weights, colmap = S.flanked_case(field, k)
    f = Folded(sctx, dev, field, k, *S.colmap_inputs(k, chals, weights, colmap))
    got, rose = f.segments([(100, 400)])
    assert rose == {"mfma_segments": 1, "valu_segments": 0, "mfma_passes": 1}, rose
    assert (got[0] == closed(field, k, chals, weights, colmap, (100, 400))).all()
    segs = list(S.FLANKED_SEGMENTS)                                      # (100, 400), one proof, two proofs across a tile edge
    got, rose = f.segments(segs, min_len=1)
    assert rose == {"mfma_segments": 3, "valu_segments": 0, "mfma_passes": 1}, rose
    for i, seg in enumerate(segs):
        assert (got[i] == closed(field, k, chals, weights, colmap, seg)).all(), seg


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("name", ["all_minus_128", "plus_127_times_minus_128"])
def test_accumulator_bound(sctx, dev, name, field):
    """2^17 - 1 proofs, unaligned at both ends, are the longest segment of the path (accumulators up to 2^31 - 2^14); 2^17 proofs stay on the VALU kernels"""
    k, batch = 2, (1 << 17) + 200
    chals, weights = B.named_case(name, field, k)
    colmap = S.tiled_colmap(batch, len(chals))
    f = Folded(sctx, dev, field, k, *B.tile_inputs(k, batch, chals, weights))
    segs = [(100, 100 + (1 << 17) - 1), (0, 1 << 17), (200, (1 << 17) + 200)]
    got, rose = f.segments(segs)
    assert rose == {"mfma_segments": 1, "valu_segments": 2, "mfma_passes": 1}, rose
    for i, seg in enumerate(segs):
        assert (got[i] == closed(field, k, chals, weights, colmap, seg)).all(), seg


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("k", [4, 6])
def test_stale_pad_columns(sctx, dev, k, field):
    """a single fold of 512 proofs of all -128 digits fills the lane's digit planes; segment (0, 257) of a batch of 257 (kpad 384) must not see them"""
    fc, fw = B.named_case("all_minus_128", field, k)
    c8, w8 = B.tile_inputs(k, 512, fc, fw)
    assert (sctx.b_poly_fold(field, k, c8, w8) == B.to_le(B.closed_form(field, k, fc, fw, B.tile_counts(512, len(fc))))).all()
    chals, weights = B.named_case("mixed", field, k)
    f = Folded(sctx, dev, field, k, *B.tile_inputs(k, 257, chals, weights))
    got, rose = f.segments([(0, 257)])
    assert rose["mfma_segments"] == 1
    assert (got[0] == closed(field, k, chals, weights, S.tiled_colmap(257, len(chals)), (0, 257))).all()


@pytest.mark.parametrize("field", FIELDS)
def test_more_segments_than_one_pass_holds(sctx, dev, field):
    """k = 10: 512 KiB of column sums per segment, so a pass holds budget / 512 KiB segments; one segment more than a whole pass goes out in two"""
    k, batch = 10, 40
    per_pass = COLSUM_BUDGET >> (k + 9)
    nseg = per_pass + 1
    assert nseg == 513
    chals, weights = B.named_case("mixed", field, k)
    f = Folded(sctx, dev, field, k, *B.tile_inputs(k, batch, chals, weights))
    segs = [(i % 39, i % 39 + 1 + (i & 1)) for i in range(nseg)]        # single- and two-proof segments
    got, rose = f.segments(segs, min_len=1)
    assert rose == {"mfma_segments": nseg, "valu_segments": 0, "mfma_passes": 2}, rose
    off, rose = f.segments(segs, min_len=0)
    assert rose == {"mfma_segments": 0, "valu_segments": nseg, "mfma_passes": 0}, rose
    assert (got == off).all()
    for i in (0, 1, per_pass - 1, per_pass, 300):                       # the first and the last of the first pass, the one of the second
        assert (got[i] == f.single(*segs[i])).all(), i


# ------------------------------------------------------------------------------------------------ the search
@pytest.fixture(scope="module")
def minted(oracle):
    from state_job_helpers import mint_job
    srs = {c: oracle.srs_create(c, 1024, threads=4) for c in (0, 1)}
    return [mint_job(srs[0], srs[1], 300 + 10 * i, **GS.SHAPE) for i in range(4)]


def searched(ctx, jobs, groups, min_len):
    ctx.set_seg_fold_mfma_min(min_len)
    try:
        before = ctx.seg_fold_stats()
        v, stats = GS.run(ctx, jobs, groups)
        after = ctx.seg_fold_stats()
    finally:
        ctx.set_seg_fold_mfma_min(256)
    return v, stats, {key: after[key] - before[key] for key in after}


@pytest.mark.parametrize("G", [2, 4])
@pytest.mark.parametrize("case", ["first", "boundary", "opening_and_accumulator", "malformed_acc_sg"])
def test_grouped_search_with_its_long_parts_on_the_matrix_cores(sctx, minted, case, G):
    B_, min_len = 70, 8
    jobs, bad, ipa_culprits, acc_culprits = GS.make_case(case, minted, B_, G)
    expect = [0 if b in bad else 1 for b in range(B_)]
    fan_v, fan_stats = GS.run(sctx, jobs, 0)
    assert fan_v == expect and fan_stats == {"searches": 0, "rounds": 0, "parts": 0}
    v, stats, rose = searched(sctx, jobs, G, min_len)
    sims = [GS.simulate(B_, G, c) for c in (ipa_culprits, acc_culprits) if c is not None]
    print(case, G, stats, rose)
    assert v == expect
    assert stats == {"searches": len(sims), "rounds": sum(s[0] for s in sims), "parts": sum(s[1] for s in sims)}
    assert rose["mfma_segments"] > 0 and rose["mfma_passes"] > 0 and rose["mfma_segments"] + rose["valu_segments"] == stats["parts"]
    v0, stats0, rose0 = searched(sctx, jobs, G, 0)
    assert v0 == expect and stats0 == stats and rose0 == {"mfma_segments": 0, "valu_segments": stats["parts"], "mfma_passes": 0}


def test_grouped_search_default_rule_parts_of_300(sctx, minted):
    B_, G = 600, 2
    jobs, bad, ipa_culprits, _ = GS.make_case("first", minted, B_, G)
    v, stats, rose = searched(sctx, jobs, G, 256)
    assert v == [0 if b in bad else 1 for b in range(B_)]
    rounds, parts = GS.simulate(B_, G, ipa_culprits)
    assert stats == {"searches": 1, "rounds": rounds, "parts": parts}
    assert rose == {"mfma_segments": 2, "valu_segments": parts - 2, "mfma_passes": 1}, rose      # the two parts of 300; every later part is 150 proofs or fewer


def test_setter(sctx):
    import mina_bridge_amd as m
    lib = m.load_library()
    before = sctx.seg_fold_stats()
    for bad in (1 << 17, (1 << 17) + 1, 0xFFFFFFFF):
        assert lib.mina_ctx_set_seg_fold_mfma_min(sctx._h, ctypes.c_uint32(bad)) == MINA_ERR_ARG
    for ok in (0, 1, (1 << 17) - 1, 256):
        sctx.set_seg_fold_mfma_min(ok)
    z = ctypes.c_uint64(0)
    assert lib.mina_ctx_seg_fold_stats(sctx._h, None, ctypes.byref(z), ctypes.byref(z)) == MINA_ERR_ARG
    assert lib.mina_ctx_seg_fold_stats(sctx._h, ctypes.byref(z), ctypes.byref(z), None) == MINA_ERR_ARG
    assert sctx.seg_fold_stats() == before
