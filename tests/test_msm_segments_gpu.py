"""GPU parity of the segmented building blocks (mina_msm_segments_dev, mina_b_poly_fold_segments_dev): every segment's result is byte-equal to the single-range
call over that range alone (mina_msm_dev / mina_b_poly_fold_dev) and, for the MSM, to the CPU oracle's naive sum.

Shapes are the smallest at which the pipeline takes another path: segment lengths on both sides of the 32-point switch between the 8 x 32 and the 29-bit group
law, segment counts on both sides of nprob >= 4 (tasks against one lane per bucket), and for the fold a range long enough for the
single-range call to run on the matrix cores (256 proofs) beside ranges that keep it on the VALU kernel."""
import ctypes

import numpy as np
import pytest

from conftest import rand_scalars
from dev_helpers import Dev, record_to_affine

pytestmark = pytest.mark.gpu

P = 0x40000000000000000000000000000000224698FC094CF91B992D30ED00000001
Q = 0x40000000000000000000000000000000224698FC0994A8DD8C46EB2100000001
SCALAR_MOD = {0: Q, 1: P}
BASE_MOD = {0: P, 1: Q}
MINA_ERR_ARG = -1
NPTS = 640


@pytest.fixture(scope="module")
def points(oracle):
    """NPTS distinct points per curve (the first bases of a generated SRS)"""
    return {c: oracle.srs_create(c, NPTS, threads=4)[0] for c in (0, 1)}


@pytest.fixture
def dev(ctx):
    d = Dev(ctx)
    yield d
    d.close()


def msm_segments(ctx, dev, curve, bases, scalars, segs):
    """-> (records [nseg, 68] of the segmented call, records of mina_msm_dev over each non-empty segment alone)"""
    n, nseg = len(bases), len(segs)
    d_b, d_s = dev.put(bases), dev.put(scalars)
    d_lo, d_hi = dev.put(np.array([s[0] for s in segs], np.uint32)), dev.put(np.array([s[1] for s in segs], np.uint32))
    d_out, d_ref = dev.alloc(nseg * 68), dev.alloc(nseg * 68)
    ctx.msm_segments_dev(curve, n, nseg, d_lo, d_hi, d_b, d_s, d_out)
    for i, (lo, hi) in enumerate(segs):
        if hi > lo:
            ctx.msm_dev(curve, hi - lo, d_b + 64 * lo, d_s + 32 * lo, d_ref + 68 * i)
    return dev.get(d_out, nseg * 68).reshape(nseg, 68), dev.get(d_ref, nseg * 68).reshape(nseg, 68)


def check_msm(ctx, dev, oracle, curve, bases, scalars, segs, naive=True):
    got, ref = msm_segments(ctx, dev, curve, bases, scalars, segs)
    for i, (lo, hi) in enumerate(segs):
        if hi == lo:
            assert got[i, 64:68].view(np.uint32)[0] == 1 and not got[i, :64].any(), (i, lo, hi)
            continue
        assert (record_to_affine(got[i]) == record_to_affine(ref[i])).all() and (got[i, 64:68] == ref[i, 64:68]).all(), ("mina_msm_dev", i, lo, hi)
        if naive:
            assert (record_to_affine(got[i]) == oracle.msm_naive(curve, bases[lo:hi], scalars[lo:hi])).all(), ("oracle", i, lo, hi)
    return got


LENGTHS = [0, 1, 31, 32, 33, 257]


def contiguous(lengths):
    out, at = [], 0
    for ln in lengths:
        out.append((at, at + ln)); at += ln
    return out


@pytest.mark.parametrize("curve", [1, 0])
def test_segment_lengths_around_the_group_law_switch(ctx, dev, oracle, points, curve):
    """one call with segments of 0, 1, 31, 32, 33 and 257 points (six problems: one lane per bucket), then each length as a call of its own (one problem: tasks)"""
    segs = contiguous(LENGTHS)
    n = segs[-1][1]
    bases, sc = points[curve][:n], rand_scalars(n, SCALAR_MOD[curve], seed=7 + curve)
    check_msm(ctx, dev, oracle, curve, bases, sc, segs)
    for lo, hi in segs:
        check_msm(ctx, dev, oracle, curve, bases, sc, [(lo, hi)], naive=False)


@pytest.mark.parametrize("curve", [1, 0])
@pytest.mark.parametrize("nseg", [1, 2, 3, 4, 5, 65])
def test_segment_counts_around_the_accumulate_switch(ctx, dev, oracle, points, curve, nseg):
    """nprob = 3 | 4 is where the pipeline goes from tasks to one lane per bucket; 65 segments of 1 .. 9 points make more than one block of every per-problem launch"""
    lengths = [1 + (5 * i + nseg) % 9 for i in range(nseg)]
    segs = contiguous(lengths)
    n = segs[-1][1]
    check_msm(ctx, dev, oracle, curve, points[curve][:n], rand_scalars(n, SCALAR_MOD[curve], seed=100 + nseg), segs, naive=nseg <= 5)


@pytest.mark.parametrize("curve", [1, 0])
def test_ragged_overlapping_and_out_of_order_segments(ctx, dev, oracle, points, curve):
    n = 200
    segs = [(150, 200), (0, 0), (3, 40), (40, 41), (10, 120), (199, 200), (200, 200), (60, 93)]      # gaps (41 .. 59 of no segment but the long one), overlaps, empties
    check_msm(ctx, dev, oracle, curve, points[curve][:n], rand_scalars(n, SCALAR_MOD[curve], seed=31), segs)


@pytest.mark.parametrize("curve", [1, 0])
@pytest.mark.parametrize("pad", [0, 40])
def test_no_leak_across_a_segment_boundary(ctx, dev, oracle, points, curve, pad):
    """P in segment s and -P with the same scalar at the start of segment s + 1: neither result may be infinity (a reference that crossed the boundary would cancel
    them); the same pair inside one segment sums to infinity.  pad = 40 puts the pair into segments long enough for the 29-bit law and its redo queue."""
    g = points[curve]
    neg = g[0].copy()
    neg[32:] = oracle.int_to_le(BASE_MOD[curve] - oracle.le_to_int(g[0, 32:]))
    k = rand_scalars(1, SCALAR_MOD[curve], seed=5)[0]
    zeros = np.zeros((pad, 32), np.uint8)
    fill = g[1:1 + pad]
    #         segment 0: fill, P | segment 1: -P, fill | segment 2: fill, P, -P
    bases = np.concatenate([fill, g[:1], neg[None], fill, fill, g[:1], neg[None]])
    sc = np.concatenate([zeros, k[None], k[None], zeros, zeros, k[None], k[None]])
    segs = [(0, pad + 1), (pad + 1, 2 * pad + 2), (2 * pad + 2, 3 * pad + 4)]
    got = check_msm(ctx, dev, oracle, curve, bases, sc, segs)
    assert not got[0, 64:68].any() and not got[1, 64:68].any() and got[0, :32].any()
    assert (got[0, :32] == got[1, :32]).all() and not (got[0, 32:64] == got[1, 32:64]).all()      # k P and -k P
    assert got[2, 64:68].view(np.uint32)[0] == 1 and not got[2, :64].any()


@pytest.mark.parametrize("curve", [1, 0])
def test_scalar_distributions(ctx, dev, oracle, points, curve):
    """per distribution five segments of 1, 33, 32, 257 and 31 points: every scalar equal (one bucket per window holds a whole segment: the heavy-bucket kernel),
    all zero (no entry at all), every window at half range (the carry chain of the signed digits runs through every window), duplicated points"""
    r = SCALAR_MOD[curve]
    segs = contiguous([1, 33, 32, 257, 31])
    n = segs[-1][1]
    g = points[curve][:n]
    half = sum(0x80 << (8 * i) for i in range(31)) | (0x20 << 248)       # c = 8: every raw digit 128 = half the window; the top one below the modulus
    assert half < r
    cases = {
        "all_equal": (g, np.repeat(rand_scalars(1, r, seed=10), n, axis=0)),
        "zeros": (g, np.zeros((n, 32), np.uint8)),
        "half_range_windows": (g, np.repeat(oracle.ints_to_le([half]), n, axis=0)),
        "half_range_then_carry": (g, oracle.ints_to_le([half + 1 if i % 2 else half for i in range(n)])),
        "duplicated_points": (np.repeat(g[:3], (n + 2) // 3, axis=0)[:n], rand_scalars(n, r, seed=11)),
        "duplicated_points_equal_scalars": (np.repeat(g[:1], n, axis=0), oracle.ints_to_le([7] * n)),
    }
    for name, (bases, sc) in cases.items():
        got = check_msm(ctx, dev, oracle, curve, bases, sc, segs)
        if name == "zeros":
            assert (np.ascontiguousarray(got[:, 64:68]).view(np.uint32) == 1).all(), name


def test_long_segments_on_the_atomic_counting_sort(oracle, srs_oracle):
    """The atomic counting sort over segments (msm_digits_seg_kernel, msm_scatter_kernel): the driver leaves the partitioned sort when its table of
    partitions x sort blocks x problems outgrows 2^22 words.  A longest segment of 2^17 - 1 points takes c = 13: 20 windows of 4096 buckets = 81920 buckets per
    problem in partitions of 2^9 = 160 partitions, and 512 sort blocks of 256 scalars.  160 x 512 x 53 segments = 4 341 760 > 2^22 = 4 194 304 (51 segments
    would still fit); 131071 x 20 x 53 = 1.39 x 10^8 entries are below the pipeline's 2^28.  The segments are overlapping ranges of ONE array of 2^17 points (the
    65536 SRS points twice: the repeats meet in one bucket wherever their digits agree), three of them long, two empty, the rest short and ragged.  On a
    context of its own: the workspace of this shape is several GiB and grow-only."""
    import mina_bridge_amd as m
    curve, n = 0, 131072
    g, _ = srs_oracle[curve]
    bases = np.concatenate([g, g])
    sc = rand_scalars(n, SCALAR_MOD[curve], seed=53)
    sc[::11] = 0
    segs = [(0, n - 1), (1, n), (65536, n), (0, 0), (n, n), (40000, 40001), (70000, 70031), (70000, 70032), (65000, 66000)]
    segs += [(2500 * i, 2500 * i + 1 + 37 * i) for i in range(44)]
    assert len(segs) == 53 and max(hi - lo for lo, hi in segs) == (1 << 17) - 1
    c = m.MinaContext(0)
    d = Dev(c)
    try:
        got = check_msm(c, d, oracle, curve, bases, sc, segs, naive=False)
        lo, hi = segs[8]
        assert (record_to_affine(got[8]) == oracle.msm_pippenger(curve, bases[lo:hi], sc[lo:hi], threads=8)).all()
    finally:
        d.close()
        c.close()


# ------------------------------------------------------------------------------------------------ the fold
def fold_segments(ctx, dev, field, k, chals, weights, segs):
    batch, nseg, n = len(chals) // k, len(segs), 1 << k
    d_c, d_w = dev.put(chals), (dev.put(weights) if weights is not None else 0)
    d_lo, d_hi = dev.put(np.array([s[0] for s in segs], np.uint32)), dev.put(np.array([s[1] for s in segs], np.uint32))
    d_out, d_ref = dev.alloc(nseg * n * 32), dev.alloc(nseg * n * 32)
    ctx.b_poly_fold_segments_dev(field, k, batch, nseg, d_lo, d_hi, d_c, d_w, d_out)
    for i, (lo, hi) in enumerate(segs):
        if hi > lo:
            ctx.b_poly_fold_dev(field, k, hi - lo, d_c + 32 * k * lo, (d_w + 32 * lo) if d_w else 0, d_ref + 32 * n * i)
    return dev.get(d_out, nseg * n * 32).reshape(nseg, n * 32), dev.get(d_ref, nseg * n * 32).reshape(nseg, n * 32)


def fold_patterns(batch):
    """segment tables for a batch: the whole batch; halves; ragged with empties, a gap and an overlap; single proofs"""
    pats = [[(0, batch)]]
    if batch >= 2:
        h = batch // 2
        pats.append([(0, h), (h, batch)])
        pats.append([(batch - 1, batch), (0, 0), (0, 1), (1, max(1, h - 1)), (h, batch), (batch, batch), (h // 2, h + 1)])
    if batch >= 65:
        pats.append([(i, i + 1) for i in range(0, 65)])
    return pats


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("k,batch", [(1, 1), (1, 2), (1, 65), (1, 300), (4, 1), (4, 2), (4, 65), (4, 300), (15, 1), (15, 2), (15, 65), (15, 300)])
def test_fold_segments_equal_the_single_fold(ctx, dev, oracle, field, k, batch):
    """batch 300 holds a range of 300 proofs, which mina_b_poly_fold_dev folds on the matrix cores (256 and more), beside ranges it folds with the VALU kernel and
    single proofs; the sums are exact modulo p, so every byte agrees.  At k = 4 one segment is also checked against the CPU oracle's coefficients."""
    mod = P if field == 0 else Q
    chals, w = rand_scalars(batch * k, mod, seed=k * 1000 + batch), rand_scalars(batch, mod, seed=k * 1000 + batch + 1)
    pats = fold_patterns(batch) if k < 15 else fold_patterns(batch)[:3]      # k = 15: 1 MiB per segment -- not the 65 single-proof segments
    for segs in pats:
        got, ref = fold_segments(ctx, dev, field, k, chals, w, segs)
        for i, (lo, hi) in enumerate(segs):
            if hi == lo:
                assert not got[i].any(), (segs, i)
            else:
                assert (got[i] == ref[i]).all(), (segs, i)
    if k == 4:
        got, _ = fold_segments(ctx, dev, field, k, chals, None, [(0, 1), (batch - 1, batch)])      # null weights: every weight 1 -> the coefficients themselves
        assert (got[0] == np.asarray(oracle.b_poly_coefficients(field, chals[:k])).reshape(-1)).all()
        assert (got[1] == np.asarray(oracle.b_poly_coefficients(field, chals[(batch - 1) * k:])).reshape(-1)).all()


# ------------------------------------------------------------------------------------------------ bad arguments
def test_bad_arguments_are_refused(ctx, dev, points):
    import mina_bridge_amd as m
    lib, h = m.load_library(), ctx._h
    v, z = ctypes.c_void_p, ctypes.c_size_t
    n = 8
    d_b, d_s = dev.put(points[1][:n]), dev.put(rand_scalars(n, P, seed=1))
    d_lo, d_hi, d_out = dev.put(np.array([0, 4], np.uint32)), dev.put(np.array([4, 8], np.uint32)), dev.alloc(2 * 68 + 1024)

    def msm(n_total=n, nseg=2, lo=d_lo, hi=d_hi, b=d_b, s=d_s, out=d_out, ctx_h=h, curve=1):
        return lib.mina_msm_segments_dev(ctx_h, curve, z(n_total), z(nseg), v(lo), v(hi), v(b), v(s), v(out))
    assert msm() == 0
    assert msm(ctx_h=None) == MINA_ERR_ARG and lib.mina_last_error()
    for kw in ({"lo": None}, {"hi": None}, {"b": None}, {"s": None}, {"out": None}, {"curve": 2}, {"nseg": 0},
               {"lo": d_lo + 2}, {"hi": d_hi + 1}, {"out": d_out + 2}, {"b": d_b + 4}, {"s": d_s + 8},          # misaligned
               {"n_total": (1 << 24) + 1}, {"nseg": 16385}):                                                 # 128 buckets x 32 windows x 16385 segments > 2^26
        assert msm(**kw) == MINA_ERR_ARG, kw
    d_rev, d_past = dev.put(np.array([5, 4], np.uint32)), dev.put(np.array([4, 9], np.uint32))
    assert msm(lo=d_rev, hi=d_hi) == MINA_ERR_ARG              # segment 0 = [5, 4): end < begin
    assert msm(hi=d_past) == MINA_ERR_ARG                      # end > n_total
    # the entry limit: a longest segment of 2048 points takes 20 windows, 2048 x 20 x 7000 > 2^28 (and 4096 buckets x 20 x 7000 > 2^26)
    big_lo, big_hi = dev.put(np.zeros(7000, np.uint32)), dev.put(np.full(7000, 2048, np.uint32))
    d_bb, d_ss = dev.alloc(2048 * 64), dev.alloc(2048 * 32)
    assert msm(n_total=2048, nseg=7000, lo=big_lo, hi=big_hi, b=d_bb, s=d_ss) == MINA_ERR_ARG

    k, batch = 3, 4
    d_c, d_w = dev.put(rand_scalars(batch * k, P, seed=2)), dev.put(rand_scalars(batch, P, seed=3))
    d_fo = dev.alloc(2 * 8 * 32 + 64)
    d_fhi = dev.put(np.array([4, 4], np.uint32))

    def fold(field=0, k_=k, batch_=batch, nseg=2, lo=d_lo, hi=d_fhi, c=d_c, w=d_w, out=d_fo, ctx_h=h):
        return lib.mina_b_poly_fold_segments_dev(ctx_h, field, ctypes.c_uint32(k_), z(batch_), z(nseg), v(lo), v(hi), v(c), v(w), v(out))
    assert fold() == 0
    assert fold(w=None) == 0                                   # null weights are weight 1
    assert fold(ctx_h=None) == MINA_ERR_ARG
    for kw in ({"lo": None}, {"hi": None}, {"c": None}, {"out": None}, {"field": 2}, {"k_": 0}, {"k_": 21}, {"batch_": 0}, {"nseg": 0}, {"nseg": 65536},
               {"lo": d_lo + 2}, {"hi": d_fhi + 2}, {"c": d_c + 2}, {"w": d_w + 2}, {"out": d_fo + 8}, {"k_": 20, "nseg": 257}):
        assert fold(**kw) == MINA_ERR_ARG, kw
    assert fold(hi=d_hi) == MINA_ERR_ARG                       # end 8 > batch 4
    assert fold(lo=d_rev) == MINA_ERR_ARG                      # begin 5 > end 4
    ctx.synchronize()
