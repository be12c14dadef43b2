"""The divstep inversion on the device (mina_bridge_amd/csrc/fe_modinv.cuh): mina_field_inv_gcd against mina_field_inv and the CPU oracle, and the MSM finishes
under mina_ctx_set_fast_inverse (msm_finish_gcd_kernel, msm_tail_gcd_kernel) against the mode off on the same context and the CPU oracle.  The inverse of a field
element is unique, so every comparison is byte equality.  Shapes are the small ones of tests/test_gpu_msm_fused_tail.py: the inversion sees one XYZZ result per
problem whatever the size of the MSM in front of it."""
import numpy as np
import pytest

import modinv_model as M
from conftest import rand_scalars
from dev_helpers import Dev, record_to_affine

pytestmark = pytest.mark.gpu

P = 0x40000000000000000000000000000000224698FC094CF91B992D30ED00000001
Q = 0x40000000000000000000000000000000224698FC0994A8DD8C46EB2100000001
SCALAR_MOD = {0: Q, 1: P}
BASE_MOD = {0: P, 1: Q}


@pytest.fixture(scope="module")
def ictx():
    """a context of its own with both 2^16 SRS: the mode is context state, and the session's shared context never sees it"""
    import mina_bridge_amd as m
    c = m.MinaContext(0)
    for f in (0, 1):
        c.poseidon_set_params(f, m.poseidon_params.default_params_bytes(f))
    for curve in (0, 1):
        c.srs_create(curve, 65536)
    yield c
    c.set_fast_inverse(False)
    c.set_msm_fused_tail(False)
    c.close()


@pytest.fixture
def dev(ictx):
    d = Dev(ictx)
    yield d
    d.close()


# ------------------------------------------------------------------------------------------------ the batch entry point
def check_inv(ictx, oracle, F, xs):
    a = oracle.ints_to_le(xs)
    gcd, fermat = ictx.field_inv_gcd(F, a), ictx.field_inv(F, a)
    assert gcd.shape == (len(xs), 32) and (gcd == fermat).all()
    want = oracle.field_inv(F, oracle.ints_to_le([x or 1 for x in xs]))     # (the oracle's inverse is defined away from zero)
    for i, x in enumerate(xs):
        assert (gcd[i] == want[i]).all() if x else not gcd[i].any(), hex(x)


@pytest.mark.parametrize("F", [0, 1])
def test_field_inv_gcd_on_the_corner_set(ictx, oracle, F):
    xs = M.corners(F) + M.sized(F, 4, "modinv/gpu")
    check_inv(ictx, oracle, F, xs)
    got = ictx.field_inv_gcd(F, oracle.ints_to_le(xs))
    for x, row in zip(xs, got):
        assert oracle.le_to_int(row) == pow(x, M.P[F] - 2, M.P[F]), hex(x)


@pytest.mark.parametrize("F", [0, 1])
def test_field_inv_gcd_on_4096_random_elements(ictx, oracle, F):
    check_inv(ictx, oracle, F, M.randoms(F, 4096, "modinv/gpu"))


@pytest.mark.parametrize("F", [0, 1])
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_field_inv_gcd_at_the_edges_of_the_block(ictx, oracle, F, n):
    xs = M.randoms(F, n, f"modinv/gpu/{n}")
    xs[n // 2] = 0                                               # zero maps to zero, in the middle of a block
    xs[-1] = M.P[F] - 1
    check_inv(ictx, oracle, F, xs)


def test_field_inv_gcd_refuses_what_field_inv_refuses(ictx):
    import mina_bridge_amd as m
    with pytest.raises(m.MinaError):
        ictx.field_inv_gcd(2, np.zeros((1, 32), np.uint8))
    assert ictx.field_inv_gcd(0, np.zeros((0, 32), np.uint8)).shape == (0, 32)


# ------------------------------------------------------------------------------------------------ the MSM finishes
def off_on(ictx, call, finishes=1):
    """call() with the mode off, then on -> (off result, on result); `finishes` finishes are counted under the form that ran and none under the other"""
    ictx.set_fast_inverse(False)
    s0 = ictx.inverse_stats()
    off = call()
    s1 = ictx.inverse_stats()
    ictx.set_fast_inverse(True)
    try:
        on = call()
        s2 = ictx.inverse_stats()
    finally:
        ictx.set_fast_inverse(False)
    assert s1["fermat_finishes"] - s0["fermat_finishes"] == finishes and s1["gcd_finishes"] == s0["gcd_finishes"], (s0, s1)
    assert s2["gcd_finishes"] - s1["gcd_finishes"] == finishes and s2["fermat_finishes"] == s1["fermat_finishes"], (s1, s2)
    return off, on


def negated(oracle, curve, pt):
    out = pt.copy()
    out[32:] = oracle.int_to_le(BASE_MOD[curve] - oracle.le_to_int(pt[32:]))
    return out


@pytest.mark.parametrize("fused_tail", [False, True])
@pytest.mark.parametrize("curve", [1, 0])
@pytest.mark.parametrize("n", [1, 9, 1000])
def test_msm_srs(ictx, oracle, srs_oracle, curve, n, fused_tail):
    """the staged finish, and -- the fused tail on together with the fast inverse -- msm_tail_gcd_kernel"""
    sc = rand_scalars(n, SCALAR_MOD[curve], seed=1600 + n)
    ictx.set_msm_fused_tail(fused_tail)
    try:
        t0 = ictx.msm_tail_stats()
        off, on = off_on(ictx, lambda: ictx.msm_srs(curve, sc))
        t1 = ictx.msm_tail_stats()
    finally:
        ictx.set_msm_fused_tail(False)
    assert t1["fused_runs" if fused_tail else "staged_runs"] - t0["fused_runs" if fused_tail else "staged_runs"] == 2
    g = srs_oracle[curve][0]
    exp = oracle.msm_naive(curve, g[:n], sc) if n < 16 else oracle.msm_pippenger(curve, g[:n], sc, threads=8)
    assert (on == off).all() and (on == exp).all()


@pytest.mark.parametrize("fused_tail", [False, True])
@pytest.mark.parametrize("curve", [1, 0])
@pytest.mark.parametrize("n", [1, 257, 2100])
def test_msm_on_user_bases(ictx, oracle, srs_oracle, curve, n, fused_tail):
    """a single point; one row per bucket set (c = 8); 32 rows in each of 20 sets (c = 13): the Horner in front of the inversion has 1, 32 and 20 sets"""
    bases = srs_oracle[curve][0][:n][::-1].copy()
    sc = rand_scalars(n, SCALAR_MOD[curve], seed=1700 + n)
    ictx.set_msm_fused_tail(fused_tail)
    try:
        off, on = off_on(ictx, lambda: ictx.msm(curve, bases, sc))
    finally:
        ictx.set_msm_fused_tail(False)
    exp = oracle.msm_naive(curve, bases, sc) if n < 64 else oracle.msm_pippenger(curve, bases, sc, threads=8)
    assert (on == off).all() and (on == exp).all()


@pytest.mark.parametrize("fused_tail", [False, True])
@pytest.mark.parametrize("curve", [1, 0])
def test_a_result_at_infinity_has_flag_one_and_zero_coordinates(ictx, dev, oracle, srs_oracle, curve, fused_tail):
    n = 9
    d_s, d_out = dev.put(np.zeros((n, 32), np.uint8)), dev.alloc(2 * 68)

    def zero_scalars():
        ictx.dev_upload(d_out, np.full(68, 0xEE, np.uint8))
        ictx.msm_srs_dev(curve, n, d_s, d_out)
        return dev.get(d_out, 68)
    g = srs_oracle[curve][0]
    pair = np.stack([g[3], negated(oracle, curve, g[3])])
    d_b, d_s2 = dev.put(pair), dev.put(oracle.ints_to_le([99, 99]))
    d_lo, d_hi = dev.put(np.array([0], np.uint32)), dev.put(np.array([2], np.uint32))

    def point_plus_its_negative():
        ictx.dev_upload(d_out, np.full(68, 0xEE, np.uint8))
        ictx.msm_segments_dev(curve, 2, 1, d_lo, d_hi, d_b, d_s2, d_out)
        return dev.get(d_out, 68)
    ictx.set_msm_fused_tail(fused_tail)
    try:
        for call in (zero_scalars, point_plus_its_negative):
            off, on = off_on(ictx, call)
            assert (on == off).all() and on[64:68].view(np.uint32)[0] == 1 and not on[:64].any()
        off, on = off_on(ictx, lambda: ictx.msm(curve, pair, oracle.ints_to_le([99, 99])))
        assert not on.any() and not off.any()
    finally:
        ictx.set_msm_fused_tail(False)


@pytest.mark.parametrize("curve", [1, 0])
@pytest.mark.parametrize("nprob", [3, 5])
def test_msm_srs_multi_on_either_side_of_the_bucket_lane_plan(ictx, oracle, srs_oracle, curve, nprob):
    """one finish workgroup per problem; 3 problems accumulate in tasks, 5 give every bucket a lane (the staged tail in both modes)"""
    n = 600
    g = srs_oracle[curve][0]
    sc = rand_scalars(n * nprob, SCALAR_MOD[curve], seed=1800 + nprob).reshape(nprob, n, 32)
    sc[1] = 0                                                    # one problem of the group at infinity: its lane takes the other branch of the finish
    off, on = off_on(ictx, lambda: ictx.msm_srs_multi(curve, sc, nprob))
    assert (on == off).all() and not on[1].any()
    for i in [i for i in range(nprob) if i != 1]:
        assert (on[i] == oracle.msm_pippenger(curve, g[:n], sc[i], threads=4)).all(), i


@pytest.mark.parametrize("fused_tail", [False, True])
@pytest.mark.parametrize("curve", [1, 0])
def test_msm_segments_dev_with_two_segments(ictx, dev, oracle, srs_oracle, curve, fused_tail):
    segs = [(0, 33), (33, 290)]
    n = segs[-1][1]
    bases, sc = srs_oracle[curve][0][100:100 + n], rand_scalars(n, SCALAR_MOD[curve], seed=1900)
    d_b, d_s = dev.put(bases), dev.put(sc)
    d_lo, d_hi = dev.put(np.array([s[0] for s in segs], np.uint32)), dev.put(np.array([s[1] for s in segs], np.uint32))
    d_out = dev.alloc(2 * 68)

    def call():
        ictx.dev_upload(d_out, np.full(2 * 68, 0xEE, np.uint8))
        ictx.msm_segments_dev(curve, n, 2, d_lo, d_hi, d_b, d_s, d_out)
        return dev.get(d_out, 2 * 68).reshape(2, 68)
    ictx.set_msm_fused_tail(fused_tail)
    try:
        off, on = off_on(ictx, call)
    finally:
        ictx.set_msm_fused_tail(False)
    assert (on == off).all()
    for i, (lo, hi) in enumerate(segs):
        ref = oracle.msm_naive if hi - lo < 64 else oracle.msm_pippenger
        assert (record_to_affine(on[i]) == ref(curve, bases[lo:hi], sc[lo:hi])).all(), i


def test_eight_calls_over_four_lanes(oracle, srs_oracle):
    """a context with 4 pipeline lanes: 8 MSMs queued back to back, one wait, the records of the mode off and the oracle's points"""
    import mina_bridge_amd as m
    curve, n, calls = 1, 500, 8
    g = srs_oracle[curve][0]
    sc = rand_scalars(n * calls, P, seed=2000).reshape(calls, n, 32)
    c = m.MinaContext(0)
    try:
        c.srs_create(curve, 65536)
        c.set_pipeline(4)
        d = Dev(c)
        try:
            d_s, d_out = d.put(sc), d.alloc(calls * 68 + 16)
            got = {}
            for on in (False, True):
                c.set_fast_inverse(on)
                c.dev_upload(d_out, np.full(calls * 68, 0xEE, np.uint8))
                before = c.inverse_stats()
                for i in range(calls):
                    c.msm_srs_dev(curve, n, d_s + i * n * 32, d_out + i * 68)
                got[on] = d.get(d_out, calls * 68).reshape(calls, 68)
                after = c.inverse_stats()
                moved, still = ("gcd_finishes", "fermat_finishes") if on else ("fermat_finishes", "gcd_finishes")
                assert after[moved] - before[moved] == calls and after[still] == before[still]
            assert (got[True] == got[False]).all()
            for i in range(calls):
                assert (record_to_affine(got[True][i]) == oracle.msm_pippenger(curve, g[:n], sc[i], threads=4)).all(), i
        finally:
            c.set_fast_inverse(False)
            d.close()
    finally:
        c.close()


def test_inverse_stats_follow_the_mode(ictx):
    """off: only fermat_finishes moves; on: only gcd_finishes; off again: the first"""
    import mina_bridge_amd as m
    sc = rand_scalars(20, P, seed=2100)
    seen = []
    for on in (False, True, False):
        ictx.set_fast_inverse(on)
        before = ictx.inverse_stats()
        ictx.msm_srs(1, sc)
        ictx.msm_srs(0, rand_scalars(20, Q, seed=2101))
        after = ictx.inverse_stats()
        seen.append((after["gcd_finishes"] - before["gcd_finishes"], after["fermat_finishes"] - before["fermat_finishes"]))
    assert seen == [(0, 2), (2, 0), (0, 2)]
    with pytest.raises(m.MinaError):
        ictx._ck(ictx._lib.mina_ctx_set_fast_inverse(ictx._h, 2), "mina_ctx_set_fast_inverse")
    assert ictx.inverse_stats()["fermat_finishes"] == after["fermat_finishes"]


def test_accumulator_check_multi_gives_the_same_verdicts(ictx, srs_oracle):
    from oracle import state_job_ref as J
    curve, k = 1, 10
    g = srs_oracle[curve][0]
    inst = [J.make_accumulator(curve, g, k, 2200 + b) for b in range(2)]
    pre = np.concatenate([np.asarray(i[0], np.uint8).reshape(-1, 32) for i in inst]); sg = np.stack([np.asarray(i[1], np.uint8).reshape(64) for i in inst])
    bad = sg.copy(); bad[1] = sg[0]                              # another proof's commitment: a valid point, the wrong one

    def call():
        return [ictx.accumulator_check_multi(curve, k, pre, s).tolist() for s in (sg, bad)]
    ictx.set_fast_inverse(False)
    off = call()
    before = ictx.inverse_stats()
    ictx.set_fast_inverse(True)
    try:
        on = call()
    finally:
        ictx.set_fast_inverse(False)
    after = ictx.inverse_stats()
    assert on == off == [[1, 1], [1, 0]]
    assert after["fermat_finishes"] == before["fermat_finishes"]          # whatever finishes the check queued with the mode on were the divstep ones
