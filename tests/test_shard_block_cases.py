"""The case generator of the exchange-kernel tests (tests/shard_block_cases.py) under the CPU oracle: every relation a case is named after holds, every edge the
GPU test relies on is really among the values, and the comparisons reject a reference that is wrong in the way a kernel could be -- so that
tests/test_gpu_shard_blocks.py cannot pass vacuously."""
import numpy as np
import pytest

import shard_block_cases as S


@pytest.fixture(scope="module")
def points(oracle):
    return {c: oracle.srs_create(c, 32, threads=4)[0] for c in (0, 1)}


@pytest.fixture(scope="module")
def point_cases(oracle, points):
    return {c: S.points_sum_cases(oracle, c, points[c]) for c in (0, 1)}


INF = np.zeros(64, np.uint8)


def test_records_round_trip():
    pt = np.arange(1, 65, dtype=np.uint8)
    r = S.rec(pt)
    assert r.shape == (68,) and (r[:64] == pt).all() and not r[64:].any() and (S.unrec(r) == pt).all()
    r = S.rec(INF)
    assert not r[:64].any() and r[64:].tolist() == [1, 0, 0, 0] and not S.unrec(r).any()
    assert (S.rec_inf() == r).all()
    a, b, c = S.rec_inf(1), S.rec_inf(2), S.rec_inf_nonunit(1)
    assert a[:64].all() and b[:64].all() and (a[:64] != b[:64]).any() and a[64:].tolist() == [1, 0, 0, 0]
    assert (c[:64] == a[:64]).all() and c[64:].tolist() == [0, 1, 0, 0] and S.is_flagged(c) and not S.unrec(c).any()


@pytest.mark.parametrize("curve", [0, 1])
def test_garbage_is_canonical_and_off_both_curves(oracle, curve):
    for i in range(256):
        g = S.garbage_coords(i)
        assert g.all() and max(S.from_le(g)) < min(S.P, S.Q) and not oracle.is_on_curve(curve, g), i


@pytest.mark.parametrize("curve", [0, 1])
def test_point_cases_are_what_their_names_say(oracle, points, point_cases, curve):
    g, cases = points[curve], point_cases[curve]
    Pt, Qt, Rt = g[0], g[1], g[2]
    assert len({x.tobytes() for x in g[:24]}) == 24
    two_p = oracle.scalar_mul(curve, Pt, S.to_le([2])[0])
    pq = oracle.point_add(curve, Pt, Qt)
    assert set(cases) == {"single", "pair", "double_at_once", "double_late", "cancel_late_then_go_on", "cancel_at_once", "all_infinite", "infinite_first_mid_last",
                          "nonunit_flag", "pallas_total_shape", "long_sparse", "long_dense"}
    total = {name: S.ref_points_sum(oracle, curve, recs) for name, recs in cases.items()}
    # every finite record is on its curve and canonical; every flagged one is not accidentally a point
    for name, recs in cases.items():
        assert recs.dtype == np.uint8 and recs.shape[1:] == (68,), name
        fin = recs[~recs[:, 64:68].any(axis=1)]
        for r in (fin if len(fin) <= 64 else np.unique(fin, axis=0)):
            assert r[:64].any() and oracle.is_on_curve(curve, r[:64]) and max(S.from_le(r[:64])) < S.BASE_MOD[curve], name
    assert (total["single"] == Pt).all() and (total["pair"] == pq).all()
    assert (total["double_at_once"] == two_p).all() and two_p.any()
    assert (cases["double_late"][2, :64] == pq).all() and (total["double_late"] == oracle.scalar_mul(curve, pq, S.to_le([2])[0])).all()
    c = cases["cancel_late_then_go_on"]
    assert not S.ref_points_sum(oracle, curve, c[:3]).any() and (total["cancel_late_then_go_on"] == Rt).all()
    assert (c[2, :32] == pq[:32]).all() and (c[2, 32:64] != pq[32:]).any()
    for name in ("cancel_at_once", "all_infinite", "pallas_total_shape"):
        assert not total[name].any(), name
    a = cases["all_infinite"]
    assert len(a) == 3 and a[:, 64:68].any(axis=1).all() and len({r[:64].tobytes() for r in a}) == 3 and a[:, :64].all()
    f = cases["infinite_first_mid_last"]
    assert [S.is_flagged(r) for r in f] == [True, False, True, False, True] and (total["infinite_first_mid_last"] == pq).all()
    n = cases["nonunit_flag"]
    assert n[1, 64:68].tolist() == [0, 1, 0, 0] and n[1, :64].all() and (total["nonunit_flag"] == pq).all()
    t = cases["pallas_total_shape"]
    assert len(t) == 16 and not t[:, 64:68].any() and len({r.tobytes() for r in t}) == 16
    assert S.ref_points_sum(oracle, curve, t[:8]).any() and S.ref_points_sum(oracle, curve, t[:15]).any()
    s = cases["long_sparse"]
    assert len(s) == 65536 and s[1:-1, 64:68].any(axis=1).all() and s[1:-1, :64].all() and (total["long_sparse"] == pq).all()
    assert (s[1:-1, 65] == 1).any() and (s[1:-1, 64] == 1).any()
    d = cases["long_dense"]
    flagged = d[:, 64:68].any(axis=1)
    assert len(d) == 1000 and 60 <= flagged.sum() <= 140 and len(np.unique(d[~flagged], axis=0)) == 12 and total["long_dense"].any()
    # equal and opposite neighbours are really there, and the fold goes through the special branches of a mixed addition: acc == next (doubling), acc == -next
    acc, doubled, cancelled = INF, 0, 0
    for r in d[~flagged]:
        doubled += bool((acc == r[:64]).all())
        cancelled += bool(acc.any() and (acc == S.neg(curve, r[:64])).all())
        acc = oracle.point_add(curve, acc, r[:64])
    assert doubled >= 3 and cancelled >= 3, (doubled, cancelled)


def fold_without_skipping(oracle, curve, recs):
    """a WRONG reference: the flag word is ignored, the coordinates of every record go into the group law"""
    acc = INF
    for r in recs:
        acc = oracle.point_add(curve, acc, r[:64])
    return acc


@pytest.mark.parametrize("curve", [0, 1])
def test_a_fold_that_does_not_skip_flagged_records_is_rejected(oracle, point_cases, curve):
    for name in ("all_infinite", "infinite_first_mid_last", "nonunit_flag", "long_dense"):
        recs = point_cases[curve][name]
        assert (S.rec(fold_without_skipping(oracle, curve, recs)) != S.rec(S.ref_points_sum(oracle, curve, recs))).any(), name


def sum_without_final_reduction(field, mat):
    """a WRONG reference: every step but the last reduces, the last conditional subtraction is left out"""
    p = S.FIELD_MOD[field]
    return [sum(col[:-1]) % p + col[-1] for col in zip(*mat)]


def sum_transposed(field, rows, m, mat):
    """a WRONG reference: the matrix read as [m][rows]"""
    flat = [v for row in mat for v in row]
    return S.ref_sum_rows(field, [[flat[j * rows + r] for j in range(m)] for r in range(rows)])


@pytest.mark.parametrize("field", [0, 1])
def test_row_sum_cases_hold_every_edge(field):
    p = S.FIELD_MOD[field]
    cases = S.sum_rows_cases(field)
    assert [(r, m) for r, m, _ in cases.values()] == S.SUM_ROWS_SHAPES and all(r != m for r, m in S.SUM_ROWS_SHAPES[1:])
    hits = high = zeros = 0
    for name, (rows, m, mat) in cases.items():
        assert len(mat) == rows and all(len(row) == m for row in mat), name
        vals = [v for row in mat for v in row]
        assert all(0 <= v < p for v in vals), name
        ref = S.ref_sum_rows(field, mat)
        assert len(ref) == m and ref == [sum(mat[r][j] for r in range(rows)) % p for j in range(m)]
        hits += S.running_sums_hit_p(field, mat)
        high += sum(v >= 1 << 254 for v in vals)
        zeros += sum(v == 0 for v in vals)
        fams = {(j + list(cases).index(name)) % S.N_FAMILIES: j for j in range(m)}
        if 0 in fams:
            assert ref[fams[0]] == (p - rows) % p, name
        if rows > 1:
            assert S.to_le(sum_without_final_reduction(field, mat)).tobytes() != S.to_le(ref).tobytes(), name
            assert sum_transposed(field, rows, m, mat) != ref, name
        if rows % 2 == 0 and 1 in fams:
            assert ref[fams[1]] == 0, name
    assert hits >= 1 and high >= 1 and zeros >= 1
    # the full-width shapes hold every family; in each of them some column's running sum equals p exactly and some value lies in [2^254, p)
    for name in ("3x257", "8x255", "8x256"):
        _, _, mat = cases[name]
        assert S.running_sums_hit_p(field, mat) >= 3 and any(1 << 254 <= v < p for row in mat for v in row), name
    # seeded: a second call gives the same matrices
    assert S.sum_rows_cases(field)["8x255"][2] == cases["8x255"][2]


def test_references_on_hand_made_inputs():
    assert S.ref_sum_rows(0, [[S.P - 1, 1, 5], [1, S.P - 1, 6]]) == [0, 0, 11]
    assert S.ref_sum_rows(1, [[S.Q - 1], [S.Q - 1], [S.Q - 1]]) == [S.Q - 3]
    assert S.running_sums_hit_p(0, [[S.P - 1, 1], [1, 1]]) == 1
    assert S.from_le(S.to_le([0, 1, S.P - 1])) == [0, 1, S.P - 1]
