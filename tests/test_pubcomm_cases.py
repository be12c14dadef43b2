"""The inputs of tests/test_gpu_pubcomm_degenerate.py, validated on the CPU: a big-int model of the direct commitment kernels' digit walk (srs_helpers.walk) must
report, for every named row, the exceptional case of the group law the row claims to meet -- at the claimed scalar, window and lane -- and none for the control
rows; and the crafted SRSs must really have the Lagrange basis L_i = c_i G.  If the lane rule or the digit rule of lagrange.cuh changes, the model changes with
it and these tests say which GPU rows went dead."""
import pytest

import srs_helpers as S


@pytest.mark.parametrize("curve", [0, 1])
def test_named_rows_meet_the_exceptional_cases_they_claim(curve):
    r = S.scalar_modulus(curve)
    c, t = S.s1_coefficients(curve), S.blinder(curve)
    assert c[0] == c[1] == c[8] == 1 and c[2] == c[16] == r - 1 and c[3] == c[24] == 0 and c[4] == 2 and all(c[i] for i in range(64) if i not in (3, 24))
    cases = S.s1_cases(curve, c, t)
    for name, case in cases.items():
        pubs = case["pubs"]
        assert len(pubs) == S.NPUB and all(0 <= p < 1 << 255 for p in pubs), name
        w8, w64 = S.walk(c, pubs, 8, r), S.walk(c, pubs, 64, r)
        assert w8["total"] == w64["total"] == case.get("total", w8["total"]), name
        for step in case.get("steps8", []):
            assert step in w8["steps"], (name, step, w8["steps"])
        for node in case.get("tree64", []):
            assert node in w64["tree"], (name, node, w64["tree"])
        if case.get("clean"):
            assert not (w8["steps"] or w8["tree"] or w8["pairs"] or w64["steps"] or w64["tree"] or w64["pairs"]), (name, w8, w64)
    # the rows for the finish: A = +-H
    for name in ("a_eq_h_one", "a_eq_h"):
        assert S.walk(c, cases[name]["pubs"], 8, r)["total"] == t
    for name in ("a_eq_neg_h_one", "a_eq_neg_h"):
        assert S.walk(c, cases[name]["pubs"], 8, r)["total"] == r - t
    # "equal" in the 64-lane form: lanes 0 and 8 end equal; "large" reduces to "large_reduced" and really holds scalars at and above r
    assert ("equal", 0, 8) in S.walk(c, cases["equal"]["pubs"], 64, r)["pairs"]
    assert [p % r for p in cases["large"]["pubs"]] == cases["large_reduced"]["pubs"] and sum(p >= r for p in cases["large"]["pubs"]) >= 7
    assert ("opposite", 0, 31, 0) in S.walk(c, cases["large"]["pubs"], 64, r)["steps"]
    # the exceptional add of the two "after a negative digit" rows comes after the digit -7 and its carry
    assert S.signed_digits(cases["mid_neg"]["pubs"][8])[:3] == [-7, 1, 3] and S.signed_digits(cases["mid_neg"]["pubs"][0])[:3] == [7, -1, 3]
    assert S.signed_digits(cases["mid"]["pubs"][0])[:3] == [-7, 0, 3]
    # 5 public inputs: one scalar per lane in either form, the cases sit in the tree
    small = S.s1_cases_small(curve, c, t)
    for name, case in small.items():
        for lanes in (8, 64):
            w = S.walk(c[:S.NPUB_SMALL], case["pubs"], lanes, r)
            assert w["total"] == case.get("total", w["total"]), name
            for node in case.get("tree8", []):
                assert node in w["tree"], (name, lanes, w["tree"])
            if case.get("clean"):
                assert not (w["steps"] or w["tree"] or w["pairs"]), (name, lanes, w)


def test_walk_model_on_hand_worked_scalars():
    """the model itself, on walks short enough to follow by hand (r = 1009, every basis point G)"""
    r = 1009
    assert S.signed_digits(0x0300F9)[:4] == [-7, 1, 3, 0] and S.signed_digits(0x80)[:2] == [128, 0] and S.signed_digits(0x81)[:2] == [-127, 1]
    assert S.signed_digits((1 << 255) - 1) == [-1] + [0] * 30 + [128]
    assert S.prefix_below(0x0300F9, 2) == 249 and S.prefix_below(0x0300F9, 1) == -7
    w = S.walk([1, 1], [5, 5], 1, r)                               # one lane: 5 G, then 5 G again
    assert w["steps"] == [("equal", 1, 0, 0)] and w["total"] == 10 and not w["tree"]
    w = S.walk([1, r - 1], [5, 5], 2, r)                           # two lanes: 5 G and -5 G meet in the tree
    assert not w["steps"] and w["tree"] == [("opposite", 1, 0)] and w["pairs"] == [("opposite", 0, 1)] and w["total"] == 0
    w = S.walk([1, 0, 1], [5, 5, 6], 1, r)                         # a basis point at infinity is skipped, 5 G + 6 G is an ordinary add
    assert not w["steps"] and w["total"] == 11
    w = S.walk([1], [r], 1, r)                                     # r = 0x3f1: digits -15, +4; -15 G + 1024 G = r G = infinity
    assert S.signed_digits(r)[:2] == [-15, 4] and w["steps"] == [("opposite", 0, 1, 0)] and w["total"] == 0


@pytest.mark.parametrize("curve", [0, 1])
def test_crafted_srs_has_the_claimed_lagrange_basis(oracle, curve):
    """L_i = (1/n) sum_j w^(-ij) g_j = c_i G, by the oracle's MSM over the defining sum, for the indices that carry relations and a random one; S2 as well"""
    r = S.scalar_modulus(curve)
    n = 1 << S.LOG2_DOMAIN
    w_inv, n_inv = pow(S.domain_root(r, S.LOG2_DOMAIN), r - 2, r), pow(n, r - 2, r)
    t = S.blinder(curve)
    for c, sample in ((S.s1_coefficients(curve), (0, 1, 2, 3, 8, 16, 24, 37)), (S.s2_coefficients(), (0, 1, 33))):
        g, h, G = S.structured_srs(oracle, curve, c, t)
        assert g.shape == (S.DEPTH, 64) and all(oracle.is_on_curve(curve, p) for p in g[:n]) and oracle.is_on_curve(curve, h)
        for i in sample:
            sc = [pow(w_inv, (i * j) % n, r) * n_inv % r for j in range(n)]
            assert (oracle.msm_pippenger(curve, g[:n], oracle.ints_to_le(sc), threads=4) == S.point_mul(oracle, curve, G, c[i])).all(), i
        assert (S.reference_commitment(oracle, curve, c, t, G, [0] * S.NPUB) == h).all()
        assert not S.reference_commitment(oracle, curve, c, t, G, [t * pow(c[0], r - 2, r) % r] + [0] * (S.NPUB - 1)).any()      # A = H -> infinity
