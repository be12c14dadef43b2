"""tests/ipa_rows_model.py (the big-integer statement of the rows `ipa_prepare_kernel` writes, which tests/test_gpu_ipa_rows.py holds the kernel to) tied to the
restatement the suite already trusts: on minted openings the model's rows, together with the folded challenge polynomials over g, must sum to the identity exactly
when oracle/ipa_ref.ipa_verify_batch accepts.  CPU only."""
import random

import numpy as np
import pytest

import ipa_rows_model as M
from ipa_helpers import mint, poseidon_pp

K, BATCH = 4, 3
RB, SB = 0x1234567890ABCDEF1234567890ABCDEF, 0xFEDCBA0987654321


@pytest.fixture(scope="module")
def minted(oracle):
    """{curve: (g bytes [16, 64], h bytes, h point, [(entry, sponge)] * 3)}"""
    out = {}
    for curve in (0, 1):
        g, h = oracle.srs_create(curve, 1 << K, threads=4)
        out[curve] = (g, h, oracle.bytes_to_point(h), [mint(curve, g, h, K, n_polys=3, n_points=2, seed=7100 + 10 * curve + b) for b in range(BATCH)])
    return out


def total(oracle, curve, g, rows):
    """the MSM the opening check evaluates: the rows, plus sigma_b * b_poly_coefficients(chals_b) over g; 64 bytes (zeros = the identity)"""
    from oracle import pasta_ref as R
    r = R.scalar_modulus(curve)
    folded = [0] * len(g)
    for sigma, chals in zip(rows["sigma"], rows["chals"]):
        for j, s in enumerate(R.b_poly_coefficients(chals, r)):
            folded[j] = (folded[j] + sigma * s) % r
    pts = np.concatenate([g, M.pts_bytes(rows["points"])])
    return oracle.msm_pippenger(curve, pts, oracle.ints_to_le(folded + rows["scalars"]), threads=4)


def cpu_verdict(oracle, curve, g, h, made, z1_delta=0):
    from oracle import ipa_ref as I
    batch = []
    for n, (e, sp) in enumerate(made):
        e2 = dict(e); e2["sponge"] = sp.clone()
        if z1_delta and n == len(made) - 1:
            e2["opening"] = dict(e["opening"]); e2["opening"]["z1"] = (e["opening"]["z1"] + z1_delta)
        batch.append(e2)
    return I.ipa_verify_batch(curve, g, h, batch, RB, SB)


@pytest.mark.parametrize("pow_first", [0, 1])
@pytest.mark.parametrize("curve", [0, 1])
def test_model_rows_sum_to_the_identity_exactly_when_the_restatement_accepts(oracle, minted, curve, pow_first):
    from oracle import pasta_ref as R
    g, _, h, made = minted[curve]
    r = R.scalar_modulus(curve)
    pp = poseidon_pp(curve)
    proofs = [M.from_minted(e, sp) for e, sp in made]
    rows = M.ipa_rows(curve, pp, h, proofs, RB % r, SB % r, pow_first=pow_first)
    assert not rows["malformed"] and rows["per"] == 2 * K + 3 + 4 and len(rows["points"]) == BATCH * rows["per"] == len(rows["scalars"])
    assert rows["sigma"] == [pow(SB % r, b + pow_first, r) for b in range(BATCH)]
    assert all(rows["chals"][b] == made[b][0]["opening"]["chals"] for b in range(BATCH))
    assert not total(oracle, curve, g, rows).any(), "valid openings: the rows and the folded polynomials must cancel"
    bad = [dict(q) for q in proofs]; bad[-1]["z1"] = (bad[-1]["z1"] + 1) % r
    rows_bad = M.ipa_rows(curve, pp, h, bad, RB % r, SB % r, pow_first=pow_first)
    assert total(oracle, curve, g, rows_bad).any(), "one tampered z1: the sum must not be the identity"
    if pow_first == 0:                                          # upstream's powers: the restatement the suite trusts gives the same two verdicts
        assert cpu_verdict(oracle, curve, g, h, made) is True
        assert cpu_verdict(oracle, curve, g, h, made, z1_delta=1) is False


@pytest.mark.parametrize("curve", [0, 1])
def test_folding_shared_entries_keeps_the_sum_and_restore_undoes_it(oracle, minted, curve):
    """h, and commitments 0 and 2 made the same point in every proof (no valid openings any more: the sum is some point, and it must not move)"""
    from oracle import pasta_ref as R
    g, _, h, made = minted[curve]
    r = R.scalar_modulus(curve)
    pp = poseidon_pp(curve)
    proofs = [M.from_minted(e, sp) for e, sp in made]
    for q in proofs:
        q["comms"][0], q["comms"][2] = oracle.bytes_to_point(g[5]), oracle.bytes_to_point(g[9])
    plain = M.ipa_rows(curve, pp, h, proofs, RB % r, SB % r)
    shared = M.ipa_rows(curve, pp, h, proofs, RB % r, SB % r, shared_mask=0b101, shared_h=1)
    per, o = plain["per"], 4 + 2 * K
    assert shared["nshared"] == 3 and shared["offsets"] == [0, o, o + 2] and shared["per"] == per
    assert shared["points"][: BATCH * per] == plain["points"] and shared["points"][BATCH * per:] == [plain["points"][i] for i in (0, o, o + 2)]
    assert all(shared["scalars"][b * per + i] == 0 for b in range(BATCH) for i in (0, o, o + 2))
    want = total(oracle, curve, g, plain)
    assert want.any() and (total(oracle, curve, g, shared) == want).all()
    back = M.restore(shared, 0, BATCH)
    assert back["scalars"][: BATCH * per] == plain["scalars"] and back["scalars"][BATCH * per:] == shared["scalars"][BATCH * per:] and back["side"] == shared["side"]
    one = M.restore(shared, 1, 1)
    assert one["scalars"][per: 2 * per] == plain["scalars"][per: 2 * per] and one["scalars"][:per] == shared["scalars"][:per] and one["scalars"][2 * per:] == shared["scalars"][2 * per:]


def test_malformed_inputs_are_named(oracle, minted):
    from oracle import pasta_ref as R
    curve = 0
    g, _, h, _ = minted[curve]
    r, p = R.scalar_modulus(curve), R.base_modulus(curve)
    pts = [oracle.bytes_to_point(b) for b in g]
    rng = random.Random(5)
    base = [M.random_proof(rng, curve, pts, 2, 2, 1) for _ in range(3)]
    run = lambda ps: M.ipa_rows(curve, poseidon_pp(curve), h, ps, 3, 5)      # noqa: E731
    clean = run(base)
    assert clean["malformed_each"] == [False] * 3
    x, y = pts[3]
    for key, val in (("z1", r), ("cip", r + 1), ("delta", (x, (y + 1) % p)), ("sg", (x + p, y)), ("sponge_state", [p, 0, 0]), ("comms", [pts[1], (1, 1)])):
        bad = [dict(q) for q in base]; bad[1][key] = val
        got = run(bad)
        assert got["malformed_each"] == [False, True, False] and got["malformed"], key
        per = got["per"]
        assert got["scalars"][:per] == clean["scalars"][:per] and got["scalars"][2 * per:] == clean["scalars"][2 * per:], key
    inf = [dict(q) for q in base]; inf[0]["delta"] = None; inf[2]["comms"] = [(0, 0), None]
    assert not run(inf)["malformed"]
