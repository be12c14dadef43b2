"""Generates tests/golden/statement_k15_alt.json: a SECOND (wrap index, step index) pair with complete wrap proofs of its own, for the
tests that hold two index sets at once (one per Mina network).  Pair A is the existing one -- the wrap index of kimchi_k15.json
(circuit seed 0xC15) with `make_step_index(99)`, proofs in statement_k15.json; pair B, written here, is the wrap index of
`K.synthetic_circuit(..., seed=0xC16)` with `make_step_index(7)`.

The file holds (1) B's wrap index under "wrap_index", in the field layout kimchi_k15.json uses for its index, and (2) "proofs": complete
wrap proofs for pair B in the layout `kimchi_helpers.load_statement_fixture(path)` reads.  All seeds (statement, accumulator, chain,
prover) are disjoint from gen_statement_fixture.py's.  Minted by the repo's own CPU oracle, as there; data only.

Before it writes, the generator asserts that the oracle ACCEPTS each minted proof under pair B, REJECTS it under pair A, and REJECTS
each proof of statement_k15.json under pair B: the two-network tests rely on a proof failing under the other network's pair.
Run:  python tests/golden/gen_alt_network_fixture.py [count]   (~6 min per proof; the proofs are minted in parallel processes)"""
import json
import multiprocessing
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
count = int(sys.argv[1]) if len(sys.argv) > 1 else 2
out_path = os.path.join(ROOT, "tests/golden/statement_k15_alt.json")
sys.argv = [sys.argv[0], "0", "--out", os.devnull]              # gen_statement_fixture runs on import: zero proofs, nothing written; its setup (SRS, Poseidon, circuit A) is what is wanted
import gen_statement_fixture as G
from gen_statement_fixture import ACC_K, I, J, K, K_LOG2, NPUB, O, PK, R, STATEMENT_KEYS, g, gv, hp, hx, pb, ps, synth_wrap_proof
from kimchi_helpers import load_statement_fixture, make_chain, make_step_index

ALT_CIRCUIT_SEED, ALT_STEP_SEED = 0xC16, 7
index_comms = lambda ix: list(ix.sigma_comm) + list(ix.coefficients_comm) + list(ix.selector_comm)
t0 = time.time()
circ = K.synthetic_circuit(0, g, hp, pb, ps, K_LOG2, NPUB, seed=ALT_CIRCUIT_SEED)
print("alt circuit", round(time.time() - t0, 1), "s", flush=True)
ix_a, step_a = G.ix, G.step
ix_b, step_b = circ.index, make_step_index(ALT_STEP_SEED)
assert ix_b.digest != ix_a.digest


def verifies(item, ix, step):
    """the oracle's verdict on the kimchi step of a complete wrap proof (load_statement_fixture item) under the pair (ix, step)"""
    pubs = PK.statement_public_input(item["wrap"], step, index_comms(ix), item["app"], pb, ps)[0]
    _, entry = K.oracles_and_batch(ix, item["proof"], pubs, pb, ps, g, hp)
    return bool(I.ipa_verify_batch(0, g, hp, [entry], 7, 9))


def mint(i):
    t0 = time.time()
    rng = random.Random(0xA17057A7 + i)
    wrap = synth_wrap_proof(rng, k=K_LOG2, lookups=False)
    pres = [[rng.getrandbits(128) for _ in range(15)] for _ in range(2)]
    chals = [[R.challenge_to_field(p, R.endo_r(0), R.Q) for p in row] for row in pres]
    wrap["prev_optional"] = [None] * 19
    wrap["old_bulletproof_challenges"] = pres
    prev_comms = []
    for ch in chals:
        sc = [O.le_to_int(x) for x in O.b_poly_coefficients(1, O.ints_to_le(ch))]
        prev_comms.append(I.commit(0, g[: 1 << K_LOG2], hp, sc, 0))
    wrap["step_comms"] = prev_comms
    pre, sg = J.make_accumulator(1, gv, ACC_K, 0xA170ACC + i)
    wrap["bulletproof_challenges"] = [int.from_bytes(pre[j].tobytes(), "little") for j in range(16)]
    wrap["challenge_polynomial_commitment"] = O.bytes_to_point(sg)
    chain_seed = 0xA170C4A1 + i
    app = make_chain(random.Random(chain_seed), pb)[1][15]
    pubs = PK.statement_public_input(wrap, step_b, index_comms(ix_b), app, pb, ps)[0]
    proof = K.synthetic_proof(circ, g, hp, pb, ps, pubs, seed=0xA1709000 + i, prev_chals=chals)
    assert [cm for _, cm in proof["prev"]] == prev_comms
    assert J.accumulator_ok(1, gv, ACC_K, pre, sg)
    op = proof["opening"]
    enc = lambda v: (None if v is None else [enc(x) for x in v] if isinstance(v, (list, tuple)) else bool(v) if isinstance(v, bool) else str(v))
    print("alt proof", i, "minted", round(time.time() - t0, 1), "s", flush=True)
    return {"statement": {k: enc(wrap[k]) for k in STATEMENT_KEYS}, "app_state": str(app), "chain_seed": chain_seed, "pubs": [str(x) for x in pubs],
            "acc_pre": pre.tobytes().hex(), "acc_sg": bytes(sg).hex(),
            "w_comm": [hx(p) for p in proof["w_comm"]], "z_comm": hx(proof["z_comm"]), "t_comm": [hx(p) for p in proof["t_comm"]],
            "evals": [[str(a), str(b)] for a, b in proof["evals"]], "ft_eval1": str(proof["ft_eval1"]),
            "lr": [[hx(l), hx(r)] for l, r in op["lr"]], "delta": hx(op["delta"]), "sg": hx(op["sg"]), "z1": str(op["z1"]), "z2": str(op["z2"])}


if __name__ == "__main__":
    with multiprocessing.get_context("fork").Pool(count) as pool:
        proofs = pool.map(mint, range(count), chunksize=1)
    out = {"poseidon_constants": G.PP.NAME, "step_index": "kimchi_helpers.make_step_index(%d)" % ALT_STEP_SEED,
           "wrap_index": {"log2_domain": K_LOG2, "zk_rows": ix_b.zk_rows, "perm_alpha_offset": ix_b.perm_alpha_offset, "npub": NPUB, "n_prev": 2,
                          "shifts": [str(x) for x in ix_b.shifts], "sigma_comm": [hx(p) for p in ix_b.sigma_comm], "coefficients_comm": [hx(p) for p in ix_b.coefficients_comm],
                          "selector_comm": [hx(p) for p in ix_b.selector_comm], "constant_term": [[int(x) for x in tok] for tok in ix_b.constant_term], "digest": str(ix_b.digest)},
           "proofs": proofs}
    tmp = out_path + ".tmp"
    json.dump(out, open(tmp, "w"), indent=0)
    # the round trip through the reader the tests use, then the verdicts the tests rely on: each pair accepts its own proofs and rejects the other's
    alt, _ = load_statement_fixture(tmp)
    existing, _ = load_statement_fixture()
    for i, item in enumerate(alt):
        assert item["pubs"] == [int(x) for x in proofs[i]["pubs"]]
        assert verifies(item, ix_b, step_b), "alt proof %d does not verify under the alt pair" % i
        assert not verifies(item, ix_a, step_a), "alt proof %d verifies under the existing pair" % i
        print("alt proof", i, "accepted by its pair, rejected by the existing one", flush=True)
    for i, item in enumerate(existing):
        assert verifies(item, ix_a, step_a), "existing proof %d does not verify under its own pair" % i
        assert not verifies(item, ix_b, step_b), "existing proof %d verifies under the alt pair" % i
        print("existing proof", i, "accepted by its pair, rejected by the alt one", flush=True)
    os.replace(tmp, out_path)
    print("wrote", out_path, flush=True)
