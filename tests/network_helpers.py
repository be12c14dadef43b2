"""shared by the two-network tests: the two (wrap index, step index) pairs with proofs of their own, as serialized boundary inputs.
  pair A: the wrap index of tests/golden/kimchi_k15.json with make_step_index(99); proofs of tests/golden/statement_k15.json (four)
  pair B: the wrap index of tests/golden/statement_k15_alt.json with make_step_index(7); the proofs of the same file (two)
tests/golden/gen_alt_network_fixture.py asserts that the oracle accepts every proof under its own pair and rejects it under the other."""
import copy
import json
import os
import random

import numpy as np

ALL = 1 | 2 | 4 | 8 | 16 | 32
KIMCHI = 32
ALT_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "statement_k15_alt.json")


def load_alt_index():
    """the wrap index of pair B as an oracle VerifierIndex (the layout of kimchi_k15.json's index fields, under "wrap_index")"""
    from ipa_helpers import poseidon_pp
    from oracle import kimchi_ref as K, oracle as O
    fx = json.load(open(ALT_PATH))["wrap_index"]
    pt = lambda hx: O.bytes_to_point(np.frombuffer(bytes.fromhex(hx), np.uint8))
    ix = K.VerifierIndex(curve=0, log2_domain=fx["log2_domain"], zk_rows=fx["zk_rows"], shifts=[int(x) for x in fx["shifts"]],
                         sigma_comm=[pt(x) for x in fx["sigma_comm"]], coefficients_comm=[pt(x) for x in fx["coefficients_comm"]],
                         selector_comm=[pt(x) for x in fx["selector_comm"]], constant_term=[tuple(t) for t in fx["constant_term"]],
                         perm_alpha_offset=fx["perm_alpha_offset"], digest=int(fx["digest"]))
    ix.mds = [list(row) for row in poseidon_pp(1).mds]
    return ix


def boundary_cases(items):
    """load_statement_fixture items -> dicts with the full wrap proof, its chain, the serialized proof and the public input under either network flag"""
    from ipa_helpers import poseidon_pp
    from kimchi_helpers import make_chain
    from oracle import mina_state_ref as S
    from wire_writers import state_proof_bytes, state_pub_bytes
    cases = []
    for it in items:
        states, hashes = make_chain(random.Random(it["chain_seed"]), poseidon_pp(0))
        assert hashes[15] == it["app"]
        p, ev = it["proof"], it["proof"]["evals"]
        wrap = dict(it["wrap"])
        wrap.update(w_comm=p["w_comm"], z_comm=p["z_comm"], t_comm=p["t_comm"], z_eval=ev[0], selector_eval=ev[1:7], w_eval=ev[7:22], coefficients_eval=ev[22:37],
                    s_eval=ev[37:43], ft_eval1=p["ft_eval1"], lr=p["opening"]["lr"], z1=p["opening"]["z1"], z2=p["opening"]["z2"], delta=p["opening"]["delta"],
                    sg=p["opening"]["sg"])
        ledger = [S.snarked_ledger_hash(s) for s in states[:16]]
        pubs = [state_pub_bytes(bool(n), hashes[16], hashes[:16], ledger) for n in (0, 1)]
        assert pubs[0][0] == 0 and pubs[1][0] == 1 and pubs[0][1:] == pubs[1][1:]
        cases.append({"wrap": wrap, "states": states, "proof": state_proof_bytes(wrap, states), "pub": pubs})
    return cases


class Pair:
    def __init__(self, name, ix, step, cases):
        self.name, self.ix, self.step, self.cases = name, ix, step, cases

    def install(self, target):
        """target: a MinaContext, lib.verify_all_devices() or lib.verify_network_devices(n)"""
        from kimchi_helpers import install_index, install_step_index
        install_index(target, self.ix)
        install_step_index(target, self.step)

    def good(self, net):
        return [(c["proof"], c["pub"][net]) for c in self.cases]

    def tampered(self, net):
        """one tamper per stage: a flipped public hash (CHAIN), a changed statement field (KIMCHI through the public input), a changed opening scalar z2
        (KIMCHI / opening: costs a culprit search), a changed step prechallenge (ACCUMULATOR and the statement)"""
        from wire_writers import state_proof_bytes
        cs = self.cases
        pick = lambda i: cs[i % len(cs)]
        bad_pub = bytearray(pick(0)["pub"][net]); bad_pub[40] ^= 1
        w1 = copy.deepcopy(pick(1)["wrap"]); w1["feature_flags"][0] = not w1["feature_flags"][0]
        w2 = copy.deepcopy(pick(2)["wrap"]); w2["z2"] = (w2["z2"] + 1) % (1 << 254)
        w3 = copy.deepcopy(pick(3)["wrap"]); w3["bulletproof_challenges"][5] ^= 1
        return [(pick(0)["proof"], bytes(bad_pub)), (state_proof_bytes(w1, pick(1)["states"]), pick(1)["pub"][net]),
                (state_proof_bytes(w2, pick(2)["states"]), pick(2)["pub"][net]), (state_proof_bytes(w3, pick(3)["states"]), pick(3)["pub"][net])]


def load_pairs():
    from kimchi_helpers import load_k15_fixture, load_statement_fixture, make_step_index
    ix_a, _, _ = load_k15_fixture()
    items_a, _ = load_statement_fixture()
    items_b, fx_b = load_statement_fixture(ALT_PATH)
    assert fx_b["step_index"] == "kimchi_helpers.make_step_index(7)" and len(items_a) == 4 and len(items_b) == 2
    return Pair("A", ix_a, make_step_index(99), boundary_cases(items_a)), Pair("B", load_alt_index(), make_step_index(7), boundary_cases(items_b))
