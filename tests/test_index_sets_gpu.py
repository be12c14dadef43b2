"""Two index sets on ONE caller-owned context (mina_ctx_select_index_set): everything that belongs to an installed (wrap index, step index) pair exists twice,
one of the two is selected, and every installer, getter and job acts on the selected one.  Pair A in set 0 and pair B in set 1 (tests/network_helpers.py): with
either selected, the kimchi and Pickles stages give the bytes of a fresh context that holds that pair alone, and the oracle's values."""
import ctypes

import numpy as np
import pytest

from network_helpers import load_pairs

pytestmark = pytest.mark.gpu
ERR_ARG = -1


def fresh_ctx(m):
    c = m.MinaContext(0)
    for field in (0, 1):
        c.poseidon_set_params(field, m.poseidon_params.default_params_bytes(field))
    for curve in (0, 1):
        c.srs_create(curve, 65536)
    return c


@pytest.fixture(scope="module")
def sets(oracle):
    import mina_bridge_amd as m
    from kimchi_helpers import load_statement_fixture
    from network_helpers import ALT_PATH
    A, B = load_pairs()
    items = {"A": load_statement_fixture()[0], "B": load_statement_fixture(ALT_PATH)[0]}
    two, only_a, only_b = fresh_ctx(m), fresh_ctx(m), fresh_ctx(m)
    assert two.index_set() == 0
    A.install(two)
    two.select_index_set(1); assert two.index_set() == 1
    B.install(two)
    two.select_index_set(0)
    A.install(only_a); B.install(only_b)
    yield {"m": m, "A": A, "B": B, "items": items, "two": two, "alone": {"A": only_a, "B": only_b}}
    for c in (two, only_a, only_b):
        c.close()


def stages(m, c, items):
    """the bytes of mina_kimchi_to_batch and mina_pickles_public_inputs_batch on `items` under the context's selected set"""
    from kimchi_helpers import kimchi_arrays, statements_soa
    arrays, _ = kimchi_arrays([it["proof"] for it in items], [it["pubs"] for it in items])
    got = c.kimchi_to_batch(m.MinaContext.make_kimchi_proofs(len(items), 2, 40, arrays), 15)
    n_old, n_evals, sec = statements_soa([it["wrap"] for it in items], [it["app"] for it in items])
    pub, ok = c.pickles_public_inputs_batch(m.MinaContext.make_pickles_statements(n_old, n_evals, sec), len(items))
    out = {k: np.asarray(v).tobytes() for k, v in got.items()}
    out["pickles_pub"] = np.asarray(pub).tobytes(); out["pickles_ok"] = np.asarray(ok).tobytes()
    return out, got, pub, ok


def test_each_set_is_the_pair_installed_into_it(sets, oracle, srs_oracle):
    from ipa_helpers import poseidon_pp
    from oracle import kimchi_ref as K
    m, two = sets["m"], sets["two"]
    g, h = srs_oracle[0]
    cips = {}
    for s, name in ((0, "A"), (1, "B"), (0, "A")):              # and back again: selecting moves handles, it loses nothing
        pair, items = sets[name], sets["items"][name]
        two.select_index_set(s)
        assert oracle.le_to_int(two.verifier_index_digest()) == pair.ix.digest
        out, got, pub, ok = stages(m, two, items)
        alone, _, _, _ = stages(m, sets["alone"][name], items)
        assert out.keys() == alone.keys()
        for k in out:
            assert out[k] == alone[k], (name, k)
        assert not got["malformed"][0] and ok.tolist() == [1] * len(items)
        for b, it in enumerate(items):
            assert [oracle.le_to_int(x) for x in pub[b]] == it["pubs"]
        o, _ = K.oracles_and_batch(pair.ix, items[0]["proof"], items[0]["pubs"], poseidon_pp(0), poseidon_pp(1), g, oracle.bytes_to_point(h), ft_comm=False)
        assert oracle.le_to_int(got["ft_eval0"][0]) == o["ft_eval0"] and oracle.le_to_int(got["cip"][0]) == o["combined_inner_product"]
        assert oracle.le_to_int(got["polyscale"][0]) == o["v"] and oracle.le_to_int(got["evalscale"][0]) == o["u"]
        cips[name] = got["cip"].tobytes()
    # A's proofs under B's set: another index digest in the transcript, another combined inner product
    two.select_index_set(1)
    _, got, pub, _ = stages(m, two, sets["items"]["A"])
    assert got["cip"].tobytes() != cips["A"]
    assert [oracle.le_to_int(x) for x in pub[0]] != sets["items"]["A"][0]["pubs"], "the statement's public input binds the pair's commitments and step index"
    two.select_index_set(0)


def test_changed_poseidon_tables_invalidate_the_derived_state_of_both_sets(sets):
    m, two = sets["m"], sets["two"]
    before = {}
    for s, name in ((0, "A"), (1, "B")):
        two.select_index_set(s)
        before[name] = stages(m, two, sets["items"][name])[0]
    fp = bytearray(m.poseidon_params.default_params_bytes(0)); fp[9 * 32] ^= 1      # another first round constant: other tables of the same shape
    two.poseidon_set_params(0, bytes(fp))
    for s, name in ((0, "A"), (1, "B")):                        # both sets rebuild their Tick sponge state under the changed tables
        two.select_index_set(s)
        changed = stages(m, two, sets["items"][name])[0]
        assert changed["pickles_pub"] != before[name]["pickles_pub"]
    two.select_index_set(1)                                     # set back while set 1 is selected: the parked set 0 must be invalidated as well
    two.poseidon_set_params(0, m.poseidon_params.default_params_bytes(0))
    for s, name in ((0, "A"), (1, "B")):
        two.select_index_set(s)
        after = stages(m, two, sets["items"][name])[0]
        for k in after:
            assert after[k] == before[name][k], (name, k)
    two.select_index_set(0)


def test_selection_arguments_and_the_chain_inverse_under_set_1(sets):
    m, two = sets["m"], sets["two"]
    lib = m.lib.load_library()
    assert lib.mina_ctx_select_index_set(two._h, ctypes.c_uint32(2)) == ERR_ARG and two.index_set() == 0
    assert lib.mina_ctx_select_index_set(None, ctypes.c_uint32(0)) == ERR_ARG
    two.select_index_set(1)
    try:
        off = stages(m, two, sets["items"]["B"])[0]
        two.set_chain_inverse(True)
        on = stages(m, two, sets["items"]["B"])[0]
        for k in off:
            assert on[k] == off[k], k
    finally:
        two.set_chain_inverse(False)
        two.select_index_set(0)
