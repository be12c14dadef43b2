"""The `_net` twins of the index-reading kernels (api_kimchi.hip kimchi_fq / _rows / _pub / _scalar / _ftcomm `_net_kernel`, api_pickles.hip pickles_digest / _scalar
`_net_kernel`) through their host-buffer calls, mina_kimchi_to_batch_net and mina_pickles_public_inputs_batch_net: proofs of BOTH index sets of one context in one
call, proof b checked against set net[b].

The checker is the existing single-set code: the same proof through mina_kimchi_to_batch / mina_pickles_public_inputs_batch on the context with that set selected
(those calls are held to the oracle by tests/test_index_sets_gpu.py and tests/test_gpu_kimchi_rows.py).  Every comparison is equality of bytes, per proof, of every
output: sponge state and position, cip, evaluation points, v, u, all n_prev + 45 commitment rows (the ft row among them), ft_eval0, the 40 public inputs and the
statement's ok byte; and the call's malformed byte.  ref[s][i] -- the outputs of proof i under set s, for both sets -- is computed once and never written to.

Pair A (4 proofs) is installed in set 0 and pair B (2 proofs) in set 1 (tests/network_helpers.py); the oracle rejects every proof under the other pair
(tests/golden/gen_alt_network_fixture.py), and a proof's rows under the other set differ from its own: a wrong pick shows."""
import numpy as np
import pytest

from network_helpers import load_pairs

pytestmark = pytest.mark.gpu

KIMCHI_FIELDS = ("sponge_state", "sponge_pos", "cip", "evalpoints", "polyscale", "evalscale", "comms", "ft_eval0")
# the transcript lane forms, forced as tests/test_gpu_kimchi_rows.py forces them (ctx.h transcript_lanes)
FORMS = {16: dict(coop16_max=1 << 30), 8: dict(coop16_max=0, kimchi_coop8_max=1 << 30, transcript_coop8_max=1 << 30), 3: dict(coop16_max=0, transcript_coop8_max=1)}
SIX = (("A", 0), ("B", 0), ("A", 1), ("A", 2), ("B", 1), ("A", 3))          # the six proofs interleaved
SIX_NET = [0, 1, 0, 0, 1, 0]                                                  # ... and the set each belongs to


def fresh_ctx(m, pallas=65536, vesta=65536):
    c = m.MinaContext(0)
    for field in (0, 1):
        c.poseidon_set_params(field, m.poseidon_params.default_params_bytes(field))
    c.srs_create(0, pallas)
    if vesta:
        c.srs_create(1, vesta)
    return c


def single(m, c, items):
    """the two single-set stage calls on `items` under the context's selected set -> {field: [batch, bytes]}, malformed"""
    from kimchi_helpers import kimchi_arrays, statements_soa
    n = len(items)
    arrays, _ = kimchi_arrays([it["proof"] for it in items], [it["pubs"] for it in items])
    got = c.kimchi_to_batch(m.MinaContext.make_kimchi_proofs(n, 2, 40, arrays), 15)
    n_old, n_evals, sec = statements_soa([it["wrap"] for it in items], [it["app"] for it in items])
    pub, ok = c.pickles_public_inputs_batch(m.MinaContext.make_pickles_statements(n_old, n_evals, sec), n)
    return rows(got, pub, ok, n), int(got["malformed"][0])


def mixed(m, c, items, net):
    from kimchi_helpers import kimchi_arrays, statements_soa
    n = len(items)
    arrays, _ = kimchi_arrays([it["proof"] for it in items], [it["pubs"] for it in items])
    got = c.kimchi_to_batch_net(m.MinaContext.make_kimchi_proofs(n, 2, 40, arrays), 15, net)
    n_old, n_evals, sec = statements_soa([it["wrap"] for it in items], [it["app"] for it in items])
    pub, ok = c.pickles_public_inputs_batch_net(m.MinaContext.make_pickles_statements(n_old, n_evals, sec), n, net)
    return rows(got, pub, ok, n), int(got["malformed"][0])


def rows(got, pub, ok, n):
    out = {f: np.ascontiguousarray(got[f]).view(np.uint8).reshape(n, -1).copy() for f in KIMCHI_FIELDS}
    out["pickles_pub"] = np.asarray(pub).reshape(n, -1).copy()
    out["pickles_ok"] = np.asarray(ok).reshape(n, 1).copy()
    assert out["comms"].shape[1] == 47 * 64
    return out


@pytest.fixture(scope="module")
def env(oracle):
    import mina_bridge_amd as m
    from kimchi_helpers import load_statement_fixture
    from network_helpers import ALT_PATH
    A, B = load_pairs()
    pool = {"A": load_statement_fixture()[0], "B": load_statement_fixture(ALT_PATH)[0]}
    six = [pool[name][i] for name, i in SIX]
    two = fresh_ctx(m)
    try:
        two.set_pipeline(1)
        A.install(two)
        two.select_index_set(1)
        B.install(two)
        two.select_index_set(0)
        ref = []
        for s in (0, 1):                                         # every one of the six under either set: the single-set code, set s selected
            two.select_index_set(s)
            r, bad = single(m, two, six)
            assert not bad
            for v in r.values():
                v.setflags(write=False)
            ref.append(r)
        two.select_index_set(0)
        for i, s in enumerate(SIX_NET):                          # the fixture's premise: under its own set a statement is well-formed and gives its public input,
            assert ref[s]["pickles_ok"][i, 0] == 1              # and the other set's rows are other bytes in every stage
            for f in ("sponge_state", "cip", "comms", "ft_eval0", "pickles_pub"):
                assert (ref[0][f][i] != ref[1][f][i]).any(), (i, f)
        yield {"m": m, "two": two, "six": six, "ref": ref, "A": A}
    finally:
        two.close()


def want(ref, idx, net):
    """the reference rows of proofs six[idx[b]] under sets net[b]"""
    return {f: np.stack([ref[s][f][i] for i, s in zip(idx, net)]) for f in ref[0]}


def same(got, exp, skip=()):
    for f in exp:
        bad = [b for b in np.nonzero((got[f] != exp[f]).any(axis=1))[0].tolist() if b not in skip]
        if bad and f == "comms":
            b = bad[0]
            r = np.nonzero((got[f][b].reshape(47, 64) != exp[f][b].reshape(47, 64)).any(axis=1))[0].tolist()
            raise AssertionError(f"comms differs for proofs {bad[:8]}; proof {b}: commitment rows {r}")
        assert not bad, f"{f} differs for proofs {bad[:8]} of {len(exp[f])}"


def test_stage_equality_interleaved_and_uniform(env):
    m, two, six, ref = env["m"], env["two"], env["six"], env["ref"]
    idx = list(range(6))
    for sel in (0, 1):                                           # the bytes name the set, whichever is selected; the selection is left alone
        two.select_index_set(sel)
        got, bad = mixed(m, two, six, SIX_NET)
        assert two.index_set() == sel and not bad
        same(got, want(ref, idx, SIX_NET))
    two.select_index_set(0)
    for s in (0, 1):                                             # all of one set = the single-set call on the whole batch
        got, bad = mixed(m, two, six, [s] * 6)
        assert not bad
        same(got, want(ref, idx, [s] * 6))
    # and the `_net` stages of a mixed call count as power-form launches whatever the mode: pub, scalar, ftcomm + the statement's scalar stage.  The one divstep
    # launch is the public-input commitment's finish inside mina_kimchi_to_batch_net: it reads no index, has no twin and follows the mode as it always has
    two.set_chain_inverse(True)
    try:
        c0 = two.chain_inverse_stats()
        got, _ = mixed(m, two, six, SIX_NET)
        c1 = two.chain_inverse_stats()
    finally:
        two.set_chain_inverse(False)
    same(got, want(ref, idx, SIX_NET))
    assert c1["gcd_launches"] - c0["gcd_launches"] == 1 and c1["fermat_launches"] - c0["fermat_launches"] == 4, (c0, c1)


# a batch of 67: the network changes inside a wave and exactly at the boundaries of a wave or of a lane group -- 3 | 4 (16 lanes per sponge: 4 proofs per wave),
# 7 | 8 (8 lanes: 8 per wave), 20 | 21 (the 3-lane form: 21 per wave), 63 | 64 (the scalar kernels: 64 proofs per wave)
EDGE_NET = [0] * 4 + [1] * 4 + [0] * 13 + [1] * 43 + [0] * 3


@pytest.mark.parametrize("form", sorted(FORMS))
def test_wave_and_group_edges_in_every_lane_form(env, form):
    m, two, six, ref = env["m"], env["two"], env["six"], env["ref"]
    assert len(EDGE_NET) == 67 and [b for b in range(1, 67) if EDGE_NET[b] != EDGE_NET[b - 1]] == [4, 8, 21, 64]
    idx = [b % 6 for b in range(67)]
    with m.lib.tuning(**FORMS[form]):
        t = m.lib.verify_tuning_get()
        lanes = 16 if 67 <= t.coop16_max else (8 if 67 <= t.transcript_coop8_max else 3)      # ctx.h transcript_lanes with one pipeline lane and transcript_coop8_max set
        assert lanes == form
        got, bad = mixed(m, two, [six[i] for i in idx], EDGE_NET)
    assert not bad
    same(got, want(ref, idx, EDGE_NET))


def test_a_wrong_pick_shows_and_a_byte_of_2_is_that_proof_alone(env):
    m, two, six, ref = env["m"], env["two"], env["six"], env["ref"]
    idx = list(range(6))
    for flip in (1, 3):
        net = list(SIX_NET); net[flip] ^= 1
        got, bad = mixed(m, two, six, net)
        assert not bad
        same(got, want(ref, idx, net))                           # the flipped proof has the other set's rows, every other proof its own
        own = want(ref, idx, SIX_NET)
        for f in ("sponge_state", "cip", "comms", "ft_eval0", "pickles_pub"):
            assert (got[f][flip] != own[f][flip]).any(), f
        same(got, own, skip=(flip,))
    for pos in (0, 4):
        net = list(SIX_NET); net[pos] = 2
        got, bad = mixed(m, two, six, net)
        assert bad == 1, "the call's malformed byte"
        exp = want(ref, idx, SIX_NET)
        assert got["pickles_ok"][:, 0].tolist() == [0 if b == pos else 1 for b in range(6)]
        same(got, exp, skip=(pos,))                              # nothing else moves (the malformed proof's own rows are unspecified)
    got, bad = mixed(m, two, six, [255, 7, 2, 128, 3, 254])      # and no byte value reads out of range
    assert bad == 1 and got["pickles_ok"][:, 0].tolist() == [0] * 6


def test_argument_and_state_errors_before_any_launch(env):
    from kimchi_helpers import kimchi_arrays, statements_soa
    m, two, six, A = env["m"], env["two"], env["six"], env["A"]
    arrays, _ = kimchi_arrays([it["proof"] for it in six], [it["pubs"] for it in six])
    kp = m.MinaContext.make_kimchi_proofs(6, 2, 40, arrays)
    n_old, n_evals, sec = statements_soa([it["wrap"] for it in six], [it["app"] for it in six])
    st = m.MinaContext.make_pickles_statements(n_old, n_evals, sec)
    c0 = two.chain_inverse_stats()
    with pytest.raises(m.lib.MinaError, match=r"mina_kimchi_to_batch_net failed \(-1\)"):
        two.kimchi_to_batch_net(kp, 15, None)
    with pytest.raises(m.lib.MinaError, match=r"mina_pickles_public_inputs_batch_net failed \(-1\)"):
        two.pickles_public_inputs_batch_net(st, 6, None)
    assert two.chain_inverse_stats() == c0, "a refused call queues nothing"
    # a set missing: pair A alone, in set 0 and then in set 1 (a Pallas SRS of the domain's size is all an install needs)
    one = fresh_ctx(m, pallas=32768, vesta=0)
    try:
        for s in (0, 1):
            one.select_index_set(s)
            A.install(one)
            for sel in (0, 1):
                one.select_index_set(sel)
                c0 = one.chain_inverse_stats()
                with pytest.raises(m.lib.MinaError, match=r"mina_kimchi_to_batch_net failed \(-3\)") if s == 0 else _ok():
                    one.kimchi_to_batch_net(kp, 15, SIX_NET)
                with pytest.raises(m.lib.MinaError, match=r"mina_pickles_public_inputs_batch_net failed \(-3\)") if s == 0 else _ok():
                    one.pickles_public_inputs_batch_net(st, 6, SIX_NET)
                if s == 0:
                    assert one.chain_inverse_stats() == c0
    finally:
        one.close()


class _ok:
    """with both sets installed the same calls go through"""
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False
