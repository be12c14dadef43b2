"""The 3-lane permutation on the diagonal-normalised rows (sponge.cuh poseidon_rounds_tri_norm, chosen by poseidon_permute_tri where the installed tables have
the rows), GPU tier.

1. Permutation parity: `mina_poseidon_permute` above 8192 states (ctx.h sponge_batch_lanes: the 3-lane form) against the CPU oracle's permutation, both fields,
   at sizes that cross the 21-sponge group boundary of a wave and its shadow lane 63; corner and random states; the compiled-in constants, a random set (the
   general derivation of the rows) and a set with a zero on the MDS diagonal.  For the last the derivation refuses the rows (api_sponge.hip poseidon_rows1;
   tests/test_sponge_one_lane.py holds that line) and the plain rounds must give the oracle's result: rows derived through an inverse of zero would not.
   The reference is computed once per (field, set) on PERIOD distinct states and tiled: PERIOD is coprime to 3, 21 and 64, so every state meets every lane.
2. Transcript parity: the Pickles public inputs, the kimchi `to_batch` rows and the opening check's prepared rows under the forced 3-lane form are byte-equal to
   the 8-lane form's on the same inputs (the 8-lane code is unchanged and held to the oracle by the existing suites), at 4, 22 and 43 proofs -- a partial wave,
   one past a full wave of 21, and two waves with the shadow lane in use; the jobs are accepted, one tampered evaluation at proof 21 rejects exactly that proof."""
import copy
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = [0x40000000000000000000000000000000224698FC094CF91B992D30ED00000001, 0x40000000000000000000000000000000224698FC0994A8DD8C46EB2100000001]
PERIOD = 251
SIZES = [8193, 8192 + 21, 8192 + 22, 8192 + 63, 8192 + 64]
LANES3 = dict(coop16_max=0, coop8_max=0, transcript_coop8_max=1)
LANES8 = dict(coop16_max=0, coop8_max=1 << 30, transcript_coop8_max=1 << 30, ipa_coop8_max=1 << 30, kimchi_coop8_max=1 << 30)
BATCHES = [4, 22, 43]


def le(x):
    return np.frombuffer(int(x).to_bytes(32, "little"), np.uint8)


def param_sets(field):
    import mina_bridge_amd.poseidon_params as PP
    p = P[field]
    rng = random.Random(90 + field)
    default = PP.default_params_bytes(field)
    rand = np.concatenate([le(rng.randrange(1, p)) for _ in range(9)] + [le(rng.randrange(p)) for _ in range(165)])
    zero_diag = np.frombuffer(bytes(default), np.uint8).copy()
    zero_diag[4 * 32:5 * 32] = 0                                   # mds[1][1]
    return {"compiled_in": default, "random": rand, "zero_on_diagonal": zero_diag}


def base_states(field):
    p = P[field]
    rng = random.Random(17 + field)
    m29 = (1 << 29) - 1
    vals = [0, p - 1, 1, 2, p - 2] + [(m29 << (29 * i)) % p for i in range(9)] + [(((1 << 261) - 1) ^ (m29 << (29 * i))) % p for i in range(9)]
    states = [[0, 0, 0], [p - 1, p - 1, p - 1]]
    states += [[vals[(i + j) % len(vals)] for j in (0, 5, 11)] for i in range(len(vals))]
    states += [[v if j == e else rng.randrange(p) for j in range(3)] for v in vals[:14] for e in range(3)]
    while len(states) < PERIOD:
        states.append([rng.randrange(p) for _ in range(3)])
    assert len(states) == PERIOD
    return np.stack([np.concatenate([le(x) for x in s]) for s in states])


@pytest.fixture(scope="module")
def perm_ctx():
    import mina_bridge_amd as m
    c = m.MinaContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def references(oracle):
    """(field, set) -> (parameter bytes, PERIOD states, their permutations by the CPU oracle): computed once, never written to"""
    out = {}
    for field in (0, 1):
        base = base_states(field)
        for name, params in param_sets(field).items():
            want = oracle.poseidon_permute(field, params, base.copy())
            want.setflags(write=False)
            out[(field, name)] = (params, base, want)
    return out


@pytest.mark.parametrize("name", ["compiled_in", "random", "zero_on_diagonal"])
@pytest.mark.parametrize("field", [0, 1])
def test_three_lane_permutation_equals_the_oracle(perm_ctx, references, field, name):
    params, base, want = references[(field, name)]
    perm_ctx.poseidon_set_params(field, params)
    for n in SIZES:
        idx = np.arange(n) % PERIOD
        got = perm_ctx.poseidon_permute(field, base[idx])
        bad = np.nonzero((got != want[idx]).any(axis=1))[0]
        assert not len(bad), f"field {field}, {name}, {n} states: {len(bad)} differ, first at {bad[:6].tolist()} (lane {int(bad[0]) % 21 * 3} of its wave)"


# ------------------------------------------------------------------------------------------------ transcripts
@pytest.fixture(scope="module")
def wrap(ctx_srs, oracle):
    import mina_bridge_amd as m
    from kimchi_helpers import install_index, install_step_index, load_k15_fixture, load_statement_fixture, make_step_index
    for f in (0, 1):
        ctx_srs.poseidon_set_params(f, m.poseidon_params.default_params_bytes(f))
    ix, _, _ = load_k15_fixture()
    install_index(ctx_srs, ix)
    install_step_index(ctx_srs, make_step_index(99))
    items, _ = load_statement_fixture()
    return {"m": m, "ctx": ctx_srs, "items": items}


def tiled(items, n):
    return [items[i % len(items)] for i in range(n)]


def statements(m, its, wraps=None, apps=None):
    from kimchi_helpers import statements_soa
    n_old, n_evals, sec = statements_soa(wraps or [it["wrap"] for it in its], apps or [it["app"] for it in its])
    return m.MinaContext.make_pickles_statements(n_old, n_evals, sec)


@pytest.mark.parametrize("batch", BATCHES)
def test_pickles_public_inputs_equal_the_eight_lane_form(wrap, batch):
    m, c = wrap["m"], wrap["ctx"]
    its = tiled(wrap["items"], batch)
    with m.lib.tuning(**LANES8):
        pub8, ok8 = c.pickles_public_inputs_batch(statements(m, its), batch)
    with m.lib.tuning(**LANES3):
        pub3, ok3 = c.pickles_public_inputs_batch(statements(m, its), batch)
    assert ok8.tolist() == [1] * batch and ok3.tolist() == [1] * batch
    assert (pub3 == pub8).all(), np.nonzero((pub3 != pub8).any(axis=(1, 2)))[0][:6]
    for b, it in enumerate(its[:4]):
        assert [int.from_bytes(x.tobytes(), "little") for x in pub3[b]] == it["pubs"]


@pytest.mark.parametrize("batch", BATCHES)
def test_kimchi_batch_rows_equal_the_eight_lane_form(wrap, batch):
    from kimchi_helpers import kimchi_arrays
    m, c = wrap["m"], wrap["ctx"]
    its = tiled(wrap["items"], batch)
    arrays, _ = kimchi_arrays([it["proof"] for it in its], [it["pubs"] for it in its])
    with m.lib.tuning(**LANES8):
        got8 = c.kimchi_to_batch(m.MinaContext.make_kimchi_proofs(batch, 2, 40, arrays), 15)
    with m.lib.tuning(**LANES3):
        got3 = c.kimchi_to_batch(m.MinaContext.make_kimchi_proofs(batch, 2, 40, arrays), 15)
    assert not got8["malformed"][0] and not got3["malformed"][0]
    for name in got8:
        assert (got3[name] == got8[name]).all(), name


@pytest.mark.parametrize("batch", BATCHES)
def test_opening_rows_equal_the_eight_lane_form(wrap, oracle, srs_oracle, batch):
    import ipa_rows_model as M
    m, c = wrap["m"], wrap["ctx"]
    g = [oracle.bytes_to_point(b) for b in srs_oracle[0][0][:64]]
    rng = random.Random(500 + batch)
    proofs = [M.random_proof(rng, 0, g, 3, 2, 2) for _ in range(batch)]
    packed = c.pack_ipa_openings([M.to_abi(q) for q in proofs])
    rb, sb = M.le32(rng.randrange(P[1])), M.le32(rng.randrange(P[1]))
    got = {}
    for form, tune in ((8, LANES8), (3, LANES3)):
        with m.lib.tuning(ipa_side_stream=1, **tune):
            got[form] = c.selftest_ipa_rows(0, packed, rb, sb)
        assert got[form]["lanes"] == form and got[form]["malformed"] == 0
    for name in ("points", "scalars", "chals", "sigma", "side"):
        assert (got[3][name] == got[8][name]).all(), name


@pytest.mark.parametrize("batch", BATCHES)
def test_jobs_accepted_and_one_tampered_evaluation_rejected(wrap, oracle, batch):
    from kimchi_helpers import kimchi_arrays
    m, c = wrap["m"], wrap["ctx"]
    its = tiled(wrap["items"], batch)

    def job(plist):
        a, o = kimchi_arrays(plist, [])
        kp = m.MinaContext.make_kimchi_proofs(batch, 2, 40, a, statements=statements(m, its))
        ja = dict(o); ja["rand_base"] = oracle.int_to_le(7); ja["sg_rand_base"] = oracle.int_to_le(9)
        ja["acc_prechallenges"] = np.concatenate([it["acc_pre"].reshape(-1) for it in its]); ja["acc_sg"] = np.concatenate([it["acc_sg"] for it in its])
        rho = np.random.Generator(np.random.PCG64(5)).integers(0, 256, (batch, 32), dtype=np.uint8); rho[:, 31] &= 0x3F
        ja["acc_rho"] = rho.reshape(-1)
        return m.MinaContext.make_state_jobs(batch, ja, with_ipa=1, with_accumulator=1, kimchi=kp, k=15, log2_domain=15, npub=40, n_evalpoints=2, n_comms=47, acc_k=16)
    plist = [it["proof"] for it in its]
    with m.lib.tuning(**LANES3):
        assert c.state_job_batch(job(plist)).tolist() == [1] * batch
        if batch > 21:
            bad = list(plist); bad[21] = copy.deepcopy(plist[21])
            bad[21]["evals"][40] = (bad[21]["evals"][40][0], (bad[21]["evals"][40][1] + 1) % (1 << 254))
            assert c.state_job_batch(job(bad)).tolist() == [0 if b == 21 else 1 for b in range(batch)]
