"""The device interpreter of PolishToken programs (kimchi_dev.cuh `ft_eval0_dev`, compiled into pickles_scalar_kernel for the step proof in Fp with per-lane feature
flags and into kimchi_scalar_kernel for the wrap proof in Fq) on the generated programs of tests/polish_model.py, installed through the real installs: 70 statements
in one launch on the step side (lanes on both sides of a 64-lane block, all flags different), 66 proofs on the wrap side, against tests/polish_model.py and, on at
least six lanes per program, the full oracle (oracle/pickles_ref.py, oracle/kimchi_ref.py); the single-proof host form (polish.h `polish_eval_host`) on three lanes
per program; and the programs both installs must refuse."""
import dataclasses
import random

import numpy as np
import pytest

import polish_model as PM
from oracle import kimchi_ref as K

pytestmark = pytest.mark.gpu
K_LOG2, NPUB, SEED = 6, 5, 20
N_STEP, N_WRAP, N_OLD = 70, 66, 1
ALWAYS = (0, 63, 64, 69)                                       # lanes checked against the full oracle for every program, beside two that rotate
STEP_PROGS = {p.name: p for p in PM.programs(PM.STEP, SEED)}
WRAP_PROGS = {p.name: p for p in PM.programs(PM.WRAP, SEED)}
ZK8 = ("lagrange", "regions")                                 # the families installed at zk_rows = 8 as well


def cases(progs, zk8=ZK8):
    out = [(n, 3) for n, p in progs.items() if p.valid and not n.startswith("bad_load")]
    return out + [(n, 8) for n, z in out if n.split("/")[0] in zk8]


@pytest.fixture(scope="module")
def world(srs_oracle):
    """a context of this file's own: both SRS, the Poseidon parameters, the k = 6 wrap index of tests/test_kimchi.py and the step index of make_step_index"""
    import mina_bridge_amd as m
    from ipa_helpers import poseidon_pp
    from kimchi_helpers import install_index, install_step_index, make_step_index
    from oracle import oracle as O
    g, h = srs_oracle[0]
    ctx = m.MinaContext(0)
    try:
        for f in (0, 1):
            ctx.poseidon_set_params(f, m.poseidon_params.default_params_bytes(f))
        for curve in (0, 1):
            ctx.srs_create(curve, 65536)
        circ = K.synthetic_circuit(0, g, O.bytes_to_point(h), poseidon_pp(0), poseidon_pp(1), K_LOG2, NPUB, seed=21)
        step = make_step_index(99)
        install_index(ctx, circ.index)
        install_step_index(ctx, step)
        ix = circ.index
        yield {"ctx": ctx, "circ": circ, "step": step, "comms": list(ix.sigma_comm) + list(ix.coefficients_comm) + list(ix.selector_comm)}
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ step side
@pytest.fixture(scope="module")
def statements(world):
    """70 statements, built once: distinct feature-flag bytes (all-off and all-on among them; lanes 63, 64 and 69 differ in feature 6), domains 10 and 16, one
    previous accumulator, all 19 optional evaluations, half of the lanes with a joint combiner.  With them what does not depend on the program: the
    oracle's public input and deferred values under the EMPTY program (per zk_rows), and the environment the program runs in."""
    from ipa_helpers import poseidon_pp
    from kimchi_helpers import statements_soa
    from oracle import pasta_ref as R, pickles_ref as PK
    from wire_writers import synth_wrap_proof
    rng = random.Random(4242)
    pool = [b for b in range(256) if b not in (0x00, 0xFF, 0x04, 0x40)]
    rng.shuffle(pool)
    flag_bytes = [0x40] + pool[:N_STEP - 1]                   # lane 0: lookup alone (feature 6, LookupTables, on)
    flag_bytes[63], flag_bytes[64], flag_bytes[69] = 0x00, 0xFF, 0x04          # all off; all on; foreign_field_add alone (no lookup pattern: feature 6 off)
    assert len(set(flag_bytes)) == N_STEP
    wraps, apps = [], []
    for b, fb in enumerate(flag_bytes):
        w = synth_wrap_proof(rng, k=K_LOG2)
        w["feature_flags"] = [bool(fb >> j & 1) for j in range(8)]
        w["domain_log2"] = 10 if b % 2 == 0 else 16
        w["prev_optional"] = [([rng.randrange(PK.P)], [rng.randrange(PK.P)]) for _ in range(PM.N_SLOTS)]
        w["joint_combiner"] = rng.getrandbits(128) if b % 4 in (0, 3) else None
        w["step_comms"], w["step_old_chals"] = w["step_comms"][:N_OLD], w["step_old_chals"][:N_OLD]
        wraps.append(w); apps.append(rng.randrange(PK.P))
    feat = [K.feature_mask(w["feature_flags"]) for w in wraps]
    assert [f >> 6 & 1 for f in (feat[0], feat[63], feat[64], feat[69])] == [1, 0, 1, 0] and sum(w["joint_combiner"] is not None for w in wraps) == N_STEP // 2
    n_old, n_evals, sec = statements_soa(wraps, apps)
    assert (n_old, n_evals) == (N_OLD, 62)
    step = world["step"]
    base, msgs = {3: [], 8: []}, []
    for w, a in zip(wraps, apps):
        empty = dataclasses.replace(step, constant_term=[], zk_rows=3)
        pubs, dv, mw, ms = PK.statement_public_input(w, empty, world["comms"], a, poseidon_pp(0), poseidon_pp(1))
        msgs.append((mw, ms)); base[3].append((pubs, dv))
        dv8 = PK.compute_deferred_values(w, dataclasses.replace(empty, zk_rows=8), poseidon_pp(0))
        base[8].append((PK.wrap_public_input(w, dv8, mw, ms), dv8))

    def env(b, zk):
        w, dv = wraps[b], base[zk][b][1]
        k = w["domain_log2"]
        zetaw = dv["zeta"] * K.O_domain_generator(PK.P, k) % PK.P
        zn, zwn = pow(dv["zeta"], 1 << 16, PK.P), pow(zetaw, 1 << 16, PK.P)
        seq = [PK.combine_chunks(pr, zn, zwn, PK.P) for pr in PK.prev_evals_sequence(w)]
        joint = R.challenge_to_field(w["joint_combiner"], PK.endo_fp(), PK.P) if w["joint_combiner"] is not None else 0
        return PM.Env(PK.P, k, zk, dv["zeta"], dv["alpha"], w["beta"] % PK.P, w["gamma"] % PK.P, joint, R.endo_q(0), step.mds, seq, features=feat[b], present=(1 << PM.N_SLOTS) - 1)
    envs = {zk: [env(b, zk) for b in range(N_STEP)] for zk in (3, 8)}
    return {"wraps": wraps, "apps": apps, "feat": feat, "sec": sec, "base": base, "msgs": msgs, "envs": envs}


def expected_step(statements, tokens, zk, b):
    """the 40 public inputs of lane b under `tokens`: the oracle's under the empty program, with cip(P) = cip(empty) - xi^(n_old + 1) * model(P)"""
    from oracle import pickles_ref as PK
    pubs, dv = statements["base"][zk][b]
    cip = (dv["combined_inner_product"] - pow(dv["xi"], N_OLD + 1, PK.P) * PM.evaluate(tokens, statements["envs"][zk][b])) % PK.P
    return [PK.shifted_type1(cip) % PK.Q] + pubs[1:]


def full_oracle_step(world, statements, tokens, zk, b):
    from ipa_helpers import poseidon_pp
    from oracle import pickles_ref as PK
    w = statements["wraps"][b]
    dv = PK.compute_deferred_values(w, dataclasses.replace(world["step"], constant_term=tokens, zk_rows=zk), poseidon_pp(0))
    return PK.wrap_public_input(w, dv, *statements["msgs"][b])


def launch_step(world, statements, tokens, zk):
    from kimchi_helpers import install_step_index
    ctx = world["ctx"]
    install_step_index(ctx, dataclasses.replace(world["step"], constant_term=tokens, zk_rows=zk))
    try:
        return ctx.pickles_public_inputs_batch(ctx.make_pickles_statements(N_OLD, 62, statements["sec"]), N_STEP)
    finally:
        install_step_index(ctx, world["step"])


def rotating(name, n, count=2):
    rng = random.Random("lanes/" + name)
    return rng.sample([b for b in range(n) if b not in ALWAYS], count)


@pytest.mark.parametrize("name,zk", cases(STEP_PROGS))
def test_step_program_on_seventy_lanes_with_their_own_flags(world, statements, oracle, name, zk):
    import mina_bridge_amd as m
    from wire_writers import wrap_proof_bytes
    tokens = STEP_PROGS[name].tokens
    pub, ok = launch_step(world, statements, tokens, zk)
    assert ok.tolist() == [1] * N_STEP
    got = [[oracle.le_to_int(x) for x in pub[b]] for b in range(N_STEP)]
    want = [expected_step(statements, tokens, zk, b) for b in range(N_STEP)]
    assert [b for b in range(N_STEP) if got[b] != want[b]] == []
    # the relation the expectations rest on, proven on six lanes against the whole oracle with this program
    for b in ALWAYS + tuple(rotating(name, N_STEP)):
        assert full_oracle_step(world, statements, tokens, zk, b) == want[b], b
    # the single-proof host form (polish_eval_host) on three lanes
    from kimchi_helpers import install_step_index
    ctx = world["ctx"]
    install_step_index(ctx, dataclasses.replace(world["step"], constant_term=tokens, zk_rows=zk))
    try:
        for b in (63, 64, rotating(name, N_STEP)[0]):
            pub1, _ = ctx.pickles_public_input(wrap_proof_bytes(statements["wraps"][b], True), m.lib.ENC_BINPROT, oracle.int_to_le(statements["apps"][b]))
            assert [oracle.le_to_int(x) for x in pub1] == want[b], b
    finally:
        install_step_index(ctx, world["step"])


def test_step_load_of_a_slot_only_a_skipped_store_fills_fails_that_lane_alone(world, statements, oracle):
    """`bad_load`: ok is 0 exactly on the lanes whose feature 6 is off; every other lane's 40 outputs are what a launch without the bad lanes gives"""
    import mina_bridge_amd as m
    from kimchi_helpers import install_step_index
    from wire_writers import wrap_proof_bytes
    tokens = STEP_PROGS["bad_load/feature6"].tokens
    pub, ok = launch_step(world, statements, tokens, 3)
    on = [f >> 6 & 1 for f in statements["feat"]]
    assert ok.tolist() == on and 0 < sum(on) < N_STEP and on[63] == 0 and on[64] == 1
    good = [b for b in range(N_STEP) if on[b]]
    for b in good:
        assert [oracle.le_to_int(x) for x in pub[b]] == expected_step(statements, tokens, 3, b), b
    for b in (0, 64, good[-1], good[len(good) // 2], good[1], good[2]):
        assert full_oracle_step(world, statements, tokens, 3, b) == expected_step(statements, tokens, 3, b), b
    with pytest.raises(KeyError):
        full_oracle_step(world, statements, tokens, 3, 63)
    with pytest.raises(LookupError):
        PM.evaluate(tokens, statements["envs"][3][63])
    # a launch of the good lanes alone
    ctx = world["ctx"]
    sec = {k: (v.reshape(N_STEP, -1)[good].reshape(-1) if v.size >= N_STEP else v) for k, v in statements["sec"].items()}
    install_step_index(ctx, dataclasses.replace(world["step"], constant_term=tokens))
    try:
        pub2, ok2 = ctx.pickles_public_inputs_batch(ctx.make_pickles_statements(N_OLD, 62, sec), len(good))
        assert ok2.all() and (pub2 == pub[good]).all()
        # the host form fails such a proof too, and passes its neighbour
        with pytest.raises(m.MinaError):
            ctx.pickles_public_input(wrap_proof_bytes(statements["wraps"][63], True), m.lib.ENC_BINPROT, oracle.int_to_le(statements["apps"][63]))
        pub1, _ = ctx.pickles_public_input(wrap_proof_bytes(statements["wraps"][64], True), m.lib.ENC_BINPROT, oracle.int_to_le(statements["apps"][64]))
        assert [oracle.le_to_int(x) for x in pub1] == expected_step(statements, tokens, 3, 64)
    finally:
        install_step_index(ctx, world["step"])


# ------------------------------------------------------------------------------------------------ wrap side
@pytest.fixture(scope="module")
def wrap_lanes(world, srs_oracle):
    """66 lanes: the commitments of the four minted k = 6 proofs of tests/test_kimchi.py in turn, the evaluations and ft_eval1 random canonical values (ft_eval0
    needs no valid proof); the oracle's intermediates under the empty program per zk_rows, and the environment the program runs in"""
    import mina_bridge_amd as m
    from ipa_helpers import poseidon_pp
    from kimchi_helpers import kimchi_arrays
    from oracle import oracle as O, pasta_ref as R
    g, h = srs_oracle[0]
    circ = world["circ"]
    minted = []
    for s in range(4):
        rng = random.Random(100 + s)
        pubs = [rng.randrange(R.Q) for _ in range(NPUB)]
        minted.append((pubs, K.synthetic_proof(circ, g, O.bytes_to_point(h), poseidon_pp(0), poseidon_pp(1), pubs, seed=200 + s)))
    rng = random.Random(777)
    lanes = []
    for b in range(N_WRAP):
        pubs, proof = minted[b % 4]
        p = dict(proof)
        p["evals"] = [(rng.randrange(R.Q), rng.randrange(R.Q)) for _ in range(K.N_EVAL_COLS)]
        p["ft_eval1"] = rng.randrange(R.Q)
        lanes.append((pubs, p))
    arrays, _ = kimchi_arrays([p for _, p in lanes], [pi for pi, _ in lanes])
    kp = m.MinaContext.make_kimchi_proofs(N_WRAP, 2, NPUB, arrays)

    def oracle_call(b, tokens, zk):
        ix = dataclasses.replace(circ.index, constant_term=tokens, zk_rows=zk)
        return K.oracles_and_batch(ix, lanes[b][1], lanes[b][0], poseidon_pp(0), poseidon_pp(1), g, O.bytes_to_point(h), ft_comm=False)[0]
    base = {zk: [oracle_call(b, [(K.T_LITERAL, 0)], zk) for b in range(N_WRAP)] for zk in (3, 8)}       # the oracle wants a value on the stack: the program `0` stands for the empty one
    envs = {zk: [PM.Env(R.Q, K_LOG2, zk, o["zeta"], o["alpha"], o["beta"], o["gamma"], 0, R.endo_q(1), circ.index.mds, lanes[b][1]["evals"]) for b, o in enumerate(base[zk])] for zk in (3, 8)}
    return {"lanes": lanes, "kp": kp, "base": base, "envs": envs, "oracle_call": oracle_call}


def expected_wrap(wrap_lanes, tokens, zk, b):
    """(ft_eval0, cip) of lane b: ft_eval0(P) = ft_eval0(empty) - model(P), and the oracle's own combined inner product over the list with that entry"""
    from oracle import ipa_ref as I, pasta_ref as R
    o = wrap_lanes["base"][zk][b]
    ft = (o["ft_eval0"] - PM.evaluate(tokens, wrap_lanes["envs"][zk][b])) % R.Q
    evals = [list(e) for e in o["evaluations"]]
    assert evals[2 + 1] == [o["ft_eval0"], wrap_lanes["lanes"][b][1]["ft_eval1"]]          # two recursion rows, the public row, then ft
    evals[2 + 1][0] = ft
    return ft, I.combined_inner_product(evals, o["v"], o["u"], R.Q)


def launch_wrap(world, wrap_lanes, tokens, zk):
    from kimchi_helpers import install_index
    ctx, ix = world["ctx"], world["circ"].index
    install_index(ctx, dataclasses.replace(ix, constant_term=tokens, zk_rows=zk))
    try:
        return ctx.kimchi_to_batch(wrap_lanes["kp"], K_LOG2)
    finally:
        install_index(ctx, ix)


@pytest.mark.parametrize("name,zk", cases(WRAP_PROGS, zk8=("lagrange",)))
def test_wrap_program_on_sixty_six_lanes(world, wrap_lanes, oracle, name, zk):
    """mask 0 on this side: a SkipIf region always runs, a SkipIfNot region never does"""
    tokens = WRAP_PROGS[name].tokens
    got = launch_wrap(world, wrap_lanes, tokens, zk)
    assert not got["malformed"][0]
    want = [expected_wrap(wrap_lanes, tokens, zk, b) for b in range(N_WRAP)]
    assert [b for b in range(N_WRAP) if (oracle.le_to_int(got["ft_eval0"][b]), oracle.le_to_int(got["cip"][b])) != want[b]] == []
    for b in (0, 1, 63, 64) + tuple(rotating(name, N_WRAP)):
        o = wrap_lanes["oracle_call"](b, tokens, zk)
        assert (o["ft_eval0"], o["combined_inner_product"]) == want[b], b
    if name.startswith("regions/"):                           # the values above are the model's under mask 0, and the mask matters to them
        env = wrap_lanes["envs"][zk][0]
        assert env.features == 0 and PM.evaluate(tokens, env) != PM.evaluate(tokens, env.with_masks(K.feature_mask([True] * 8)))


def test_wrap_load_of_a_slot_only_a_skipped_store_fills_fails_the_batch(world, wrap_lanes):
    """no features on the wrap side: feature 6 is off on every lane, the LOAD finds nothing, the call says so -- and the index installed before still works"""
    got = launch_wrap(world, wrap_lanes, WRAP_PROGS["bad_load/feature6"].tokens, 3)
    assert got["malformed"][0]
    with pytest.raises(LookupError):
        PM.evaluate(WRAP_PROGS["bad_load/feature6"].tokens, wrap_lanes["envs"][3][0])


# ------------------------------------------------------------------------------------------------ refusals
def test_both_installs_refuse_what_the_validator_refuses_and_keep_the_index_they_had(world, statements, wrap_lanes, oracle):
    import mina_bridge_amd as m
    from kimchi_helpers import STEP_DOMAINS, pts
    from oracle import oracle as O
    ctx, ix, step = world["ctx"], world["circ"].index, world["step"]
    sh = np.concatenate([O.ints_to_le(step.shifts[k]).reshape(-1) for k in STEP_DOMAINS])
    before_step = ctx.pickles_public_inputs_batch(ctx.make_pickles_statements(N_OLD, 62, statements["sec"]), N_STEP)
    before_wrap = ctx.kimchi_to_batch(wrap_lanes["kp"], K_LOG2)
    for side, progs in ((PM.STEP, STEP_PROGS), (PM.WRAP, WRAP_PROGS)):
        bad = {n: PM.encode(p.tokens) for n, p in progs.items() if not p.valid}
        assert set(bad) == {"deep/stack25", "deep/cache9"}
        bad.update(PM.refusals(side))
        assert "column = ncols" in bad and "region past the end" in bad and "feature code 21" in bad and "literal = modulus" in bad
        for name, code in bad.items():
            with pytest.raises(m.MinaError):
                if side == PM.STEP:
                    ctx.step_index_install(step.zk_rows, STEP_DOMAINS, sh, code)
                else:
                    ctx.verifier_index_install(ix.log2_domain, ix.zk_rows, ix.perm_alpha_offset, O.ints_to_le(ix.shifts).reshape(-1), pts(ix.sigma_comm), pts(ix.coefficients_comm),
                                               pts(ix.selector_comm), code)
    assert PM.SIDES[PM.WRAP][2] == 43
    after_step = ctx.pickles_public_inputs_batch(ctx.make_pickles_statements(N_OLD, 62, statements["sec"]), N_STEP)
    after_wrap = ctx.kimchi_to_batch(wrap_lanes["kp"], K_LOG2)
    assert (after_step[0] == before_step[0]).all() and after_step[1].tolist() == [1] * N_STEP == before_step[1].tolist()
    assert all((after_wrap[k] == before_wrap[k]).all() for k in ("ft_eval0", "cip", "polyscale", "evalscale")) and not after_wrap["malformed"][0]
    # and what it computes is still the index of before: the step program of make_step_index, the wrap circuit's own
    b = 64
    assert [oracle.le_to_int(x) for x in after_step[0][b]] == expected_step(statements, step.constant_term, 3, b)
    assert (oracle.le_to_int(after_wrap["ft_eval0"][b]), oracle.le_to_int(after_wrap["cip"][b])) == expected_wrap(wrap_lanes, ix.constant_term, ix.zk_rows, b)
