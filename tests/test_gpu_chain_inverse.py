"""The chain inverse (mina_ctx_set_chain_inverse): the `_gcd` twins of the kernels that carry the single-lane inversions of the wrap-proof chain's scalar stages and of
the Lagrange set-up -- pickles_scalar, kimchi_scalar, kimchi_pub<8> / <10>, kimchi_ftcomm, pubcomm_finish16, pubcomm_finish, lagrange_finish, lagrange_digit_table,
points_sum -- against the mode off on the same context.  The inverse of a field element is unique, so every comparison is byte equality; where the existing tests
compare a path with oracle/, the mode on is compared with it once more.  Shapes are the k = 6 synthetic indexes of tests/test_gpu_polish_programs.py and the reduced
Proof-of-State job of smoke().  The boundary (mina_verify_*) has no flag for the mode (tests/test_fast_inverse_abi.py pins that none exists), so no test here goes
through it."""
import copy
import dataclasses
import random

import numpy as np
import pytest

import polish_model as PM
import shard_block_cases as SB
import srs_helpers as S
from dev_helpers import Dev
from oracle import kimchi_ref as K

pytestmark = pytest.mark.gpu
K_LOG2, SEED = 6, 20
N_LANES, N_OLD = 65, 1
MINA_ERR_ARG = -1
STEP_PROGS = {p.name: p for p in PM.programs(PM.STEP, SEED) if p.valid and p.name.split("/")[0] in ("lagrange", "regions")}
KIMCHI_OUTPUTS = ("cip", "ft_eval0", "evalpoints", "polyscale", "evalscale", "comms", "sponge_state", "sponge_pos", "malformed")


@pytest.fixture(scope="module")
def world(srs_oracle):
    """a context of this file's own (the mode is context state): both SRS, the Poseidon parameters, the k = 6 wrap index of tests/test_kimchi.py, the step index"""
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
        circ = K.synthetic_circuit(0, g, O.bytes_to_point(h), poseidon_pp(0), poseidon_pp(1), K_LOG2, 5, seed=21)
        step = make_step_index(99)
        install_index(ctx, circ.index)
        install_step_index(ctx, step)
        ix = circ.index
        yield {"ctx": ctx, "circ": circ, "step": step, "comms": list(ix.sigma_comm) + list(ix.coefficients_comm) + list(ix.selector_comm)}
    finally:
        ctx.set_chain_inverse(False); ctx.set_fast_inverse(False)
        ctx.close()


def off_on(ctx, call, launches=None):
    """call() with the mode off, then on -> (off result, on result).  The covered launches are counted under the form that ran and none under the other: off moves
    fermat_launches alone, on moves gcd_launches alone, both by `launches` where the caller knows the number"""
    ctx.set_chain_inverse(False)
    s0 = ctx.chain_inverse_stats()
    off = call()
    s1 = ctx.chain_inverse_stats()
    ctx.set_chain_inverse(True)
    try:
        on = call()
        s2 = ctx.chain_inverse_stats()
    finally:
        ctx.set_chain_inverse(False)
    d_off, d_on = s1["fermat_launches"] - s0["fermat_launches"], s2["gcd_launches"] - s1["gcd_launches"]
    assert s1["gcd_launches"] == s0["gcd_launches"] and s2["fermat_launches"] == s1["fermat_launches"], (s0, s1, s2)
    assert d_off == d_on and d_on > 0 and (launches is None or d_on == launches), (launches, s0, s1, s2)
    return off, on


# ------------------------------------------------------------------------------------------------ mina_kimchi_to_batch
@pytest.fixture(scope="module")
def wrap_lanes(world, srs_oracle):
    """65 lanes: one minted k = 6 proof's commitments, the evaluations, ft_eval1 and 41 public inputs random canonical values per lane (the call builds rows, it does
    not verify, and ft_eval0 needs no valid proof)"""
    from ipa_helpers import poseidon_pp
    from oracle import oracle as O, pasta_ref as R
    g, h = srs_oracle[0]
    rng = random.Random(100)
    proof = K.synthetic_proof(world["circ"], g, O.bytes_to_point(h), poseidon_pp(0), poseidon_pp(1), [rng.randrange(R.Q) for _ in range(5)], seed=200)
    rng = random.Random(778)
    lanes = []
    for b in range(N_LANES):
        p = dict(proof)
        p["evals"] = [(rng.randrange(R.Q), rng.randrange(R.Q)) for _ in range(K.N_EVAL_COLS)]
        p["ft_eval1"] = rng.randrange(R.Q)
        lanes.append(([rng.randrange(R.Q) for _ in range(41)], p))
    return lanes


@pytest.mark.parametrize("npub", [5, 9, 33, 40, 41])
@pytest.mark.parametrize("batch", [1, 8, 9, 64, 65])
def test_kimchi_to_batch(world, wrap_lanes, srs_oracle, oracle, batch, npub):
    """8 proofs per 64-lane block in kimchi_pub / kimchi_ftcomm, 64 in kimchi_scalar: batches on both sides of either; npub: one short chunk of 8, a short second
    chunk, chunks of 10 with a 3-term tail, exactly one pass of the lanes, and a second pass (41 > 40: chunks of 8 again, 6 chunks x 2 sides = 12 items on 8 lanes)"""
    import mina_bridge_amd as m
    from ipa_helpers import poseidon_pp
    from kimchi_helpers import kimchi_arrays
    ctx = world["ctx"]
    lanes = wrap_lanes[:batch]
    arrays, _ = kimchi_arrays([p for _, p in lanes], [pi[:npub] for pi, _ in lanes])
    kp = m.MinaContext.make_kimchi_proofs(batch, 2, npub, arrays)
    ctx.state_jobs_prepare(K_LOG2, npub)                         # the Lagrange tables are current: the call below launches its own four covered kernels and no set-up
    off, on = off_on(ctx, lambda: ctx.kimchi_to_batch(kp, K_LOG2), launches=4)       # pubcomm_finish16, kimchi_pub, kimchi_scalar, kimchi_ftcomm
    for key in KIMCHI_OUTPUTS:
        assert (np.asarray(on[key]) == np.asarray(off[key])).all(), key
    assert not on["malformed"][0]
    if batch == 1:                                               # once per npub: the oracle's rows for lane 0, as tests/test_kimchi.py compares them
        g, h = srs_oracle[0]
        pubs, proof = lanes[0]
        o, entry = K.oracles_and_batch(world["circ"].index, proof, pubs[:npub], poseidon_pp(0), poseidon_pp(1), g, oracle.bytes_to_point(h))
        assert oracle.le_to_int(on["ft_eval0"][0]) == o["ft_eval0"] and oracle.le_to_int(on["cip"][0]) == o["combined_inner_product"]
        assert [oracle.le_to_int(on["evalpoints"][0, :32]), oracle.le_to_int(on["evalpoints"][0, 32:])] == entry["evalpoints"]
        assert [oracle.bytes_to_point(c) for c in on["comms"][0]] == o["comms"]       # with the public-input commitment and the ft row


# ------------------------------------------------------------------------------------------------ mina_pickles_public_inputs_batch
@pytest.fixture(scope="module")
def statements(world):
    """65 statements over the step domains 2^10 and 2^16, distinct feature flags, all 19 optional evaluations, half with a joint combiner"""
    from kimchi_helpers import statements_soa
    from oracle import pickles_ref as PK
    from wire_writers import synth_wrap_proof
    rng = random.Random(4343)
    flag_bytes = rng.sample(range(256), N_LANES)
    wraps, apps = [], []
    for b, fb in enumerate(flag_bytes):
        w = synth_wrap_proof(rng, k=K_LOG2)
        w["feature_flags"] = [bool(fb >> j & 1) for j in range(8)]
        w["domain_log2"] = 10 if b % 2 == 0 else 16
        w["prev_optional"] = [([rng.randrange(PK.P)], [rng.randrange(PK.P)]) for _ in range(PM.N_SLOTS)]
        w["joint_combiner"] = rng.getrandbits(128) if b % 4 in (0, 3) else None
        w["step_comms"], w["step_old_chals"] = w["step_comms"][:N_OLD], w["step_old_chals"][:N_OLD]
        wraps.append(w); apps.append(rng.randrange(PK.P))
    n_old, n_evals, sec = statements_soa(wraps, apps)
    assert (n_old, n_evals) == (N_OLD, 62)
    return {"wraps": wraps, "apps": apps, "sec": sec}


@pytest.mark.parametrize("zk", [3, 8])
@pytest.mark.parametrize("name", sorted(STEP_PROGS))
def test_pickles_public_inputs_batch(world, statements, oracle, name, zk):
    """1, 64 and 65 statements (one block, a full block, a second block) under the `lagrange` and `regions` programs at zk_rows 3 and 8: `lagrange/rows` holds the
    token's three offset forms (a row from the start, from the first zero-knowledge row, that row itself)"""
    from ipa_helpers import poseidon_pp
    from kimchi_helpers import install_step_index
    from oracle import pickles_ref as PK
    ctx, tokens = world["ctx"], STEP_PROGS[name].tokens
    if name == "lagrange/rows":
        offs = [t[1] for t in tokens if t[0] == K.T_LAGRANGE]
        assert any(o >= 0 for o in offs) and any(PM.INT32_MIN < o < 0 for o in offs) and PM.INT32_MIN in offs
    step = dataclasses.replace(world["step"], constant_term=tokens, zk_rows=zk)
    install_step_index(ctx, step)
    try:
        for n in (1, 64, 65):
            sec = {k: (v.reshape(N_LANES, -1)[:n].reshape(-1).copy() if v.size >= N_LANES else v) for k, v in statements["sec"].items()}
            st = ctx.make_pickles_statements(N_OLD, 62, sec)
            (pub0, ok0), (pub1, ok1) = off_on(ctx, lambda: ctx.pickles_public_inputs_batch(st, n), launches=1)
            assert (pub1 == pub0).all() and (ok1 == ok0).all() and ok1.tolist() == [1] * n, n
        if name == "lagrange/rows":                              # the whole oracle on the two lanes either side of the block edge, mode on
            for b in (63, 64):
                w, a = statements["wraps"][b], statements["apps"][b]
                _, _, mw, ms = PK.statement_public_input(w, dataclasses.replace(step, constant_term=[]), world["comms"], a, poseidon_pp(0), poseidon_pp(1))
                want = PK.wrap_public_input(w, PK.compute_deferred_values(w, step, poseidon_pp(0)), mw, ms)
                assert [oracle.le_to_int(x) for x in pub1[b]] == want, b
    finally:
        install_step_index(ctx, world["step"])


# ------------------------------------------------------------------------------------------------ public-input commitments
@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("k", [4, 5, 6])
def test_srs_lagrange_basis(world, oracle, srs_oracle, curve, k):
    from oracle import pasta_ref as R
    from test_lagrange import expected_basis_point
    ctx = world["ctx"]
    off, on = off_on(ctx, lambda: ctx.srs_lagrange_basis(curve, k), launches=1)       # lagrange_finish
    assert (on == off).all()
    g, _ = srs_oracle[curve]
    for i in (0, 1, (1 << k) - 1):
        assert (on[i] == expected_basis_point(oracle, R, curve, g, k, i)).all(), i


def _prepare_again(ctx, k, npub):
    """mina_state_jobs_prepare rebuilds nothing that is current: another domain first, so that the basis, the window table and the digit table are built under the
    mode the context is in"""
    ctx.state_jobs_prepare(k - 1, min(npub, 1 << (k - 1)))
    ctx.state_jobs_prepare(k, npub)


@pytest.mark.parametrize("npub", [5, 40])
def test_public_input_commitment_batch_after_a_prepare_under_each_mode(world, oracle, srs_oracle, npub):
    """the tables of lagrange_finish and lagrange_digit_table built with the mode off and with it on; under either, batches of 1, 64 and 65 commitments with the
    finish in both forms: one set of bytes, the oracle's h - sum_i pub_i L_i; all-zero inputs give h itself (A at infinity going into the addition)"""
    from conftest import rand_scalars
    from oracle import pasta_ref as R
    ctx, curve, k = world["ctx"], 0, K_LOG2
    mod = R.base_modulus(curve)
    h = srs_oracle[curve][1]
    pub = rand_scalars(65 * npub, R.Q, seed=3100 + npub).reshape(65, npub, 32)
    pub[7] = 0
    seen = {}
    for prepared_on in (False, True):
        ctx.set_chain_inverse(prepared_on)
        before = ctx.chain_inverse_stats()
        try:
            _prepare_again(ctx, k, npub)
        finally:
            ctx.set_chain_inverse(False)
        after = ctx.chain_inverse_stats()
        moved, still = ("gcd_launches", "fermat_launches") if prepared_on else ("fermat_launches", "gcd_launches")
        assert after[moved] - before[moved] == 4 and after[still] == before[still], (before, after)       # two prepares: a basis and a digit table each
        for n in (1, 64, 65):
            off, on = off_on(ctx, lambda: ctx.public_input_commitment_batch(curve, k, pub[:n], n), launches=1)       # pubcomm_finish
            assert (on == off).all()
            seen[prepared_on, n] = on
    for n in (1, 64, 65):
        assert (seen[True, n] == seen[False, n]).all(), n
    got = seen[True, 65]
    assert (got[7] == h).all()
    basis = ctx.srs_lagrange_basis(curve, k)
    for b in (0, 63, 64):
        a = oracle.bytes_to_point(oracle.msm_naive(curve, basis[:npub], pub[b]))
        assert oracle.bytes_to_point(got[b]) == R.add(oracle.bytes_to_point(h), R.neg(a, mod), mod), b


@pytest.mark.parametrize("curve", [0, 1])
def test_commitments_on_related_lagrange_points(oracle, curve):
    """the degenerate rows of tests/test_gpu_pubcomm_degenerate.py on its crafted SRS S1 (L_i = c_i G, h = t G): a commitment at infinity (A = H), A at infinity,
    A = -H (a doubling in the finish), all-zero inputs -- with the basis and the tables built under the mode on, against the big-integer reference"""
    import mina_bridge_amd as m
    c, t = S.s1_coefficients(curve), S.blinder(curve)
    g, h, G = S.structured_srs(oracle, curve, c, t)
    ctx = m.MinaContext(0)
    try:
        for field in (0, 1):
            ctx.poseidon_set_params(field, m.poseidon_params.default_params_bytes(field))
        ctx.srs_load(curve, S.srs_blob(oracle, curve, g, h))
        for key, cases in (("rows", S.s1_cases(curve, c, t)), ("rows_small", S.s1_cases_small(curve, c, t))):
            names = list(cases)
            cases = dict(cases, all_zero={"pubs": [0] * len(next(iter(cases.values()))["pubs"])})
            names.append("all_zero")
            pub = S.rows_le(oracle, cases)
            want = np.stack([S.reference_commitment(oracle, curve, c, t, G, v["pubs"]) for v in cases.values()])
            assert not want[names.index("a_eq_h")].any() and (want[names.index("all_zero")] == h).all()
            call = lambda: ctx.public_input_commitment_batch(curve, S.LOG2_DOMAIN, pub, len(names))
            ctx.set_chain_inverse(True)
            first = call()                                       # the first call of all builds the basis and the tables, under the mode on
            off, on = off_on(ctx, call, launches=1)
            wrong = [n for n, f, a, b, w in zip(names, first, off, on, want) if not ((f == b).all() and (a == b).all() and (b == w).all())]
            assert not wrong, (key, wrong)
    finally:
        ctx.set_chain_inverse(False)
        ctx.close()


# ------------------------------------------------------------------------------------------------ mina_points_sum_dev
@pytest.mark.parametrize("curve", [1, 0])
def test_points_sum_dev(world, oracle, srs_oracle, curve):
    ctx = world["ctx"]
    g = srs_oracle[curve][0]
    P, Q, R_ = g[0], g[1], g[2]
    cases = {"n1": [SB.rec(P)], "n1_inf": [SB.rec_inf(garbage=3)], "n2_cancel": [SB.rec(P), SB.rec(SB.neg(curve, P))], "n2": [SB.rec(P), SB.rec(Q)],
             "n5_inf_among": [SB.rec(P), SB.rec_inf(garbage=5), SB.rec(Q), SB.rec(R_), SB.rec(P)],
             "n5_sum_inf": [SB.rec(P), SB.rec(Q), SB.rec_inf(), SB.rec(SB.neg(curve, Q)), SB.rec(SB.neg(curve, P))]}
    d = Dev(ctx)
    try:
        for name, recs in cases.items():
            recs = np.stack(recs)
            d_recs, d_out = d.put(recs), d.alloc(72)

            def call():
                ctx.dev_upload(d_out, np.full(72, 0xEE, np.uint8))
                ctx.points_sum_dev(curve, len(recs), d_recs, d_out)
                return d.get(d_out, 72)
            off, on = off_on(ctx, call, launches=1)
            want = SB.rec(SB.ref_points_sum(oracle, curve, recs))
            assert (on == off).all() and on[:68].tobytes() == want.tobytes() and (on[68:] == 0xEE).all(), name
            assert bool(on[64:68].view(np.uint32)[0]) == ("inf" in name.split("_")[-1] or name == "n2_cancel"), name
    finally:
        d.close()


# ------------------------------------------------------------------------------------------------ a reduced Proof-of-State job
SHAPE = dict(k=7, log2_domain=7, npub=8, n_comms=6, slot=2, n_points=2, acc_k=8)
MODES = [(False, False), (True, False), (False, True), (True, True)]        # (fast inverse: the MSM finish, chain inverse)


@pytest.fixture(scope="module")
def minted():
    """the job smoke() runs, on the 2^10 SRS it runs on: two valid proofs, and the pair with one public input of the second tampered"""
    from oracle import oracle as O
    from state_job_helpers import mint_job
    srs = {c: O.srs_create(c, 1 << 10, threads=4) for c in (0, 1)}
    jobs = [mint_job(srs[0], srs[1], 2900 + 10 * i, **SHAPE) for i in range(2)]
    bad = [jobs[0], copy.deepcopy(jobs[1])]
    bad[1]["pubs"][0] ^= 1
    return jobs, bad


def _job_ctx(m):
    c = m.MinaContext(0)
    for f in (0, 1):
        c.poseidon_set_params(f, m.poseidon_params.default_params_bytes(f))
    c.srs_create(0, 1 << 10); c.srs_create(1, 1 << 10)
    return c


def _build(m, jobs):
    from state_job_helpers import build_jobs
    return build_jobs(m, jobs, SHAPE["k"], SHAPE["log2_domain"], SHAPE["slot"], SHAPE["acc_k"])


def test_state_job_on_a_lone_lane_and_on_four_pipelined_lanes(minted):
    """mina_state_job_batch on the lone lane and mina_state_job_batch_dev on four pipelined lanes (five jobs back to back: a lane is used twice), with each mode alone
    and with both: verdicts and flags are the mode off's; the tampered public input -- the one input that reaches the verdict through pubcomm_finish16 alone -- is
    rejected in every mode"""
    import mina_bridge_amd as m
    ctx = _job_ctx(m)
    try:
        _state_job_in_every_mode(m, ctx, minted)
    finally:
        ctx.close()


def _state_job_in_every_mode(m, ctx, minted):
    jobs, bad = minted
    ctx.state_jobs_prepare(SHAPE["log2_domain"], SHAPE["npub"])
    nb, seen = len(jobs), {}
    ptrs = []
    try:
        dev = {}
        for tag, js in (("good", jobs), ("bad", bad)):
            dev[tag], p = ctx.state_jobs_to_device(_build(m, js)); ptrs += p
        outs = [ctx.dev_malloc(4 * nb + 16) for _ in range(5)]; ptrs += outs
        for fast, chain in MODES:
            ctx.set_fast_inverse(fast); ctx.set_chain_inverse(chain)
            c0, f0 = ctx.chain_inverse_stats(), ctx.inverse_stats()
            lone = {tag: ctx.state_job_batch(_build(m, js)).tolist() for tag, js in (("good", jobs), ("bad", bad))}
            ctx.set_pipeline(4)
            try:
                for i, o in enumerate(outs):
                    ctx.dev_upload(o, np.full(4 * nb + 16, 0xEE, np.uint8))
                    ctx.state_job_batch_dev(dev["bad" if i == 2 else "good"], o, o + 4 * nb)
                ctx.synchronize()
                piped = [ctx.dev_download(o, 4 * nb + 16).view(np.uint32).tolist() for o in outs]
            finally:
                ctx.synchronize(); ctx.set_pipeline(1)
            c1, f1 = ctx.chain_inverse_stats(), ctx.inverse_stats()
            moved, still = ("gcd_launches", "fermat_launches") if chain else ("fermat_launches", "gcd_launches")
            assert c1[moved] > c0[moved] and c1[still] == c0[still], (fast, chain, c0, c1)
            moved, still = ("gcd_finishes", "fermat_finishes") if fast else ("fermat_finishes", "gcd_finishes")
            assert f1[still] == f0[still], (fast, chain, f0, f1)           # the chain mode does not move the MSM finish, nor the other way round
            seen[fast, chain] = (lone, piped)
    finally:
        ctx.set_fast_inverse(False); ctx.set_chain_inverse(False)
        ctx.synchronize()
        for p in ptrs:
            ctx.dev_free(p)
    lone, piped = seen[False, False]
    assert lone == {"good": [1, 1], "bad": [1, 0]}
    assert [w[:nb] for w in piped] == [[1, 1], [1, 1], [0, 0], [1, 1], [1, 1]]          # the device form answers for the folded batch: it does not search for the culprit
    assert [w[nb:] for w in piped][:2] == [[1, 0, 1, 0]] * 2                               # flags: folded opening ok, nothing malformed, folded accumulator ok
    for mode in MODES[1:]:
        assert seen[mode] == seen[False, False], mode


# ------------------------------------------------------------------------------------------------ the counters and the arguments
def test_stats_follow_the_mode_and_bad_arguments_are_refused(minted):
    import ctypes
    import mina_bridge_amd as m
    c = _job_ctx(m)
    try:
        assert c.chain_inverse_stats() == {"gcd_launches": 0, "fermat_launches": 0}
        c.state_jobs_prepare(SHAPE["log2_domain"], SHAPE["npub"])
        assert c.chain_inverse_stats() == {"gcd_launches": 0, "fermat_launches": 2}           # the basis and its digit table
        assert c.state_job_batch(_build(m, minted[0])).tolist() == [1, 1]
        s = c.chain_inverse_stats()
        assert s["gcd_launches"] == 0 and s["fermat_launches"] == 3, s                         # the job's one covered launch: pubcomm_finish16
        c.set_chain_inverse(True)
        assert c.state_job_batch(_build(m, minted[0])).tolist() == [1, 1]
        assert c.chain_inverse_stats() == {"gcd_launches": 1, "fermat_launches": 3}
        assert c.inverse_stats()["gcd_finishes"] == 0                                        # the MSM finish has a mode of its own
        for bad in (2, -1, 256):
            assert c._lib.mina_ctx_set_chain_inverse(c._h, ctypes.c_int(bad)) == MINA_ERR_ARG
        assert c.state_job_batch(_build(m, minted[0])).tolist() == [1, 1]
        assert c.chain_inverse_stats() == {"gcd_launches": 2, "fermat_launches": 3}           # a refused argument leaves the mode where it was
        n = ctypes.c_uint64(0)
        assert c._lib.mina_ctx_chain_inverse_stats(c._h, None, ctypes.byref(n)) == MINA_ERR_ARG
        assert c._lib.mina_ctx_chain_inverse_stats(c._h, ctypes.byref(n), None) == MINA_ERR_ARG
        assert c._lib.mina_ctx_chain_inverse_stats(None, ctypes.byref(n), ctypes.byref(n)) == MINA_ERR_ARG
        assert c._lib.mina_ctx_set_chain_inverse(None, ctypes.c_int(1)) == MINA_ERR_ARG
        c.set_chain_inverse(False)
        assert c.state_job_batch(_build(m, minted[0])).tolist() == [1, 1]
        assert c.chain_inverse_stats() == {"gcd_launches": 2, "fermat_launches": 4}
    finally:
        c.close()
