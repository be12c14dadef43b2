"""The grouped culprit search of a failed Proof-of-State job (mina_ctx_set_search_groups) and the per-proof verdicts of a device-resident job
(mina_state_job_each_dev), on small oracle-minted jobs (k = 3 opening, 2^4 accumulator): for every batch size, group count and culprit set the verdicts equal
those of the fan search AND the known tamper set, and the counters of mina_ctx_search_stats equal a simulation of the splitting rule -- they depend on
(batch, groups, culprits) alone."""
import copy
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPE = dict(k=3, log2_domain=3, npub=4, n_comms=4, slot=2, n_points=2, acc_k=4)
MINA_ERR_ARG = -1
Q = 0x40000000000000000000000000000000224698FC0994A8DD8C46EB2100000001      # z1, z2 live in the scalar field of Pallas


@pytest.fixture(scope="module")
def small_srs(oracle):
    return {c: oracle.srs_create(c, 1024, threads=4) for c in (0, 1)}


@pytest.fixture(scope="module")
def minted(small_srs):
    from state_job_helpers import mint_job
    return [mint_job(small_srs[0], small_srs[1], 300 + 10 * i, **SHAPE) for i in range(4)]


@pytest.fixture(scope="module")
def gctx():
    """a context of its own: the group count and the counters are context state"""
    import mina_bridge_amd as m
    c = m.MinaContext(0)
    for f in (0, 1):
        c.poseidon_set_params(f, m.poseidon_params.default_params_bytes(f))
    c.srs_create(0, 1 << 10); c.srs_create(1, 1 << 10)
    c.state_jobs_prepare(SHAPE["log2_domain"], SHAPE["npub"])
    yield c
    c.close()


def batch_of(minted, B):
    return [copy.copy(minted[i % len(minted)]) for i in range(B)]      # shallow: a tamper below replaces the entry it changes


def bad_opening(job):
    job["abi"] = dict(job["abi"]); z = np.array(job["abi"]["z1"], np.uint8).copy(); z[0] ^= 1; job["abi"]["z1"] = z


def bad_accumulator(job, other):
    job["acc_sg"] = other["acc_sg"].copy()                              # another proof's commitment: a valid point, the wrong one


def bad_state(job):
    job["expected"] = list(job["expected"]); job["expected"][16] ^= 1


def malformed_acc_sg(job):
    sg = np.array(job["acc_sg"], np.uint8).copy(); sg[32] ^= 1; job["acc_sg"] = sg      # off the curve


def malformed_opening_point(job):
    job["abi"] = dict(job["abi"]); d = np.array(job["abi"]["delta"], np.uint8).copy(); d[0] ^= 1; job["abi"]["delta"] = d


def first_level_parts(B, G):
    g = min(G, B)
    return [(B * q // g, B * (q + 1) // g) for q in range(g)]


def two_in_one_part(B, G):
    """two proofs of the first first-level part that holds two (B = 5 in groups of 8 has none: every part is one proof -- then the last two proofs)"""
    for a, e in first_level_parts(B, G):
        if e - a >= 2:
            return {a, a + 1}
    return {B - 2, B - 1}


def first_boundary(B, G):
    """the last proof of first-level part 0 and the first proof of part 1"""
    g = min(G, B)
    e = B * 1 // g
    return e - 1, e


def make_case(name, minted, B, G):
    """-> (jobs, bad proofs, culprits of the opening leg searched in groups or None, culprits of the accumulator leg or None)"""
    jobs = batch_of(minted, B)
    other = lambda b: minted[(b + 1) % len(minted)]
    if name == "none":
        return jobs, set(), None, None
    if name in ("first", "last", "boundary", "same_part", "every"):
        lo, hi = first_boundary(B, G)
        bad = {"first": {0}, "last": {B - 1}, "boundary": {lo, hi}, "same_part": two_in_one_part(B, G), "every": set(range(B))}[name]
        for b in bad:
            bad_opening(jobs[b])
        return jobs, bad, bad, None
    if name == "opening_and_accumulator":
        bad_opening(jobs[1]); bad_accumulator(jobs[B - 2], other(B - 2))
        return jobs, {1, B - 2}, {1}, {B - 2}
    if name == "state_only":
        bad_state(jobs[2])
        return jobs, {2}, None, None
    if name == "malformed_acc_sg":
        malformed_acc_sg(jobs[3])
        return jobs, {3}, None, {3}
    if name == "malformed_opening_point":                               # that leg cannot use the rows: the fan search, no grouped search counted
        malformed_opening_point(jobs[B - 1])
        return jobs, {B - 1}, None, None
    raise KeyError(name)


def simulate(B, G, culprits):
    """rounds and parts of one leg's grouped search: the splitting rule of include/mina_verify.h"""
    failing, rounds, parts = [(0, B)], 0, 0
    while failing:
        level = []
        for lo, cnt in failing:
            if cnt == 1:
                continue
            g = min(G, cnt)
            level += [(lo + cnt * q // g, lo + cnt * (q + 1) // g) for q in range(g)]
        if not level:
            break
        rounds += 1; parts += len(level)
        failing = [(a, e - a) for a, e in level if any(a <= c < e for c in culprits)]
    return rounds, parts


def run(ctx, jobs, groups, **kw):
    import mina_bridge_amd as m
    from state_job_helpers import build_jobs
    ctx.set_search_groups(groups)
    try:
        before = ctx.search_stats()
        v = ctx.state_job_batch(build_jobs(m, jobs, SHAPE["k"], SHAPE["log2_domain"], SHAPE["slot"], SHAPE["acc_k"], **kw)).tolist()
        after = ctx.search_stats()
    finally:
        ctx.set_search_groups(0)
    return v, {k: after[k] - before[k] for k in after}


CASES = ["none", "first", "last", "boundary", "same_part", "every", "opening_and_accumulator", "state_only", "malformed_acc_sg", "malformed_opening_point"]
_fan = {}


@pytest.mark.parametrize("G", [2, 4, 8])
@pytest.mark.parametrize("B", [5, 9, 70])
@pytest.mark.parametrize("case", CASES)
def test_grouped_search_equals_the_fan_search_and_the_tamper_set(gctx, minted, case, B, G):
    jobs, bad, ipa_culprits, acc_culprits = make_case(case, minted, B, G)
    expect = [0 if b in bad else 1 for b in range(B)]
    key = (case, B, tuple(sorted(bad)))
    if key not in _fan:                                                 # the fan search's answer: once per input
        _fan[key] = run(gctx, jobs, 0)
    fan_v, fan_stats = _fan[key]
    assert fan_v == expect and fan_stats == {"searches": 0, "rounds": 0, "parts": 0}, (case, B)
    v, stats = run(gctx, jobs, G)
    sims = [simulate(B, G, c) for c in (ipa_culprits, acc_culprits) if c is not None]
    want = {"searches": len(sims), "rounds": sum(s[0] for s in sims), "parts": sum(s[1] for s in sims)}
    print(case, B, G, stats)
    assert v == expect, (case, B, G)
    assert stats == want, (case, B, G, stats, want)


def test_a_clean_job_after_a_grouped_search_and_the_setter(gctx, minted):
    """a failed job searched in groups leaves the context as it was: the next clean job gives its verdicts, on one lane and with a pipeline of four; the setter
    takes 0 and 2 .. 128 only"""
    import mina_bridge_amd as m
    lib = m.load_library()
    B = 9
    jobs = batch_of(minted, B); bad_opening(jobs[4]); bad_accumulator(jobs[7], minted[0])
    for lanes in (1, 4):
        gctx.set_pipeline(lanes)
        try:
            assert run(gctx, jobs, 8)[0] == [0 if b in (4, 7) else 1 for b in range(B)]
            assert run(gctx, batch_of(minted, B), 8) == ([1] * B, {"searches": 0, "rounds": 0, "parts": 0})
            assert run(gctx, batch_of(minted, B), 0)[0] == [1] * B
        finally:
            gctx.set_pipeline(1)
    for g in (1, 129, 1 << 20):
        assert lib.mina_ctx_set_search_groups(gctx._h, ctypes.c_uint32(g)) == MINA_ERR_ARG
    assert lib.mina_ctx_set_search_groups(None, ctypes.c_uint32(4)) == MINA_ERR_ARG
    z = ctypes.c_uint64(0)
    assert lib.mina_ctx_search_stats(gctx._h, None, ctypes.byref(z), ctypes.byref(z)) == MINA_ERR_ARG
    for g in (2, 128, 0):
        gctx.set_search_groups(g)


def fresh_context():
    import mina_bridge_amd as m
    c = m.MinaContext(0)
    for f in (0, 1):
        c.poseidon_set_params(f, m.poseidon_params.default_params_bytes(f))
    c.srs_create(0, 1 << 10); c.srs_create(1, 1 << 10)
    c.state_jobs_prepare(SHAPE["log2_domain"], SHAPE["npub"])
    return c


def test_a_grouped_search_creates_no_stream_and_uses_no_other_lane(minted):
    """On a context that has only ever held lane 0's stream, a job of more than 1024 proofs (no forked legs: everything on lane 0) with one bad opening and one bad
    accumulator: searched in groups, the lanes hold exactly the streams they held before and no search has created one; the SAME job searched over the fan shows
    that the probe sees a stream when one is made (three per searched leg, for lanes 1 .. 3).  Then with a pipeline of four: every lane's stream is the one it was."""
    B = 1030
    jobs = batch_of(minted, B); bad_opening(jobs[517]); bad_accumulator(jobs[1029], minted[0])
    want = [0 if b in (517, 1029) else 1 for b in range(B)]
    c = fresh_context()
    try:
        assert c.lane_streams() == {"live": 1, "made_by_searches": 0}
        assert run(c, batch_of(minted, B), 64)[0] == [1] * B               # a clean job first: whatever a job itself sets up on its lane (the opening check's side stream) exists
        base = c.lane_streams()
        assert base["made_by_searches"] == 0 and base["live"] <= 2
        v, stats = run(c, jobs, 64)
        assert v == want and stats["searches"] == 2
        assert c.lane_streams() == base, "the grouped search made or left a stream"
        v, stats = run(c, jobs, 0)
        assert v == want and stats["searches"] == 0
        after_fan = c.lane_streams()
        assert after_fan["made_by_searches"] == 6, "the fan search of each of the two legs creates (and destroys) the streams of lanes 1 .. 3: the probe must see them"
        assert after_fan["live"] == base["live"]
        c.set_pipeline(4)
        handles = []
        for lane in range(4):
            c.pin_lane(lane); handles.append(c.stream)
        c.pin_lane(-1)
        live = c.lane_streams()
        assert run(c, jobs, 64)[0] == want
        assert c.lane_streams() == live
        for lane in range(4):
            c.pin_lane(lane); assert c.stream == handles[lane], lane
        c.pin_lane(-1)
        assert run(c, batch_of(minted, 9), 64)[0] == [1] * 9
    finally:
        c.close()


def test_a_round_of_more_parts_than_one_pass_holds(gctx, minted):
    """300 proofs in groups of 128, every opening and every accumulator commitment bad: the second round has 300 parts of one proof, more than the 128 one pass
    holds -- three passes queued back to back with their own table slices and flag words -- on both legs.  Every proof is named, and the counters are the simulation's."""
    B, G = 300, 128
    jobs = batch_of(minted, B)
    for b in range(B):
        bad_opening(jobs[b]); bad_accumulator(jobs[b], minted[(b + 1) % len(minted)])
    v, stats = run(gctx, jobs, G)
    r, p = simulate(B, G, set(range(B)))
    assert p > 128 + 128 and r == 2
    assert v == [0] * B
    assert stats == {"searches": 2, "rounds": 2 * r, "parts": 2 * p}, stats
    # a few culprits among 300 in groups of 2: deep, narrow rounds beside the wide ones above
    jobs = batch_of(minted, B)
    for b in (0, 149, 150, 299):
        bad_opening(jobs[b])
    v, stats = run(gctx, jobs, 2)
    assert v == [0 if b in (0, 149, 150, 299) else 1 for b in range(B)]
    assert (stats["rounds"], stats["parts"]) == simulate(B, 2, {0, 149, 150, 299})


def test_cancelling_pair_gets_the_same_verdicts_in_groups(gctx, minted):
    """tests/test_soundness.py's pair on this file's small openings: z2_0 + rho_1 t, z2_1 - rho_0 t with rho_b = rand_base^b cancels in the fold under the
    randomiser it was built for (both ride through, the caller's contract) and fails under any other, where the search names exactly the two -- in groups as over the fan"""
    B, rb, t = 6, 7, 0x1234567890ABCDEF1234567890ABCDEF
    jobs = batch_of(minted, B)
    for b, delta in ((0, rb * t), (1, -t)):
        jobs[b]["abi"] = dict(jobs[b]["abi"])
        z2 = int.from_bytes(bytes(np.array(jobs[b]["abi"]["z2"], np.uint8)), "little")
        jobs[b]["abi"]["z2"] = np.frombuffer(((z2 + delta) % Q).to_bytes(32, "little"), np.uint8).copy()
    for groups in (0, 2, 8):
        assert run(gctx, jobs, groups, rand_base=rb)[0] == [1] * B, groups
        assert run(gctx, jobs, groups, rand_base=0x55AA55AA1234567)[0] == [0, 0] + [1] * (B - 2), groups


def test_each_dev_equals_the_host_buffer_form(gctx, minted):
    """mina_state_job_each_dev: the same verdicts as mina_state_job_batch from inputs already in HBM, with the fan search and in groups of 8; the flag words are those
    of the whole job; null and misaligned arguments are refused"""
    import mina_bridge_amd as m
    from state_job_helpers import build_jobs
    lib = m.load_library()
    B = 9
    variants = {"good": batch_of(minted, B)}
    j = batch_of(minted, B); bad_opening(j[8]); bad_state(j[0]); variants["opening_and_state"] = j
    j = batch_of(minted, B); bad_accumulator(j[3], minted[0]); malformed_acc_sg(j[4]); variants["accumulator"] = j
    j = batch_of(minted, B); malformed_opening_point(j[2]); variants["malformed_opening"] = j
    flags = {"good": [1, 0, 1, 0], "opening_and_state": [0, 0, 1, 0], "accumulator": [1, 0, 0, 0]}
    for name, jobs in variants.items():
        sj = build_jobs(m, jobs, SHAPE["k"], SHAPE["log2_domain"], SHAPE["slot"], SHAPE["acc_k"])
        host = gctx.state_job_batch(sj).tolist()
        d, ptrs = gctx.state_jobs_to_device(sj)
        out = gctx.dev_malloc(4 * B + 16)
        try:
            for groups in (0, 8):
                gctx.set_search_groups(groups)
                gctx.dev_upload(out, np.full(4 * B + 16, 0xEE, np.uint8))
                gctx.state_job_each_dev(d, out, out + 4 * B)
                w = gctx.dev_download(out, 4 * B + 16).view(np.uint32)      # no synchronize: the call has waited for its lane
                assert w[:B].tolist() == host, (name, groups)
                if name in flags:
                    assert w[B:].tolist() == flags[name], (name, groups)
                gctx.state_job_each_dev(d, out)                             # flags are optional
                assert gctx.dev_download(out, 4 * B).view(np.uint32).tolist() == host
            if name == "good":
                h = gctx._h
                assert lib.mina_state_job_each_dev(None, ctypes.byref(d), ctypes.c_void_p(out), None) == MINA_ERR_ARG
                assert lib.mina_state_job_each_dev(h, None, ctypes.c_void_p(out), None) == MINA_ERR_ARG
                assert lib.mina_state_job_each_dev(h, ctypes.byref(d), None, None) == MINA_ERR_ARG
                assert lib.mina_state_job_each_dev(h, ctypes.byref(d), ctypes.c_void_p(out + 2), None) == MINA_ERR_ARG
                assert lib.mina_state_job_each_dev(h, ctypes.byref(d), ctypes.c_void_p(out), ctypes.c_void_p(out + 4 * B + 1)) == MINA_ERR_ARG
        finally:
            gctx.set_search_groups(0)
            gctx.synchronize()
            for p in ptrs + [out]:
                gctx.dev_free(p)


# ------------------------------------------------------------------------------------------------ the boundary
def test_boundary_searches_in_groups_with_the_same_verdicts_and_masks(oracle):
    """MINA_VERIFY_GROUPED_SEARCH, alone and with MINA_VERIFY_PACK_ON_DEVICE | MINA_VERIFY_DEDUP_STATES: one call of 20 full-size proofs (the committed k = 15
    statements) with two tampered openings gives the verdict bytes and the mina_verify_state_checks masks it gives without the flag, and the device's context
    counts a grouped search where the flag is set and none where it is not"""
    import random

    import mina_bridge_amd as m
    import state_pack_helpers as H
    from ipa_helpers import poseidon_pp
    from kimchi_helpers import install_index, install_step_index, load_k15_fixture, load_statement_fixture, make_chain, make_step_index
    from oracle import mina_state_ref as S
    from wire_writers import state_pub_bytes, wrap_proof_bytes
    ix, _, _ = load_k15_fixture()
    items, _ = load_statement_fixture()
    proof_bytes = lambda wrap, states: wrap_proof_bytes(wrap, binprot=False) + b"".join(H.bincode_state(s) for s in states)
    cases = []
    for it in items[:3]:
        states, hashes = make_chain(random.Random(it["chain_seed"]), poseidon_pp(0))
        p, ev = it["proof"], it["proof"]["evals"]
        wrap = dict(it["wrap"])
        wrap.update(w_comm=p["w_comm"], z_comm=p["z_comm"], t_comm=p["t_comm"], z_eval=ev[0], selector_eval=ev[1:7], w_eval=ev[7:22], coefficients_eval=ev[22:37],
                    s_eval=ev[37:43], ft_eval1=p["ft_eval1"], lr=p["opening"]["lr"], z1=p["opening"]["z1"], z2=p["opening"]["z2"], delta=p["opening"]["delta"], sg=p["opening"]["sg"])
        bad = dict(wrap); bad["z2"] = (wrap["z2"] + 1) % (1 << 254)           # as tests/test_verify_boundary.py tampers an opening
        pub = state_pub_bytes(True, hashes[16], hashes[:16], [S.snarked_ledger_hash(s) for s in states[:16]])
        cases.append(dict(good=proof_bytes(wrap, states), bad=proof_bytes(bad, states), pub=pub))
    n, culprits = 20, (6, 13)
    proofs = [cases[i % 3]["bad" if i in culprits else "good"] for i in range(n)]
    pubs = [cases[i % 3]["pub"] for i in range(n)]
    want = [0 if i in culprits else 1 for i in range(n)]
    probes = {"good": (cases[0]["good"], cases[0]["pub"]), "bad opening": (cases[1]["bad"], cases[1]["pub"])}
    base = m.lib.VERIFY_ALLOW_SURROGATE
    both = m.lib.VERIFY_PACK_ON_DEVICE | m.lib.VERIFY_DEDUP_STATES
    assert m.lib.VERIFY_GROUPED_SEARCH == 64 and m.lib.VERIFY_GROUPED_SEARCH & (base | both | m.lib.VERIFY_ACCOUNT_ON_DEVICE | m.lib.VERIFY_ALLOW_MISSING_KIMCHI | m.lib.VERIFY_ALLOW_UNBOUND_STATEMENT) == 0
    modes = (base, base | m.lib.VERIFY_GROUPED_SEARCH, base | both, base | both | m.lib.VERIFY_GROUPED_SEARCH)
    got, masks, stats = {}, {}, {}
    try:
        for flags in modes:
            m.lib.verify_shutdown()
            m.lib.verify_configure(flags)
            gctx = m.lib.verify_global_ctx()
            install_index(gctx, ix)
            install_step_index(gctx, make_step_index(99))
            with m.lib.tuning(merge=0):                                            # one call of its own: one chunk of 20
                got[flags] = m.lib.verify_state_batch(proofs, pubs).tolist()
            stats[flags] = gctx.search_stats()
            masks[flags] = {name: tuple(m.lib.verify_state_checks(pr, pu)) for name, (pr, pu) in probes.items()}
            print(flags, stats[flags], masks[flags])
    finally:
        m.lib.verify_configure(0)
        m.lib.verify_shutdown()
    for flags in modes:
        assert got[flags] == want, (flags, got[flags])
        assert masks[flags] == masks[base], flags
        if flags & m.lib.VERIFY_GROUPED_SEARCH:                                    # one leg (the opening) searched in groups of 64: 20 parts of one proof, one round
            assert stats[flags] == {"searches": 1, "rounds": 1, "parts": 20}, (flags, stats[flags])
        else:
            assert stats[flags] == {"searches": 0, "rounds": 0, "parts": 0}, (flags, stats[flags])
    assert masks[base]["good"][0] & m.lib.CHECK_KIMCHI and not masks[base]["bad opening"][0] & m.lib.CHECK_KIMCHI
