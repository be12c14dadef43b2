"""The masks form of the Proof-of-State job (mina_state_job_checks / _checks_dev, mina_verify_state_checks_batch): `passed` / `ran` MINA_CHECK_* masks for every
proof of a batch from ONE pass of the job.  The checker for bit X of proof b is the EXISTING job on that one proof with only leg X switched on
(mina_state_job_batch), never the code under test; the rule that composes the bits is the restatement of tests/test_state_masks_model.py.  Small oracle-minted jobs
at the shape of tests/test_grouped_search_gpu.py (k = 3 opening, 2^4 accumulator, 4 public inputs, a 1024-point SRS); the boundary on the committed k = 15 statements."""
import copy
import ctypes

import numpy as np
import pytest

from test_grouped_search_gpu import (SHAPE, bad_accumulator, bad_opening, bad_state, batch_of, first_boundary, fresh_context, malformed_acc_sg, malformed_opening_point,
                                     minted, simulate, small_srs)  # noqa: F401  (small_srs, minted: module-scoped fixtures, minted once for this file)
from test_state_masks_model import ACCUMULATOR, CHAIN, CONSENSUS, FORMAT, KIMCHI, LEDGER, masks_rule

pytestmark = pytest.mark.gpu
MINA_ERR_ARG = -1
LEGS = {CHAIN: dict(with_states=True, with_ipa=False, with_acc=False), ACCUMULATOR: dict(with_states=False, with_ipa=False, with_acc=True),
        KIMCHI: dict(with_states=False, with_ipa=True, with_acc=False)}


@pytest.fixture(scope="module")
def cctx():
    """a context of its own: the group count, the pipeline and the counters are context state"""
    c = fresh_context()
    yield c
    c.close()


def build(jobs, **kw):
    import mina_bridge_amd as m
    from state_job_helpers import build_jobs
    return build_jobs(m, jobs, SHAPE["k"], SHAPE["log2_domain"], SHAPE["slot"], SHAPE["acc_k"], **kw)


def tagged_batch(minted, B):
    jobs = batch_of(minted, B)
    for i, j in enumerate(jobs):
        j["tag"] = (i % len(minted),)                                   # what the proof is: the checker's answers are kept per tag
    return jobs


def tamper(job, fn, *args, tag=None):
    fn(job, *args)
    job["tag"] = job["tag"] + (tag or fn.__name__,)


_single = {}


def leg_bits(ctx, job):
    """{CHAIN, ACCUMULATOR, KIMCHI} -> 0 / 1: the existing job on this ONE proof with only that leg switched on"""
    if job["tag"] not in _single:
        _single[job["tag"]] = {bit: int(ctx.state_job_batch(build([job], **kw))[0]) for bit, kw in LEGS.items()}
    return _single[job["tag"]]


def want_masks(ctx, jobs, front=None, deny=None, sections=(True, True, True)):
    out = []
    for b, job in enumerate(jobs):
        bits = leg_bits(ctx, job)
        out.append(masks_rule(None if front is None else int(front[b]), 0 if deny is None else int(deny[b]), sections[0], sections[1], sections[2],
                              bits[CHAIN], 1, bits[KIMCHI], bits[ACCUMULATOR]))      # (no Pickles statement in these jobs: stmt = 1)
    return [p for p, _ in out], [r for _, r in out]


def make_case(name, minted, B, G):
    """-> (jobs, culprits of the opening leg where it can be searched in groups or None, culprits of the accumulator leg or None)"""
    jobs = tagged_batch(minted, B)
    other = lambda b: (b + 1) % len(minted)
    acc = lambda b: tamper(jobs[b], bad_accumulator, minted[other(b)], tag=("bad_accumulator", other(b)))
    if name == "clean":
        return jobs, None, None
    if name in ("first", "last", "boundary", "every"):
        bad = {"first": {0}, "last": {B - 1}, "boundary": set(first_boundary(B, G or 4)), "every": set(range(B))}[name]
        for b in bad:
            tamper(jobs[b], bad_opening)
        return jobs, bad, None
    if name == "acc_wrong_point":
        acc(min(3, B - 1))
        return jobs, None, {min(3, B - 1)}
    if name == "acc_off_curve":
        tamper(jobs[min(3, B - 1)], malformed_acc_sg)
        return jobs, None, {min(3, B - 1)}
    if name == "malformed_opening_point":                               # that leg cannot use the rows: the fan search, no grouped search counted
        tamper(jobs[B - 1], malformed_opening_point)
        return jobs, None, None
    if name == "state_only":
        tamper(jobs[min(2, B - 1)], bad_state)
        return jobs, None, None
    if name == "three_bits_of_one_proof":                               # a bad opening AND a bad state AND a bad accumulator: three bits down, the others up
        t = B // 2
        tamper(jobs[t], bad_opening); tamper(jobs[t], bad_state); acc(t)
        return jobs, {t}, {t}
    if name == "opening_and_accumulator":
        tamper(jobs[1], bad_opening); acc(B - 2)
        return jobs, {1}, {B - 2}
    raise KeyError(name)


CASES = ["clean", "first", "last", "boundary", "every", "acc_wrong_point", "acc_off_curve", "malformed_opening_point", "state_only", "three_bits_of_one_proof",
         "opening_and_accumulator"]
PARAMS = [(case, B) for B in (1, 5, 9, 70) for case in CASES if B >= {"boundary": 2, "opening_and_accumulator": 4}.get(case, 1)]
ALL_RAN = FORMAT | CHAIN | ACCUMULATOR | KIMCHI


def want_search_stats(B, G, ipa_culprits, acc_culprits):
    if G < 2:
        return {"searches": 0, "rounds": 0, "parts": 0}
    sims = [simulate(B, G, c) for c in (ipa_culprits, acc_culprits if B > 1 else None) if c is not None]      # one accumulator has no randomiser: the fan search
    return {"searches": len(sims), "rounds": sum(s[0] for s in sims), "parts": sum(s[1] for s in sims)}


_whole = {}


def whole_batch_bytes(ctx, jobs, precheck=None):
    """the existing job's verdict bytes for the whole batch (fan search), once per input"""
    key = (tuple(j["tag"] for j in jobs), None if precheck is None else tuple(precheck))
    if key not in _whole:
        j, keep = build(jobs)
        if precheck is not None:
            pre = np.array(precheck, np.uint8); keep.append(pre); j.precheck = pre.ctypes.data
        _whole[key] = ctx.state_job_batch((j, keep)).tolist()
    return _whole[key]


@pytest.mark.parametrize("lanes", [1, 4])
@pytest.mark.parametrize("G", [0, 8])
@pytest.mark.parametrize("case,B", PARAMS)
def test_masks_equal_the_existing_job_one_leg_and_one_proof_at_a_time(cctx, minted, case, B, G, lanes):
    jobs, ipa_culprits, acc_culprits = make_case(case, minted, B, G)
    want_p, want_r = want_masks(cctx, jobs)
    whole = whole_batch_bytes(cctx, jobs)
    cctx.set_pipeline(lanes); cctx.set_search_groups(G)
    try:
        s0, c0 = cctx.search_stats(), cctx.checks_stats()
        passed, ran = cctx.state_job_checks(build(jobs))
        s1, c1 = cctx.search_stats(), cctx.checks_stats()
    finally:
        cctx.set_search_groups(0); cctx.set_pipeline(1)
    print(case, B, G, lanes, passed.tolist(), {k: s1[k] - s0[k] for k in s1})
    assert ran.tolist() == want_r == [ALL_RAN] * B, (case, B, G, lanes)
    assert passed.tolist() == want_p, (case, B, G, lanes)
    assert [int(p == r) for p, r in zip(passed, ran)] == whole, "passed == ran <=> the verdict byte of the existing job for the whole batch"
    assert (c1["jobs"] - c0["jobs"], c1["proofs"] - c0["proofs"]) == (1, B), "one full job pass per checks call, whatever fails"
    assert {k: s1[k] - s0[k] for k in s1} == want_search_stats(B, G, ipa_culprits, acc_culprits), (case, B, G)
    if case == "three_bits_of_one_proof":
        t = B // 2
        assert passed[t] == FORMAT and all(passed[b] == ALL_RAN for b in range(B) if b != t)


def test_front_and_deny_words_and_the_section_flags(cctx, minted):
    B = 9
    jobs = tagged_batch(minted, B)
    tamper(jobs[1], bad_state); tamper(jobs[7], bad_opening); tamper(jobs[8], bad_accumulator, minted[1], tag=("bad_accumulator", 1))
    every = FORMAT | LEDGER | CONSENSUS
    front = np.array([every, FORMAT, FORMAT | LEDGER, FORMAT | CONSENSUS, 0, every, every, every, every], np.uint32)
    deny = np.zeros(B, np.uint32); deny[5] = KIMCHI; deny[6] = FORMAT
    c0 = cctx.checks_stats()
    passed, ran = cctx.state_job_checks(build(jobs), front=front, deny=deny)
    want_p, want_r = want_masks(cctx, jobs, front, deny)
    assert (passed.tolist(), ran.tolist()) == (want_p, want_r)
    assert (passed[4], ran[4]) == (0, FORMAT) and (passed[6], ran[6]) == (0, FORMAT), "a proof that fails FORMAT is done"
    assert ran[5] & KIMCHI and not passed[5] & KIMCHI and passed[5] == (every | CHAIN | ACCUMULATOR), "deny takes the bit out of passed, not out of ran"
    precheck = [int(front[b] & every == every and not deny[b]) for b in range(B)]
    assert [int(p == r) for p, r in zip(passed, ran)] == whole_batch_bytes(cctx, jobs, precheck)
    # the job's own `precheck` is not read by the masks
    j, keep = build(jobs); pre = np.zeros(B, np.uint8); keep.append(pre); j.precheck = pre.ctypes.data
    p2, r2 = cctx.state_job_checks((j, keep), front=front, deny=deny)
    assert (p2.tolist(), r2.tolist()) == (want_p, want_r)
    # front absent: LEDGER and CONSENSUS are in no `ran`
    passed, ran = cctx.state_job_checks(build(jobs), deny=deny)
    assert (passed.tolist(), ran.tolist()) == want_masks(cctx, jobs, None, deny)
    assert not any(r & (LEDGER | CONSENSUS) for r in ran) and not any(p & (LEDGER | CONSENSUS) for p in passed)
    # the section flags, off one at a time: the bit leaves `ran`
    for off, bit in enumerate((CHAIN, ACCUMULATOR, KIMCHI)):
        sections = tuple(i != off for i in range(3))
        passed, ran = cctx.state_job_checks(build(jobs, with_states=sections[0], with_acc=sections[1], with_ipa=sections[2]), front=front, deny=deny)
        assert (passed.tolist(), ran.tolist()) == want_masks(cctx, jobs, front, deny, sections), bit
        assert not any(r & bit for r in ran) and all(r & (ALL_RAN & ~bit) == ALL_RAN & ~bit for b, r in enumerate(ran) if b not in (4, 6))
    c1 = cctx.checks_stats()
    assert (c1["jobs"] - c0["jobs"], c1["proofs"] - c0["proofs"]) == (6, 6 * B)
    with pytest.raises(ValueError):
        cctx.state_job_checks(build(jobs), front=front[:3])


def test_device_form_equals_the_host_form(cctx, minted):
    """mina_state_job_checks_dev: the host form's words from inputs already in HBM, on one lane and with a pipeline of four, with the fan search and in groups of 8;
    the four flag words are mina_state_job_each_dev's; null and misaligned arguments are refused before any launch; the context is left as it was"""
    import mina_bridge_amd as m
    lib = m.load_library()
    B, G = 9, 8
    every = FORMAT | LEDGER | CONSENSUS
    front = np.full(B, every, np.uint32); front[3] = FORMAT | LEDGER
    deny = np.zeros(B, np.uint32); deny[0] = KIMCHI
    for case in ("clean", "three_bits_of_one_proof", "opening_and_accumulator", "malformed_opening_point", "acc_off_curve"):
        jobs, ipa_culprits, acc_culprits = make_case(case, minted, B, G)
        sj = build(jobs)
        host = tuple(x.tolist() for x in cctx.state_job_checks(sj, front=front, deny=deny))
        assert host == want_masks(cctx, jobs, front, deny)
        d, ptrs = cctx.state_jobs_to_device(sj)
        out = cctx.dev_malloc(16 * B + 32)                              # passed | ran | front | deny | flags | flags of each_dev
        o_ran, o_front, o_deny, o_flags = out + 4 * B, out + 8 * B, out + 12 * B, out + 16 * B
        try:
            cctx.dev_upload(o_front, front.view(np.uint8)); cctx.dev_upload(o_deny, deny.view(np.uint8))
            cctx.state_job_each_dev(d, out, o_flags + 16)
            each_flags = cctx.dev_download(o_flags + 16, 16).view(np.uint32).tolist()
            for lanes in (1, 4):
                for groups in (0, G):
                    cctx.set_pipeline(lanes); cctx.set_search_groups(groups)
                    cctx.dev_upload(out, np.full(8 * B, 0xEE, np.uint8)); cctx.dev_upload(o_flags, np.full(16, 0xEE, np.uint8))
                    s0, c0 = cctx.search_stats(), cctx.checks_stats()
                    cctx.state_job_checks_dev(d, o_front, o_deny, out, o_ran, o_flags)
                    s1, c1 = cctx.search_stats(), cctx.checks_stats()
                    w = cctx.dev_download(out, 8 * B).view(np.uint32)        # no synchronize: the call has waited for its lane
                    assert (w[:B].tolist(), w[B:].tolist()) == host, (case, lanes, groups)
                    assert cctx.dev_download(o_flags, 16).view(np.uint32).tolist() == each_flags, (case, lanes, groups)
                    assert (c1["jobs"] - c0["jobs"], c1["proofs"] - c0["proofs"]) == (1, B)
                    assert {k: s1[k] - s0[k] for k in s1} == want_search_stats(B, groups, ipa_culprits, acc_culprits), (case, lanes, groups)
                    cctx.state_job_checks_dev(d, 0, 0, out, o_ran)            # front, deny and flags are optional
                    w = cctx.dev_download(out, 8 * B).view(np.uint32)
                    assert (w[:B].tolist(), w[B:].tolist()) == want_masks(cctx, jobs), (case, lanes, groups)
            if case == "clean":
                h, v, J = cctx._h, ctypes.c_void_p, ctypes.byref(d)
                c0 = cctx.checks_stats()
                assert lib.mina_state_job_checks_dev(None, J, None, None, v(out), v(o_ran), None) == MINA_ERR_ARG
                assert lib.mina_state_job_checks_dev(h, None, None, None, v(out), v(o_ran), None) == MINA_ERR_ARG
                assert lib.mina_state_job_checks_dev(h, J, None, None, None, v(o_ran), None) == MINA_ERR_ARG
                assert lib.mina_state_job_checks_dev(h, J, None, None, v(out), None, None) == MINA_ERR_ARG
                assert lib.mina_state_job_checks_dev(h, J, None, None, v(out + 2), v(o_ran), None) == MINA_ERR_ARG
                assert lib.mina_state_job_checks_dev(h, J, None, None, v(out), v(o_ran + 1), None) == MINA_ERR_ARG
                assert lib.mina_state_job_checks_dev(h, J, None, None, v(out), v(o_ran), v(o_flags + 1)) == MINA_ERR_ARG
                assert lib.mina_state_job_checks_dev(h, J, v(o_front + 2), None, v(out), v(o_ran), None) == MINA_ERR_ARG
                assert lib.mina_state_job_checks_dev(h, J, None, v(o_deny + 3), v(out), v(o_ran), None) == MINA_ERR_ARG
                z = ctypes.c_uint64(0)
                assert lib.mina_ctx_checks_stats(h, None, ctypes.byref(z)) == MINA_ERR_ARG and lib.mina_ctx_checks_stats(None, ctypes.byref(z), ctypes.byref(z)) == MINA_ERR_ARG
                assert lib.mina_state_job_checks(h, ctypes.byref(sj[0]), None, None, None, None) == MINA_ERR_ARG
                assert cctx.checks_stats() == c0, "a refused call queues nothing"
        finally:
            cctx.set_search_groups(0); cctx.set_pipeline(1)
            cctx.synchronize()
            for p in ptrs + [out]:
                cctx.dev_free(p)
    assert cctx.state_job_batch(build(tagged_batch(minted, B))).tolist() == [1] * B, "a clean job afterwards on the same context"


# ------------------------------------------------------------------------------------------------ the boundary
def boundary_pairs():
    """20 (proof, pub) pairs from the committed full-size (k = 15) statements, as tests/test_grouped_search_gpu.py builds them: -> (proofs, pubs, what each pair is)"""
    import random

    import state_pack_helpers as H
    from ipa_helpers import poseidon_pp
    from kimchi_helpers import load_statement_fixture, make_chain
    from oracle import mina_state_ref as S
    from wire_writers import state_pub_bytes, wrap_proof_bytes
    items, _ = load_statement_fixture()
    pp = poseidon_pp(0)
    proof_bytes = lambda wrap, states: wrap_proof_bytes(wrap, binprot=False) + b"".join(H.bincode_state(s) for s in states)
    base = []
    for it in items[:3]:
        states, hashes = make_chain(random.Random(it["chain_seed"]), pp)
        p, ev = it["proof"], it["proof"]["evals"]
        wrap = dict(it["wrap"])
        wrap.update(w_comm=p["w_comm"], z_comm=p["z_comm"], t_comm=p["t_comm"], z_eval=ev[0], selector_eval=ev[1:7], w_eval=ev[7:22], coefficients_eval=ev[22:37],
                    s_eval=ev[37:43], ft_eval1=p["ft_eval1"], lr=p["opening"]["lr"], z1=p["opening"]["z1"], z2=p["opening"]["z2"], delta=p["opening"]["delta"], sg=p["opening"]["sg"])
        base.append(dict(wrap=wrap, states=states, hashes=hashes, ledger=[S.snarked_ledger_hash(s) for s in states[:16]]))
    pub_of = lambda c, hashes=None, ledger=None: state_pub_bytes(True, (hashes or c["hashes"])[16], (hashes or c["hashes"])[:16], ledger or c["ledger"])
    n = 20
    proofs, pubs, what = [], [], ["clean"] * n
    for i in range(n):
        c = base[i % 3]
        proofs.append(proof_bytes(c["wrap"], c["states"])); pubs.append(pub_of(c))

    def put(i, name, wrap=None, states=None, hashes=None, ledger=None):
        c = base[i % 3]
        proofs[i] = proof_bytes(wrap or c["wrap"], states or c["states"]); pubs[i] = pub_of(c, hashes, ledger); what[i] = name
    for i in (6, 13):                                                   # as tests/test_verify_boundary.py tampers an opening
        w = dict(base[i % 3]["wrap"]); w["z2"] = (w["z2"] + 1) % (1 << 254); put(i, "bad opening", wrap=w)
    proofs[2] = proofs[2][:100]; what[2] = "truncated proof"
    pubs[4] = pubs[4][:-1]; what[4] = "public input one byte short"
    hs = list(base[8 % 3]["hashes"]); hs[5] ^= 1; put(8, "tampered state hash", hashes=hs)
    led = list(base[9 % 3]["ledger"]); led[3] ^= 1; put(9, "tampered ledger hash", ledger=led)
    c = base[11 % 3]
    st = copy.deepcopy(c["states"]); st[16]["body"]["consensus_state"]["blockchain_length"] = 5000
    hs = list(c["hashes"]); hs[16] = S.protocol_state_hash(st[16], pp); put(11, "bridge tip wins", states=st, hashes=hs)
    w = dict(base[15 % 3]["wrap"]); bc = list(w["bulletproof_challenges"]); bc[7] ^= 1; w["bulletproof_challenges"] = bc; put(15, "changed step prechallenge", wrap=w)
    # the donor trap: a proof of the wrong shape for the index (14 L/R pairs; tests/test_soundness.py) whose accumulator is bad as well
    w = copy.deepcopy(base[17 % 3]["wrap"]); w["lr"] = w["lr"][:14]; bc = list(w["bulletproof_challenges"]); bc[3] ^= 1; w["bulletproof_challenges"] = bc
    put(17, "wrong shape and bad accumulator", wrap=w)
    w = copy.deepcopy(base[18 % 3]["wrap"]); w["feature_flags"][6] = True; put(18, "lookup feature on", wrap=w)
    return proofs, pubs, what


def test_boundary_batch_equals_the_single_proof_form_pair_by_pair():
    import mina_bridge_amd as m
    from kimchi_helpers import install_index, install_step_index, load_k15_fixture, make_step_index
    L = m.lib
    ix, _, _ = load_k15_fixture()
    proofs, pubs, what = boundary_pairs()
    n = len(proofs)
    base = L.VERIFY_ALLOW_SURROGATE
    modes = (base, base | L.VERIFY_PACK_ON_DEVICE | L.VERIFY_DEDUP_STATES, base | L.VERIFY_GROUPED_SEARCH)
    ALL = FORMAT | LEDGER | CHAIN | CONSENSUS | ACCUMULATOR | KIMCHI
    try:
        for flags in modes:
            L.verify_shutdown()
            L.verify_configure(flags)
            gctx = L.verify_global_ctx()
            install_index(gctx, ix)
            install_step_index(gctx, make_step_index(99))
            single = [tuple(L.verify_state_checks(p, q)) for p, q in zip(proofs, pubs)]
            c0 = gctx.checks_stats()
            passed, ran = L.verify_state_checks_batch(proofs, pubs)
            c1 = gctx.checks_stats()
            got = list(zip(passed.tolist(), ran.tolist()))
            print(flags, [(w, hex(p), hex(r)) for w, (p, r) in zip(what, got)])
            assert got == single, (flags, [(i, what[i], got[i], single[i]) for i in range(n) if got[i] != single[i]])
            # every pair of the call has the evaluation shape of the committed statements: one group, one job; the truncated proof reaches no group
            assert (c1["jobs"] - c0["jobs"], c1["proofs"] - c0["proofs"]) == (1, n - 1), flags
            with L.tuning(merge=0):
                assert L.verify_state_batch(proofs, pubs).tolist() == [int(p == r) for p, r in got], flags
            e = L.verify_state_checks_batch([], [])
            assert len(e[0]) == 0 and len(e[1]) == 0
            if flags == base:                                           # the single-proof form itself says what each pair is: the comparison above is not vacuous
                by = dict(zip(what, single))
                assert by["clean"] == (ALL, ALL) and by["bad opening"] == (ALL & ~KIMCHI, ALL) and by["truncated proof"] == (0, FORMAT)
                assert by["public input one byte short"] == (0, FORMAT) and by["tampered state hash"] == (ALL & ~CHAIN, ALL) and by["tampered ledger hash"] == (ALL & ~LEDGER, ALL)
                assert by["bridge tip wins"] == (ALL & ~CONSENSUS, ALL) and by["changed step prechallenge"] == (ALL & ~ACCUMULATOR & ~KIMCHI, ALL)
                assert by["wrong shape and bad accumulator"] == (ALL & ~ACCUMULATOR & ~KIMCHI, ALL) and by["lookup feature on"] == (ALL & ~KIMCHI, ALL)
                # nothing of the call parses: answered from the host bits alone, without a job
                c0 = gctx.checks_stats()
                p0, r0 = L.verify_state_checks_batch([proofs[2], b""], [pubs[2], pubs[0]])
                assert (p0.tolist(), r0.tolist()) == ([0, 0], [FORMAT, FORMAT]) and gctx.checks_stats() == c0
        # once more without an installed verifier index: KIMCHI is in no `ran`
        L.verify_shutdown()
        L.verify_configure(base)
        single =[tuple(L.verify_state_checks(p, q)) for p, q in zip(proofs, pubs)]
        passed, ran = L.verify_state_checks_batch(proofs, pubs)
        assert list(zip(passed.tolist(), ran.tolist())) == single
        assert not any(r & KIMCHI for r in ran) and ran[0] == ALL & ~KIMCHI and passed[0] == ALL & ~KIMCHI
    finally:
        L.verify_configure(0)
        L.verify_shutdown()
