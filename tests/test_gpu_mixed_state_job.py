"""A Proof-of-State job over proofs of BOTH index sets of one context: mina_state_job_batch_net_dev and mina_state_job_each_net_dev (ctx.h StateJobPlan::d_net;
the `_net` forms of the Pickles statement and kimchi stages, an opening check whose only batch-shared point is h, one fold, one fixed-base MSM, one accumulator
check for the proofs of both sets).

Six full cases -- 17 protocol states, the Pickles statement, the wrap proof with its opening, the step accumulator -- of pair A (set 0, four proofs) and pair B
(set 1, two proofs), interleaved (tests/network_helpers.py; the oracle rejects every proof under the other pair).  The checker is the existing single-set code:
mina_state_job_each_dev on the proofs of one set, with that set selected."""
import random

import numpy as np
import pytest

from network_helpers import load_pairs

pytestmark = pytest.mark.gpu

SIX = (("A", 0), ("B", 0), ("A", 1), ("A", 2), ("B", 1), ("A", 3))
SIX_NET = [0, 1, 0, 0, 1, 0]


def fresh_ctx(m):
    c = m.MinaContext(0)
    for field in (0, 1):
        c.poseidon_set_params(field, m.poseidon_params.default_params_bytes(field))
    for curve in (0, 1):
        c.srs_create(curve, 65536)
    return c


def full_case(m, it):
    """one fixture item -> its sections in the C-ABI's layouts (as tests/golden/encode_statement_fixture.py lays them out) + its chain of 17 states"""
    import state_pack_helpers as H
    from ipa_helpers import poseidon_pp
    from kimchi_helpers import kimchi_arrays, make_chain, statements_soa
    from oracle import oracle as O
    states, hashes = make_chain(random.Random(it["chain_seed"]), poseidon_pp(0))
    assert hashes[15] == it["app"]
    packed = [m.lib.protocol_state_pack(H.bincode_state(s), m.lib.ENC_BINCODE) for s in states]
    n_old, n_evals, sec = statements_soa([it["wrap"]], [it["app"]])
    arrays, op = kimchi_arrays([it["proof"]], [])
    arrays.pop("prev_chals")                                     # the recursion challenges are the statement's
    u8 = lambda a: np.ascontiguousarray(a, dtype=np.uint8).reshape(-1)
    return {"n_old": n_old, "n_evals": n_evals, "statement": {k: u8(v) for k, v in sec.items()}, "kimchi": {k: u8(v) for k, v in arrays.items() if v is not None},
            "opening": {k: u8(v) for k, v in op.items()}, "acc_prechallenges": u8(it["acc_pre"]), "acc_sg": u8(it["acc_sg"]),
            "state_records": np.concatenate([u8(p[0]) for p in packed]), "state_nfields": np.concatenate([np.asarray(p[1], np.uint32).reshape(-1) for p in packed]),
            "expected_hashes": u8(O.ints_to_le(hashes))}


def build_job(m, cases, seed=5):
    """host-side job; its statement sections go to HBM apart (DevJob): MinaContext.state_jobs_to_device uploads the job's and the kimchi section's arrays"""
    B = len(cases)
    cat = lambda f: np.concatenate([f(c) for c in cases])
    kp = m.MinaContext.make_kimchi_proofs(B, 2, 40, {k: cat(lambda c: c["kimchi"][k]) for k in cases[0]["kimchi"]})
    rng = np.random.Generator(np.random.PCG64(seed))
    rnd = lambda n: np.concatenate([rng.integers(0, 256, size=(n, 31), dtype=np.uint8), np.zeros((n, 1), np.uint8)], axis=1).reshape(-1)      # < 2^248: canonical
    arrays = dict(state_records=cat(lambda c: c["state_records"]), state_nfields=cat(lambda c: c["state_nfields"]), expected_hashes=cat(lambda c: c["expected_hashes"]),
                  rand_base=rnd(1), sg_rand_base=rnd(1), acc_prechallenges=cat(lambda c: c["acc_prechallenges"]), acc_sg=cat(lambda c: c["acc_sg"]), acc_rho=rnd(B),
                  **{k: cat(lambda c: c["opening"][k]) for k in ("lr", "delta", "sg", "z1", "z2")})
    jobs = m.MinaContext.make_state_jobs(B, arrays, with_states=1, with_ipa=1, with_accumulator=1, log2_domain=15, npub=40, k=15, n_evalpoints=2, n_comms=47, acc_k=16, kimchi=kp)
    return jobs, (cases[0]["n_old"], cases[0]["n_evals"], {k: cat(lambda c: c["statement"][k]) for k in cases[0]["statement"]})


class DevJob:
    """a job resident in HBM with its verdict / flag words and, for the mixed calls, its bytes"""
    def __init__(self, ctx, built, net=None):
        import ctypes
        jobs, (n_old, n_evals, sections) = built
        self.ctx, self.B = ctx, jobs[0].batch
        self.d, self.ptrs = ctx.state_jobs_to_device(jobs)
        self.dk = ctx._keep_dk
        at = {}
        for name, a in sections.items():                         # every statement section resident in HBM as well
            at[name] = ctx.dev_malloc(max(a.nbytes, 4)); self.ptrs.append(at[name])
            ctx.dev_upload(at[name], a)
        self.st = type(ctx).make_pickles_statements(n_old, n_evals, at)
        self.dk.statements = ctypes.addressof(self.st[0])
        self.out = ctx.dev_malloc(4 * self.B + 16); self.ptrs.append(self.out)
        self.net = 0
        if net is not None:
            self.net = ctx.dev_malloc(max(self.B, 4)); self.ptrs.append(self.net)
            ctx.dev_upload(self.net, np.asarray(net, np.uint8))

    def words(self):
        self.ctx.synchronize()
        w = self.ctx.dev_download(self.out, 4 * self.B + 16).view(np.uint32)
        return w[:self.B].tolist(), w[self.B:self.B + 4].tolist()

    def clear(self):
        self.ctx.dev_upload(self.out, np.full(4 * self.B + 16, 0xEE, np.uint8))

    def free(self):
        self.ctx.synchronize()
        for p in self.ptrs:
            self.ctx.dev_free(p)


@pytest.fixture(scope="module")
def env(oracle):
    import mina_bridge_amd as m
    from kimchi_helpers import load_statement_fixture
    from network_helpers import ALT_PATH
    A, B = load_pairs()
    pool = {"A": load_statement_fixture()[0], "B": load_statement_fixture(ALT_PATH)[0]}
    cases = [full_case(m, pool[name][i]) for name, i in SIX]
    two = fresh_ctx(m)
    try:
        two.set_pipeline(1)
        A.install(two)
        two.select_index_set(1)
        B.install(two)
        two.select_index_set(0)
        two.state_jobs_prepare(15, 40)
        yield {"m": m, "two": two, "cases": cases}
    finally:
        two.close()


def per_network(m, two, cases, net):
    """the existing calls, per network: the proofs whose byte is s through mina_state_job_each_dev with set s selected -> verdicts in the call's order"""
    out = [None] * len(cases)
    for s in (0, 1):
        at = [b for b, n in enumerate(net) if n == s]
        two.select_index_set(s)
        job = DevJob(two, build_job(m, [cases[b] for b in at]))
        try:
            two.state_job_each_dev(job.d, job.out, job.out + 4 * job.B)
            v, _ = job.words()
        finally:
            job.free()
        for b, x in zip(at, v):
            out[b] = x
    two.select_index_set(0)
    return out


def test_device_job_over_both_sets(env):
    m, two, cases = env["m"], env["two"], env["cases"]
    B = len(cases)
    assert per_network(m, two, cases, SIX_NET) == [1] * B
    s0 = two.mixed_job_stats()
    job = DevJob(two, build_job(m, cases), SIX_NET)
    try:
        for sel in (0, 1):                                       # the bytes name the sets, whichever is selected
            two.select_index_set(sel)
            job.clear()
            two.state_job_batch_net_dev(job.d, job.net, job.out, job.out + 4 * B)
            v, f = job.words()
            assert v == [1] * B and f[0] == 1 and f[1] == 0 and f[2] == 1, (sel, v, f)
            job.clear()
            two.state_job_each_net_dev(job.d, job.net, job.out, job.out + 4 * B)
            v, f = job.words()
            assert v == [1] * B and f[0] == 1 and f[2] == 1 and two.index_set() == sel, (sel, v, f)
        two.select_index_set(0)
        s1 = two.mixed_job_stats()
        assert s1["jobs"] - s0["jobs"] == 4, "one per call"
        assert (s1["proofs_set0"] - s0["proofs_set0"], s1["proofs_set1"] - s0["proofs_set1"]) == (4 * 4, 4 * 2), "the proofs of every call, by the set their byte names"
        # proof 4 (of pair B) under set 0: the folded opening fails -> the batch call answers 0 for all, the each call for proof 4 alone
        wrong = list(SIX_NET); wrong[4] = 0
        two.dev_upload(job.net, np.asarray(wrong, np.uint8))
        job.clear()
        two.state_job_batch_net_dev(job.d, job.net, job.out, job.out + 4 * B)
        v, f = job.words()
        assert v == [0] * B and f[0] == 0 and f[2] == 1, (v, f)
        job.clear()
        two.state_job_each_net_dev(job.d, job.net, job.out, job.out + 4 * B)
        v, f = job.words()
        want = [1, 1, 1, 1, 0, 1]
        assert v == want and f[0] == 0, (v, f)
        assert per_network(m, two, cases, wrong) == want, "the existing calls, per network, on the same proofs"
        s2 = two.mixed_job_stats()
        assert s2["jobs"] - s1["jobs"] == 2, "the passes a culprit search re-queues are not counted"
        assert (s2["proofs_set0"] - s1["proofs_set0"], s2["proofs_set1"] - s1["proofs_set1"]) == (2 * 5, 2 * 1), "nor their proofs a second time"
        # grouped search: the same verdicts
        two.set_search_groups(64)
        try:
            job.clear()
            two.state_job_each_net_dev(job.d, job.net, job.out, job.out + 4 * B)
            assert job.words()[0] == want
        finally:
            two.set_search_groups(0)
        # a byte of 2: that proof alone
        two.dev_upload(job.net, np.asarray([0, 1, 2, 0, 1, 0], np.uint8))
        job.clear()
        two.state_job_each_net_dev(job.d, job.net, job.out, job.out + 4 * B)
        assert job.words()[0] == [1, 1, 0, 1, 1, 1]
        s3 = two.mixed_job_stats()                               # (one grouped-search call over `wrong` in between: 5 + 1)
        assert (s3["jobs"] - s2["jobs"], s3["proofs_set0"] - s2["proofs_set0"], s3["proofs_set1"] - s2["proofs_set1"]) == (2, 5 + 3, 1 + 2), "a byte of 2 counts in neither set"
        # ... and the batch form: the kimchi stage's malformed word is one for the whole job, so every verdict is 0 and flags[1] says why (as for any malformed input)
        job.clear()
        two.state_job_batch_net_dev(job.d, job.net, job.out, job.out + 4 * B)
        v, f = job.words()
        assert v == [0] * B and f[0] == 0 and f[1] == 1, (v, f)
    finally:
        job.free()


def test_argument_and_state_errors(env):
    m, two, cases = env["m"], env["two"], env["cases"]
    job = DevJob(two, build_job(m, cases), SIX_NET)
    one = None
    try:
        s0 = two.mixed_job_stats()
        with pytest.raises(m.lib.MinaError, match=r"mina_state_job_batch_net_dev failed \(-1\)"):
            two.state_job_batch_net_dev(job.d, 0, job.out)
        with pytest.raises(m.lib.MinaError, match=r"mina_state_job_each_net_dev failed \(-1\)"):
            two.state_job_each_net_dev(job.d, 0, job.out)
        assert two.mixed_job_stats() == s0
        from network_helpers import load_pairs as _lp
        A, _ = _lp()
        one = fresh_ctx(m)
        A.install(one)
        one.state_jobs_prepare(15, 40)
        with pytest.raises(m.lib.MinaError, match=r"mina_state_job_batch_net_dev failed \(-3\)"):
            one.state_job_batch_net_dev(job.d, job.net, job.out)
        with pytest.raises(m.lib.MinaError, match=r"mina_state_job_each_net_dev failed \(-3\)"):
            one.state_job_each_net_dev(job.d, job.net, job.out)
        assert one.mixed_job_stats() == {"jobs": 0, "proofs_set0": 0, "proofs_set1": 0}
    finally:
        if one is not None:
            one.close()
        job.free()


# ------------------------------------------------------------------------------------------------ the boundary: MINA_VERIFY_MIXED_NETWORK_JOB
# Pair A serves devnet (set 1) and pair B mainnet (set 0), as in tests/test_network_indexes_gpu.py.  The reference of every comparison is the same call in the same
# process with the flag off: the sequential passes, one per network.
MAINNET, DEVNET = 0, 1


@pytest.fixture(scope="module")
def net(oracle):
    import mina_bridge_amd as m
    A, B = load_pairs()
    m.lib.verify_shutdown()
    m.lib.verify_set_network(-1)
    m.lib.verify_configure(m.lib.VERIFY_ALLOW_SURROGATE)
    yield {"m": m, "A": A, "B": B}
    m.lib.verify_drop_network_indexes()
    m.lib.verify_set_network(-1)
    m.lib.verify_shutdown()
    m.lib.verify_configure(0)


def install_both(net):
    m = net["m"]
    m.lib.verify_drop_network_indexes()
    net["A"].install(m.lib.verify_network_devices(DEVNET))
    net["B"].install(m.lib.verify_network_devices(MAINNET))
    assert m.lib.verify_networks() == (1, 1)


def interleave(x, y):
    out = []
    for i in range(max(len(x), len(y))):
        out += x[i:i + 1] + y[i:i + 1]
    return out


def issue_inputs(A, B):
    """good proofs of both networks interleaved, the tampered ones of either, an A proof under the mainnet flag, a truncated proof, an empty public input"""
    a = A.cases
    return (interleave(A.good(DEVNET), B.good(MAINNET)) + A.tampered(DEVNET) + B.tampered(MAINNET) + [(a[3]["proof"], a[3]["pub"][MAINNET])]
            + [(a[0]["proof"][:100], a[0]["pub"][DEVNET])] + [(a[1]["proof"], b"")])


def batch(m, calls):
    return m.lib.verify_state_batch([c[0] for c in calls], [c[1] for c in calls]).tolist()


def stats(m):
    return m.lib.verify_device_ctx(0).mixed_job_stats()


def delta(a, b):
    return b["jobs"] - a["jobs"], (b["proofs_set0"] - a["proofs_set0"]) + (b["proofs_set1"] - a["proofs_set1"])


def test_boundary_flag_on_equals_flag_off(net):
    m, A, B = net["m"], net["A"], net["B"]
    base = m.lib.VERIFY_ALLOW_SURROGATE
    install_both(net)
    calls = issue_inputs(A, B)
    n = len(calls)
    try:
        s0 = stats(m)
        off = batch(m, calls)
        assert delta(s0, stats(m)) == (0, 0), "without the flag no mixed job is formed"
        assert off[:6] == [1] * 6 and off[6:] == [0] * (n - 6), off
        m.lib.verify_configure(base | m.lib.VERIFY_MIXED_NETWORK_JOB)
        s1 = stats(m)
        on = batch(m, calls)
        assert on == off
        assert delta(s1, stats(m)) == (1, n), "one chunk: one mixed job over every entry of the call"
        with m.lib.tuning(chunk=8, single_max=4):                # chunks of 8 at the most: a mixed job each
            s2 = stats(m)
            assert batch(m, calls) == off
            assert n == 17 and delta(s2, stats(m)) == (3, n)
        s3 = stats(m)                                            # a call whose proofs all claim one network runs as without the flag
        assert batch(m, A.good(DEVNET)) == [1] * 4 and delta(s3, stats(m)) == (0, 0)
        # the flag with the other modes of the boundary: the same verdicts for the mixed tampered call
        for extra in (m.lib.VERIFY_PACK_ON_DEVICE | m.lib.VERIFY_DEDUP_STATES, m.lib.VERIFY_GROUPED_SEARCH):
            m.lib.verify_configure(base | m.lib.VERIFY_MIXED_NETWORK_JOB | extra)
            s4 = stats(m)
            assert batch(m, calls) == off, extra
            assert delta(s4, stats(m))[0] == 1, extra
    finally:
        m.lib.verify_configure(base)


def test_merged_callers_of_one_network_each_share_a_mixed_job(net):
    import threading
    m, A, B = net["m"], net["A"], net["B"]
    base = m.lib.VERIFY_ALLOW_SURROGATE
    install_both(net)
    calls = [A.good(DEVNET)[0], B.good(MAINNET)[0]]
    assert [m.lib.verify_state(*c) for c in calls] == [True, True]       # warm
    m.lib.verify_configure(base | m.lib.VERIFY_MIXED_NETWORK_JOB)
    try:
        merged = False
        for _ in range(5):                                       # the two calls merge when they arrive together: a few rounds at the most
            got = [None, None]
            gate = threading.Barrier(2)
            def worker(i):
                gate.wait()
                got[i] = m.lib.verify_state(*calls[i])
            s0 = stats(m)
            th = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
            for t in th: t.start()
            for t in th: t.join()
            assert got == [True, True], "each caller its own verdict"
            d = delta(s0, stats(m))
            assert d in ((0, 0), (1, 2)), d
            if d == (1, 2):
                merged = True
                break
        assert merged, "the two callers never shared a job in 5 rounds"
    finally:
        m.lib.verify_configure(base)


def test_completion_queue_burst_of_both_networks_is_one_job(net):
    m, A, B = net["m"], net["A"], net["B"]
    base = m.lib.VERIFY_ALLOW_SURROGATE
    install_both(net)
    calls = interleave(A.good(DEVNET)[:2], B.good(MAINNET)) + [A.tampered(DEVNET)[1]]
    want = [int(m.lib.verify_state(*c)) for c in calls]
    assert want == [1, 1, 1, 1, 0]
    m.lib.verify_configure(base | m.lib.VERIFY_MIXED_NETWORK_JOB)
    try:
        s0 = stats(m)
        with m.lib.VerifyQueue(capacity=16, workers=1) as q:
            for tag, (p, pub) in enumerate(calls):
                assert q.submit_state(p, pub, tag=tag, more=tag + 1 < len(calls)) == 0
            done = {}
            while len(done) < len(calls):
                got = q.wait(timeout_us=60_000_000)
                assert got, "the completion queue answered nothing within a minute"
                for tag, verdict, rc, _ in got:
                    assert rc == 0
                    done[tag] = verdict
        assert [done[i] for i in range(len(calls))] == want
        assert delta(s0, stats(m)) == (1, len(calls))
    finally:
        m.lib.verify_configure(base)


def test_ineligible_cases_change_nothing(net):
    m, A, B = net["m"], net["A"], net["B"]
    base = m.lib.VERIFY_ALLOW_SURROGATE
    calls = issue_inputs(A, B)
    try:
        # one network installed
        m.lib.verify_drop_network_indexes()
        A.install(m.lib.verify_network_devices(DEVNET))
        assert m.lib.verify_networks() == (0, 1)
        off = batch(m, calls)
        m.lib.verify_configure(base | m.lib.VERIFY_MIXED_NETWORK_JOB)
        s0 = stats(m)
        assert batch(m, calls) == off and delta(s0, stats(m)) == (0, 0)
        # outside network mode: one pair, no network declared
        m.lib.verify_configure(base)
        m.lib.verify_drop_network_indexes()
        m.lib.verify_shutdown()
        A.install(m.lib.verify_all_devices())
        off = batch(m, calls)
        assert [off[i] for i in (0, 2, 4, 5)] == [1] * 4, "the flag of a public input is not looked at: A's proofs pass"
        m.lib.verify_configure(base | m.lib.VERIFY_MIXED_NETWORK_JOB)
        s0 = stats(m)
        assert batch(m, calls) == off and delta(s0, stats(m)) == (0, 0)
    finally:
        m.lib.verify_configure(base)
        m.lib.verify_shutdown()
