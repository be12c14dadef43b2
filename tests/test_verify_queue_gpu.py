"""The completion queue of the boundary on the GPU (`mina_verify_queue_*`, include/mina_verify.h): proofs are submitted, verdicts are collected later.  The queue
feeds the jobs `mina_verify_state` / `mina_verify_account` feed, so every check here is against those calls: same verdicts for good, tampered and malformed bytes
under three flag sets; one burst = one job; back-pressure by slots; the queue owns the bytes; beside synchronous callers; `wait` and the descriptor; teardown and
shutdown; argument errors.  The world is test_verify_boundary.py's (K_LOG2 = 6, surrogate tables); proofs and account pairs are minted once per module."""
import copy
import os
import random
import select
import struct
import threading
import time

import pytest

from test_verify_boundary import K_LOG2, mint_state_proof, to_bytes, world  # noqa: F401  (`world` is the module fixture)

pytestmark = pytest.mark.gpu
assert K_LOG2 == 6
TIMEOUT_US = 120_000_000          # a bound for `wait`, never reached: a lost completion fails the test instead of hanging it


@pytest.fixture(scope="module")
def minted(world, srs_oracle):
    """state proofs: 4 good ones and one of each tamper class of test_verify_state_end_to_end on the first, all as bytes; account pairs as
    test_verify_account_end_to_end makes them, with a tampered Merkle sibling and a tampered ABI byte"""
    from ipa_helpers import poseidon_pp
    from oracle import mina_account_ref as A, mina_state_ref as S, pasta_ref as R
    items = [mint_state_proof(world, srs_oracle, 8800 + 10 * i) for i in range(4)]
    good = [to_bytes(*it) for it in items]
    wrap, states, hashes = items[0]
    bad = {}
    led = [S.snarked_ledger_hash(s) for s in states[:16]]; led[3] ^= 1
    bad["ledger"] = to_bytes(wrap, states, hashes, led)
    hs = list(hashes); hs[5] ^= 1
    bad["chain"] = to_bytes(wrap, states, hs)
    st = copy.deepcopy(states); st[16]["body"]["consensus_state"]["blockchain_length"] = 5000
    hs = list(hashes); hs[16] = S.protocol_state_hash(st[16], poseidon_pp(0))
    bad["consensus"] = to_bytes(wrap, st, hs)
    w2 = dict(wrap); bc = list(wrap["bulletproof_challenges"]); bc[7] ^= 1; w2["bulletproof_challenges"] = bc
    bad["accumulator"] = to_bytes(w2, states, hashes)
    w2 = dict(wrap); we = list(wrap["w_eval"]); we[2] = ((we[2][0] + 1) % (1 << 254), we[2][1]); w2["w_eval"] = we
    bad["kimchi evaluation"] = to_bytes(w2, states, hashes)
    w2 = dict(wrap); w2["z1"] = (wrap["z1"] + 1) % (1 << 254)
    bad["opening scalar"] = to_bytes(w2, states, hashes)
    pp = poseidon_pp(0)
    rng = random.Random(31)
    accounts = [A.synth_account(rng, zk, timed, deleg, with_vk=vk) for zk, timed, deleg, vk in
                [(False, False, False, True), (True, True, True, True), (True, False, True, False), (False, True, True, True)]]
    acct = []
    for a in accounts:
        path = [(rng.randrange(2), rng.randrange(R.P)) for _ in range(35)]
        enc = A.abi_encode_account(a)
        acct.append((A.write_account_proof(path, a), R.merkle_root(A.account_hash(a, pp), path, pp).to_bytes(32, "little") + struct.pack("<Q", len(enc)) + enc))
    p3 = bytearray(acct[2][0]); p3[8 + 12 + 3] ^= 1                               # a Merkle sibling
    q0 = bytearray(acct[0][1]); q0[40 + 32 + 5 * 32 + 31] ^= 1                    # an ABI byte (the balance word)
    return {"good": good, "bad": bad, "acct": acct, "acct_bad": {"sibling": (bytes(p3), acct[2][1]), "abi": (acct[0][0], bytes(q0))}}


def drain(q, n):
    """the next n completions, by `wait`"""
    out = []
    while len(out) < n:
        got = q.wait(TIMEOUT_US)
        assert got, "no completion within the bound"
        out += got
    return out


@pytest.mark.parametrize("extra", ["none", "pack_dedup_grouped", "account_on_device"])
def test_queue_verdicts_equal_the_synchronous_calls(world, minted, extra):
    """about 20 entries from one thread -- good proofs, every tamper class, junk, an empty proof, a proof cut by one byte, a public input of 1056 bytes; good
    account pairs, a tampered sibling, a tampered ABI byte -- every tag back exactly once, (verdict, rc) = (mina_verify_state / _account of the same bytes, MINA_OK)"""
    import mina_bridge_amd as m
    L = m.lib
    flags = {"none": 0, "pack_dedup_grouped": L.VERIFY_PACK_ON_DEVICE | L.VERIFY_DEDUP_STATES | L.VERIFY_GROUPED_SEARCH, "account_on_device": L.VERIFY_ACCOUNT_ON_DEVICE}[extra]
    g = minted["good"]
    entries = [(L.QUEUE_STATE, p, q, 1) for p, q in g[:3]]
    entries += [(L.QUEUE_STATE, p, q, 0) for p, q in minted["bad"].values()]
    entries += [(L.QUEUE_STATE, b"junk", g[0][1], 0), (L.QUEUE_STATE, b"", g[0][1], 0), (L.QUEUE_STATE, g[1][0][:-1], g[1][1], 0), (L.QUEUE_STATE, g[2][0], g[2][1][:-1], 0)]
    entries += [(L.QUEUE_ACCOUNT, p, q, 1) for p, q in minted["acct"]]
    entries += [(L.QUEUE_ACCOUNT, p, q, 0) for p, q in minted["acct_bad"].values()]
    assert len(entries) == 19 and len(g[2][1][:-1]) == 1056
    L.verify_configure(L.VERIFY_ALLOW_SURROGATE | flags)
    try:
        want = [int((L.verify_state if kind == L.QUEUE_STATE else L.verify_account)(p, q)) for kind, p, q, _ in entries]
        assert want == [e[3] for e in entries], want                                # the reference itself answers as the bytes were made
        with L.VerifyQueue(capacity=32, workers=1) as q:
            for i, (kind, p, pub, _) in enumerate(entries):
                rc = (q.submit_state if kind == L.QUEUE_STATE else q.submit_account)(p, pub, tag=1000 + i)
                assert rc == 0
            got = drain(q, len(entries))
            assert q.poll() == [] and q.stats()["submitted"] == q.stats()["completed"] == len(entries)
        assert sorted(t for t, _, _, _ in got) == [1000 + i for i in range(len(entries))]
        for tag, verdict, rc, kind in got:
            assert (verdict, rc, kind) == (want[tag - 1000], 0, entries[tag - 1000][0]), (tag, verdict, rc, kind)
    finally:
        L.verify_configure(L.VERIFY_ALLOW_SURROGATE)


def test_one_burst_is_one_job(world, minted):
    """31 state entries with more=True and a 32nd without leave as ONE group of 32; 8 account entries with more=True leave at flush()"""
    import mina_bridge_amd as m
    L = m.lib
    pairs = minted["good"] + [minted["bad"]["ledger"]]
    with L.VerifyQueue(capacity=64) as q:
        for i in range(32):
            assert q.submit_state(*pairs[i % 5], tag=i, more=i < 31) == 0
        got = drain(q, 32)
        assert sorted(got) == [(i, 0 if i % 5 == 4 else 1, 0, L.QUEUE_STATE) for i in range(32)]
        st = q.stats()
        assert (st["jobs"], st["max_job"], st["submitted"], st["completed"]) == (1, 32, 32, 32), st
    acct = minted["acct"] + [minted["acct_bad"]["abi"]]
    with L.VerifyQueue(capacity=8) as q:
        for i in range(8):
            assert q.submit_account(*acct[i % 5], tag=i, more=True) == 0
        assert q.stats()["jobs"] == 0
        q.flush()
        got = drain(q, 8)
        assert sorted(got) == [(i, 0 if i % 5 == 4 else 1, 0, L.QUEUE_ACCOUNT) for i in range(8)]
        st = q.stats()
        assert (st["jobs"], st["max_job"]) == (1, 8), st


def test_back_pressure_by_slots(world, minted):
    """capacity 4: a slot is held from submit until its completion has been HANDED OUT, not until its job has ended"""
    import mina_bridge_amd as m
    L = m.lib
    p, pub = minted["good"][0]
    with L.VerifyQueue(capacity=4) as q:
        for i in range(4):
            assert q.submit_state(p, pub, tag=i, more=True) == 0
        assert q.stats()["completed"] == 0 and q.stats()["jobs"] == 0                # nothing runs
        assert q.submit_state(p, pub, tag=99) == L.ERR_FULL
        assert q.stats()["submitted"] == 4
        q.flush()
        assert select.select([q.fileno()], [], [], TIMEOUT_US / 1e6)[0]              # the four entries' job has ended (one group: the descriptor is written after it)
        assert q.stats()["completed"] == 4
        assert q.submit_state(p, pub, tag=99) == L.ERR_FULL                          # ... and still no slot before a completion is taken
        one = q.wait(TIMEOUT_US, max_items=1)
        assert len(one) == 1 and one[0][1:] == (1, 0, L.QUEUE_STATE)
        assert q.submit_state(p, pub, tag=4) == 0
        assert q.submit_state(p, pub, tag=99) == L.ERR_FULL
        rest = drain(q, 4)
        assert sorted([one[0][0]] + [t for t, _, _, _ in rest]) == [0, 1, 2, 3, 4] and all(v == 1 for _, v, _, _ in rest)


def test_the_queue_owns_the_bytes(world, minted):
    import mina_bridge_amd as m
    L = m.lib
    p, pub = bytearray(minted["good"][1][0]), bytearray(minted["good"][1][1])
    with L.VerifyQueue(capacity=4) as q:
        assert q.submit_state(p, pub, tag=7, more=True) == 0
        p[:] = bytes(len(p)); pub[:] = bytes(len(pub))
        # the C call itself on a caller-owned buffer, overwritten after it returns
        import ctypes
        raw = ctypes.create_string_buffer(minted["good"][2][0], len(minted["good"][2][0])); rawq = ctypes.create_string_buffer(minted["good"][2][1], len(minted["good"][2][1]))
        assert q.submit_raw(L.QUEUE_STATE, ctypes.addressof(raw), len(raw), ctypes.addressof(rawq), len(rawq), 8, L.SUBMIT_MORE) == 0
        ctypes.memset(raw, 0, len(raw)); ctypes.memset(rawq, 0, len(rawq))
        q.flush()
        assert sorted(drain(q, 2)) == [(7, 1, 0, L.QUEUE_STATE), (8, 1, 0, L.QUEUE_STATE)]
    assert L.verify_state(bytes(p), bytes(pub)) is False                              # (what the overwritten bytes would have given)


def test_beside_synchronous_callers(world, minted):
    """four threads x three mina_verify_state calls while the queue holds 16 entries: every verdict right on both sides, and the device queued less work than 28
    proofs one by one would have: the MSM finishes the device's context counts, in units of a lone proof's job"""
    import mina_bridge_amd as m
    L = m.lib
    pairs = minted["good"] + [minted["bad"]["ledger"]]                              # (a ledger mismatch is found on the host: no culprit search adds MSMs)
    dev = L.verify_device_ctx(0)
    count = lambda: sum(dev.inverse_stats().values())
    c0 = count(); assert L.verify_state(*pairs[0]) is True; lone = count() - c0
    assert lone > 0
    errors = []

    def caller(t):
        for k in range(3):
            i = (t + k) % 5
            if L.verify_state(*pairs[i]) is not (i != 4): errors.append((t, k))
    with L.VerifyQueue(capacity=16) as q:
        c0 = count()
        th = [threading.Thread(target=caller, args=(t,)) for t in range(4)]
        for i in range(16):
            assert q.submit_state(*pairs[i % 5], tag=i, more=True) == 0
        for t in th: t.start()
        q.flush()
        got = drain(q, 16)
        for t in th: t.join()
        used = count() - c0
        st = q.stats()
    assert not errors, errors
    assert sorted(got) == [(i, 0 if i % 5 == 4 else 1, 0, L.QUEUE_STATE) for i in range(16)]
    print(f"MSM finishes: {lone} for a lone proof, {used} for 12 synchronous + 16 queued proofs ({used / lone:.1f} jobs' worth); queue jobs {st['jobs']}, largest {st['max_job']}")
    assert st["jobs"] == 1 and st["max_job"] == 16
    assert used < 28 * lone


def test_wait_times_out_and_the_descriptor_follows_the_completions(world, minted):
    import mina_bridge_amd as m
    L = m.lib
    with L.VerifyQueue(capacity=4) as q:
        fd = q.fileno()
        assert fd >= 0 and not select.select([fd], [], [], 0)[0]
        t0 = time.monotonic(); got = q.wait(timeout_us=20_000); dt = time.monotonic() - t0
        assert got == [] and dt >= 0.020, dt
        assert q.submit_account(*minted["acct"][0], tag=5) == 0
        assert select.select([fd], [], [], TIMEOUT_US / 1e6)[0]                      # readable after the job
        assert len(os.read(fd, 8)) == 8                                              # the consumer clears it ...
        assert q.poll() == [(5, 1, 0, L.QUEUE_ACCOUNT)] and q.poll() == []           # ... and polls until nothing comes
        assert not select.select([fd], [], [], 0)[0]
        # a consumer that never reads the descriptor: poll clears it with the last completion
        assert q.submit_account(*minted["acct"][1], tag=6) == 0
        assert select.select([fd], [], [], TIMEOUT_US / 1e6)[0]
        assert q.poll() == [(6, 1, 0, L.QUEUE_ACCOUNT)]
        assert not select.select([fd], [], [], 0)[0]


def test_arguments(world, minted):
    """every bad argument is MINA_ERR_ARG and leaves the queue as it was"""
    import ctypes
    import mina_bridge_amd as m
    L = m.lib
    lib = L._queue_lib()
    for capacity, workers in ((0, 1), (65537, 1), (16, 0), (16, 5)):
        h = ctypes.c_void_p(1)
        assert lib.mina_verify_queue_create(capacity, workers, ctypes.byref(h)) == L.ERR_ARG and not h.value
        with pytest.raises(m.MinaError):
            L.VerifyQueue(capacity, workers)
    assert lib.mina_verify_queue_create(16, 1, None) == L.ERR_ARG
    lib.mina_verify_queue_destroy(None)                                              # a no-op
    big = ctypes.create_string_buffer((1 << 20) + 1)
    with L.VerifyQueue(capacity=2) as q:
        before = q.stats()
        a = ctypes.addressof(big)
        assert q.submit_raw(2, a, 4, a, 4, 1, 0) == L.ERR_ARG                         # unknown kind
        assert q.submit_raw(L.QUEUE_STATE, None, 4, a, 4, 1, 0) == L.ERR_ARG          # null proof, non-zero length
        assert q.submit_raw(L.QUEUE_ACCOUNT, a, 4, None, 4, 1, 0) == L.ERR_ARG
        assert q.submit_raw(L.QUEUE_STATE, a, (1 << 20) + 1, a, 4, 1, 0) == L.ERR_ARG  # above the 1 MiB cap
        assert q.submit_raw(L.QUEUE_STATE, a, 4, a, (1 << 20) + 1, 1, 0) == L.ERR_ARG
        assert q.submit_raw(L.QUEUE_STATE, a, 4, a, 4, 1, 2) == L.ERR_ARG             # unknown flag
        assert lib.mina_verify_queue_submit(None, 0, a, 4, a, 4, 1, 0) == L.ERR_ARG
        n = ctypes.c_size_t(9)
        assert lib.mina_verify_queue_poll(q._h, None, 1, ctypes.byref(n)) == L.ERR_ARG and lib.mina_verify_queue_poll(q._h, None, 0, None) == L.ERR_ARG
        assert lib.mina_verify_queue_wait(None, None, 0, ctypes.byref(n), 0) == L.ERR_ARG and lib.mina_verify_queue_fd(None) == L.ERR_ARG
        assert lib.mina_verify_queue_flush(None) == L.ERR_ARG and lib.mina_verify_queue_stats(None, None, None, None, None) == L.ERR_ARG
        assert q.stats() == before == {"submitted": 0, "completed": 0, "jobs": 0, "max_job": 0}
        # both slots are still free, and a null pointer with length 0 is legal: an empty proof is `false`
        assert q.submit_raw(L.QUEUE_STATE, None, 0, None, 0, 1, 0) == 0 and q.submit_raw(L.QUEUE_ACCOUNT, None, 0, None, 0, 2, 0) == 0
        assert sorted(drain(q, 2)) == [(1, 0, 0, L.QUEUE_STATE), (2, 0, 0, L.QUEUE_ACCOUNT)]


def test_teardown_and_shutdown(world, minted):
    """close() with entries never flushed returns (it runs them); a new queue works; after mina_verify_shutdown an idle queue is still usable: the process-wide
    contexts come back with its next job (the indexes are installed again, as after any shutdown).  Last in the file: it replaces the module's contexts."""
    import mina_bridge_amd as m
    from kimchi_helpers import install_index, install_step_index
    L = m.lib
    p, pub = minted["good"][0]
    q = L.VerifyQueue(capacity=8)
    for i in range(8):
        assert q.submit_state(p, pub, tag=i, more=True) == 0
    q.close()
    q.close()                                                                        # (idempotent in the Python class)
    with L.VerifyQueue(capacity=8, workers=2) as q:
        assert q.submit_state(p, pub, tag=1) == 0 and q.submit_account(*minted["acct"][3], tag=2) == 0
        assert sorted(drain(q, 2)) == [(1, 1, 0, L.QUEUE_STATE), (2, 1, 0, L.QUEUE_ACCOUNT)]
        assert q.stats()["submitted"] == q.stats()["completed"]                      # idle
        L.verify_shutdown()
        assert q.submit_state(minted["bad"]["chain"][0], minted["bad"]["chain"][1], tag=3) == 0     # the contexts come back lazily, without an index: `false` either way
        assert drain(q, 1) == [(3, 0, 0, L.QUEUE_STATE)]
        gctx = L.verify_global_ctx()
        install_index(gctx, world["circ"].index); install_step_index(gctx, world["step"])
        world["gctx"] = gctx
        assert q.submit_state(p, pub, tag=4) == 0 and q.submit_state(*minted["bad"]["opening scalar"], tag=5) == 0
        assert sorted(drain(q, 2)) == [(4, 1, 0, L.QUEUE_STATE), (5, 0, 0, L.QUEUE_STATE)]
        assert L.verify_state(p, pub) is True
