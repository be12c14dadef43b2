"""Mainnet and devnet proofs through ONE process: an index pair per network at the boundary (mina_verify_install_*_net, network mode).  The reference verifier
picks the devnet or the mainnet blockchain-snark index per proof by `is_state_proof_from_devnet`; so does the boundary once a pair is installed per network --
the kimchi step of a proof runs against the index set of the network its public input names (csrc/net_route.h), through every Proof-of-State entry point.
Two pairs with proofs of their own (tests/network_helpers.py): the oracle accepts each proof under its own pair only (tests/golden/gen_alt_network_fixture.py).
All at k = 15, the one size the wrap fixtures exist at; calls of 1 to 12 proofs."""
import ctypes
import json
import os
import subprocess
import sys
import threading

import pytest

from network_helpers import ALL, KIMCHI, load_pairs

pytestmark = pytest.mark.gpu
MAINNET, DEVNET = 0, 1
ERR_ARG, ERR_STATE = -1, -3
JUNK = b"\x00" * 100


@pytest.fixture(scope="module")
def net(oracle):
    import mina_bridge_amd as m
    A, B = load_pairs()
    m.lib.verify_shutdown()                                    # a fresh boundary: whatever an earlier module installed is gone
    m.lib.verify_set_network(-1)
    m.lib.verify_configure(m.lib.VERIFY_ALLOW_SURROGATE)      # the tests run on the surrogate Poseidon tables (the real ones are not offline)
    yield {"m": m, "A": A, "B": B}
    m.lib.verify_drop_network_indexes()
    m.lib.verify_set_network(-1)
    m.lib.verify_shutdown()
    m.lib.verify_configure(0)


def install(m, by_network):
    """{network: pair}: each pair into the set of its network, on every device"""
    for n, pair in by_network.items():
        pair.install(m.lib.verify_network_devices(n))


def six(A, B):
    """the mixed call of the issue and its verdicts under (A for devnet, B for mainnet)"""
    a, b = A.cases, B.cases
    calls = [(a[0]["proof"], a[0]["pub"][DEVNET]), (b[0]["proof"], b[0]["pub"][MAINNET]), (a[1]["proof"], a[1]["pub"][MAINNET]), (b[1]["proof"], b[1]["pub"][DEVNET]),
             (JUNK, JUNK), (a[2]["proof"], a[2]["pub"][DEVNET])]
    return calls, [1, 1, 0, 0, 0, 1]


def batch(m, calls):
    return m.lib.verify_state_batch([c[0] for c in calls], [c[1] for c in calls]).tolist()


def test_both_networks_in_one_call(net):
    m, A, B = net["m"], net["A"], net["B"]
    install(m, {DEVNET: A, MAINNET: B})
    assert m.lib.verify_networks() == (1, 1)
    calls, want = six(A, B)
    assert batch(m, calls) == want
    assert [int(m.lib.verify_state(p, q)) for p, q in calls] == want, "each proof gives the same answer singly"
    singles = [m.lib.verify_state_checks(p, q) for p, q in calls]
    for i in (2, 3):                                           # wrong network: the kimchi step ran and failed, the other five passed
        assert singles[i] == (ALL & ~KIMCHI, ALL), (i, singles[i])
    for i in (0, 1, 5):
        assert singles[i] == (ALL, ALL), (i, singles[i])
    passed, ran = m.lib.verify_state_checks_batch([c[0] for c in calls], [c[1] for c in calls])
    assert list(zip(passed.tolist(), ran.tolist())) == [tuple(int(x) for x in s) for s in singles]
    with m.lib.VerifyQueue(capacity=16, workers=1) as q:
        for tag, (p, pub) in enumerate(calls):
            assert q.submit_state(p, pub, tag=100 + tag, more=tag + 1 < len(calls)) == 0
        done = {}
        while len(done) < len(calls):
            got = q.wait(timeout_us=60_000_000)
            assert got, "the completion queue answered nothing within a minute"
            for tag, verdict, rc, _ in got:
                assert rc == 0
                done[tag] = verdict
    assert [done[100 + i] for i in range(len(calls))] == want


def test_the_sets_are_per_network(net):
    m, A, B = net["m"], net["A"], net["B"]
    install(m, {DEVNET: A, MAINNET: B})
    calls, want = six(A, B)
    assert batch(m, calls) == want
    install(m, {MAINNET: A, DEVNET: B})                         # the other way round, in the same process
    assert batch(m, calls) == [0, 0, 1, 1, 0, 0], "the verdicts of the pairs' proofs swap with the pairs"
    assert [int(m.lib.verify_state(p, q)) for p, q in calls[:4]] == [0, 0, 1, 1]


def test_one_network_only(net):
    m, A, B = net["m"], net["A"], net["B"]
    m.lib.verify_drop_network_indexes()
    assert m.lib.verify_networks() == (0, 0)
    install(m, {DEVNET: A})
    assert m.lib.verify_networks() == (0, 1)
    dev = A.good(DEVNET)
    assert batch(m, dev) == [1] * len(dev)
    for p, q in A.good(MAINNET)[:2] + B.good(MAINNET):
        assert m.lib.verify_state(p, q) is False, "no pair for mainnet: a mainnet-flagged proof fails alone"
        assert m.lib.verify_state_checks(p, q) == (ALL & ~KIMCHI, ALL)
        assert batch(m, [dev[0], (p, q), dev[1]]) == [1, 0, 1], "and costs its clean devnet neighbours nothing"


def interleave(x, y):
    out = []
    for i in range(max(len(x), len(y))):
        out += [("x", i)] * (i < len(x)) + [("y", i)] * (i < len(y))
    return out


def test_equal_to_the_single_network_library_failures_included(net):
    m, A, B = net["m"], net["A"], net["B"]
    lists = {DEVNET: A.good(DEVNET) + A.tampered(DEVNET), MAINNET: B.good(MAINNET) + B.tampered(MAINNET)}
    pair_of = {DEVNET: A, MAINNET: B}
    ref = {}
    for n in (DEVNET, MAINNET):                                 # what a process holding n's pair alone, with n declared, answers
        m.lib.verify_drop_network_indexes()
        m.lib.verify_shutdown()
        pair_of[n].install(m.lib.verify_all_devices())
        m.lib.verify_set_network(n)
        v = batch(m, lists[n])
        p, r = m.lib.verify_state_checks_batch([c[0] for c in lists[n]], [c[1] for c in lists[n]])
        ref[n] = list(zip(v, p.tolist(), r.tolist()))
        m.lib.verify_set_network(-1)
    ngood = {DEVNET: len(A.cases), MAINNET: len(B.cases)}
    for n in ref:
        assert [v for v, _, _ in ref[n]] == [1] * ngood[n] + [0] * 4, (n, ref[n])
        assert [(p, r) for _, p, r in ref[n]][:ngood[n]] == [(ALL, ALL)] * ngood[n]
    m.lib.verify_shutdown()
    install(m, pair_of)
    order = interleave(lists[DEVNET], lists[MAINNET])
    calls = [lists[DEVNET if w == "x" else MAINNET][i] for w, i in order]
    want = [ref[DEVNET if w == "x" else MAINNET][i] for w, i in order]
    base = m.lib.VERIFY_ALLOW_SURROGATE
    try:
        for flags in (0, m.lib.VERIFY_PACK_ON_DEVICE | m.lib.VERIFY_DEDUP_STATES, m.lib.VERIFY_GROUPED_SEARCH):
            m.lib.verify_configure(base | flags)
            v = batch(m, calls)
            p, r = m.lib.verify_state_checks_batch([c[0] for c in calls], [c[1] for c in calls])
            got = list(zip(v, p.tolist(), r.tolist()))
            assert got == want, (flags, [(i, got[i], want[i]) for i in range(len(got)) if got[i] != want[i]])
    finally:
        m.lib.verify_configure(base)


def test_merged_callers_each_get_their_own_verdict(net):
    m, A, B = net["m"], net["A"], net["B"]
    m.lib.verify_drop_network_indexes()
    install(m, {DEVNET: A, MAINNET: B})
    z2 = A.tampered(DEVNET)[2]
    wrong = (A.cases[3]["proof"], A.cases[3]["pub"][MAINNET])   # an A proof that claims mainnet, where B is installed
    calls = A.good(DEVNET)[:3] + [z2] + [B.good(MAINNET)[0], B.good(MAINNET)[1], B.good(MAINNET)[0]] + [wrong]
    want = [True, True, True, False, True, True, True, False]
    assert m.lib.verify_state(*calls[0]) is True               # warm: contexts, tables, buffers
    got = [None] * len(calls)
    gate = threading.Barrier(len(calls))
    def worker(i):
        gate.wait()
        got[i] = m.lib.verify_state(*calls[i])
    th = [threading.Thread(target=worker, args=(i,)) for i in range(len(calls))]
    for t in th: t.start()
    for t in th: t.join()
    assert got == want


def test_mode_errors(net):
    m, A, B = net["m"], net["A"], net["B"]
    lib = m.lib.load_library()
    from mina_bridge_amd.lib import MinaContext
    from kimchi_helpers import STEP_DOMAINS, encode_tokens, pts
    from oracle import oracle as O
    import numpy as np
    ix, st = A.ix, A.step
    vi, keep_v = MinaContext._verifier_index_struct(ix.log2_domain, ix.zk_rows, ix.perm_alpha_offset, O.ints_to_le(ix.shifts).reshape(-1), pts(ix.sigma_comm),
                                                    pts(ix.coefficients_comm), pts(ix.selector_comm), encode_tokens(ix.constant_term))
    si, keep_s = MinaContext._step_index_struct(st.zk_rows, STEP_DOMAINS, np.concatenate([O.ints_to_le(st.shifts[k]).reshape(-1) for k in STEP_DOMAINS]), encode_tokens(st.constant_term))
    m.lib.verify_drop_network_indexes()
    # bad arguments: before any device is touched, and without entering network mode
    assert lib.mina_verify_install_verifier_index_net(ctypes.c_int(2), ctypes.byref(vi)) == ERR_ARG
    assert lib.mina_verify_install_verifier_index_net(ctypes.c_int(-1), ctypes.byref(vi)) == ERR_ARG
    assert lib.mina_verify_install_verifier_index_net(ctypes.c_int(0), None) == ERR_ARG
    assert lib.mina_verify_install_step_index_net(ctypes.c_int(2), ctypes.byref(si)) == ERR_ARG
    assert lib.mina_verify_install_step_index_net(ctypes.c_int(1), None) == ERR_ARG
    assert lib.mina_verify_set_network(ctypes.c_int(-1)) == 0, "still outside network mode"
    # in network mode the single-pair calls answer MINA_ERR_STATE and change nothing
    install(m, {DEVNET: A, MAINNET: B})
    calls, want = six(A, B)
    assert lib.mina_verify_set_network(ctypes.c_int(0)) == ERR_STATE
    assert lib.mina_verify_install_verifier_index(ctypes.byref(vi)) == ERR_STATE
    assert lib.mina_verify_install_step_index(ctypes.byref(si)) == ERR_STATE
    assert batch(m, calls) == want
    # with a network declared, the per-network installers answer MINA_ERR_STATE
    m.lib.verify_drop_network_indexes()
    m.lib.verify_set_network(1)
    try:
        assert lib.mina_verify_install_verifier_index_net(ctypes.c_int(1), ctypes.byref(vi)) == ERR_STATE
        assert lib.mina_verify_install_step_index_net(ctypes.c_int(0), ctypes.byref(si)) == ERR_STATE
        assert m.lib.verify_networks() == (0, 0)
        # ... and the single-pair library is what it was: the flag must match the declared network
        A.install(m.lib.verify_all_devices())
        c = A.cases[0]
        assert m.lib.verify_state(c["proof"], c["pub"][DEVNET]) is True
        m.lib.verify_set_network(0)
        assert m.lib.verify_state(c["proof"], c["pub"][DEVNET]) is False
        assert m.lib.verify_state_checks(c["proof"], c["pub"][DEVNET]) == (ALL & ~KIMCHI, ALL)
        assert batch(m, [(c["proof"], c["pub"][MAINNET]), (c["proof"], c["pub"][DEVNET])]) == [1, 0]
    finally:
        m.lib.verify_set_network(-1)
    c = A.cases[0]
    assert m.lib.verify_state(c["proof"], c["pub"][DEVNET]) is True and m.lib.verify_state(c["proof"], c["pub"][MAINNET]) is True
    m.lib.verify_shutdown()


CHILD = r"""
import json, os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import mina_bridge_amd as m
from network_helpers import load_pairs
A, B = load_pairs()
m.lib.verify_configure(m.lib.VERIFY_ALLOW_SURROGATE)
assert m.lib.verify_device_count() == 2
A.install(m.lib.verify_network_devices(1)); B.install(m.lib.verify_network_devices(0))
a, b = A.cases, B.cases
calls = [(a[0]["proof"], a[0]["pub"][1]), (b[0]["proof"], b[0]["pub"][0]), (a[1]["proof"], a[1]["pub"][0]), (b[1]["proof"], b[1]["pub"][1]),
         (b"\x00" * 100, b"\x00" * 100), (a[2]["proof"], a[2]["pub"][1]), (b[1]["proof"], b[1]["pub"][0]), (a[3]["proof"], a[3]["pub"][1])]
with m.lib.tuning(min_shard=2, merge_batch_max=0):
    v = m.lib.verify_state_batch([c[0] for c in calls], [c[1] for c in calls]).tolist()
digests = []
for d in range(2):
    c = m.lib.verify_device_ctx(d)
    row = []
    for s in range(2):
        c.select_index_set(s)
        row.append(bytes(c.verifier_index_digest()).hex())
    c.select_index_set(0)
    digests.append(row)
want_digests = [int(B.ix.digest).to_bytes(32, "little").hex(), int(A.ix.digest).to_bytes(32, "little").hex()]
m.lib.verify_shutdown()
print("RESULT " + json.dumps({"verdicts": v, "digests": digests, "want_digests": want_digests}))
"""


def test_two_logical_devices_share_the_rule(net, tmp_path):
    """a fresh process with two logical contexts on the GPU: an 8-proof mixed call cut into two shards, each shard with passes of its own per network"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "two_devices_child.py"
    script.write_text(CHILD)
    env = dict(os.environ, MINA_VERIFY_DEVICES="0,0")
    done = subprocess.run([sys.executable, str(script), root], env=env, capture_output=True, text=True, timeout=600)
    assert done.returncode == 0, done.stderr[-4000:]
    line = [l for l in done.stdout.splitlines() if l.startswith("RESULT ")][-1]
    res = json.loads(line[len("RESULT "):])
    assert res["verdicts"] == [1, 1, 0, 0, 0, 1, 1, 1]
    assert res["digests"][0] == res["digests"][1], "both device contexts hold the same two sets"
    assert res["digests"][0] == res["want_digests"], "set 0 = mainnet's pair (B), set 1 = devnet's (A)"
