"""The device path of Proof-of-Account on the GPU (mina_account_frontend_dev, mina_account_job_dev, MINA_VERIFY_ACCOUNT_ON_DEVICE).  The checker is the HOST path:
`passed` / `ran` equal mina_verify_account_ctx, account hashes equal mina_account_hash_batch, roots equal mina_merkle_roots, the reader's outputs equal
mina_parse_merkle_path / mina_parse_account_pub_inputs / mina_account_abi_encode and the oracle's `to_input` fields (tests/account_pack_helpers.py) -- for
well-formed pairs of every account shape and depth, for every truncation and byte position of a proof and of a public input in one launch each, for a shuffled
mixed batch, across a change of Poseidon tables, and through the boundary with the flag off and on.  Every sweep asserts on the checker's output that all four
outcomes (FORMAT fails; FORMAT passes, ABI fails; ABI passes, MERKLE fails; everything passes) occur.
Jobs of more than 8192 pairs and forced lane forms, against the CPU oracle and the CPU model of the fold: tests/test_gpu_account_forms.py."""
import os
import random
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import account_pack_helpers as H  # noqa: E402

pytestmark = pytest.mark.gpu
OK = H.CHECK_FORMAT | H.CHECK_ACCOUNT_ABI | H.CHECK_MERKLE
CLASSES = ("FORMAT fails", "FORMAT passes, ABI fails", "ABI passes, MERKLE fails", "everything passes")


class Dev:
    """device buffers of one test, freed together"""
    def __init__(self, ctx): self.ctx, self.ptrs = ctx, []
    def put(self, data):
        a = np.frombuffer(bytes(data), np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        p = self.ctx.dev_malloc(max(a.size, 16)); self.ptrs.append(p)
        if a.size: self.ctx.dev_upload(p, a)
        return p
    def new(self, nbytes, fill=0xcd):
        return self.put(np.full(max(nbytes, 16), fill, np.uint8))
    def free(self):
        for p in self.ptrs: self.ctx.dev_free(p)
        self.ptrs = []


def job_dev(ctx, pairs, outputs=True):
    """mina_account_job_dev over pairs [(proof, pub)] in ONE launch sequence -> passed, ran, account hashes, roots"""
    blob, po, pl, qo, ql = H.blob_of(pairs)
    n = len(pairs)
    d = Dev(ctx)
    try:
        d_blob, d_po, d_pl, d_qo, d_ql = d.put(blob), d.put(po), d.put(pl), d.put(qo), d.put(ql)
        d_p, d_r, d_h, d_t = d.new(4 * n), d.new(4 * n), d.new(32 * n), d.new(32 * n)
        ctx.account_job_dev(n, d_blob, len(blob), d_po, d_pl, d_qo, d_ql, d_p, d_r, d_h if outputs else 0, d_t if outputs else 0)
        ctx.synchronize()
        return (ctx.dev_download(d_p, 4 * n).view(np.uint32).copy(), ctx.dev_download(d_r, 4 * n).view(np.uint32).copy(), ctx.dev_download(d_h, 32 * n).reshape(n, 32).copy(),
                ctx.dev_download(d_t, 32 * n).reshape(n, 32).copy())
    finally:
        d.free()


def frontend_dev(ctx, pairs):
    blob, po, pl, qo, ql = H.blob_of(pairs)
    n = len(pairs)
    d = Dev(ctx)
    try:
        ins = [d.put(x) for x in (blob, po, pl, qo, ql)]
        outs = {name: d.new(size(n), 0) for name, size in H.FRONTEND_SIZES}
        ctx.account_frontend_dev(n, ins[0], len(blob), ins[1], ins[2], ins[3], ins[4], *[outs[name] for name, _ in H.FRONTEND_SIZES])
        ctx.synchronize()
        return H.unpack_frontend({name: ctx.dev_download(outs[name], size(n)).copy() for name, size in H.FRONTEND_SIZES}, n)
    finally:
        d.free()


def check_job(ctx, m, pairs, passed, ran, hashes, roots):
    """everything the job wrote against the host path -> how many pairs fell into each of the four outcomes (by the CHECKER's masks)"""
    proofs, pubs = [p for p, _ in pairs], [q for _, q in pairs]
    hp, hr = ctx.verify_account_checks(proofs, pubs)
    assert (passed == hp).all() and (ran == hr).all(), [(i, hex(int(passed[i])), hex(int(hp[i])), hex(int(ran[i])), hex(int(hr[i]))) for i in np.nonzero((passed != hp) | (ran != hr))[0][:5]]
    accepted = [i for i in range(len(pairs)) if int(hp[i]) & H.CHECK_FORMAT]
    if accepted:
        parsed = [m.lib.parse_merkle_path(proofs[i], H.MAXD) for i in accepted]
        want = ctx.account_hash_batch([proofs[i][off:] for i, (_, _, off) in zip(accepted, parsed)], m.lib.ENC_BINCODE)
        assert (hashes[accepted] == want).all(), "account hashes"
        by_depth = {}
        for k, (i, (sib, dirs, _)) in enumerate(zip(accepted, parsed)): by_depth.setdefault(len(dirs), []).append((k, i, sib, dirs))
        for depth, group in by_depth.items():
            leaves = np.stack([want[k] for k, _, _, _ in group])
            r = leaves if depth == 0 else ctx.merkle_roots(0, leaves, np.concatenate([s.reshape(-1) for _, _, s, _ in group]), np.concatenate([x for _, _, _, x in group]), depth)
            assert (roots[[i for _, i, _, _ in group]] == r).all(), ("roots", depth)
    counts = dict.fromkeys(CLASSES, 0)
    for p in hp:
        p = int(p)
        counts[CLASSES[0] if not p & H.CHECK_FORMAT else (CLASSES[1] if not p & H.CHECK_ACCOUNT_ABI else (CLASSES[2] if not p & H.CHECK_MERKLE else CLASSES[3]))] += 1
    return counts


def host_ledger(ctx, m):
    """ledger_of(account, path) for account_pack_helpers.well_formed_pairs: the root the HOST path computes"""
    from oracle import mina_account_ref as A
    def ledger_of(a, path):
        leaf = ctx.account_hash_batch([A.write_account(a, False)], m.lib.ENC_BINCODE)
        if not path: return int.from_bytes(leaf[0].tobytes(), "little")
        sib = np.concatenate([np.frombuffer(int(s).to_bytes(32, "little"), np.uint8) for _, s in path]); dirs = np.array([d for d, _ in path], np.uint8)
        return int.from_bytes(ctx.merkle_roots(0, leaf, sib, dirs, len(path))[0].tobytes(), "little")
    return ledger_of


def with_failures(cases):
    """well-formed cases [(name, proof, pub, ..)] -> pairs [(proof, pub)] with the other three outcomes added for every fifth: a cut proof; its own ledger hash in
    front of another account's encoding; another pair's ledger hash in front of its own encoding"""
    pairs = [(c[1], c[2]) for c in cases]
    extra = []
    for i in range(0, len(cases), 5):
        p, q = pairs[i]; q2 = pairs[(i + 1) % len(pairs)][1]
        extra += [(p[:-1], q), (p, q[:32] + q2[32:]), (p, q2[:32] + q[32:])]
    return pairs + extra


def test_well_formed_pairs_of_every_shape_and_their_failures(ctx):
    """every combination of zkApp / key / timing / delegate, symbol lengths 0 and 6, URI lengths 0, 31, 32, 255, depths 0, 1, 35, 64 in one batch: the oracle's own
    account hash, the host path's masks, hashes and roots; and the reader's records against the oracle's `to_input` fields"""
    import mina_bridge_amd as m
    from ipa_helpers import poseidon_pp
    cases = H.well_formed_pairs(ledger_of=host_ledger(ctx, m))
    n = len(cases)
    f = frontend_dev(ctx, [(c[1], c[2]) for c in cases])
    refs, classes = H.check_frontend(m, [(c[0], c[1], c[2]) for c in cases], f)
    assert classes == ["abi passes"] * n
    oracle_hashes = H.check_records(cases, f, poseidon_pp(0))
    pairs = with_failures(cases)
    passed, ran, hashes, roots = job_dev(ctx, pairs)
    counts = check_job(ctx, m, pairs, passed, ran, hashes, roots)
    print(counts)
    assert all(counts[c] >= 1 for c in CLASSES) and counts[CLASSES[3]] >= n, counts
    assert (passed[:n] == OK).all() and (ran[:n] == OK).all()
    assert [int.from_bytes(hashes[i].tobytes(), "little") for i in range(n)] == oracle_hashes        # the CPU oracle, which takes no shortcut for the default sub-hashes
    # without the optional outputs: the same masks
    p2, r2, _, _ = job_dev(ctx, pairs, outputs=False)
    assert (p2 == passed).all() and (r2 == ran).all()


def sweep_subject(ctx, m):
    from oracle import mina_account_ref as A
    rng = random.Random(H.SEED + 7)
    a = A.synth_account(rng, True, True, True, with_vk=True)
    a["token_symbol"] = b"SWEEP!"; a["zkapp"]["zkapp_uri"] = bytes(rng.randrange(256) for _ in range(31))
    path = H.random_path(rng, 2)
    return A.write_account_proof(path, a), H.pub_input(host_ledger(ctx, m)(a, path), A.abi_encode_account(a))


@pytest.mark.parametrize("side", ["proof", "public input"])
def test_every_truncation_and_byte_position_in_one_launch(ctx, side):
    """one full zkApp pair: every truncation, a trailing byte and every byte position with several replacement values, of the proof and of the public input -- one job
    each, every case compared with the host path, none skipped"""
    import mina_bridge_amd as m
    proof, pub = sweep_subject(ctx, m)
    muts = H.proof_mutations(proof if side == "proof" else pub)
    pairs = [(b, pub) if side == "proof" else (proof, b) for _, b in muts]
    passed, ran, hashes, roots = job_dev(ctx, pairs)
    counts = check_job(ctx, m, pairs, passed, ran, hashes, roots)
    print(side, len(pairs), "cases:", counts)
    assert all(counts[c] >= 1 for c in CLASSES), counts
    assert counts[CLASSES[0]] >= len(muts[0][1])              # every truncation at the least
    f = frontend_dev(ctx, pairs)
    H.check_frontend(m, [(name, p, q) for (name, _), (p, q) in zip(muts, pairs)], f)


def test_mixed_batch_in_random_order(ctx):
    """plain and zkApp accounts and all four depths shuffled, with failures of each kind in between, n not a multiple of 3, 4, 8, 16, 21 or 64"""
    import mina_bridge_amd as m
    cases = H.well_formed_pairs(seed=H.SEED + 100, ledger_of=host_ledger(ctx, m))
    pairs = with_failures(cases) * 9
    random.Random(3).shuffle(pairs)
    pairs = pairs[:len(pairs) - 1 if len(pairs) % 2 == 0 else len(pairs)]
    while any(len(pairs) % k == 0 for k in (3, 4, 7, 8, 16, 21, 64)): pairs.pop()
    passed, ran, hashes, roots = job_dev(ctx, pairs)
    counts = check_job(ctx, m, pairs, passed, ran, hashes, roots)
    print(len(pairs), counts)
    assert all(counts[c] >= 9 for c in CLASSES) and len(pairs) > 250, counts
    # twice the same job: the compacted list may come in another order, the results may not differ
    again = job_dev(ctx, pairs)
    assert all((a == b).all() for a, b in zip((passed, ran), again[:2]))
    acc = [i for i in range(len(pairs)) if int(passed[i]) & H.CHECK_FORMAT]
    assert (again[2][acc] == hashes[acc]).all() and (again[3][acc] == roots[acc]).all()


def test_default_sub_hashes_follow_the_poseidon_tables():
    """the cached hashes of the empty URI, the dummy key and the default zkApp record are dropped by mina_poseidon_set_params: a job before, one after a different
    table and one after the first table again each equal the host path under the same table (which hashes the defaults per account), and the tables do differ"""
    import mina_bridge_amd as m
    c = m.MinaContext(0)
    try:
        tables = [m.poseidon_params.default_params_bytes(0)]
        other = bytearray(tables[0]); other[9 * 32] ^= 1; tables.append(bytes(other))          # the first round constant, one bit: still below the modulus
        for f in (0, 1): c.poseidon_set_params(f, m.poseidon_params.default_params_bytes(f))
        cases = H.well_formed_pairs(seed=H.SEED + 200, ledger_of=host_ledger(c, m))
        pairs = with_failures(cases)
        plain = [i for i, cs in enumerate(cases) if cs[3]["zkapp"] is None]
        seen = []
        for t in (0, 1, 0):
            c.poseidon_set_params(0, tables[t])
            passed, ran, hashes, roots = job_dev(c, pairs)
            counts = check_job(c, m, pairs, passed, ran, hashes, roots)
            assert counts[CLASSES[0]] >= 1 and counts[CLASSES[1]] >= 1, counts
            assert (counts[CLASSES[3]] >= len(cases)) == (t == 0), (t, counts)          # the ledger hashes were made under table 0
            seen.append(hashes[plain].copy())
        assert len(plain) >= 8 and (seen[0] == seen[2]).all() and (seen[0] != seen[1]).any(axis=1).all()
    finally:
        c.close()


def test_bad_arguments_are_refused(ctx):
    import mina_bridge_amd as m
    d = Dev(ctx)
    try:
        p = d.new(4096)
        with pytest.raises(m.lib.MinaError): ctx.account_job_dev(1, p, 64, p + 4, p, p, p, p, p)              # misaligned offsets
        with pytest.raises(m.lib.MinaError): ctx.account_job_dev(1, p, 64, p, p, p, p, 0, p)                  # null output
        with pytest.raises(m.lib.MinaError): ctx.account_job_dev(1 << 23, p, 64, p, p, p, p, p, p)            # too many
        ctx.account_job_dev(0, 0, 0, 0, 0, 0, 0, 0, 0)
        bare = m.MinaContext(0)
        try:
            with pytest.raises(m.lib.MinaError, match="Poseidon"): bare.account_job_dev(1, p, 64, p, p, p, p, p, p)
        finally:
            bare.close()
    finally:
        d.free()


# ------------------------------------------------------------------------------------------------ the boundary
from test_verify_boundary import mint_state_proof, to_bytes, world  # noqa: E402,F401  (the module-scoped fixture and the state-proof writers of the boundary's own tests)


def boundary_cases(m, gctx):
    cases = H.well_formed_pairs(seed=H.SEED + 300, ledger_of=host_ledger(gctx, m))
    return with_failures(cases)


def run_boundary(m, pairs):
    proofs, pubs = [p for p, _ in pairs], [q for _, q in pairs]
    checks = [m.lib.verify_account_checks(p, q) for p, q in pairs[:40]]
    singles = [m.lib.verify_account(p, q) for p, q in pairs[:12]]
    return checks, singles, m.lib.verify_account_batch(proofs, pubs).tolist(), m.lib.verify_account_batch(proofs * 12, pubs * 12).tolist()


def test_boundary_flag_off_and_on(world):
    """mina_verify_account, _account_batch (a merged small batch and a direct one) and _account_checks return the same verdicts and masks with
    MINA_VERIFY_ACCOUNT_ON_DEVICE off and on; the checker's verdicts cover all four outcomes"""
    import mina_bridge_amd as m
    base = m.lib.VERIFY_ALLOW_SURROGATE
    pairs = boundary_cases(m, world["gctx"])
    try:
        off = run_boundary(m, pairs)
        m.lib.verify_configure(base | m.lib.VERIFY_ACCOUNT_ON_DEVICE)
        on = run_boundary(m, pairs)
        on2 = run_boundary(m, pairs)
    finally:
        m.lib.verify_configure(base)
    assert off == on == on2
    hp, hr = world["gctx"].verify_account_checks([p for p, _ in pairs], [q for _, q in pairs])
    assert off[0] == [(int(a), int(b)) for a, b in zip(hp[:40], hr[:40])] and off[2] == [1 if int(a) == OK else 0 for a in hp]
    kinds = {(bool(p & 1), bool(p & 64), bool(p & 128)) for p, _ in off[0]}
    assert {(False, False, False), (True, False, True), (True, True, False), (True, True, True)} <= kinds, kinds
    assert sum(off[2]) >= 24 and off[2].count(0) >= 10


def test_boundary_flag_on_beside_state_proof_callers(world, srs_oracle):
    """the shape of test_state_and_account_callers_at_once with the flag on: single state proofs and state batches (one tampered), single account proofs and account
    batches from nine threads; every caller gets the verdicts the host path gave with the flag off"""
    import copy
    import mina_bridge_amd as m
    base = m.lib.VERIFY_ALLOW_SURROGATE
    minted = [mint_state_proof(world, srs_oracle, 7300 + i) for i in range(2)]
    good = [to_bytes(*x) for x in minted]
    w_bad = copy.deepcopy(minted[1][0]); w_bad["z1"] = (w_bad["z1"] + 3) % (1 << 254)
    bad = to_bytes(w_bad, minted[1][1], minted[1][2])
    pairs = boundary_cases(m, world["gctx"])
    want_single = [m.lib.verify_account(p, q) for p, q in pairs]
    want_batch = m.lib.verify_account_batch([p for p, _ in pairs], [q for _, q in pairs]).tolist()
    assert want_batch == [1 if w else 0 for w in want_single] and 0 < sum(want_batch) < len(pairs)
    errors = []

    def state_single(t):
        for k in range(4):
            is_bad = (t + k) % 3 == 0
            if m.lib.verify_state(*(bad if is_bad else good[k % 2])) is not (not is_bad): errors.append(("state single", t, k))

    def state_batch(t):
        for k in range(3):
            items = [(bad, 0) if (j == t + k) else (good[j % 2], 1) for j in range(9)]
            got = m.lib.verify_state_batch([x[0][0] for x in items], [x[0][1] for x in items]).tolist()
            if got != [x[1] for x in items]: errors.append(("state batch", t, k, got))

    def account_single(t):
        for k in range(12):
            i = (5 * t + k) % len(pairs)
            if m.lib.verify_account(*pairs[i]) is not want_single[i]: errors.append(("account single", t, k))

    def account_batch(t):
        for k in range(4):
            idx = [(t + 3 * k + j) % len(pairs) for j in range(len(pairs) - 3)]
            got = m.lib.verify_account_batch([pairs[i][0] for i in idx], [pairs[i][1] for i in idx]).tolist()
            if got != [want_batch[i] for i in idx]: errors.append(("account batch", t, k, got))

    m.lib.verify_configure(base | m.lib.VERIFY_ACCOUNT_ON_DEVICE)
    try:
        th = [threading.Thread(target=f, args=(t,)) for t, f in enumerate([state_single, state_single, state_batch, state_batch, account_single, account_single, account_single, account_batch, account_batch])]
        for t in th: t.start()
        for t in th: t.join()
    finally:
        m.lib.verify_configure(base)
    assert not errors, errors[:3]
