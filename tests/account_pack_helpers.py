"""Shared by tests/test_account_pack_abi.py (the device reader's text compiled for the host) and tests/test_account_job_gpu.py (the kernels): Proof-of-Account
pairs from the oracle's writers (oracle/mina_account_ref.py synth_account, write_account, write_account_proof, abi_encode_account), seeded; their deliberate
mutations; and the HOST reference for every output -- mina_parse_merkle_path, mina_parse_account_pub_inputs, mina_account_abi_encode, and on the GPU tier
mina_verify_account_ctx, mina_account_hash_batch and mina_merkle_roots.  The code under test is never its own reference."""
import random
import struct

import numpy as np

from oracle import mina_account_ref as A, mina_state_ref as S

SLOTS, REC = 64, 64 * 32
MAXD = 64
P = A.P
CHECK_FORMAT, CHECK_ACCOUNT_ABI, CHECK_MERKLE = 1, 64, 128
AB_PATH, AB_PUB, AB_ACCOUNT = 0x100, 0x200, 0x400
STAGE_URI, STAGE_VK, STAGE_ZKAPP, STAGE_ACCOUNT = 0, 1, 2, 3
PREFIX_OF_STAGE = {STAGE_URI: "MinaZkappUri", STAGE_VK: "MinaSideLoadedVk", STAGE_ZKAPP: "MinaZkappAccount", STAGE_ACCOUNT: "MinaAccount"}
SALT_OF_STAGE = {STAGE_URI: 4, STAGE_VK: 5, STAGE_ZKAPP: 3, STAGE_ACCOUNT: 2}          # ctx.h MB_SALT_*
PATCHED = {STAGE_URI: (), STAGE_VK: (), STAGE_ZKAPP: (0, 6), STAGE_ACCOUNT: (0,)}      # slots that hold a hash of an earlier stage: zero in the front end's record
DEPTHS = (0, 1, 35, 64)
SEED = 20261017


# ------------------------------------------------------------------------------------------------ cases
def accounts(seed=SEED):
    """-> [(name, account)]: every combination of {no zkApp, zkApp with key, zkApp without key} x {untimed, timed} x {no delegate, delegate}, twice over, with symbol
    lengths 0 / 6 / whatever the generator drew and URI lengths 0, 31, 32, 255 (any byte value) going round"""
    rng = random.Random(seed)
    out, nz = [], 0
    for rep in range(2):
        for zk, vk in ((False, True), (True, True), (True, False)):
            for timed in (False, True):
                for deleg in (False, True):
                    a = A.synth_account(rng, zk, timed, deleg, with_vk=vk)
                    k = len(out) % 3
                    if k == 0: a["token_symbol"] = b""
                    if k == 1: a["token_symbol"] = bytes(rng.randrange(1, 256) for _ in range(6))
                    if zk:
                        a["zkapp"]["zkapp_uri"] = bytes(rng.randrange(256) for _ in range((0, 31, 32, 255)[nz % 4])); nz += 1
                    out.append(("%s%s%s sym%d%s" % ("zkapp" + ("+vk" if vk else "-vk") if zk else "plain", " timed" if timed else "", " delegate" if deleg else "",
                                                     len(a["token_symbol"]), " uri%d" % len(a["zkapp"]["zkapp_uri"]) if zk else ""), a))
    assert {len(a["token_symbol"]) for _, a in out} >= {0, 6} and {len(a["zkapp"]["zkapp_uri"]) for _, a in out if a["zkapp"]} == {0, 31, 32, 255}
    return out


def random_path(rng, depth):
    return [(rng.randrange(2), rng.randrange(P)) for _ in range(depth)]


def pub_input(ledger: int, enc: bytes) -> bytes:
    return int(ledger).to_bytes(32, "little") + struct.pack("<Q", len(enc)) + enc


def well_formed_pairs(seed=SEED, ledger_of=None):
    """-> [(name, proof, pub, account, path)]: the accounts above, depths 0 / 1 / 35 / 64 going round.  ledger_of(account, path) -> the ledger hash to write (default:
    a random canonical element: the readers do not care)"""
    rng = random.Random(seed + 1)
    out = []
    for i, (name, a) in enumerate(accounts(seed)):
        path = random_path(rng, DEPTHS[(i + i // 4) % 4])
        ledger = ledger_of(a, path) if ledger_of else rng.randrange(P)
        out.append(("%s depth%d" % (name, len(path)), A.write_account_proof(path, a), pub_input(ledger, A.abi_encode_account(a)), a, path))
    assert {len(c[4]) for c in out} == set(DEPTHS)
    return out


def well_formed_pairs_at(depths, ledger_of, seed=SEED):
    """-> [(name, proof, pub, account, path)] as well_formed_pairs, pair i behind a random path of depths[i]: the accounts above going round.
    ledger_of(account, path) -> the ledger hash to write (tests/test_gpu_account_forms.py: the CPU model of the fold over the oracle's account hash)"""
    rng = random.Random(seed + 2)
    accts = accounts(seed)
    out = []
    for i, depth in enumerate(depths):
        name, a = accts[i % len(accts)]
        path = random_path(rng, depth)
        out.append(("%s depth%d" % (name, depth), A.write_account_proof(path, a), pub_input(ledger_of(a, path), A.abi_encode_account(a)), a, path))
    return out


def sweep_values(x):
    return sorted({x ^ 0x01, x ^ 0x80, 0xff} - {x})


def proof_mutations(proof: bytes):
    """the proof itself, every truncation, one trailing byte, and every byte position with several replacement values"""
    out = [("as it is", proof), ("one byte more", proof + b"\0")]
    out += [("cut to %d" % k, proof[:k]) for k in range(len(proof))]
    for at in range(len(proof)):
        for v in sweep_values(proof[at]):
            out.append(("byte %d = %02x" % (at, v), proof[:at] + bytes([v]) + proof[at + 1:]))
    return out


def blob_of(pairs, lead=3):
    """pairs [(proof, pub)] -> blob, and u64 arrays proof_off, proof_len, pub_off, pub_len.  Equal byte strings share their place in the blob (a sweep keeps one side
    fixed); `lead` odd bytes in front so that nothing is aligned."""
    parts, at, seen = [b"\xa5" * lead], lead, {}
    cols = [[], [], [], []]
    for proof, pub in pairs:
        for j, b in enumerate((proof, pub)):
            if b not in seen:
                seen[b] = at; parts.append(b); at += len(b)
            cols[2 * j].append(seen[b]); cols[2 * j + 1].append(len(b))
    return (b"".join(parts),) + tuple(np.array(c, np.uint64) for c in cols)


# ------------------------------------------------------------------------------------------------ references
def oracle_inputs(a, pp):
    """the oracle's account hash and the `to_input` field lists it hashes on the way, by prefix"""
    got, real = {}, S.hash_with_kimchi
    def spy(prefix, xs, pp_):
        got[prefix] = [int(x) for x in xs]
        return real(prefix, xs, pp_)
    S.hash_with_kimchi = spy
    try:
        h = A.account_hash(a, pp)
    finally:
        S.hash_with_kimchi = real
    return got, h


def host_reference(m, proof: bytes, pub: bytes):
    """what the host path's three readers say about one pair -> dict(path, pub, account: accepted?; depth, sib, dirs, ledger, abi: as far as they got; format, abi_ok)"""
    r = dict(path=False, pub=False, account=False, abi_ok=False, depth=0, sib=None, dirs=None, ledger=bytes(32), acc_off=None)
    try:
        sib, dirs, off = m.lib.parse_merkle_path(proof, MAXD)
        r.update(path=True, depth=len(dirs), sib=sib, dirs=dirs, acc_off=off)
    except m.lib.MinaError:
        pass
    enc = None
    try:
        ledger, enc = m.lib.parse_account_pub_inputs(pub)
        r.update(pub=True, ledger=ledger)
    except m.lib.MinaError:
        pass
    if r["path"]:
        try:
            mine = m.lib.account_abi_encode(proof[r["acc_off"]:], m.lib.ENC_BINCODE)
            r["account"] = True
            r["abi_ok"] = enc is not None and mine == enc
        except m.lib.MinaError:
            pass
    r["format"] = r["path"] and r["pub"] and r["account"]
    return r


def unpack_frontend(raw: dict, n: int):
    """byte arrays of the front end's outputs (by name) -> typed views"""
    u32 = lambda k: np.frombuffer(bytes(raw[k]), np.uint32)
    return dict(records=np.frombuffer(bytes(raw["records"]), np.uint8).reshape(4 * n, REC), nfields=u32("nfields"), salt_idx=u32("salt_idx"),
                siblings=np.frombuffer(bytes(raw["siblings"]), np.uint8).reshape(n, MAXD, 32), dirs=np.frombuffer(bytes(raw["dirs"]), np.uint8).reshape(n, MAXD),
                depths=u32("depths"), ledger=np.frombuffer(bytes(raw["ledger"]), np.uint8).reshape(n, 32), marks=u32("marks"), zk_index=u32("zk_index"),
                zk_count=int(u32("zk_count")[0]), bits=u32("bits"))


FRONTEND_SIZES = (("records", lambda n: 4 * n * REC), ("nfields", lambda n: 16 * n), ("salt_idx", lambda n: 16 * n), ("siblings", lambda n: n * MAXD * 32), ("dirs", lambda n: n * MAXD),
                  ("depths", lambda n: 4 * n), ("ledger", lambda n: 32 * n), ("marks", lambda n: 4 * n), ("zk_index", lambda n: 4 * n), ("zk_count", lambda n: 4), ("bits", lambda n: 4 * n))


def check_frontend(m, pairs, f):
    """pairs [(name, proof, pub)], f = unpack_frontend(...): every output against host_reference.  -> (refs, classes) with the class of each pair:
    'format fails' / 'abi fails' / 'abi passes' (FORMAT passed in the last two)"""
    n = len(pairs)
    refs, classes = [], []
    slots = {int(f["zk_index"][s]): s for s in range(f["zk_count"])}
    assert len(slots) == f["zk_count"] <= n, "a pair took two slots of the compacted list"
    for i, (name, proof, pub) in enumerate(pairs):
        r = host_reference(m, proof, pub); refs.append(r)
        b = int(f["bits"][i])
        want = (CHECK_FORMAT if r["format"] else 0) | (CHECK_ACCOUNT_ABI if r["format"] and r["abi_ok"] else 0) | (AB_PATH if r["path"] else 0) | (AB_PUB if r["pub"] else 0)
        got = b & ~AB_ACCOUNT if not r["path"] else b                # the account reader's own bit means nothing behind a path that did not parse
        if r["path"] and r["account"]: want |= AB_ACCOUNT
        assert got == want, (name, hex(b), hex(want))
        assert int(f["depths"][i]) == r["depth"], name
        if r["path"]:
            assert (f["siblings"][i, :r["depth"]] == r["sib"]).all() and (f["dirs"][i, :r["depth"]] == r["dirs"]).all(), name
        assert f["ledger"][i].tobytes() == (r["ledger"] if r["pub"] else bytes(32)), name
        if not r["format"]:
            assert int(f["nfields"][STAGE_ACCOUNT * n + i]) == 0 and int(f["marks"][i]) == 0, name
            if i in slots:
                assert all(int(f["nfields"][s * n + slots[i]]) == 0 for s in (STAGE_URI, STAGE_VK, STAGE_ZKAPP)), name
        else:
            assert (int(f["marks"][i]) == 1) == (i in slots), name
        classes.append("format fails" if not r["format"] else ("abi passes" if r["abi_ok"] else "abi fails"))
    return refs, classes


def check_records(pairs, f, pp):
    """well-formed pairs [(name, proof, pub, account, path)]: the front end's records, field counts and salt indices against the oracle's `to_input` fields"""
    n = len(pairs)
    slots = {int(f["zk_index"][s]): s for s in range(f["zk_count"])}
    hashes = []
    for i, (name, _, _, a, _) in enumerate(pairs):
        want, h = oracle_inputs(a, pp); hashes.append(h)
        assert (a["zkapp"] is not None) == (i in slots) == bool(f["marks"][i]), name
        for stage in ((STAGE_URI, STAGE_VK, STAGE_ZKAPP, STAGE_ACCOUNT) if i in slots else (STAGE_ACCOUNT,)):
            e = stage * n + (i if stage == STAGE_ACCOUNT else slots[i])
            fields = want[PREFIX_OF_STAGE[stage]]
            assert int(f["nfields"][e]) == len(fields) <= SLOTS and int(f["salt_idx"][e]) == SALT_OF_STAGE[stage], (name, stage, int(f["nfields"][e]), len(fields))
            rec = f["records"][e]
            for j, x in enumerate(fields):
                got = int.from_bytes(rec[32 * j:32 * j + 32].tobytes(), "little")
                assert got == (0 if j in PATCHED[stage] else x), (name, stage, j)
    return hashes
