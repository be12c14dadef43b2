"""Shared by tests/test_state_pack_abi.py (the device reader's text compiled for the host) and tests/test_state_pack_gpu.py (the kernels): serialized
protocol states and their deliberate mutations, proofs' state halves built per chain-selection branch, and the HOST reference for every output --
`mina_protocol_state_pack`, the `mina_consensus_*` entry points and hashlib's Blake2b.  The code under test is never its own reference."""
import copy
import hashlib
import random
import struct

import numpy as np

SLOTS, REC = 64, 64 * 32
STATES = 17
P = 0x40000000000000000000000000000000224698fc094cf91b992d30ed00000001          # the Pallas base field modulus
CHECK_FORMAT, CHECK_LEDGER, CHECK_CONSENSUS = 1, 2, 8


# ------------------------------------------------------------------------------------------------ writer (bincode of the serde derives), with marks
def bincode_state_marked(st):
    """-> (bytes, marks): marks["fields"] = offsets of the 40 field elements, ["strlens"] = of the four string lengths, ["m"] = of the density count.
    `failure_status_tbl` is written as it stands (rows of constructor tags)."""
    out = bytearray(); marks = {"fields": [], "strlens": [], "m": None}
    def big(v): marks["fields"].append(len(out)); out.extend(int(v).to_bytes(32, "little"))
    def u32(v): out.extend(struct.pack("<I", v))
    def u64(v): out.extend(struct.pack("<Q", v))
    def byts(b): marks["strlens"].append(len(out)); u64(len(b)); out.extend(b)
    def signed(a): u64(a["magnitude"]); u32(a["sgn"])
    def local(l):
        for k in ("stack_frame", "call_stack", "transaction_commitment", "full_transaction_commitment"): big(l[k])
        signed(l["excess"]); signed(l["supply_increase"]); big(l["ledger"]); out.append(int(l["success"])); u32(l["account_update_index"])
        u64(len(l["failure_status_tbl"]))
        for row in l["failure_status_tbl"]:
            u64(len(row))
            for tag in row: u32(tag)
        out.append(int(l["will_succeed"]))
    def regs(g):
        pc = g["pending_coinbase_stack"]
        big(g["first_pass_ledger"]); big(g["second_pass_ledger"]); big(pc["data"]); big(pc["state"]["init"]); big(pc["state"]["curr"]); local(g["local_state"])
    def epoch(e): big(e["ledger"]["hash"]); u64(e["ledger"]["total_currency"]); big(e["seed"]); big(e["start_checkpoint"]); big(e["lock_checkpoint"]); u32(e["epoch_length"])
    def pk(k): big(k["x"]); out.append(int(k["is_odd"]))
    b = st["body"]; bs, cs, kk = b["blockchain_state"], b["consensus_state"], b["constants"]
    ns, ps, fe = bs["staged_ledger_hash"]["non_snark"], bs["ledger_proof_statement"], bs["ledger_proof_statement"]["fee_excess"]
    big(st["previous_state_hash"]); big(b["genesis_state_hash"]); big(ns["ledger_hash"]); byts(ns["aux_hash"]); byts(ns["pending_coinbase_aux"])
    big(bs["staged_ledger_hash"]["pending_coinbase_hash"]); big(bs["genesis_ledger_hash"]); regs(ps["source"]); regs(ps["target"])
    big(ps["connecting_ledger_left"]); big(ps["connecting_ledger_right"]); signed(ps["supply_increase"])
    big(fe["fee_token_l"]); signed(fe["fee_excess_l"]); big(fe["fee_token_r"]); signed(fe["fee_excess_r"])
    u64(bs["timestamp"]); byts(bs["body_reference"])
    u32(cs["blockchain_length"]); u32(cs["epoch_count"]); u32(cs["min_window_density"]); marks["m"] = len(out); u64(len(cs["sub_window_densities"]))
    for x in cs["sub_window_densities"]: u32(x)
    byts(cs["last_vrf_output"]); u64(cs["total_currency"])
    u32(0); u32(cs["curr_global_slot_since_hard_fork"]["slot_number"]); u32(cs["curr_global_slot_since_hard_fork"]["slots_per_epoch"])
    u32(0); u32(cs["global_slot_since_genesis"]); epoch(cs["staking_epoch_data"]); epoch(cs["next_epoch_data"])
    out.append(int(cs["has_ancestor_in_same_checkpoint_window"])); pk(cs["block_stake_winner"]); pk(cs["block_creator"]); pk(cs["coinbase_receiver"])
    out.append(int(cs["supercharge_coinbase"]))
    u32(kk["k"]); u32(kk["slots_per_epoch"]); u32(kk["slots_per_sub_window"]); u32(kk["grace_period_slots"]); u32(kk["delta"]); u64(kk["genesis_state_timestamp"])
    assert len(marks["fields"]) == 40 and len(marks["strlens"]) == 4
    return bytes(out), marks


def bincode_state(st):
    return bincode_state_marked(st)[0]


def synth(seed, height=1000, n_sub_windows=11):
    from oracle import mina_state_ref as S, state_job_ref as J
    rng = random.Random(seed)
    return J.synth_state(rng, rng.randrange(S.P), height, n_sub_windows)


def well_formed_states():
    """(name, state dict): synthetic chains, 1 / 11 / 16 / 64 (and 0) sub-windows, non-empty failure-status tables, the reference's own tip state re-encoded"""
    import base64, json, os
    from ipa_helpers import poseidon_pp
    from kimchi_helpers import make_chain
    from oracle import mina_state_ref as S
    out = []
    states, _ = make_chain(random.Random(77), poseidon_pp(0))
    out += [(f"chain[{i}]", s) for i, s in enumerate(states)]
    for m in (0, 1, 11, 16, 64):
        out.append((f"sub_windows={m}", synth(500 + m, 2000 + m, m)))
    t = synth(901); t["body"]["blockchain_state"]["ledger_proof_statement"]["source"]["local_state"]["failure_status_tbl"] = [[1, 2], [], [3]]
    t["body"]["blockchain_state"]["ledger_proof_statement"]["target"]["local_state"]["failure_status_tbl"] = [[], [7] * 9]
    out.append(("failure tables", t))
    edge = synth(902)                                                # the largest canonical element, zero, extreme scalars
    edge["previous_state_hash"] = P - 1; edge["body"]["genesis_state_hash"] = 0
    edge["body"]["blockchain_state"]["timestamp"] = (1 << 64) - 1; edge["body"]["consensus_state"]["total_currency"] = (1 << 64) - 1
    edge["body"]["consensus_state"]["sub_window_densities"] = [0xffffffff] * 11
    out.append(("edge values", edge))
    fx = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tip_protocol_state.json")))
    out.append(("reference tip state", S.parse_protocol_state(base64.b64decode(fx["protocol_state_base64"]))))
    return out


def mutations(st):
    """(name, bytes) for ONE state: every truncation, a trailing byte, one flipped bit at every byte position, a non-canonical element in each of the 40
    positions, every string length 31 and 33 (the length alone, and with the string really that long), 65 sub-windows (likewise)"""
    raw, mk = bincode_state_marked(st)
    out = [("intact", raw)]
    out += [(f"truncated to {k}", raw[:k]) for k in range(len(raw))]
    out.append(("trailing byte", raw + b"\0"))
    for pos in range(len(raw)):
        b = bytearray(raw); b[pos] ^= 1 << (pos % 8); out.append((f"bit flipped at {pos}", bytes(b)))
    for i, at in enumerate(mk["fields"]):
        for name, v in (("p", P), ("2^255", 1 << 255), ("p - 1", P - 1)):
            b = bytearray(raw); b[at:at + 32] = v.to_bytes(32, "little"); out.append((f"field {i} = {name}", bytes(b)))
    for i, at in enumerate(mk["strlens"]):
        for n in (31, 33):
            b = bytearray(raw); b[at:at + 8] = struct.pack("<Q", n); out.append((f"string {i}: length {n}, bytes kept", bytes(b)))
            b = bytearray(raw); b[at:at + 40] = struct.pack("<Q", n) + (bytes(raw[at + 8:at + 40]) + b"\x55")[:n]; out.append((f"string {i}: {n} bytes", bytes(b)))
    b = bytearray(raw); b[mk["m"]:mk["m"] + 8] = struct.pack("<Q", 65); out.append(("m = 65, bytes kept", bytes(b)))
    st65 = copy.deepcopy(st); st65["body"]["consensus_state"]["sub_window_densities"] = [3] * 65; out.append(("65 sub-windows", bincode_state(st65)))
    b = bytearray(raw); b[mk["m"]:mk["m"] + 8] = struct.pack("<Q", (1 << 64) - 1); out.append(("m = 2^64 - 1", bytes(b)))
    return out


# ------------------------------------------------------------------------------------------------ the host reference
def host_pack(m, data):
    """mina_protocol_state_pack (bincode, the slice filled exactly) -> None if rejected, else (record bytes, n_body_fields, info bytes)"""
    import ctypes
    try:
        rec, nf, info, _ = m.lib.protocol_state_pack(data, m.lib.ENC_BINCODE)
    except m.MinaError:
        return None
    return rec.tobytes(), int(nf), bytes(ctypes.string_at(ctypes.addressof(info), ctypes.sizeof(info)))


def info_size(m):
    import ctypes
    return ctypes.sizeof(m.lib.ProtocolStateInfo)


def blob_of(cases, pad=3):
    """cases one behind the other at odd offsets (`pad` bytes of filler before each) -> (blob, off u64[], len u32[])"""
    blob = bytearray(); off, ln = [], []
    for _, data in cases:
        blob.extend(b"\xee" * pad); off.append(len(blob)); ln.append(len(data)); blob.extend(data)
    blob.extend(b"\xee" * 5)
    return bytes(blob), np.array(off, np.uint64), np.array(ln, np.uint32)


def check_pack_results(m, cases, status, nf, recs, infos):
    """every case against the host: status = accept / reject; where accepted, record, field count and info struct byte for byte; where rejected a zero record.
    Returns (accepted, rejected)."""
    acc = rej = 0
    for i, (name, data) in enumerate(cases):
        want = host_pack(m, data)
        assert int(status[i]) == (0 if want is None else 1), (name, int(status[i]))
        if want is None:
            rej += 1
            assert int(nf[i]) == 0 and not recs[i].any(), name
            continue
        acc += 1
        assert int(nf[i]) == want[1], (name, int(nf[i]), want[1])
        assert recs[i].tobytes() == want[0], (name, "record", int(np.flatnonzero(recs[i] != np.frombuffer(want[0], np.uint8))[0]) // 32)
        assert infos[i].tobytes() == want[2], (name, "info", int(np.flatnonzero(infos[i] != np.frombuffer(want[2], np.uint8))[0]))
    return acc, rej


def host_frontend(m, states_bytes, expected, ledger, and_bits):
    """what api_verify.hip parse_states_half does for ONE proof, from the host entry points: (records[17*REC] bytes, nf[17], precheck, mask, branch)
    `branch` names the chain-selection path taken (for the tests' class counts)"""
    import ctypes
    recs, nfs, infos, vrfs = [], [], [], []
    pos, ok = 0, True
    for _ in range(STATES):
        try:
            rec, nf, info, used = m.lib.protocol_state_pack(states_bytes[pos:], m.lib.ENC_BINCODE, exact=False)
        except m.MinaError:
            ok = False; break
        recs.append(rec.tobytes()); nfs.append(int(nf)); infos.append(info); pos += used
    if not ok or pos != len(states_bytes):
        return bytes(STATES * REC), [0] * STATES, 0, 0, "malformed"
    led = all(bytes(infos[i].snarked_ledger_hash) == ledger[32 * i:32 * i + 32] for i in range(16))
    tip, cand = infos[16].consensus, infos[15].consensus
    for st_, h in ((tip, expected[16 * 32:17 * 32]), (cand, expected[15 * 32:16 * 32])):
        dg = hashlib.blake2b(bytes(st_.last_vrf_output_hash), digest_size=32).digest()
        ctypes.memmove(st_.last_vrf_output_hash, dg, 32); ctypes.memmove(st_.state_hash, h, 32)
    params = m.lib.ConsensusParams(infos[15].slots_per_sub_window, infos[15].sub_windows_per_window)
    cons, branch = False, "bad parameters"
    if infos[16].sub_windows_per_window == params.sub_windows_per_window and 1 <= params.sub_windows_per_window <= 16 and params.slots_per_sub_window >= 1:
        cons = m.lib.consensus_select_secure_chain(tip, cand, params)
        if m.lib.consensus_is_short_range(cand, tip):
            branch = "short/same epoch" if tip.epoch_count == cand.epoch_count else "short/adjacent epochs"
            if tip.blockchain_length == cand.blockchain_length:
                branch = "tie/vrf" if bytes(tip.last_vrf_output_hash) != bytes(cand.last_vrf_output_hash) else "tie/state hash"
        else:
            td = m.lib.consensus_relative_min_window_density(tip, cand, params); cd = m.lib.consensus_relative_min_window_density(cand, tip, params)
            branch = "long/candidate denser" if cd > td else ("long/equal density" if cd == td else "long/candidate sparser")
    elif infos[16].sub_windows_per_window != params.sub_windows_per_window:
        branch = "mismatched sub-window counts"
    elif params.slots_per_sub_window == 0:
        branch = "slots_per_sub_window = 0"
    mask = CHECK_FORMAT | (CHECK_LEDGER if led else 0) | (CHECK_CONSENSUS if cons else 0)
    return b"".join(recs), nfs, 1 if (led and cons and and_bits) else 0, mask, branch + ("/selected" if cons else "/kept")


def precheck_proofs():
    """(name, states bytes, expected hashes 17*32, ledger hashes 16*32, and byte): one proof per chain-selection branch, one wrong ledger hash in each of the 16
    positions, the and byte cleared, malformed state halves.  State hashes are arbitrary labels here (the pre-check only compares them)."""
    from oracle import mina_state_ref as S
    rng = random.Random(4242)
    base = [synth(3000 + i, 1000 + i) for i in range(STATES)]

    def proof(name, cand_edit=None, tip_edit=None, exp_edit=None, ledger_edit=None, and_byte=1, bytes_edit=None):
        sts = copy.deepcopy(base)
        lock = 12345678901234567890
        for s_, length in ((sts[15], 1015), (sts[16], 990)):          # default: short range, same epoch, candidate longer
            cs = s_["body"]["consensus_state"]
            cs["epoch_count"] = 7; cs["staking_epoch_data"]["lock_checkpoint"] = lock; cs["blockchain_length"] = length
        if cand_edit: cand_edit(sts[15])
        if tip_edit: tip_edit(sts[16])
        data = b"".join(bincode_state(s_) for s_ in sts)
        if bytes_edit: data = bytes_edit(data)
        exp = bytearray(b"".join(hashlib.sha256(b"label %d" % i).digest() for i in range(STATES)))
        if exp_edit: exp_edit(exp)
        led = bytearray(b"".join(int(S.snarked_ledger_hash(s_)).to_bytes(32, "little") for s_ in sts[:16]))
        if ledger_edit: ledger_edit(led)
        return (name, data, bytes(exp), bytes(led), and_byte)

    cs = lambda s_: s_["body"]["consensus_state"]
    def setc(**kw):
        def f(s_):
            for k, v in kw.items():
                if k == "staking_lock": cs(s_)["staking_epoch_data"]["lock_checkpoint"] = v
                elif k == "next_lock": cs(s_)["next_epoch_data"]["lock_checkpoint"] = v
                elif k == "slot": cs(s_)["curr_global_slot_since_hard_fork"]["slot_number"] = v
                elif k == "spsw": s_["body"]["constants"]["slots_per_sub_window"] = v
                else: cs(s_)[k] = v
        return f
    out = [proof("short, same epoch, candidate longer"), proof("short, same epoch, candidate shorter", cand_edit=setc(blockchain_length=900))]
    # adjacent epochs: the later block's staking lock checkpoint is the earlier block's next-epoch one
    out.append(proof("short, candidate one epoch ahead", cand_edit=setc(epoch_count=8, staking_lock=777), tip_edit=setc(next_lock=777)))
    out.append(proof("short, tip one epoch ahead, candidate shorter", cand_edit=setc(next_lock=888, blockchain_length=5), tip_edit=setc(epoch_count=8, staking_lock=888)))
    out.append(proof("two epochs apart: long range", cand_edit=setc(epoch_count=9)))
    # long range: different staking lock checkpoints in the same epoch; densities decide
    win = lambda d: dict(sub_window_densities=[d] * 11, slot=11 * 7 * 50 + 3)
    out.append(proof("long, candidate denser", cand_edit=setc(staking_lock=1, min_window_density=60, **win(7)), tip_edit=setc(min_window_density=20, **win(7))))
    out.append(proof("long, candidate sparser", cand_edit=setc(staking_lock=1, min_window_density=10, **win(7)), tip_edit=setc(min_window_density=20, **win(7))))
    out.append(proof("long, equal density, candidate longer", cand_edit=setc(staking_lock=1, min_window_density=20, **win(7)), tip_edit=setc(min_window_density=20, **win(7))))
    out.append(proof("long, equal density, candidate shorter", cand_edit=setc(staking_lock=1, min_window_density=20, blockchain_length=3, **win(7)), tip_edit=setc(min_window_density=20, **win(7))))
    # long range with the windows projected: the tip is many sub-windows behind, its window is partly / wholly zeroed
    for gap in (2, 5, 11, 40):
        out.append(proof(f"long, tip {gap} sub-windows behind", cand_edit=setc(staking_lock=1, min_window_density=30, sub_window_densities=list(range(1, 12)), slot=7 * (300 + gap) + 2),
                         tip_edit=setc(min_window_density=30, sub_window_densities=list(range(11, 0, -1)), slot=7 * 300 + 6)))
        out.append(proof(f"long, candidate {gap} sub-windows behind", cand_edit=setc(staking_lock=1, min_window_density=30, sub_window_densities=list(range(1, 12)), slot=7 * 300),
                         tip_edit=setc(min_window_density=30, sub_window_densities=list(range(11, 0, -1)), slot=7 * (300 + gap) + 1)))
    # length ties
    vrf_hi, vrf_lo = None, None
    a, b = rng.randbytes(32), rng.randbytes(32)
    if hashlib.blake2b(a, digest_size=32).digest() < hashlib.blake2b(b, digest_size=32).digest(): a, b = b, a      # blake2b(a) > blake2b(b)
    out.append(proof("length tie, candidate VRF hash greater", cand_edit=setc(blockchain_length=990, last_vrf_output=a), tip_edit=setc(last_vrf_output=b)))
    out.append(proof("length tie, candidate VRF hash smaller", cand_edit=setc(blockchain_length=990, last_vrf_output=b), tip_edit=setc(last_vrf_output=a)))
    def hashes(c15, t16):
        def f(exp): exp[15 * 32:16 * 32] = c15; exp[16 * 32:17 * 32] = t16
        return f
    out.append(proof("length and VRF tie, candidate state hash greater", cand_edit=setc(blockchain_length=990, last_vrf_output=a), tip_edit=setc(last_vrf_output=a), exp_edit=hashes(b"\x90" * 32, b"\x8f" * 32)))
    out.append(proof("length and VRF tie, candidate state hash smaller", cand_edit=setc(blockchain_length=990, last_vrf_output=a), tip_edit=setc(last_vrf_output=a), exp_edit=hashes(b"\x8f" * 32, b"\x90" * 32)))
    out.append(proof("everything tied", cand_edit=setc(blockchain_length=990, last_vrf_output=a), tip_edit=setc(last_vrf_output=a), exp_edit=hashes(b"\x90" * 32, b"\x90" * 32)))
    # parameters
    out.append(proof("mismatched sub-window counts", cand_edit=setc(sub_window_densities=[2] * 11), tip_edit=setc(sub_window_densities=[2] * 10)))
    out.append(proof("slots_per_sub_window = 0, short range", cand_edit=setc(spsw=0)))
    out.append(proof("slots_per_sub_window = 0, long range", cand_edit=setc(spsw=0, staking_lock=1)))
    out.append(proof("64 sub-windows", cand_edit=setc(sub_window_densities=[2] * 64), tip_edit=setc(sub_window_densities=[2] * 64)))
    out.append(proof("no sub-window", cand_edit=setc(sub_window_densities=[]), tip_edit=setc(sub_window_densities=[])))
    out.append(proof("16 sub-windows, long range", cand_edit=setc(staking_lock=1, min_window_density=99, sub_window_densities=[5] * 16, slot=16 * 7 * 9), tip_edit=setc(min_window_density=99, sub_window_densities=[4] * 16, slot=16 * 7 * 9 + 40)))
    out.append(proof("1 sub-window, long range", cand_edit=setc(staking_lock=1, sub_window_densities=[5]), tip_edit=setc(sub_window_densities=[4])))
    # ledger hashes
    for i in range(16):
        def wrong(led, i=i): led[32 * i + (i % 32)] ^= 0x40
        out.append(proof(f"wrong ledger hash {i}", ledger_edit=wrong))
    out.append(proof("host-side bits cleared", and_byte=0))
    # malformed state halves
    out.append(proof("truncated by a byte", bytes_edit=lambda d: d[:-1]))
    out.append(proof("trailing byte", bytes_edit=lambda d: d + b"\0"))
    out.append(proof("cut inside state 9", bytes_edit=lambda d: d[:len(d) // 2]))
    out.append(proof("empty", bytes_edit=lambda d: b""))
    def noncanon(d):
        _, mk = bincode_state_marked(base[0]); d = bytearray(d); at = len(bincode_state(base[0])) * 3 + mk["fields"][20]; d[at:at + 32] = P.to_bytes(32, "little"); return bytes(d)
    out.append(proof("non-canonical element in state 3", bytes_edit=noncanon))
    def boolean2(d): d = bytearray(d); d[-29] = 2; return bytes(d)          # supercharge_coinbase of the bridge tip state
    out.append(proof("boolean 2 in the last state", bytes_edit=boolean2))
    return out


def well_formed_proof(seed=5100):
    """the state half of ONE well-formed proof, built as precheck_proofs builds its default one (short range, same epoch, candidate longer: FORMAT and CONSENSUS
    pass): -> (the 17 state dicts, states bytes, expected hashes 17*32 -- labels, the pre-check only compares them --, the 16 snarked ledger hashes 16*32)"""
    from oracle import mina_state_ref as S
    sts = [synth(seed + i, 1000 + i) for i in range(STATES)]
    for s_, length in ((sts[15], 1015), (sts[16], 990)):
        cs = s_["body"]["consensus_state"]
        cs["epoch_count"] = 7; cs["staking_epoch_data"]["lock_checkpoint"] = 12345678901234567890; cs["blockchain_length"] = length
    data = b"".join(bincode_state(s_) for s_ in sts)
    exp = b"".join(hashlib.sha256(b"label %d" % i).digest() for i in range(STATES))
    led = b"".join(int(S.snarked_ledger_hash(s_)).to_bytes(32, "little") for s_ in sts[:16])
    return sts, data, exp, led


def frontend_inputs(proofs, pad=5):
    """-> blob, begin u64[], end u64[], expected bytes, ledger bytes, and u8[]"""
    blob = bytearray(); begin, end = [], []
    for _, data, _, _, _ in proofs:
        blob.extend(b"\xdd" * pad); begin.append(len(blob)); blob.extend(data); end.append(len(blob))
    blob.extend(b"\xdd" * 3)
    return (bytes(blob), np.array(begin, np.uint64), np.array(end, np.uint64), b"".join(p[2] for p in proofs), b"".join(p[3] for p in proofs),
            np.array([p[4] for p in proofs], np.uint8))


def check_frontend_results(m, proofs, recs, nf, pre, masks):
    """device outputs of a batch against host_frontend; returns the branch names met"""
    branches = []
    for b, (name, data, exp, led, and_byte) in enumerate(proofs):
        wrec, wnf, wpre, wmask, branch = host_frontend(m, data, exp, led, and_byte)
        branches.append(branch)
        assert int(masks[b]) == wmask, (name, branch, int(masks[b]), wmask)
        assert int(pre[b]) == wpre, (name, branch, int(pre[b]), wpre)
        assert [int(x) for x in nf[b * STATES:(b + 1) * STATES]] == wnf, name
        assert recs[b * STATES * REC:(b + 1) * STATES * REC].tobytes() == wrec, (name, "records")
    return branches


REQUIRED_BRANCHES = ["short/same epoch/selected", "short/same epoch/kept", "short/adjacent epochs/selected", "short/adjacent epochs/kept",
                     "long/candidate denser/selected", "long/equal density/selected", "long/equal density/kept", "long/candidate sparser/kept",
                     "tie/vrf/selected", "tie/vrf/kept", "tie/state hash/selected", "tie/state hash/kept",
                     "mismatched sub-window counts/kept", "slots_per_sub_window = 0/kept", "malformed"]
