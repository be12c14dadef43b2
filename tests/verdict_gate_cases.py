"""Case tables and plain models for the kernels that turn arithmetic into a verdict (CPU only; nothing here touches a GPU path):

  the chain gate   api_state.hip pstate_chain_check_kernel / pstate_chain_detail_kernel: 17 x 8 hash words against the expected hashes, and record slot 0 of states
                   1 .. 15 against the hash of the state before
  the ledger gate  state_pack.cuh pstate_precheck_entry and its host twin api_verify.hip parse_states_half: four 64-bit words per ledger position
  the sg gate      api_ipa.hip xyzz_eq_affine_kernel / xyzz_compare_kernel / xyzz_compare_parts_kernel behind the accumulator check

Every table changes ONE thing per proof, so that a comparison that skips a state, a word or a coordinate lets exactly the proofs through that name it.  The models
are word equality written out in Python; their weakened forms (the keyword arguments) are the bugs tests/test_verdict_gate_cases.py shows the tables to catch.
tests/test_gpu_verdict_gates.py takes every expectation from the models."""
import functools
import random

import numpy as np

P = 0x40000000000000000000000000000000224698FC094CF91B992D30ED00000001          # Pallas base field: protocol-state hashes live here
Q = 0x40000000000000000000000000000000224698FC0994A8DD8C46EB2100000001          # Vesta base field
SLOTS, STATES, NFIELDS = 64, 17, 3
FORMAT, LEDGER, CONSENSUS = 1, 2, 8
CLEAN_EVERY = 7


def word(v, i):
    return (v >> (32 * i)) & 0xFFFFFFFF


def interleave(variants, clean):
    """the variants in order with a clean proof after every CLEAN_EVERY of them, and one at the end"""
    out = []
    for n, v in enumerate(variants):
        out.append(v)
        if (n + 1) % CLEAN_EVERY == 0:
            out.append(clean)
    if out[-1] is not clean:
        out.append(clean)
    return out


# ------------------------------------------------------------------------------------------------ the chain gate
@functools.lru_cache(maxsize=None)
def _sponge():
    """the two salts and the CPU oracle's permutation, as tests/test_gpu_state_hash_one_lane.py _oracle_hashes uses them"""
    import mina_bridge_amd.poseidon_params as PP
    from oracle import mina_state_ref as S, oracle as O
    from state_job_helpers import pp_fp
    pp = pp_fp(); params = PP.default_params_bytes(0)
    salts = (S.salt(S.PREFIX_PROTOCOL_STATE_BODY, pp), S.salt(S.PREFIX_PROTOCOL_STATE, pp))
    perm = lambda st: [int.from_bytes(x.tobytes(), "little") for x in O.poseidon_permute(0, params, O.ints_to_le(st).reshape(1, 96)).reshape(3, 32)]
    return salts, perm


@functools.lru_cache(maxsize=None)
def body_hash(fields):
    """H_"MinaProtoStateBody"(fields) for a tuple of 3 elements: two blocks of two"""
    (salt, _), perm = _sponge()
    assert len(fields) == NFIELDS
    st = list(salt)
    st[0] = (st[0] + fields[0]) % P; st[1] = (st[1] + fields[1]) % P
    st = perm(st)
    st[0] = (st[0] + fields[2]) % P
    return perm(st)[0]


@functools.lru_cache(maxsize=None)
def state_hash(slot0, fields):
    """H_"MinaProtoState"(slot 0, body hash).  Slot 0 is ADDED to the salt mod p, so a word that is no canonical element hashes as its residue"""
    (_, salt), perm = _sponge()
    return perm([(salt[0] + slot0) % P, (salt[1] + body_hash(fields)) % P, salt[2]])[0]


class ChainCase:
    """one proof of the chain table: slot 0 and the 3 body fields of its 17 records, its 17 expected hashes, its precheck byte"""
    def __init__(self, name, cls, slot0, body, expected, precheck=1, key=None):
        self.name, self.cls, self.slot0, self.body, self.expected, self.precheck = name, cls, tuple(slot0), tuple(body), tuple(expected), precheck
        self.key = key                                                   # (state, word) of an E or L proof

    def hashes(self):
        """the 17 state hashes of the records by the CPU oracle's permutation"""
        return [state_hash(self.slot0[s], self.body[s]) for s in range(STATES)]

    def edit(self, name, cls, slot0=None, body=None, expected=None, precheck=None, key=None):
        return ChainCase(name, cls, self.slot0 if slot0 is None else slot0, self.body if body is None else body, self.expected if expected is None else expected,
                         self.precheck if precheck is None else precheck, self.key if key is None else key)

    def records(self):
        rec = np.zeros((STATES, SLOTS * 32), np.uint8)
        for s in range(STATES):
            b = self.slot0[s].to_bytes(32, "little") + b"".join(f.to_bytes(32, "little") for f in self.body[s])
            rec[s, :len(b)] = np.frombuffer(b, np.uint8)
        return rec


def relinked(slot0, body, start):
    """slot 0 of states start .. 15 set to the hash of the state before"""
    slot0 = list(slot0)
    for s in range(max(start, 1), STATES - 1):
        slot0[s] = state_hash(slot0[s - 1], body[s - 1])
    return slot0


def _with_own_hashes(case):
    return case.edit(case.name, case.cls, expected=case.hashes())


@functools.lru_cache(maxsize=None)
def chain_table(seed=20261021):
    """-> the proofs of ONE batch: every variant, a clean proof after every 7"""
    rng = random.Random(seed)
    body = tuple(tuple(rng.randrange(P) for _ in range(NFIELDS)) for _ in range(STATES))
    slot0 = relinked([rng.randrange(P)] + [0] * 15 + [rng.randrange(P)], body, 1)      # states 0 .. 15 linked, the bridge tip (16) independent
    clean = _with_own_hashes(ChainCase("clean", "clean", slot0, body, [0] * STATES))
    h = clean.hashes()
    v = []
    for s in range(STATES):                                                             # E(s, i): one bit of one expected word
        for i in range(8):
            x = list(clean.expected); x[s] ^= 1 << (32 * i + (31 if i & 1 else 0))
            v.append(clean.edit(f"E({s},{i})", "E", expected=x, key=(s, i)))
    link = {}
    for s in range(1, STATES - 1):                                                      # L(s, i): one bit of one link word; every hash still matches
        for i in range(8):
            z = list(clean.slot0); z[s] ^= 1 << (32 * i + (29 if i == 7 else 0))
            assert z[s] < P
            link[s, i] = _with_own_hashes(clean.edit(f"L({s},{i})", "L", slot0=relinked(z, body, s + 1), key=(s, i)))
            v.append(link[s, i])
    for s in (1, 8, 15):                                                                # the same residue in other words: the hashes do not move, the words do
        z = list(clean.slot0); z[s] = h[s - 1] + P
        v.append(clean.edit(f"alias({s})", "alias", slot0=z))
    for name, x in (("0", 0), ("p-1", P - 1), ("2^256-1", (1 << 256) - 1)):              # state 0 has no predecessor in the proof: its slot 0 is free
        z = list(clean.slot0); z[0] = x
        v.append(_with_own_hashes(clean.edit(f"free(0,{name})", "free", slot0=relinked(z, body, 1))))
    for name, x in (("h[15]", h[15]), ("random", rng.randrange(P))):                    # ... and the bridge tip is not linked to the candidate tip
        z = list(clean.slot0); z[16] = x
        v.append(_with_own_hashes(clean.edit(f"free(16,{name})", "free", slot0=z)))
    x = list(clean.expected); x[15], x[16] = x[16], x[15]
    v.append(clean.edit("order(expected 15<->16)", "order", expected=x))
    sw = lambda t: tuple(t[8] if s == 7 else t[7] if s == 8 else t[s] for s in range(STATES))
    v.append(clean.edit("order(states 7<->8)", "order", slot0=sw(clean.slot0), body=sw(clean.body), expected=sw(clean.expected)))
    v.append(clean.edit("precheck(0,clean)", "precheck", precheck=0))
    v.append(clean.edit("precheck(1,clean)", "precheck", precheck=1))
    v.append(clean.edit("precheck(0xff,clean)", "precheck", precheck=0xFF))
    v.append(link[8, 3].edit("precheck(1,L(8,3))", "precheck", precheck=1))
    return tuple(interleave(v, clean))


CHAIN_COUNTS = {"E": 136, "L": 120, "alias": 3, "free": 5, "order": 2, "precheck": 4}
CHAIN_EXPECTED = {"E": 0, "L": 0, "alias": 0, "free": 1, "order": 0, "clean": 1,
                  "precheck(0,clean)": 0, "precheck(1,clean)": 1, "precheck(0xff,clean)": 1, "precheck(1,L(8,3))": 0}


def chain_model(case, precheck=True, links=range(1, STATES - 1), link_words=range(8), hash_words=range(8), n_hashes=STATES, mod_p=False):
    """the gate: the 17 x 8 words of the oracle's hashes equal the expected words, record slot 0 of states 1 .. 15 equals, word for word, the hash of the state
    before, and the precheck byte (where the job has one) is not 0.  The keyword arguments weaken it."""
    h, x = case.hashes(), case.expected
    ok = case.precheck != 0 if precheck else True
    for s in range(n_hashes):
        ok = ok and all(word(h[s], i) == word(x[s], i) for i in hash_words)
    for s in links:
        if s == 0:                                                                       # (a loop that starts at state 0 has no hash of this proof to compare with)
            ok = False; continue
        a = case.slot0[s] % P if mod_p else case.slot0[s]
        ok = ok and all(word(a, i) == word(h[s - 1], i) for i in link_words)
    return int(ok)


def chain_jobs(cases):
    """the table as the job dicts tests/state_job_helpers.py build_jobs takes (state leg only) and its precheck bytes"""
    jobs = [{"records": c.records(), "nfields": np.full(STATES, NFIELDS, np.uint32), "expected": list(c.expected), "abi": None} for c in cases]
    return jobs, np.array([c.precheck for c in cases], np.uint8)


# ------------------------------------------------------------------------------------------------ the ledger gate
@functools.lru_cache(maxsize=None)
def ledger_table():
    """-> (proofs as tests/state_pack_helpers.py precheck_proofs lists them, the states): one well-formed chain; per position, 64-bit word and lowest / highest
    byte of the word one proof with one bit of that ledger hash flipped; a clean proof after every 7; at the end a clean proof whose `and` byte is 0"""
    import state_pack_helpers as H
    states, data, exp, led = H.well_formed_proof()
    clean = ("clean", data, exp, led, 1)
    v = []
    for pos in range(16):
        for w in range(4):
            for which, byte, bit in (("low", 0, 0x01), ("high", 7, 0x80)):
                b = bytearray(led); b[32 * pos + 8 * w + byte] ^= bit
                v.append((f"ledger({pos},{w},{which})", data, exp, bytes(b), 1))
    return tuple(interleave(v, clean)) + (("clean, and byte 0", data, exp, led, 0),), states


def ledger_model(proof, states, use_and=True, words=range(4), positions=range(16)):
    """-> (mask, precheck byte): the chain is well formed and its candidate tip wins, so FORMAT and CONSENSUS are set; LEDGER iff the 16 x 32 bytes are the
    states' snarked ledger hashes; the byte is 0 iff a bit is clear (or the caller's `and` byte is 0)"""
    from oracle import mina_state_ref as S
    _, _, _, led, and_byte = proof
    ok = True
    for pos in positions:
        want = int(S.snarked_ledger_hash(states[pos])).to_bytes(32, "little")
        ok = ok and all(led[32 * pos + 8 * w:32 * pos + 8 * w + 8] == want[8 * w:8 * w + 8] for w in words)
    mask = FORMAT | CONSENSUS | (LEDGER if ok else 0)
    return mask, int(mask == FORMAT | LEDGER | CONSENSUS and (and_byte != 0 or not use_and))


# ------------------------------------------------------------------------------------------------ the sg gate
SG_SHAPES = ((1, 8), (0, 7))                                                            # (curve, k): Vesta at k = 8, Pallas at k = 7
SG_INSTANCES = 4


def base_modulus(curve):
    return P if curve == 0 else Q


def cube_root_of_unity(m):
    """a primitive cube root of unity of F_m"""
    for g in range(2, 50):
        z = pow(g, (m - 1) // 3, m)
        if z != 1:
            assert pow(z, 3, m) == 1 and (z * z + z + 1) % m == 0
            return z
    raise AssertionError


@functools.lru_cache(maxsize=None)
def sg_world(curve, k):
    """-> (g of the oracle's SRS [2^k, 64], [(prechallenges [k, 16], sg [64])] x SG_INSTANCES): sg = <b_poly_coefficients(chals), g> by the CPU oracle, as
    tests/test_gpu_sponge_ipa.py make_accumulator_instance computes it"""
    from oracle import oracle as O
    g, _ = O.srs_create(curve, 1 << k, threads=4)
    fs = O.scalar_field_of(curve)
    _, endo_r = O.endo(curve)
    inst = []
    for t in range(SG_INSTANCES):
        rng = np.random.Generator(np.random.PCG64(7100 + 100 * curve + t))
        pre = rng.integers(0, 256, size=(k, 16), dtype=np.uint8)
        chals = np.stack([O.challenge_to_field(fs, pre[i].copy(), endo_r) for i in range(k)])
        sg = O.msm_pippenger(curve, g, O.b_poly_coefficients(fs, chals), threads=4)
        inst.append((pre, sg))
    return g, tuple(inst)


def sg_variants(curve, g, sg):
    """-> [(name, 64 bytes)]: the true commitment first, then the points and encodings a careless comparison takes for it"""
    from oracle import oracle as O, pasta_ref as R
    m = base_modulus(curve)
    pt = O.bytes_to_point(sg); x, y = pt
    z = cube_root_of_unity(m)
    enc = lambda p: O.point_to_bytes(p)
    out = [("sg", enc(pt)), ("-sg", enc((x, m - y))), ("(zeta x, y)", enc((z * x % m, y))), ("(zeta^2 x, y)", enc((z * z * x % m, y))),
           ("2 sg", enc(R.add(pt, pt, m))), ("sg + g[0]", enc(R.add(pt, O.bytes_to_point(g[0]), m))), ("infinity", np.zeros(64, np.uint8))]
    for wd in range(16):
        b = np.array(sg, np.uint8).copy(); b[4 * wd] ^= 1
        out.append((f"word {wd}", b))
    return out


def sg_model(got, sg, x_only=False, y_only=False, up_to_sign=False, curve=None):
    """the 64 bytes are the oracle's canonical affine point"""
    got, sg = bytes(bytearray(got)), bytes(bytearray(sg))
    if x_only:
        return int(got[:32] == sg[:32])
    if y_only:
        return int(got[32:] == sg[32:])
    if up_to_sign:
        m = base_modulus(curve)
        return int(got[:32] == sg[:32] and int.from_bytes(got[32:], "little") in (int.from_bytes(sg[32:], "little"), m - int.from_bytes(sg[32:], "little")))
    return int(got == sg)


SG_BATCH = 24
SG_BATCH_BAD = {2: "-sg", 5: "(zeta x, y)", 9: "(zeta^2 x, y)", 13: "2 sg", 17: "infinity", 21: "word 15"}


def sg_batch(curve, k, bad=True):
    """-> (prechallenges [24 k, 16], commitments [24, 64], the true commitments [24, 64], what each proof holds): 18 true instances with the six of SG_BATCH_BAD
    in between, or 24 true ones"""
    g, inst = sg_world(curve, k)
    pre, sgs, truth, what = [], [], [], []
    for b in range(SG_BATCH):
        p, sg = inst[b % SG_INSTANCES]
        name = SG_BATCH_BAD.get(b, "sg") if bad else "sg"
        pre.append(p); truth.append(sg); what.append(name); sgs.append(dict(sg_variants(curve, g, sg))[name])
    return np.concatenate(pre), np.stack(sgs), np.stack(truth), what


# ---- the folded comparison.  In the batch above one commitment is off the curve, so the folded check is refused before it compares anything and the per-proof
# kernel names the six.  In the batches below every commitment is a canonical point of the curve: the comparison of A = sum rho_b <s_b, g> with
# B = sum rho_b sg_b decides alone.  phi(x, y) = (zeta x, y) is an endomorphism of the group, so B = -A, phi(A), phi^2(A) where every proof holds that image.
SG_FOLDED = {"all -sg": lambda b: "-sg", "all (zeta x, y)": lambda b: "(zeta x, y)", "all (zeta^2 x, y)": lambda b: "(zeta^2 x, y)",
             "one -sg": lambda b: "-sg" if b == 11 else "sg"}


def sg_rho(curve, n=SG_BATCH):
    """the random weights of a folded batch: n scalars below 2^254, canonical in either scalar field"""
    rho = np.random.Generator(np.random.PCG64(4100 + curve)).integers(0, 256, size=(n, 32), dtype=np.uint8)
    rho[:, 31] &= 0x3F
    return rho


def sg_folded_batch(curve, k, name):
    """-> (prechallenges, commitments [24, 64], the true commitments, what each proof holds) of one batch of SG_FOLDED"""
    g, inst = sg_world(curve, k)
    pre, sgs, truth, what = [], [], [], []
    for b in range(SG_BATCH):
        p, sg = inst[b % SG_INSTANCES]
        pre.append(p); truth.append(sg); what.append(SG_FOLDED[name](b)); sgs.append(dict(sg_variants(curve, g, sg))[what[-1]])
    return np.concatenate(pre), np.stack(sgs), np.stack(truth), what


def sg_folded_model(curve, sgs, truth, rho, x_only=False, y_only=False, up_to_sign=False, always=False):
    """the folded check of a batch without a malformed commitment: sum rho_b sg_b (what the proofs hold) is the point sum rho_b <s_b, g> (the true commitments
    under the same weights), both by the CPU oracle's MSM.  1 = the whole batch is accepted.  The keyword arguments weaken the comparison of the two points."""
    from oracle import oracle as O
    a, b = O.msm_naive(curve, np.ascontiguousarray(truth), rho), O.msm_naive(curve, np.ascontiguousarray(sgs), rho)
    return 1 if always else sg_model(b, a, x_only=x_only, y_only=y_only, up_to_sign=up_to_sign, curve=curve)
