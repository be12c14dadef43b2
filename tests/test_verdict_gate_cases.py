"""The tables of tests/verdict_gate_cases.py, checked on the CPU: every class has the proofs it lists, every proof differs from the clean one in exactly what its
name says, the models give the verdicts the classes are listed with -- and each model, weakened into one of the bugs the tables were written against (a loop one
state short, 7 words of 8, three ledger words of four, one coordinate of two, equality up to sign ...), changes the verdict of at least one proof, which the test
names.  That is the evidence, without a GPU, that tests/test_gpu_verdict_gates.py would notice such a kernel."""
import numpy as np
import pytest

import verdict_gate_cases as C

P, STATES = C.P, C.STATES


@pytest.fixture(scope="module")
def chain(oracle):
    return C.chain_table()


def by_class(table, cls):
    return [c for c in table if c.cls == cls]


def links_intact(c):
    h = c.hashes()
    return [s for s in range(1, STATES - 1) if c.slot0[s] != h[s - 1]]


# ------------------------------------------------------------------------------------------------ the chain gate
def test_chain_hashes_are_the_oracle_sponge_of_the_one_lane_test(chain, oracle):
    """the table's hashing is tests/test_gpu_state_hash_one_lane.py _oracle_hashes on the same records, non-canonical slot 0 included"""
    from test_gpu_state_hash_one_lane import _oracle_hashes
    for c in [chain[7], by_class(chain, "alias")[1], by_class(chain, "free")[2], by_class(chain, "L")[17]]:
        vals = [[c.slot0[s], *c.body[s]] + [0] * (C.SLOTS - 1 - C.NFIELDS) for s in range(STATES)]
        want, _ = _oracle_hashes(oracle, vals, [C.NFIELDS] * STATES)
        assert c.hashes() == want, c.name
        rec = c.records()
        assert rec.shape == (STATES, C.SLOTS * 32) and not rec[:, 32 * (1 + C.NFIELDS):].any()
        assert [int.from_bytes(rec[s, :32].tobytes(), "little") for s in range(STATES)] == list(c.slot0)


def test_chain_table_layout_and_counts(chain):
    assert {cls: len(by_class(chain, cls)) for cls in C.CHAIN_COUNTS} == C.CHAIN_COUNTS
    variants = [c for c in chain if c.cls != "clean"]
    assert len(variants) == 270 and len(by_class(chain, "clean")) == 39 and len(chain) == 309
    assert len({c.name for c in variants}) == len(variants)
    run = 0
    for c in chain:                                                     # a clean proof after every 7 variants
        run = 0 if c.cls == "clean" else run + 1
        assert run <= C.CLEAN_EVERY
    assert chain[7].cls == chain[-1].cls == "clean" and chain[0].name == "E(0,0)"
    # the batch sizes the GPU test cuts the table at hold a clean proof and a rejected one on either side of the 64-lane block edge
    assert [c.cls for c in chain[62:66]] == ["E", "clean", "E", "E"]


def test_clean_proof_is_linked_and_the_bridge_tip_is_not(chain):
    clean = chain[7]
    h = clean.hashes()
    assert list(clean.expected) == h and len(set(h)) == STATES and all(0 <= x < P for x in h)
    assert links_intact(clean) == [] and clean.slot0[16] != h[15] and clean.precheck == 1
    assert all(c.slot0 == clean.slot0 and c.body == clean.body and c.expected == clean.expected for c in by_class(chain, "clean"))


def test_every_chain_variant_differs_in_exactly_what_its_name_says(chain):
    clean = chain[7]
    h = clean.hashes()
    seen = set()
    for c in by_class(chain, "E"):                                      # one bit of one expected word; the records are the clean proof's
        s, i = c.key
        assert c.name == f"{c.cls}({s},{i})"
        seen.add((s, i))
        assert c.slot0 == clean.slot0 and c.body == clean.body and c.precheck == 1
        diff = [(t, c.expected[t] ^ clean.expected[t]) for t in range(STATES) if c.expected[t] != clean.expected[t]]
        assert diff == [(s, 1 << (32 * i + (31 if i & 1 else 0)))], c.name
    assert seen == {(s, i) for s in range(STATES) for i in range(8)}
    seen = set()
    for c in by_class(chain, "L"):                                      # all 17 hashes match, exactly the link into state s is broken, in word i alone
        s, i = c.key
        assert c.name == f"{c.cls}({s},{i})"
        seen.add((s, i))
        ch = c.hashes()
        assert list(c.expected) == ch and c.body == clean.body and c.precheck == 1
        assert links_intact(c) == [s], c.name
        assert c.slot0[s] ^ ch[s - 1] == 1 << (32 * i + (29 if i == 7 else 0)) and c.slot0[s] < P
        assert c.slot0[:s] == clean.slot0[:s] and ch[:s] == h[:s] and c.slot0[16] == clean.slot0[16]
        assert all(ch[t] != h[t] for t in range(s, 16)) and ch[16] == h[16]
    assert seen == {(s, i) for s in range(1, 16) for i in range(8)}
    for c, s in zip(by_class(chain, "alias"), (1, 8, 15)):              # the same element in other words: no hash moves
        assert c.slot0[s] == h[s - 1] + P < 1 << 256 and c.hashes() == h == list(c.expected)
        assert [t for t in range(STATES) if c.slot0[t] != clean.slot0[t]] == [s] and c.body == clean.body
        assert [i for i in range(8) if C.word(c.slot0[s], i) != C.word(h[s - 1], i)] != []
    free = by_class(chain, "free")
    assert [c.slot0[0] for c in free[:3]] == [0, P - 1, (1 << 256) - 1]
    assert free[3].slot0[16] == h[15] and free[4].slot0[16] not in (h[15], clean.slot0[16]) and all(c.slot0[:16] == clean.slot0[:16] for c in free[3:])
    for c in free:
        assert list(c.expected) == c.hashes() and links_intact(c) == [] and c.body == clean.body
    o1, o2 = by_class(chain, "order")
    assert o1.slot0 == clean.slot0 and o1.body == clean.body and sorted(o1.expected) == sorted(clean.expected)
    assert [t for t in range(STATES) if o1.expected[t] != clean.expected[t]] == [15, 16]
    assert list(o2.expected) == o2.hashes() and sorted(o2.expected) == sorted(clean.expected) and links_intact(o2) == [7, 8, 9]
    p0, p1, pff, pl = by_class(chain, "precheck")
    assert [p0.precheck, p1.precheck, pff.precheck, pl.precheck] == [0, 1, 0xFF, 1]
    assert all(c.slot0 == clean.slot0 and c.expected == clean.expected for c in (p0, p1, pff))
    l83 = next(c for c in chain if c.name == "L(8,3)")
    assert pl.slot0 == l83.slot0 and pl.expected == l83.expected


def test_chain_model_gives_every_class_its_listed_verdict(chain):
    for c in chain:
        want = C.CHAIN_EXPECTED[c.name if c.cls == "precheck" else c.cls]
        assert C.chain_model(c) == want, c.name
    # without precheck bytes only the proof whose byte alone was cleared changes sides
    moved = [c.name for c in chain if C.chain_model(c, precheck=False) != C.chain_model(c)]
    assert moved == ["precheck(0,clean)"]
    v = [C.chain_model(c) for c in chain]
    assert (v.count(1), v.count(0)) == (39 + 5 + 2, 136 + 120 + 3 + 2 + 2)


CHAIN_WEAK = [("links over 1..14", dict(links=range(1, 15)), {f"L(15,{i})" for i in range(8)} | {"alias(15)"}),
              ("links over 2..15", dict(links=range(2, 16)), {f"L(1,{i})" for i in range(8)} | {"alias(1)"}),
              ("links over 1..16", dict(links=range(1, 17)), None),
              ("links over 0..15", dict(links=range(0, 16)), None),
              ("16 hashes", dict(n_hashes=16), {f"E(16,{i})" for i in range(8)}),
              ("aliases mod p", dict(mod_p=True), {"alias(1)", "alias(8)", "alias(15)"})]
CHAIN_WEAK += [(f"7 words per link (not word {j})", dict(link_words=[i for i in range(8) if i != j]), {f"L({s},{j})" for s in range(1, 16)} | ({"precheck(1,L(8,3))"} if j == 3 else set()))
               for j in range(8)]
CHAIN_WEAK += [(f"7 words per hash (not word {j})", dict(hash_words=[i for i in range(8) if i != j]), {f"E({s},{j})" for s in range(STATES)}) for j in range(8)]


@pytest.mark.parametrize("name,weak,want", CHAIN_WEAK, ids=[w[0] for w in CHAIN_WEAK])
def test_each_weakened_chain_model_changes_a_verdict(chain, name, weak, want):
    moved = sorted({c.name for c in chain if C.chain_model(c, **weak) != C.chain_model(c)})
    print(name, "->", moved)
    assert moved, name
    if want is not None:
        assert set(moved) == want, (name, moved)
        assert all(C.chain_model(c, **weak) == 1 for c in chain if c.name in want), "a false ACCEPT"
    elif name == "links over 1..16":                                    # the bridge tip linked: every proof whose state 16 does not name the candidate tip
        assert "clean" in moved and "free(16,random)" in moved and "free(16,h[15])" not in moved
    else:                                                               # a loop from state 0: no proof of the table names a predecessor of state 0
        assert "clean" in moved and all(f"free(0,{x})" in moved for x in ("0", "p-1", "2^256-1"))


# ------------------------------------------------------------------------------------------------ the ledger gate
@pytest.fixture(scope="module")
def ledger(oracle):
    return C.ledger_table()


def test_ledger_table_one_bit_per_proof_in_every_word_of_every_position(ledger):
    from oracle import mina_state_ref as S
    proofs, states = ledger
    clean = proofs[7]
    truth = b"".join(int(S.snarked_ledger_hash(s)).to_bytes(32, "little") for s in states[:16])
    assert clean[0] == "clean" and clean[3] == truth and len(truth) == 512
    variants = [p for p in proofs if p[0].startswith("ledger(")]
    assert len(variants) == 128 and len(proofs) == 128 + 19 + 1 and proofs[-1] == ("clean, and byte 0",) + clean[1:4] + (0,)
    seen = set()
    for name, data, exp, led, and_byte in variants:
        pos, w, which = name[7:-1].split(",")
        pos, w = int(pos), int(w)
        assert data == clean[1] and exp == clean[2] and and_byte == 1
        diff = [(i, led[i] ^ truth[i]) for i in range(512) if led[i] != truth[i]]
        assert diff == [(32 * pos + 8 * w + (0 if which == "low" else 7), 0x01 if which == "low" else 0x80)], name
        seen.add((pos, w, which))
    assert len(seen) == 128
    run = 0
    for p in proofs:
        run = 0 if p[0].startswith("clean") else run + 1
        assert run <= C.CLEAN_EVERY
    every = C.FORMAT | C.LEDGER | C.CONSENSUS
    for p in proofs:
        want = {"clean": (every, 1), "clean, and byte 0": (every, 0)}.get(p[0], (C.FORMAT | C.CONSENSUS, 0))
        assert C.ledger_model(p, states) == want, p[0]
    assert C.ledger_model(proofs[-1], states, use_and=False) == (every, 1)


LEDGER_WEAK = [(f"three words per hash (not word {j})", dict(words=[w for w in range(4) if w != j]), {f"ledger({pos},{j},{b})" for pos in range(16) for b in ("low", "high")})
               for j in range(4)]
LEDGER_WEAK += [("15 positions", dict(positions=range(15)), {f"ledger(15,{w},{b})" for w in range(4) for b in ("low", "high")}),
                ("positions 1..15", dict(positions=range(1, 16)), {f"ledger(0,{w},{b})" for w in range(4) for b in ("low", "high")})]


@pytest.mark.parametrize("name,weak,want", LEDGER_WEAK, ids=[w[0] for w in LEDGER_WEAK])
def test_each_weakened_ledger_model_changes_a_verdict(ledger, name, weak, want):
    proofs, states = ledger
    moved = sorted({p[0] for p in proofs if C.ledger_model(p, states, **weak) != C.ledger_model(p, states)})
    print(name, "->", moved)
    assert set(moved) == want, (name, moved)
    assert all(C.ledger_model(p, states, **weak)[1] == 1 for p in proofs if p[0] in want), "a false ACCEPT"


# ------------------------------------------------------------------------------------------------ the sg gate
@pytest.mark.parametrize("curve,k", C.SG_SHAPES)
def test_sg_variants_are_what_their_names_say(oracle, curve, k):
    from oracle import pasta_ref as R
    m = C.base_modulus(curve)
    g, inst = C.sg_world(curve, k)
    assert len(inst) == C.SG_INSTANCES and len({bytes(sg) for _, sg in inst}) == C.SG_INSTANCES
    z = C.cube_root_of_unity(m)
    assert z != 1 and pow(z, 3, m) == 1
    for pre, sg in inst:
        assert pre.shape == (k, 16) and oracle.is_on_curve(curve, sg) and sg.any()
        x, y = oracle.bytes_to_point(sg)
        var = C.sg_variants(curve, g, sg)
        assert len(var) == 23 and len({bytes(bytearray(b)) for _, b in var}) == 23
        d = {n: oracle.bytes_to_point(b) for n, b in var}
        assert var[0][0] == "sg" and bytes(var[0][1]) == bytes(sg)
        assert d["-sg"] == (x, m - y) and d["(zeta x, y)"] == (z * x % m, y) and d["(zeta^2 x, y)"] == (z * z * x % m, y) and d["infinity"] is None
        for n in ("-sg", "(zeta x, y)", "(zeta^2 x, y)", "2 sg", "sg + g[0]"):         # on the curve, canonical, and not sg
            px, py = d[n]
            assert (py * py - px * px * px - 5) % m == 0 and px < m and py < m and d[n] != (x, y), n
            assert oracle.is_on_curve(curve, dict(var)[n])
        assert d["2 sg"] == oracle.bytes_to_point(oracle.point_add(curve, sg, sg)) == R.scalar_mul(2, (x, y), m)
        assert d["sg + g[0]"] == oracle.bytes_to_point(oracle.point_add(curve, sg, g[0]))
        for wd in range(16):
            b = np.array(dict(var)[f"word {wd}"]); diff = np.flatnonzero(b != sg)
            assert diff.tolist() == [4 * wd] and b[4 * wd] ^ sg[4 * wd] == 1
        assert [C.sg_model(b, sg) for _, b in var] == [1] + [0] * 22


SG_WEAK = [("x only", dict(x_only=True), {"-sg"} | {f"word {w}" for w in range(8, 16)}),
           ("y only", dict(y_only=True), {"(zeta x, y)", "(zeta^2 x, y)"} | {f"word {w}" for w in range(8)}),
           ("equality up to sign", dict(up_to_sign=True), {"-sg"})]


@pytest.mark.parametrize("curve,k", C.SG_SHAPES)
@pytest.mark.parametrize("name,weak,want", SG_WEAK, ids=[w[0] for w in SG_WEAK])
def test_each_weakened_sg_model_changes_a_verdict(oracle, curve, k, name, weak, want):
    g, inst = C.sg_world(curve, k)
    for _, sg in inst:
        moved = {n for n, b in C.sg_variants(curve, g, sg) if C.sg_model(b, sg, curve=curve, **weak) != C.sg_model(b, sg)}
        print(name, curve, "->", sorted(moved))
        assert moved == want, (name, moved)
    # the mixed batch of 24 holds a proof that each weakened PER-PROOF comparison lets through (its folded check is refused for the off-curve word: the per-proof
    # kernel names the six; the folded comparison has batches of its own below)
    pre, sgs, truth, what = C.sg_batch(curve, k)
    assert what.count("sg") == 18 and [what[b] for b in sorted(C.SG_BATCH_BAD)] == list(C.SG_BATCH_BAD.values())
    assert not oracle.is_on_curve(curve, sgs[21]) and what[21] == "word 15"
    assert any(C.sg_model(sgs[b], truth[b], curve=curve, **weak) == 1 for b in C.SG_BATCH_BAD), name
    assert [C.sg_model(sgs[b], truth[b]) for b in range(C.SG_BATCH)] == [0 if b in C.SG_BATCH_BAD else 1 for b in range(C.SG_BATCH)]
    assert C.sg_batch(curve, k, bad=False)[3] == ["sg"] * C.SG_BATCH


SG_FOLDED_WEAK = [("x only", dict(x_only=True), {"all -sg"}), ("y only", dict(y_only=True), {"all (zeta x, y)", "all (zeta^2 x, y)"}),
                  ("equality up to sign", dict(up_to_sign=True), {"all -sg"}), ("1 where no point is malformed", dict(always=True), set(C.SG_FOLDED))]


@pytest.mark.parametrize("curve,k", C.SG_SHAPES)
def test_folded_batches_let_the_comparison_decide_and_each_weakened_form_accepts_one(oracle, curve, k):
    """every commitment of these batches is a canonical point of the curve (nothing refuses the folded check before it compares), every per-proof verdict of
    the -sg / endomorphism batches is 0, the folded model rejects all four batches and accepts the 24 true instances -- and each weakened comparison of the two
    folded points ACCEPTS a whole batch, which the test names"""
    rho = C.sg_rho(curve)
    m = C.base_modulus(curve)
    assert rho.shape == (C.SG_BATCH, 32) and all(int.from_bytes(r.tobytes(), "little") < 1 << 254 for r in rho) and len({r.tobytes() for r in rho}) == C.SG_BATCH
    batches = {name: C.sg_folded_batch(curve, k, name) for name in C.SG_FOLDED}
    for name, (pre, sgs, truth, what) in batches.items():
        assert all(oracle.is_on_curve(curve, s) and s.any() for s in sgs) and all(int.from_bytes(s[i:i + 32].tobytes(), "little") < m for s in sgs for i in (0, 32))
        want = [C.sg_model(sgs[b], truth[b]) for b in range(C.SG_BATCH)]
        assert want == ([1] * 11 + [0] + [1] * 12 if name == "one -sg" else [0] * C.SG_BATCH), name
        assert C.sg_folded_model(curve, sgs, truth, rho) == 0, name
    pre, sgs, truth, _ = C.sg_batch(curve, k, bad=False)
    assert C.sg_folded_model(curve, sgs, truth, rho) == 1
    for name, weak, want in SG_FOLDED_WEAK:
        moved = {b for b, (pre, sgs, truth, what) in batches.items() if C.sg_folded_model(curve, sgs, truth, rho, **weak) == 1}
        print(name, curve, "-> accepts", sorted(moved))
        assert moved == want, (name, moved)
