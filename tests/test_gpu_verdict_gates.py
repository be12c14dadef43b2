"""The kernels that turn arithmetic into a verdict, held to the plain models of tests/verdict_gate_cases.py word by word:

  the chain gate   pstate_chain_check_kernel (mina_state_job_batch / _batch_dev) and pstate_chain_detail_kernel (mina_state_job_checks): one flipped bit in every
                   one of the 136 expected words and of the 120 link words, alias encodings of a link, the free slots of state 0 and of the bridge tip, swapped
                   hashes and states, precheck bytes -- one batch, cut at the 64-lane block edge and tiled past 8192 states, with the deduplicated state leg too
  the ledger gate  pstate_precheck_entry (mina_state_frontend_dev): one flipped bit in the lowest and the highest byte of every 64-bit word of every ledger
                   position; the host twin parse_states_half (the boundary with MINA_VERIFY_PACK_ON_DEVICE off, and on): one flipped bit in every position
  the sg gate      xyzz_eq_affine_kernel (mina_accumulator_check_multi, a batch of one, the per-proof route of a failed batch): -sg, the endomorphism images, 2 sg,
                   sg + g[0], infinity, flipped words; xyzz_compare_kernel (the folded check of mina_accumulator_check_batch) and xyzz_compare_parts_kernel (the
                   accumulator leg of a job searched in groups, Vesta only): batches of canonical points whose folded sum is -A or an endomorphism image of A,
                   where the comparison alone decides

Every expectation is a model's; tests/test_verdict_gate_cases.py shows on the CPU which weakened comparison each table catches.  All comparisons are exact."""
import copy
import random

import numpy as np
import pytest

import verdict_gate_cases as C
from test_grouped_search_gpu import SHAPE, fresh_context, simulate, small_srs  # noqa: F401  (small_srs: a module-scoped fixture)
from test_state_masks_model import ACCUMULATOR, CHAIN, CONSENSUS, FORMAT, KIMCHI, LEDGER, masks_rule

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gctx():
    """a context of its own (both SRS at 2^10, prepared for SHAPE): the dedup mode and the group count are context state"""
    c = fresh_context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def chain(oracle):
    table = C.chain_table()
    jobs, pre = C.chain_jobs(table)
    return table, jobs, pre


def leg(jobs, pre=None, with_states=True, with_ipa=False, with_acc=False, acc_k=SHAPE["acc_k"]):
    """the job with the legs named (the state leg alone by default), its precheck bytes attached"""
    import mina_bridge_amd as m
    from state_job_helpers import build_jobs
    j, keep = build_jobs(m, jobs, SHAPE["k"], SHAPE["log2_domain"], SHAPE["slot"], acc_k, with_states=with_states, with_ipa=with_ipa, with_acc=with_acc)
    if pre is not None:
        pre = np.ascontiguousarray(pre, np.uint8); keep.append(pre); j.precheck = pre.ctypes.data
    return j, keep


def report(what, names, got, want):
    """what ran, per class, and ACCEPT / REJECT of the GPU and of the model side by side"""
    got, want = [int(x) for x in got], [int(x) for x in want]
    cls = {}
    for n in names:
        cls[n] = cls.get(n, 0) + 1
    print(f"{what}: {len(got)} proofs {cls}; GPU ACCEPT {got.count(1)} REJECT {got.count(0)}; model ACCEPT {want.count(1)} REJECT {want.count(0)}")


def differing(names, got, want):
    return [(b, names[b], int(got[b]), int(want[b])) for b in range(len(want)) if int(got[b]) != int(want[b])]


# ------------------------------------------------------------------------------------------------ the chain gate
@pytest.mark.parametrize("cut", ["whole", 1, 63, 64, 65, "twice"])
def test_chain_gate_equals_the_model_for_every_proof(gctx, chain, cut):
    """mina_state_job_batch with only the state leg on: the whole table in one call, its first 1 / 63 / 64 / 65 proofs (the gate's block edge is at 64), and the
    table twice (more than 8192 states); the whole table once more with a null precheck pointer"""
    table, jobs, pre = chain
    if cut == "twice":
        table, jobs, pre = table + table, jobs + jobs, np.concatenate([pre, pre])
    elif cut != "whole":
        table, jobs, pre = table[:cut], jobs[:cut], pre[:cut]
    names = [c.name for c in table]
    want = [C.chain_model(c) for c in table]
    got = gctx.state_job_batch(leg(jobs, pre)).tolist()
    report(f"chain gate, {cut}", [c.cls for c in table], got, want)
    assert got == want, differing(names, got, want)
    if cut == "whole":
        assert len(table) * C.STATES < 8192 < 2 * len(table) * C.STATES
        want = [C.chain_model(c, precheck=False) for c in table]
        got = gctx.state_job_batch(leg(jobs)).tolist()
        report("chain gate, whole, null precheck", [c.cls for c in table], got, want)
        assert got == want, differing(names, got, want)


def test_chain_bit_of_the_masks_equals_the_model(gctx, chain):
    """mina_state_job_checks (pstate_chain_detail_kernel) on the whole table: the CHAIN bit of `passed` is the model's verdict without the precheck byte -- the masks
    do not read it --, `ran` and the other bits follow the rule of tests/test_state_masks_model.py"""
    table, jobs, pre = chain
    names = [c.name for c in table]
    want = [C.chain_model(c, precheck=False) for c in table]
    for attach in (None, pre):
        passed, ran = gctx.state_job_checks(leg(jobs, attach))
        got = [int(p & CHAIN != 0) for p in passed]
        report("chain gate, masks", [c.cls for c in table], got, want)
        assert got == want, differing(names, got, want)
        rule = [masks_rule(None, 0, True, False, False, w, 1, 1, 1) for w in want]
        assert (passed.tolist(), ran.tolist()) == ([p for p, _ in rule], [r for _, r in rule])
        assert set(ran.tolist()) == {FORMAT | CHAIN} and not any(p & (LEDGER | CONSENSUS | ACCUMULATOR | KIMCHI) for p in passed)


def test_chain_gate_device_form_with_and_without_dedup(gctx, chain):
    """mina_state_job_batch_dev on the whole table: the variants share most of their 17 records with the clean proof and with each other, so the deduplicated leg
    and its scatter hash about a fifth of the states; verdict words equal the model, and the words with the mode on equal those with it off"""
    table, jobs, pre = chain
    B = len(table)
    names = [c.name for c in table]
    want = [C.chain_model(c) for c in table]
    d, ptrs = gctx.state_jobs_to_device(leg(jobs, pre))
    out = gctx.dev_malloc(4 * B + 16)
    words = {}
    try:
        for dedup in (False, True):
            gctx.set_state_dedup(dedup)
            gctx.dev_upload(out, np.full(4 * B + 16, 0xEE, np.uint8))
            gctx.state_job_batch_dev(d, out, out + 4 * B)
            gctx.synchronize()
            words[dedup] = gctx.dev_download(out, 4 * B + 16).view(np.uint32).tolist()
            report(f"chain gate, device form, dedup {dedup}", [c.cls for c in table], words[dedup][:B], want)
            assert words[dedup][:B] == want, (dedup, differing(names, words[dedup][:B], want))
            assert words[dedup][B:] == [1, 0, 1, 0], "no folded leg ran: both count as passed"
        st = gctx.state_dedup_stats()
        distinct = len({(c.slot0[s], c.body[s]) for c in table for s in range(C.STATES)})
        print("dedup:", st, "distinct records of the table:", distinct)
        assert (st.states, st.distinct) == (B * C.STATES, distinct) and 4 * distinct < B * C.STATES
        assert words[False] == words[True]
    finally:
        gctx.set_state_dedup(False)
        gctx.synchronize()
        for p in ptrs + [out]:
            gctx.dev_free(p)


def test_chain_gate_inside_a_job_with_all_three_legs(gctx, chain, small_srs):
    """one oracle-minted job at the shape of tests/test_grouped_search_gpu.py, five times, its chain replaced by the clean proof, L(15,7), L(1,0), E(16,7) and
    E(0,0): the verdict is 1 for the clean one only, and the flags report both folded checks as passed -- the gate alone rejected the four"""
    from state_job_helpers import mint_job
    table, jobs, _ = chain
    minted = mint_job(small_srs[0], small_srs[1], 300, **SHAPE)
    pick = ["clean", "L(15,7)", "L(1,0)", "E(16,7)", "E(0,0)"]
    at = [next(b for b, c in enumerate(table) if c.name == n) for n in pick]
    batch = []
    for b in at:
        j = copy.copy(minted)
        j["records"], j["nfields"], j["expected"] = jobs[b]["records"], jobs[b]["nfields"], jobs[b]["expected"]
        batch.append(j)
    want = [C.chain_model(table[b]) for b in at]
    assert want == [1, 0, 0, 0, 0]
    sj = leg(batch, None, with_states=True, with_ipa=True, with_acc=True)
    got = gctx.state_job_batch(sj).tolist()
    report("chain gate, all three legs", pick, got, want)
    assert got == want
    B = len(batch)
    d, ptrs = gctx.state_jobs_to_device(sj)
    out = gctx.dev_malloc(4 * B + 16)
    try:
        gctx.dev_upload(out, np.full(4 * B + 16, 0xEE, np.uint8))
        gctx.state_job_batch_dev(d, out, out + 4 * B)
        gctx.synchronize()
        w = gctx.dev_download(out, 4 * B + 16).view(np.uint32).tolist()
        assert (w[:B], w[B:]) == (want, [1, 0, 1, 0])
    finally:
        for p in ptrs + [out]:
            gctx.dev_free(p)


# ------------------------------------------------------------------------------------------------ the ledger gate
def test_ledger_gate_every_word_of_every_position_device_and_host(ctx, oracle):
    """the 128 + clean proofs through mina_state_frontend_dev, with and without the `and` bytes and the masks pointer: masks and precheck bytes equal the model;
    records and field counts are the clean proof's.  The same proofs through tests/state_pack_helpers.py host_frontend: that route packs with the host's
    mina_protocol_state_pack and selects with the host's mina_consensus_*, but compares the ledger hashes in Python -- it pins the snarked hashes the host packer
    hands out and the other two bits, not the memcmp of parse_states_half, which the boundary test below reaches with the pack on the host"""
    import mina_bridge_amd as m
    import state_pack_helpers as H
    from test_state_pack_gpu import frontend_dev
    proofs, states = C.ledger_table()
    B = len(proofs)
    names = [p[0] for p in proofs]
    model = [C.ledger_model(p, states) for p in proofs]
    recs, nf, pre, masks = frontend_dev(ctx, proofs)
    report("ledger gate, device", [n.split("(")[0] for n in names], pre, [p for _, p in model])
    assert masks.tolist() == [k for k, _ in model], differing(names, masks, [k for k, _ in model])
    assert pre.tolist() == [p for _, p in model], differing(names, pre, [p for _, p in model])
    recs = recs.reshape(B, -1); nf = nf.reshape(B, -1)
    assert names[7] == "clean" and recs[7].any() and (recs == recs[7]).all() and (nf == nf[7]).all() and nf[7].all()
    recs2, nf2, pre2, _ = frontend_dev(ctx, proofs, masks=False, use_and=False)
    want2 = [C.ledger_model(p, states, use_and=False)[1] for p in proofs]
    assert pre2.tolist() == want2 and sum(want2) == sum(p for _, p in model) + 1
    assert (recs2.reshape(B, -1) == recs).all() and (nf2.reshape(B, -1) == nf).all()
    host_pre = []
    for b, (name, data, exp, led, and_byte) in enumerate(proofs):
        wrec, wnf, wpre, wmask, branch = H.host_frontend(m, data, exp, led, and_byte)
        host_pre.append(wpre)
        assert (wmask, wpre) == model[b], (name, wmask, wpre, model[b])
        assert wrec == recs[7].tobytes() and wnf == nf[7].tolist() and branch == "short/same epoch/selected"
    report("ledger gate, host", [n.split("(")[0] for n in names], host_pre, [p for _, p in model])


def test_ledger_gate_at_the_boundary_with_the_pack_on_the_host_and_on_the_device(oracle):
    """mina_verify_state_checks on a committed k = 15 statement, MINA_VERIFY_PACK_ON_DEVICE off (parse_states_half, the host twin of the gate) and on: one bit
    flipped in ledger position 0 word 3 high byte, position 15 word 3 high byte, position 7 word 2 low byte, in one more word of EVERY position (word pos % 4, the
    lowest and the highest byte in turn), and the clean input: LEDGER is down exactly for the tampered ones, every other bit is the clean proof's"""
    import mina_bridge_amd as m
    import state_pack_helpers as H
    from ipa_helpers import poseidon_pp
    from kimchi_helpers import install_index, install_step_index, load_k15_fixture, load_statement_fixture, make_chain, make_step_index
    from oracle import mina_state_ref as S
    from wire_writers import state_pub_bytes, wrap_proof_bytes
    ix, _, _ = load_k15_fixture()
    it = load_statement_fixture()[0][0]
    states, hashes = make_chain(random.Random(it["chain_seed"]), poseidon_pp(0))
    p, ev = it["proof"], it["proof"]["evals"]
    wrap = dict(it["wrap"])
    wrap.update(w_comm=p["w_comm"], z_comm=p["z_comm"], t_comm=p["t_comm"], z_eval=ev[0], selector_eval=ev[1:7], w_eval=ev[7:22], coefficients_eval=ev[22:37],
                s_eval=ev[37:43], ft_eval1=p["ft_eval1"], lr=p["opening"]["lr"], z1=p["opening"]["z1"], z2=p["opening"]["z2"], delta=p["opening"]["delta"], sg=p["opening"]["sg"])
    proof = wrap_proof_bytes(wrap, binprot=False) + b"".join(H.bincode_state(s) for s in states)
    ledger = [S.snarked_ledger_hash(s) for s in states[:16]]
    assert all(x < 1 << 254 for x in ledger)                            # a flipped bit 253 leaves a canonical element: the public input still parses

    def pub(pos=None, bit=0):
        led = list(ledger)
        if pos is not None:
            led[pos] ^= 1 << bit
        return state_pub_bytes(True, hashes[16], hashes[:16], led)
    probes = {"clean": pub(), "ledger(0,3,high)": pub(0, 3 * 64 + 56 + 5), "ledger(15,3,high)": pub(15, 3 * 64 + 56 + 5), "ledger(7,2,low)": pub(7, 2 * 64)}
    for pos in range(16):                                               # (the high byte of word 3 holds the element's top bits: bit 253, as above)
        w, high = pos % 4, (pos // 4) & 1
        probes.setdefault(f"ledger({pos},{w},{'high' if high else 'low'})", pub(pos, 64 * w + ((56 + (5 if w == 3 else 7)) if high else 0)))
    assert len(probes) == 1 + 3 + 16 - 1 and len(set(probes.values())) == len(probes)      # (position 15's word 3 high byte is one of the three)
    base = m.lib.VERIFY_ALLOW_SURROGATE
    got = {}
    try:
        for flags in (base, base | m.lib.VERIFY_PACK_ON_DEVICE):
            m.lib.verify_shutdown()
            m.lib.verify_configure(flags)
            g = m.lib.verify_global_ctx()
            install_index(g, ix)
            install_step_index(g, make_step_index(99))
            got[flags] = {name: tuple(int(x) for x in m.lib.verify_state_checks(proof, q)) for name, q in probes.items()}
            print(flags, got[flags])
    finally:
        m.lib.verify_configure(0)
        m.lib.verify_shutdown()
    ALL = FORMAT | LEDGER | CHAIN | CONSENSUS | ACCUMULATOR | KIMCHI
    for flags, by in got.items():
        assert by["clean"] == (ALL, ALL), (flags, by)
        for name in by:
            if name != "clean":
                assert by[name] == (ALL & ~LEDGER, ALL), (flags, name, by[name])


# ------------------------------------------------------------------------------------------------ the sg gate
@pytest.mark.parametrize("curve,k", C.SG_SHAPES)
def test_sg_gate_every_variant_as_a_problem_of_its_own(gctx, oracle, curve, k):
    """mina_accumulator_check_multi (xyzz_eq_affine_kernel per problem): the 23 variants of each of the four instances, one call per curve"""
    g, inst = C.sg_world(curve, k)
    pre, sgs, names, want = [], [], [], []
    for p, sg in inst:
        for name, b in C.sg_variants(curve, g, sg):
            pre.append(p); sgs.append(b); names.append(name); want.append(C.sg_model(b, sg))
    got = gctx.accumulator_check_multi(curve, k, np.concatenate(pre), np.stack(sgs)).tolist()
    report(f"sg gate, multi, curve {curve}", names, got, want)
    assert got == want, differing(names, got, want)
    assert want.count(1) == C.SG_INSTANCES and len(want) == 23 * C.SG_INSTANCES


@pytest.mark.parametrize("curve,k", C.SG_SHAPES)
def test_sg_gate_folded_batch_and_a_batch_of_one(gctx, oracle, curve, k):
    """mina_accumulator_check_batch: 24 proofs under random rho, 18 true with -sg, both endomorphism images, 2 sg, infinity and a flipped word in between.  The
    flipped word is off the curve, so this batch's folded check is refused before xyzz_compare_kernel compares anything, and xyzz_eq_affine_kernel names the six per
    proof; the same 24 all true (the folded comparison accepts); batches of one (xyzz_eq_affine_kernel) holding each bad commitment.  Where the folded comparison
    alone must REJECT: the test below"""
    rho = C.sg_rho(curve)
    pre, sgs, truth, what = C.sg_batch(curve, k)
    want = [C.sg_model(sgs[b], truth[b]) for b in range(C.SG_BATCH)]
    got = gctx.accumulator_check_batch(curve, k, pre, sgs, rho).tolist()
    report(f"sg gate, folded batch, curve {curve}", what, got, want)
    assert got == want, differing(what, got, want)
    assert want.count(0) == 6
    pre1, sgs1, truth1, what1 = C.sg_batch(curve, k, bad=False)
    assert (sgs1 == truth1).all()
    assert gctx.accumulator_check_batch(curve, k, pre1, sgs1, rho).tolist() == [1] * C.SG_BATCH
    for b in [0] + sorted(C.SG_BATCH_BAD):
        one = gctx.accumulator_check_batch(curve, k, pre[b * k:(b + 1) * k], sgs[b]).tolist()
        assert one == [want[b]], (what[b], one)
    assert want[2] == 0 and what[2] == "-sg"


@pytest.mark.parametrize("name", list(C.SG_FOLDED))
@pytest.mark.parametrize("curve,k", C.SG_SHAPES)
def test_sg_gate_folded_comparison_alone_rejects(gctx, oracle, curve, k, name):
    """mina_accumulator_check_batch on 24 proofs under random rho whose commitments are ALL canonical points of the curve, so nothing refuses the folded check
    before xyzz_compare_kernel compares A = sum rho_b <s_b, g> with B = sum rho_b sg_b: every proof holds -sg (B = -A: the same x), every proof holds (zeta x, y) or
    (zeta^2 x, y) (B = phi(A): the same y), 23 true instances and one -sg.  A folded comparison that accepts -- x only, y only, up to sign, or 1 whenever no point
    is malformed -- answers ones for the whole batch without a per-proof check; the model's verdicts are zeros (but for the 23)"""
    rho = C.sg_rho(curve)
    pre, sgs, truth, what = C.sg_folded_batch(curve, k, name)
    assert C.sg_folded_model(curve, sgs, truth, rho) == 0
    want = [C.sg_model(sgs[b], truth[b]) for b in range(C.SG_BATCH)]
    got = gctx.accumulator_check_batch(curve, k, pre, sgs, rho).tolist()
    report(f"sg gate, folded comparison, {name}, curve {curve}", what, got, want)
    assert got == want, differing(what, got, want)
    assert want.count(0) == (1 if name == "one -sg" else C.SG_BATCH)


def test_sg_gate_in_the_parts_of_a_grouped_search(gctx, oracle):
    """The folded comparison per part (xyzz_compare_parts_kernel) decides only in the accumulator leg of a job searched in groups (mina_ctx_set_search_groups), and
    that leg is Vesta's: the 24 at k = 8 through mina_state_job_batch with only that leg on, in groups of 8 and over the fan.  The verdicts are the model's, and the
    counters say the grouped search ran: one search, the rounds and parts of the splitting rule for these culprits.  The mixed batch (its off-curve word
    fails the parts that hold it before they compare) and the batches of canonical points in which the comparison of every part decides alone: with -sg or an
    endomorphism image in every proof, EVERY part of every round has B = -A or phi(A).  mina_accumulator_check_batch has no grouped search (its per-proof route is
    xyzz_eq_affine_kernel whatever the group count), and no entry point runs a Pallas accumulator leg: the Pallas instantiation of the parts kernel in this form
    stays untested."""
    curve, k = C.SG_SHAPES[0]
    assert curve == 1
    acc_leg = dict(with_states=False, with_ipa=False, with_acc=True, acc_k=k)
    for name in C.SG_FOLDED:
        pre, sgs, truth, what = C.sg_folded_batch(curve, k, name)
        want = [C.sg_model(sgs[b], truth[b]) for b in range(C.SG_BATCH)]
        jobs = [{"acc_pre": pre[b * k:(b + 1) * k], "acc_sg": sgs[b], "abi": None} for b in range(C.SG_BATCH)]
        try:
            for G in (8, 0):
                gctx.set_search_groups(G)
                s0 = gctx.search_stats()
                got = gctx.state_job_batch(leg(jobs, None, **acc_leg)).tolist()
                s1 = gctx.search_stats()
                stats = {key: s1[key] - s0[key] for key in s1}
                report(f"sg gate, accumulator leg, {name}, groups of {G}", what, got, want)
                assert got == want, (name, G, differing(what, got, want))
                r, p = simulate(C.SG_BATCH, G, {b for b in range(C.SG_BATCH) if not want[b]}) if G else (0, 0)
                assert stats == {"searches": 1 if G else 0, "rounds": r, "parts": p}, (name, G, stats)
        finally:
            gctx.set_search_groups(0)
    pre, sgs, truth, what = C.sg_batch(curve, k)
    want = [C.sg_model(sgs[b], truth[b]) for b in range(C.SG_BATCH)]
    as_jobs = lambda s: [{"acc_pre": pre[b * k:(b + 1) * k], "acc_sg": s[b], "abi": None} for b in range(C.SG_BATCH)]
    try:
        for G in (8, 0):
            gctx.set_search_groups(G)
            s0 = gctx.search_stats()
            got = gctx.state_job_batch(leg(as_jobs(sgs), None, **acc_leg)).tolist()
            s1 = gctx.search_stats()
            stats = {key: s1[key] - s0[key] for key in s1}
            report(f"sg gate, accumulator leg, groups of {G}", what, got, want)
            print(stats)
            assert got == want, (G, differing(what, got, want))
            r, p = simulate(C.SG_BATCH, G, set(C.SG_BATCH_BAD)) if G else (0, 0)
            assert stats == {"searches": 1 if G else 0, "rounds": r, "parts": p}, (G, stats)
            s0 = gctx.search_stats()
            assert gctx.state_job_batch(leg(as_jobs(truth), None, **acc_leg)).tolist() == [1] * C.SG_BATCH
            assert gctx.search_stats() == s0, "a clean batch is searched by nobody"
    finally:
        gctx.set_search_groups(0)
