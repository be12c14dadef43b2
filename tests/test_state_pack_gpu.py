"""The packed-on-device front end on the GPU (mina_protocol_state_pack_dev, mina_state_frontend_dev, MINA_VERIFY_PACK_ON_DEVICE).  The checker is the HOST path --
mina_protocol_state_pack, the mina_consensus_* entry points, hashlib's Blake2b (tests/state_pack_helpers.py) -- and, for verdicts, the CPU oracle; every output
of the kernels is compared byte for byte, for well-formed states, for the exhaustive small mutations of one state in one launch, for proofs built per
chain-selection branch, inside a composed device-resident job, and through the boundary with the flag off and on."""
import copy
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import state_pack_helpers as H  # noqa: E402

pytestmark = pytest.mark.gpu

SMALL = dict(k=7, log2_domain=7, npub=8, n_comms=6, slot=2, n_points=2, acc_k=8)      # the small job shape of tests/test_state_job.py


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


def pack_dev(ctx, m, cases, extra=(), with_info=True):
    blob, off, ln = H.blob_of(cases)
    off = np.concatenate([off, np.array([e[0] for e in extra], np.uint64)]); ln = np.concatenate([ln, np.array([e[1] for e in extra], np.uint32)])
    n, isz = len(off), H.info_size(m)
    d = Dev(ctx)
    try:
        d_blob, d_off, d_len = d.put(blob), d.put(off), d.put(ln)
        d_rec, d_nf, d_info, d_st = d.new(n * H.REC), d.new(4 * n), d.new(n * isz), d.new(n)
        ctx.protocol_state_pack_dev(n, d_blob, len(blob), d_off, d_len, d_rec, d_nf, d_info if with_info else 0, d_st)
        ctx.synchronize()
        return (ctx.dev_download(d_st, n).copy(), ctx.dev_download(d_nf, 4 * n).view(np.uint32).copy(), ctx.dev_download(d_rec, n * H.REC).reshape(n, H.REC).copy(),
                ctx.dev_download(d_info, n * isz).reshape(n, isz).copy(), len(blob))
    finally:
        d.free()


def test_well_formed_states_are_packed_byte_for_byte(ctx):
    """chains of kimchi_helpers.make_chain, 0 / 1 / 11 / 16 / 64 sub-windows, non-empty failure-status tables, extreme values, the reference's own tip state
    re-encoded to bincode: records, field counts, info structs and status equal the host's"""
    import mina_bridge_amd as m
    cases = [(name, H.bincode_state(st)) for name, st in H.well_formed_states()]
    status, nf, recs, infos, _ = pack_dev(ctx, m, cases)
    acc, rej = H.check_pack_results(m, cases, status, nf, recs, infos)
    assert rej == 0 and acc == len(cases) >= 24
    # without info structs: the same records
    status2, nf2, recs2, infos2, _ = pack_dev(ctx, m, cases, with_info=False)
    assert (status2 == status).all() and (nf2 == nf).all() and (recs2 == recs).all() and (infos2 == 0xcd).all()


def test_every_small_mutation_in_one_launch(ctx):
    """one state: every truncation, a trailing byte, a flipped bit at every byte position, p / 2^255 / p - 1 in each of the 40 element positions, every string
    length 31 and 33, 65 sub-windows -- one launch, every case compared with the host reader, none skipped; slices past the blob are status 0"""
    import mina_bridge_amd as m
    st = dict(H.well_formed_states())["chain[3]"]
    cases = H.mutations(st)
    blob_len = len(H.blob_of(cases)[0])
    past = [(blob_len - 10, 1542), (blob_len, 1), (blob_len + 1, 0), ((1 << 64) - 1, 1), ((1 << 64) - 8, 0xffffffff)]
    status, nf, recs, infos, _ = pack_dev(ctx, m, cases, past)
    acc, rej = H.check_pack_results(m, cases, status[:len(cases)], nf, recs, infos)
    print(f"{len(cases)} mutations of one state: {acc} accepted, {rej} rejected by both readers")
    assert acc + rej == len(cases) and acc >= 40 and rej >= 1542
    assert not status[len(cases):].any() and not recs[len(cases):].any() and not nf[len(cases):].any()


def frontend_dev(ctx, proofs, masks=True, use_and=True):
    blob, begin, end, exp, led, band = H.frontend_inputs(proofs)
    B = len(proofs); ns = B * H.STATES
    d = Dev(ctx)
    try:
        d_blob, d_b, d_e, d_exp, d_led, d_and = d.put(blob), d.put(begin), d.put(end), d.put(exp), d.put(led), d.put(band)
        d_rec, d_nf, d_pre, d_m = d.new(ns * H.REC), d.new(4 * ns), d.new(B), d.new(4 * B)
        ctx.state_frontend_dev(B, d_blob, len(blob), d_b, d_e, d_exp, d_led, d_and if use_and else 0, d_rec, d_nf, d_pre, d_m if masks else 0)
        ctx.synchronize()
        return (ctx.dev_download(d_rec, ns * H.REC).copy(), ctx.dev_download(d_nf, 4 * ns).view(np.uint32).copy(), ctx.dev_download(d_pre, B).copy(),
                ctx.dev_download(d_m, 4 * B).view(np.uint32).copy())
    finally:
        d.free()


def test_precheck_per_branch(ctx):
    """short range in the same and in adjacent epochs, long range with the candidate denser / equal / sparser (windows projected over 2 .. 40 sub-windows), length
    ties decided by the VRF hash and by the state hash, mismatched sub-window counts, slots_per_sub_window = 0, a wrong ledger hash in each of the 16 positions,
    malformed state halves: precheck bytes, masks, records and field counts equal the host's; no class is empty"""
    import mina_bridge_amd as m
    proofs = H.precheck_proofs()
    recs, nf, pre, masks = frontend_dev(ctx, proofs)
    branches = H.check_frontend_results(m, proofs, recs, nf, pre, masks)
    counts = {b: branches.count(b) for b in sorted(set(branches))}
    print(counts)
    for b in H.REQUIRED_BRANCHES:
        assert counts.get(b, 0) >= 1, (b, counts)
    ledger_bad = [i for i, p in enumerate(proofs) if p[0].startswith("wrong ledger hash")]
    assert len(ledger_bad) == 16 and all(int(masks[i]) == H.CHECK_FORMAT | H.CHECK_CONSENSUS and pre[i] == 0 for i in ledger_bad)
    # no `and` bytes, no masks: the same precheck but for the one proof whose byte was cleared
    recs2, nf2, pre2, _ = frontend_dev(ctx, proofs, masks=False, use_and=False)
    cleared = [i for i, p in enumerate(proofs) if p[4] == 0]
    assert (recs2 == recs).all() and (nf2 == nf).all() and len(cleared) == 1
    assert [int(x) for x in pre2] == [1 if i in cleared else int(x) for i, x in enumerate(pre)]


def test_bad_arguments_are_refused(ctx):
    import mina_bridge_amd as m
    d = Dev(ctx)
    try:
        p = d.new(4096)
        for call in (lambda: ctx.protocol_state_pack_dev(1, p, 64, p + 4, p, p, p, 0, p),            # offsets not 8-byte aligned
                     lambda: ctx.protocol_state_pack_dev(1, p, 64, p, p, p + 8, p, 0, p),            # records not 16-byte aligned
                     lambda: ctx.protocol_state_pack_dev(1, 0, 64, p, p, p, p, 0, p),                # null blob
                     lambda: ctx.state_frontend_dev(1, p, 64, p, p + 4, p, p, 0, p, p, p, 0),        # end not 8-byte aligned
                     lambda: ctx.state_frontend_dev(1, p, 64, p, p, p, p, 0, p, p + 2, p, 0),        # field counts not 4-byte aligned
                     lambda: ctx.state_frontend_dev(1, p, 64, p, p, p, 0, 0, p, p, p, 0)):           # null ledger hashes
            with pytest.raises(m.MinaError) as e:
                call()
            assert "(-1)" in str(e.value)                                  # MINA_ERR_ARG
        ctx.protocol_state_pack_dev(0, 0, 0, 0, 0, 0, 0, 0, 0)             # nothing to do
        ctx.state_frontend_dev(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)
        ctx.synchronize()
    finally:
        d.free()


# ------------------------------------------------------------------------------------------------ the composed device-resident job
def test_frontend_then_job_on_a_pinned_lane(ctx_srs, srs_oracle):
    """serialized proofs' state bytes in HBM -> mina_state_frontend_dev -> mina_state_job_batch_dev, both queued on one pinned lane without a host wait between them.
    One batch: clean proofs, a tampered state, a wrong ledger hash in the public input, a candidate that loses chain selection, a truncated state.  The verdict
    words equal the host-packed route's and the oracle's; again with the deduplicated state leg."""
    import mina_bridge_amd as m
    from kimchi_helpers import make_chain
    from oracle import mina_state_ref as S, oracle as O, state_job_ref as J
    from state_job_helpers import build_jobs, mint_job, oracle_job, pp_fp, state_records
    ctx = ctx_srs
    minted = [mint_job(srs_oracle[0], srs_oracle[1], 700 + 10 * i, **SMALL) for i in range(3)]
    kinds = ["clean", "clean", "tampered state", "wrong ledger hash", "candidate loses", "truncated", "clean", "clean"]
    jobs, proofs = [], []
    for t, kind in enumerate(kinds):
        j = copy.deepcopy(minted[t % len(minted)])
        states, hashes = make_chain(random.Random(9000 + t // 2), pp_fp())           # pairs of proofs share a chain
        states = copy.deepcopy(states); hashes = list(hashes)
        ledger = [S.snarked_ledger_hash(s) for s in states[:16]]
        if kind == "candidate loses":
            states[15]["body"]["consensus_state"]["blockchain_length"] = 900          # shorter than the bridge tip (990) in the same epoch
            hashes[15] = S.protocol_state_hash(states[15], pp_fp())
        if kind == "tampered state":
            states[6]["body"]["consensus_state"]["total_currency"] ^= 1               # its hash no longer matches the public input's
        if kind == "wrong ledger hash":
            ledger[11] ^= 1 << 77
        data = b"".join(H.bincode_state(s) for s in states)
        if kind == "truncated":
            data = data[:-1]
        exp = O.ints_to_le(hashes).tobytes(); led = b"".join(int(x).to_bytes(32, "little") for x in ledger)
        proofs.append((kind, data, exp, led, 1))
        j["states"], j["expected"] = states, hashes
        j["records"], j["nfields"] = state_records(states)
        wrec, wnf, wpre, wmask, _ = H.host_frontend(m, data, exp, led, 1)
        if kind == "truncated":
            assert wmask == 0
            j["records"] = np.zeros_like(j["records"]); j["nfields"] = np.zeros_like(j["nfields"])
        else:
            assert j["records"].tobytes() == wrec and j["nfields"].tolist() == wnf          # host packer == oracle flattening
        j["precheck"] = wpre
        jobs.append(j)
    B = len(jobs)
    want = []
    for j, kind in zip(jobs, kinds):
        ov = kind != "truncated" and J.verify_state_job(pp_fp(), srs_oracle[0], srs_oracle[1], oracle_job(j))["verdict"]
        want.append(1 if (ov and j["precheck"]) else 0)
    assert want == [1, 1, 0, 0, 0, 0, 1, 1]
    hj, keep = build_jobs(m, jobs, SMALL["k"], SMALL["log2_domain"], SMALL["slot"], SMALL["acc_k"])
    pre = np.array([j["precheck"] for j in jobs], np.uint8); hj.precheck = pre.ctypes.data; keep.append(pre)
    assert ctx.state_job_batch((hj, keep)).tolist() == want                             # the host route, host buffers
    ctx.state_jobs_prepare(SMALL["log2_domain"], SMALL["npub"])
    dj, ptrs = ctx.state_jobs_to_device((hj, keep))
    blob, begin, end, exp, led, band = H.frontend_inputs(proofs)
    d = Dev(ctx)
    try:
        d_blob, d_b, d_e, d_led = d.put(blob), d.put(begin), d.put(end), d.put(led)
        d_rec, d_nf, d_pre = d.new(B * H.STATES * H.REC), d.new(4 * B * H.STATES), d.new(B)
        import ctypes
        fj = m.lib.StateJobs(); ctypes.memmove(ctypes.byref(fj), ctypes.byref(dj), ctypes.sizeof(fj))
        fj.state_records, fj.state_nfields, fj.precheck = d_rec, d_nf, d_pre
        words = {}
        for dedup in (False, True):
            ctx.set_state_dedup(dedup)
            outs = [d.new(4 * B + 16), d.new(4 * B + 16)]
            ctx.synchronize()
            ctx.pin_lane(0)
            try:
                ctx.state_job_batch_dev(dj, outs[0], outs[0] + 4 * B)                    # host-packed records, uploaded
                ctx.state_frontend_dev(B, d_blob, len(blob), d_b, d_e, dj.expected_hashes, d_led, 0, d_rec, d_nf, d_pre, 0)
                ctx.state_job_batch_dev(fj, outs[1], outs[1] + 4 * B)                    # packed on the device, no host wait in between
            finally:
                ctx.pin_lane(-1)
            ctx.synchronize()
            words[dedup] = [ctx.dev_download(o, 4 * B + 16).view(np.uint32).tolist() for o in outs]
            assert words[dedup][0] == words[dedup][1], dedup
            assert words[dedup][1][:B] == want, (dedup, words[dedup][1])
            assert ctx.dev_download(d_pre, B).tolist() == pre.tolist()
        assert words[False] == words[True]
    finally:
        ctx.set_state_dedup(False)
        d.free()
        for p in ptrs:
            ctx.dev_free(p)


# ------------------------------------------------------------------------------------------------ the boundary
def test_boundary_packs_on_the_device_with_the_same_verdicts_and_masks(oracle):
    """MINA_VERIFY_PACK_ON_DEVICE, alone and with MINA_VERIFY_DEDUP_STATES: the verdicts of mina_verify_state_batch and the masks of mina_verify_state_checks equal
    those without the flag -- one chunk and small streamed chunks; clean proofs, a tampered shared state, a wrong ledger hash, a candidate that loses chain
    selection, malformed state halves"""
    import mina_bridge_amd as m
    from ipa_helpers import poseidon_pp
    from kimchi_helpers import install_index, install_step_index, load_k15_fixture, load_statement_fixture, make_chain, make_step_index
    from oracle import mina_state_ref as S
    from wire_writers import state_pub_bytes, wrap_proof_bytes
    ix, _, _ = load_k15_fixture()
    items, _ = load_statement_fixture()
    proof_bytes = lambda wrap, states: wrap_proof_bytes(wrap, binprot=False) + b"".join(H.bincode_state(s) for s in states)
    cases = []
    for it in items[:3]:
        states, hashes = make_chain(random.Random(it["chain_seed"]), poseidon_pp(0))
        p, ev = it["proof"], it["proof"]["evals"]
        wrap = dict(it["wrap"])
        wrap.update(w_comm=p["w_comm"], z_comm=p["z_comm"], t_comm=p["t_comm"], z_eval=ev[0], selector_eval=ev[1:7], w_eval=ev[7:22], coefficients_eval=ev[22:37],
                    s_eval=ev[37:43], ft_eval1=p["ft_eval1"], lr=p["opening"]["lr"], z1=p["opening"]["z1"], z2=p["opening"]["z2"], delta=p["opening"]["delta"], sg=p["opening"]["sg"])
        ledger = [S.snarked_ledger_hash(s) for s in states[:16]]
        pub = state_pub_bytes(True, hashes[16], hashes[:16], ledger)
        bad_ledger = list(ledger); bad_ledger[5] ^= 1
        bad_states = copy.deepcopy(states); bad_states[6]["body"]["consensus_state"]["total_currency"] ^= 1
        # a bridge tip that wins: longer than the candidate tip in the same epoch.  Its hash is the public input's, so only CONSENSUS fails.
        strong = copy.deepcopy(states); strong[16]["body"]["consensus_state"]["blockchain_length"] = 5000
        pub_strong = state_pub_bytes(True, S.protocol_state_hash(strong[16], poseidon_pp(0)), hashes[:16], ledger)
        good = proof_bytes(wrap, states)
        cases.append(dict(good=good, bad=proof_bytes(wrap, bad_states), pub=pub, pub_bad_ledger=state_pub_bytes(True, hashes[16], hashes[:16], bad_ledger),
                          strong=proof_bytes(wrap, strong), pub_strong=pub_strong, cut=good[:-1], long=good + b"\0", half=good[:len(good) - 9000]))
    c0, c1, c2 = cases
    proofs = [c0["good"], c0["bad"], c0["good"], c1["good"], c1["strong"], c1["cut"], c2["good"], c2["long"], c2["half"], c2["good"], b"", c1["good"]]
    pubs = [c0["pub"], c0["pub"], c0["pub_bad_ledger"], c1["pub"], c1["pub_strong"], c1["pub"], c2["pub"], c2["pub"], c2["pub"], c2["pub"][:-1], c0["pub"], c1["pub"]]
    want = [1, 0, 0, 1, 0, 0, 1, 0, 0, 0, 0, 1]
    probes = {"good": (c0["good"], c0["pub"]), "ledger-bad": (c0["good"], c0["pub_bad_ledger"]), "consensus-bad": (c1["strong"], c1["pub_strong"]),
              "chain-bad": (c0["bad"], c0["pub"]), "malformed": (c1["cut"], c1["pub"]), "trailing byte": (c2["long"], c2["pub"])}
    base = m.lib.VERIFY_ALLOW_SURROGATE
    modes = (base, base | m.lib.VERIFY_PACK_ON_DEVICE, base | m.lib.VERIFY_PACK_ON_DEVICE | m.lib.VERIFY_DEDUP_STATES)
    got, masks = {}, {}
    try:
        for flags in modes:
            m.lib.verify_shutdown()
            m.lib.verify_configure(flags)
            gctx = m.lib.verify_global_ctx()
            install_index(gctx, ix)
            install_step_index(gctx, make_step_index(99))
            got[flags] = [m.lib.verify_state_batch(proofs, pubs).tolist()]
            with m.lib.tuning(chunk=5, single_max=1, early_min=1, early_sub=2, head_min=0):      # several chunks, their entries streamed in runs
                got[flags].append(m.lib.verify_state_batch(proofs, pubs).tolist())
            with m.lib.tuning(merge=0):                                                          # a call of its own, not merged with other small callers'
                got[flags].append(m.lib.verify_state_batch(proofs, pubs).tolist())
            masks[flags] = {name: tuple(m.lib.verify_state_checks(pr, pu)) for name, (pr, pu) in probes.items()}
            print(flags, masks[flags])
    finally:
        m.lib.verify_configure(0)
        m.lib.verify_shutdown()
    for flags in modes:
        assert got[flags] == [want, want, want], (flags, got[flags])
        assert masks[flags] == masks[base], flags
    F, L, C = m.lib.CHECK_FORMAT, m.lib.CHECK_LEDGER, m.lib.CHECK_CONSENSUS
    sel = lambda name: masks[base][name][0] & (F | L | C)
    assert sel("good") == F | L | C and sel("ledger-bad") == F | C and sel("consensus-bad") == F | L and sel("malformed") == 0 and sel("trailing byte") == 0
    assert masks[base]["chain-bad"][0] & m.lib.CHECK_CHAIN == 0 and masks[base]["good"][0] & m.lib.CHECK_CHAIN
