"""The deduplicated protocol-state leg (mina_ctx_set_state_dedup, MINA_VERIFY_DEDUP_STATES): identical records of a job are found on the GPU, Poseidon runs once
per distinct record, and EVERY output -- rep[], hashes, body hashes, verdict words, flags -- is bit-identical to the mode off and to the CPU oracle, also when the
fingerprint is cut to a few bits so that different records collide all the time (equality of the records decides, never the fingerprint)."""
import copy
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SLOTS = 64
SMALL = dict(k=7, log2_domain=7, npub=8, n_comms=6, slot=2, n_points=2, acc_k=8)      # the small job shape of tests/test_state_job.py


def expected_rep(recs, nf):
    """rep[] from the definition: the smallest index with the same clamped field count and the same first 1 + n_body_fields slots"""
    first, rep = {}, np.zeros(len(nf), np.uint32)
    for i in range(len(nf)):
        c = min(int(nf[i]), SLOTS - 1)
        key = (c, recs[i, : (1 + c) * 32].tobytes())
        rep[i] = first.setdefault(key, i)
    return rep


def base_records(n_states=40, seed=11):
    from oracle import mina_state_ref as S, state_job_ref as J
    from state_job_helpers import state_records
    rng = random.Random(seed)
    states = [J.synth_state(rng, rng.randrange(S.P), 100 + i) for i in range(n_states)]
    recs, nf = state_records(states)
    return states, recs, nf


@pytest.fixture(scope="module")
def mixed():
    """~400 records: 40 synthetic states repeated in shuffled order + pairs that differ in one bit of the last used slot (a), in n_body_fields only (b), only in a
    slot past n_body_fields (c), only in slot 0 (d)"""
    states, recs, nf = base_records()
    rng = np.random.Generator(np.random.PCG64(5))
    order = np.concatenate([rng.permutation(40) for _ in range(10)])[:392]
    R, N, src = [recs[i].copy() for i in order], [int(nf[i]) for i in order], [int(i) for i in order]
    a = recs[3].copy(); a[(int(nf[3]) + 1) * 32 - 1] ^= 0x20                       # (a) last used slot, one bit
    R.append(a); N.append(int(nf[3])); src.append(None)
    R.append(recs[5].copy()); N.append(int(nf[5]) - 1); src.append(None)           # (b) equal bytes, one field fewer
    c = recs[7].copy(); c[(int(nf[7]) + 1) * 32 + 9] ^= 0xff                       # (c) first slot PAST the used ones: the same record
    R.append(c); N.append(int(nf[7])); src.append(7)
    d = recs[9].copy(); d[0] ^= 1                                                  # (d) slot 0
    R.append(d); N.append(int(nf[9])); src.append(None)
    big = recs[11].copy(); R.append(big); N.append(int(nf[11]) + 1000); src.append(None)      # a count past the record clamps to 63: distinct from state 11 (more slots count)
    R.append(big.copy()); N.append(63); src.append(None)                           # ... and the same as that one after the clamp
    recs2 = np.stack(R); nf2 = np.array(N, np.uint32)
    rep = expected_rep(recs2, nf2)
    assert rep[394] == int(np.flatnonzero(order == 7)[0]) and rep[392] == 392 and rep[393] == 393 and rep[395] == 395 and rep[396] == 396 and rep[397] == 396
    return dict(states=states, recs=recs2, nf=nf2, rep=rep, src=src)


def run_dedup_dev(ctx, recs, nf, bits):
    n = len(nf)
    d_rec = ctx.dev_upload(ctx.dev_malloc(recs.size), recs); d_nf = ctx.dev_upload(ctx.dev_malloc(4 * n), nf.view(np.uint8))
    d_rep = ctx.dev_malloc(4 * n); d_cnt = ctx.dev_malloc(8)
    try:
        ctx.protocol_state_dedup_dev(n, d_rec, d_nf, d_rep, d_cnt, bits)
        rep = ctx.dev_download(d_rep, 4 * n).view(np.uint32).copy()
        cnt = ctx.dev_download(d_cnt, 8).view(np.uint32).copy()
    finally:
        for p in (d_rec, d_nf, d_rep, d_cnt):
            ctx.dev_free(p)
    return rep, int(cnt[0]), int(cnt[1])


def test_rep_is_exact_and_canonical(ctx, mixed):
    import mina_bridge_amd as m
    recs, nf, want = mixed["recs"], mixed["nf"], mixed["rep"]
    distinct = int((want == np.arange(len(want))).sum())
    assert distinct == 40 + 4                                      # (a), (b), (d) and the clamped record stand alone; (c) and the clamped record's twin merge
    for bits in (0, 16, 4, 1):
        rep, n_distinct, n_coll = run_dedup_dev(ctx, recs, nf, bits)
        print(f"fingerprint_bits={bits}: n_distinct={n_distinct} n_collisions={n_coll}")
        assert (rep == want).all(), (bits, np.flatnonzero(rep != want)[:8])
        assert n_distinct == distinct, bits
        if bits in (4, 1):
            assert n_coll > 0, bits                                # 44 distinct records in at most 16 keys
    # n = 1; all records identical; a record that clamps
    rep, nd, _ = run_dedup_dev(ctx, recs[:1].copy(), nf[:1].copy(), 0)
    assert rep.tolist() == [0] and nd == 1
    same = np.tile(recs[17], (300, 1)); same_nf = np.full(300, nf[17], np.uint32)
    for bits in (0, 1):
        rep, nd, _ = run_dedup_dev(ctx, same, same_nf, bits)
        assert not rep.any() and nd == 1
    with pytest.raises(m.MinaError) as e:
        run_dedup_dev(ctx, recs, nf, 33)
    assert "(-1)" in str(e.value)                                  # MINA_ERR_ARG


def test_hashes_equal_the_oracle_and_the_plain_path(ctx, oracle, mixed):
    from oracle import mina_state_ref as S
    from state_job_helpers import pp_fp
    recs, nf, want = mixed["recs"], mixed["nf"], mixed["rep"]
    plain_nf = np.minimum(nf, SLOTS - 1)                           # the host entry points refuse a count past the record; the device clamp is covered above
    h0, b0 = ctx.protocol_state_hash_batch(recs, plain_nf, want_body=True)
    h1, b1, nd = ctx.protocol_state_hash_batch_dedup(recs, plain_nf, want_body=True)
    assert (h0 == h1).all() and (b0 == b1).all()
    assert nd == int((expected_rep(recs, plain_nf) == np.arange(len(nf))).sum())
    h2, nd2 = ctx.protocol_state_hash_batch_dedup(recs, plain_nf)
    assert (h2 == h0).all() and nd2 == nd
    pp = pp_fp()
    ref = [S.protocol_state_hash(s, pp) for s in mixed["states"]]
    refb = [S.protocol_state_body_hash(s["body"], pp) for s in mixed["states"]]
    seen = set()
    for i, s in enumerate(mixed["src"]):
        if s is not None:
            assert oracle.le_to_int(h1[i]) == ref[s] and oracle.le_to_int(b1[i]) == refb[s], i
            seen.add(s)
    assert seen == set(range(40))


def tiled(n, distinct, recs, nf):
    """n records: `distinct` different ones (a counter in slot 0 of each), the rest repeats of them in a scrambled order"""
    base = np.arange(n) if distinct >= n else np.concatenate([np.arange(distinct), (np.arange(n - distinct) * 7919 + 13) % distinct])
    out = recs[base % len(nf)].copy(); onf = nf[base % len(nf)].copy()
    out[:, :4] = base.astype(np.uint32).view(np.uint8).reshape(-1, 4)
    return out, onf, distinct if distinct < n else n


def test_every_lane_form(ctx):
    """the deduplicated path against the plain one (which the existing tests pin to the oracle) at sizes that reach every form pstate_hash_lanes can choose"""
    _, recs, nf = base_records(12, seed=3)
    for n in (300, 2000, 8300):                                    # 16-, 8- and 3-lane form of a lone call
        for frac in (0.0, 15 / 16, 1.0):
            r, f, d = tiled(n, n if frac == 0 else max(1, int(round(n * (1 - frac)))), recs, nf)
            h0, b0 = ctx.protocol_state_hash_batch(r, f, want_body=True)
            h1, b1, nd = ctx.protocol_state_hash_batch_dedup(r, f, want_body=True)
            assert nd == d and (h0 == h1).all() and (b0 == b1).all(), (n, frac)
    # the single-lane form: several jobs in flight, and records x lanes reaches HASH1_MIN_STATES (ctx.h hash_one_lane)
    n = 16 * 1024 + 64
    ctx.set_pipeline(4)
    try:
        for frac in (0.0, 15 / 16, 1.0):
            r, f, d = tiled(n, n if frac == 0 else max(1, int(round(n * (1 - frac)))), recs, nf)
            h0 = ctx.protocol_state_hash_batch(r, f)
            h1, nd = ctx.protocol_state_hash_batch_dedup(r, f)
            assert nd == d and (h0 == h1).all(), (n, frac)
    finally:
        ctx.set_pipeline(1)


# ------------------------------------------------------------------------------------------------ the job
@pytest.fixture(scope="module")
def window_jobs(srs_oracle):
    """24 proofs whose candidate chains are the windows [t, t + 16) of ONE chain of 40 linked states, all with the same bridge tip state; a handful of minted openings /
    accumulators in the small shape, reused cyclically"""
    from oracle import state_job_ref as J
    from state_job_helpers import mint_job, pp_fp, state_records
    minted = [mint_job(srs_oracle[0], srs_oracle[1], 300 + 10 * i, **SMALL) for i in range(4)]
    states, hashes = J.synth_chain(random.Random(41), pp_fp(), n=40)
    jobs = []
    for t in range(24):
        j = copy.deepcopy(minted[t % len(minted)])
        j["states"] = [copy.deepcopy(s) for s in states[t:t + 16]] + [copy.deepcopy(states[40])]
        j["expected"] = list(hashes[t:t + 16]) + [hashes[40]]
        j["records"], j["nfields"] = state_records(j["states"])
        jobs.append(j)
    return jobs


def tamper(jobs, proofs, chain_state=20):
    from state_job_helpers import state_records
    out = [copy.deepcopy(j) for j in jobs]
    for t in proofs:
        out[t]["states"][chain_state - t]["body"]["consensus_state"]["total_currency"] ^= 1
        out[t]["records"], out[t]["nfields"] = state_records(out[t]["states"])
    return out


def build(m, jobs):
    from state_job_helpers import build_jobs
    return build_jobs(m, jobs, SMALL["k"], SMALL["log2_domain"], SMALL["slot"], SMALL["acc_k"])


def n_distinct_records(jobs):
    recs = np.concatenate([j["records"] for j in jobs]); nf = np.concatenate([j["nfields"] for j in jobs])
    return int((expected_rep(recs, nf) == np.arange(len(nf))).sum())


def test_sliding_window_job_against_the_oracle(ctx_srs, srs_oracle, window_jobs):
    import mina_bridge_amd as m
    from oracle import state_job_ref as J
    from state_job_helpers import oracle_job, pp_fp
    ctx = ctx_srs
    carriers = list(range(5, 21))                                  # the windows that hold chain state 20
    all_bad, one_bad = tamper(window_jobs, carriers), tamper(window_jobs, [9])
    assert n_distinct_records(window_jobs) == 40 and n_distinct_records(all_bad) == 40 and n_distinct_records(one_bad) == 41
    off = [ctx.state_job_batch(build(m, j)).tolist() for j in (window_jobs, all_bad, one_bad)]
    ctx.set_state_dedup(True)
    try:
        assert ctx.state_dedup_stats() == (0, 0, 0)
        v = ctx.state_job_batch(build(m, window_jobs)).tolist()
        st = ctx.state_dedup_stats()
        print("stats after the clean job:", st)
        assert v == [1] * 24 == off[0]
        assert st.states == 24 * 17 == 408 and st.distinct == 40
        v = ctx.state_job_batch(build(m, all_bad)).tolist()
        assert v == [0 if t in carriers else 1 for t in range(24)] == off[1]
        for t in (9, 2):                                           # one rejected, one accepted proof through the oracle composite
            assert J.verify_state_job(pp_fp(), srs_oracle[0], srs_oracle[1], oracle_job(all_bad[t]))["verdict"] == bool(v[t])
        v = ctx.state_job_batch(build(m, one_bad)).tolist()
        assert v == [0 if t == 9 else 1 for t in range(24)] == off[2]
        st = ctx.state_dedup_stats()
        assert st.states == 3 * 408 and st.distinct == 40 + 40 + 41
    finally:
        ctx.set_state_dedup(False)
    assert ctx.state_job_batch(build(m, window_jobs)).tolist() == [1] * 24      # off again: nothing added to the statistics
    assert ctx.state_dedup_stats().states == 3 * 408


@pytest.mark.parametrize("dev_fork", [0, 1])
def test_device_resident_forked_and_pipelined(oracle, window_jobs, dev_fork):
    """the sliding-window job through mina_state_job_batch_dev with the mode on, one stream / forked legs, 1 and 4 lanes, six jobs in flight: verdict words and flags equal
    the mode off; one run through mina_state_job_fold_dev: the per-proof verdict words equal the mode off"""
    import mina_bridge_amd as m
    B = len(window_jobs)
    variants = {"good": window_jobs, "shared_bad": tamper(window_jobs, range(5, 21)), "one_bad": tamper(window_jobs, [9])}
    with m.lib.tuning(dev_fork=dev_fork):
        c = m.MinaContext(0)                                       # a context of its own per tuning: streams keep their mask / priority for life
        try:
            for f in (0, 1):
                c.poseidon_set_params(f, m.poseidon_params.default_params_bytes(f))
            c.srs_create(0, 1 << 10); c.srs_create(1, 1 << 10)
            c.state_jobs_prepare(SMALL["log2_domain"], SMALL["npub"])
            dev = {name: c.state_jobs_to_device(build(m, jobs)) for name, jobs in variants.items()}
            calls = [name for _ in range(2) for name in variants]  # six jobs in flight
            words = {}
            for lanes in (1, 4):
                for on in (False, True):
                    c.set_pipeline(lanes)
                    c.set_state_dedup(on)
                    outs = [c.dev_malloc(4 * B + 16) for _ in calls]
                    for name, o in zip(calls, outs):
                        c.state_job_batch_dev(dev[name][0], o, o + 4 * B)
                    c.synchronize()
                    words[(lanes, on)] = [c.dev_download(o, 4 * B + 16).view(np.uint32).tolist() for o in outs]
                    for o in outs:
                        c.dev_free(o)
                assert words[(lanes, True)] == words[(lanes, False)], (dev_fork, lanes)
                for name, w in zip(calls, words[(lanes, True)]):
                    bad = {"good": [], "shared_bad": list(range(5, 21)), "one_bad": [9]}[name]
                    assert w[:B] == [0 if t in bad else 1 for t in range(B)] and w[B:] == [1, 0, 1, 0], (dev_fork, lanes, name)
                if lanes == 4:
                    st = c.state_dedup_stats()
                    assert st.states == 6 * 17 * B and st.distinct == 2 * (40 + 40 + 41)
            # the exchange variant: per-proof verdict words (the folded scalars depend on a randomiser drawn per call)
            c.set_pipeline(1)
            fold = {}
            bufs = [c.dev_malloc(x) for x in (4 * B + 16, 32 << SMALL["k"], 17 * 4, 32 << SMALL["acc_k"], 17 * 4)]
            for on in (False, True):
                c.set_state_dedup(on)
                c.state_job_fold_dev(dev["shared_bad"][0], bufs[0], bufs[0] + 4 * B, bufs[1], bufs[2], bufs[3], bufs[4])
                c.synchronize()
                fold[on] = c.dev_download(bufs[0], 4 * B).view(np.uint32).tolist()
            assert fold[True] == fold[False] == [0 if 5 <= t <= 20 else 1 for t in range(B)]
            c.set_state_dedup(False)
            for p in bufs:
                c.dev_free(p)
            for d, ptrs in dev.values():
                for p in ptrs:
                    c.dev_free(p)
        finally:
            c.close()


def test_boundary_deduplicates_per_chunk_with_the_same_verdicts(oracle):
    """MINA_VERIFY_DEDUP_STATES: serialized proofs that share all their chain states (the same case several times), one copy with a tampered shared state, and a case
    whose every copy carries the tampered state: the verdicts of mina_verify_state_batch equal those without the flag, in one chunk and in small streamed chunks"""
    import mina_bridge_amd as m
    from ipa_helpers import poseidon_pp
    from kimchi_helpers import install_index, install_step_index, load_k15_fixture, load_statement_fixture, make_chain, make_step_index
    from oracle import mina_state_ref as S
    from wire_writers import state_proof_bytes, state_pub_bytes
    ix, _, _ = load_k15_fixture()
    items, _ = load_statement_fixture()
    cases = []
    for it in items[:3]:
        states, hashes = make_chain(random.Random(it["chain_seed"]), poseidon_pp(0))
        p, ev = it["proof"], it["proof"]["evals"]
        wrap = dict(it["wrap"])
        wrap.update(w_comm=p["w_comm"], z_comm=p["z_comm"], t_comm=p["t_comm"], z_eval=ev[0], selector_eval=ev[1:7], w_eval=ev[7:22], coefficients_eval=ev[22:37],
                    s_eval=ev[37:43], ft_eval1=p["ft_eval1"], lr=p["opening"]["lr"], z1=p["opening"]["z1"], z2=p["opening"]["z2"], delta=p["opening"]["delta"], sg=p["opening"]["sg"])
        pub = state_pub_bytes(True, hashes[16], hashes[:16], [S.snarked_ledger_hash(s) for s in states[:16]])
        bad_states = copy.deepcopy(states); bad_states[6]["body"]["consensus_state"]["total_currency"] ^= 1
        cases.append(dict(good=state_proof_bytes(wrap, states), bad=state_proof_bytes(wrap, bad_states), pub=pub))
    #          case 0 x 3, one copy tampered | case 1 x 3, every copy tampered | case 2 x 2 clean
    proofs = [cases[0]["good"], cases[0]["bad"], cases[0]["good"], cases[1]["bad"], cases[1]["bad"], cases[1]["bad"], cases[2]["good"], cases[2]["good"]]
    pubs = [cases[0]["pub"]] * 3 + [cases[1]["pub"]] * 3 + [cases[2]["pub"]] * 2
    want = [1, 0, 1, 0, 0, 0, 1, 1]
    got = {}
    try:
        for flags in (m.lib.VERIFY_ALLOW_SURROGATE, m.lib.VERIFY_ALLOW_SURROGATE | m.lib.VERIFY_DEDUP_STATES):
            m.lib.verify_shutdown()
            m.lib.verify_configure(flags)
            gctx = m.lib.verify_global_ctx()
            install_index(gctx, ix)
            install_step_index(gctx, make_step_index(99))
            got[flags] = [m.lib.verify_state_batch(proofs, pubs).tolist()]
            with m.lib.tuning(chunk=3, single_max=1, early_min=1, early_sub=2, head_min=0):      # several chunks, their records streamed in runs: deduplication is per chunk
                got[flags].append(m.lib.verify_state_batch(proofs, pubs).tolist())
            if flags & m.lib.VERIFY_DEDUP_STATES:
                st = gctx.state_dedup_stats()
                print("boundary stats:", st)
                assert 0 < st.distinct < st.states and st.states % 17 == 0      # (how many of the 2 x 8 x 17 states this device saw depends on the box's GPU count)
    finally:
        m.lib.verify_configure(0)
        m.lib.verify_shutdown()
    assert got[m.lib.VERIFY_ALLOW_SURROGATE] == [want, want]
    assert got[m.lib.VERIFY_ALLOW_SURROGATE | m.lib.VERIFY_DEDUP_STATES] == [want, want]
