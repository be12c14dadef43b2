"""Error behaviour at the boundary: bad arguments come back as negative return codes with a message (`MinaError` through the
ctypes wrapper), never as a crash or a silent wrong answer; the context stays usable afterwards."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MINA_ERR_ARG = -1            # include/mina_verify.h


def test_bad_arguments_are_errors_not_crashes(ctx_srs):
    import mina_bridge_amd as m
    c = ctx_srs
    lib = c._lib
    z32, z64 = np.zeros(32, np.uint8), np.zeros(64, np.uint8)
    pre = np.zeros(16 * 16, np.uint8)
    with pytest.raises(m.MinaError):
        c.msm_srs(2, z32)                                            # bad curve
    with pytest.raises(m.MinaError):
        c.msm_srs_multi(1, np.zeros((65537, 32), np.uint8), 1)       # n beyond the SRS depth
    with pytest.raises(m.MinaError):
        c.accumulator_check_batch(1, 21, np.zeros(21 * 16, np.uint8), z64)     # k > 20
    with pytest.raises(m.MinaError):
        c.accumulator_check_batch(1, 17, np.zeros(17 * 16, np.uint8), z64)     # 2^k beyond the SRS depth
    with pytest.raises(m.MinaError):
        c.public_input_commitment_batch(0, 17, np.zeros((1, 32), np.uint8), 1)  # domain beyond the SRS depth
    with pytest.raises(m.MinaError):
        c.public_input_commitment_batch(0, 3, np.zeros((9, 32), np.uint8), 1)   # more public inputs than the domain
    with pytest.raises(m.MinaError):
        c.set_pipeline(0)
    with pytest.raises(m.MinaError):
        c.set_pipeline(33)
    d = c.dev_malloc(64)
    try:
        with pytest.raises(m.MinaError):
            c.accumulator_check_multi_dev(1, 16, 0, d, d, d)          # empty group
        with pytest.raises(m.MinaError):
            c.accumulator_check_multi_dev(1, 16, 65, d, d, d)         # group larger than 64
        with pytest.raises(m.MinaError):
            c.accumulator_check_multi_dev(1, 16, 1, 0, d, d)          # null device pointer
    finally:
        c.dev_free(d)
    # raw C calls with null pointers
    assert lib.mina_msm_srs(c._h, 1, ctypes.c_size_t(4), None, None) < 0
    assert lib.mina_dev_malloc(c._h, ctypes.c_size_t(16), None) < 0
    assert lib.mina_accumulator_check_multi(c._h, 1, ctypes.c_uint32(16), ctypes.c_size_t(1), None, None, None) < 0
    assert b"null" in lib.mina_last_error()
    # the 29-bit self-test hook: null pointers, a field that is none, an op that is none -- MINA_ERR_ARG each, before anything is launched
    rows_in, rows_out = np.zeros(m.lib.FE29_IN_WORDS, np.uint32), np.zeros(m.lib.FE29_OUT_WORDS, np.uint32)
    pin, pout, op = rows_in.ctypes.data_as(ctypes.c_void_p), rows_out.ctypes.data_as(ctypes.c_void_p), m.lib.FE29_OPS["MUL_SG"]
    for bad in ((None, 0, op, 1, pin, pout), (c._h, 0, op, 1, None, pout), (c._h, 0, op, 1, pin, None), (c._h, 2, op, 1, pin, pout), (c._h, -1, op, 1, pin, pout),
                (c._h, 0, max(m.lib.FE29_OPS.values()) + 1, 1, pin, pout), (c._h, 0, -1, 1, pin, pout), (c._h, 0, 20, 1, pin, pout)):
        assert lib.mina_selftest_fe29(bad[0], bad[1], bad[2], ctypes.c_size_t(bad[3]), bad[4], bad[5]) == MINA_ERR_ARG, bad[1:4]
    assert 20 not in m.lib.FE29_OPS.values() and lib.mina_selftest_fe29(c._h, 0, op, ctypes.c_size_t(0), None, None) == 0      # (a gap between the op groups; no rows: nothing to do)
    with pytest.raises(m.MinaError, match="bad op"):
        c.selftest_fe29(0, 31, rows_in)
    assert lib.mina_selftest_fe29(c._h, 0, op, ctypes.c_size_t(1), pin, pout) == 0 and not rows_out[9:].any()
    # the 8 x 32 self-test hook, the same way
    rows_in, rows_out = np.zeros(m.lib.FE32_IN_WORDS, np.uint32), np.full(m.lib.FE32_OUT_WORDS, 7, np.uint32)
    pin, pout, op = rows_in.ctypes.data_as(ctypes.c_void_p), rows_out.ctypes.data_as(ctypes.c_void_p), m.lib.FE32_OPS["MUL"]
    for bad in ((None, 0, op, 1, pin, pout), (c._h, 0, op, 1, None, pout), (c._h, 0, op, 1, pin, None), (c._h, 2, op, 1, pin, pout), (c._h, -1, op, 1, pin, pout),
                (c._h, 0, max(m.lib.FE32_OPS.values()) + 1, 1, pin, pout), (c._h, 0, -1, 1, pin, pout), (c._h, 0, 14, 1, pin, pout), (c._h, 0, op, (1 << 22) + 1, pin, pout)):
        assert lib.mina_selftest_fe32(bad[0], bad[1], bad[2], ctypes.c_size_t(bad[3]), bad[4], bad[5]) == MINA_ERR_ARG, bad[1:4]
    assert 14 not in m.lib.FE32_OPS.values() and lib.mina_selftest_fe32(c._h, 0, op, ctypes.c_size_t(0), None, None) == 0      # (a gap between the op groups; no rows: nothing to do)
    with pytest.raises(m.MinaError, match="bad op"):
        c.selftest_fe32(0, 31, rows_in)
    assert lib.mina_selftest_fe32(c._h, 0, op, ctypes.c_size_t(1), pin, pout) == 0 and not rows_out.any()                      # 0 * 0, unused slots and the flag zero
    # and the context still computes
    one = np.zeros(32, np.uint8); one[0] = 1
    assert (c.msm_srs(1, one) == c.srs_get_g(1, 0, 1)[0]).all()
    assert c.accumulator_check_multi(1, 16, pre, z64).tolist() == [0]


@pytest.mark.gpu
def test_scalars_with_bit_255_set_are_rejected_and_small_srs_roundtrips(ctx_srs, oracle, srs_oracle):
    """the signed-digit recoding has no window for a carry out of bit 255 -> such scalars are an argument error, not a
    silently wrong point; mina_srs_load / serialize use the minimal MessagePack array header (fixarray / array16 / array32)"""
    import mina_bridge_amd as m
    g, _ = srs_oracle[1]
    sc = np.zeros((4, 32), np.uint8); sc[2, 31] = 0x80
    for call in (lambda: ctx_srs.msm_srs(1, sc), lambda: ctx_srs.msm(1, g[:4], sc), lambda: ctx_srs.msm_srs_multi(1, sc, 2), lambda: ctx_srs.msm_srs_range(1, 0, sc),
                 lambda: ctx_srs.public_input_commitment(0, 5, sc)):
        with pytest.raises(m.MinaError, match="2\\^255"):
            call()
    sc[2, 31] = 0x7f                                            # non-canonical but below 2^255: still computed (digits are exact)
    ctx_srs.msm_srs(1, sc)
    with pytest.raises(m.MinaError):                            # k is validated before anything is sized from it
        ctx_srs.accumulator_check_batch(1, 0, np.zeros(0, np.uint8), np.zeros(64, np.uint8))
    with pytest.raises(m.MinaError):
        ctx_srs.accumulator_check_multi(1, 40, np.zeros(40 * 16, np.uint8), np.zeros(64, np.uint8))
    c2 = m.MinaContext(0)
    try:
        for depth, hdr in ((8, 2), (32, 4)):
            c2.srs_create(1, depth)
            blob = c2.srs_serialize(1)
            assert len(blob) == hdr + (depth + 1) * 35 and blob[0] == 0x92 and blob[1] == ((0x90 | depth) if depth < 16 else 0xdc)
            pts = c2.srs_get_g(1, 0, depth)
            c2.srs_load(1, blob)
            assert (c2.srs_get_g(1, 0, depth) == pts).all() and (pts == g[:depth]).all()
    finally:
        c2.close()


@pytest.mark.gpu
def test_statement_and_kimchi_sections_reject_bad_shapes(oracle):
    """round-2 entry points: misuse is an error code, never a crash or a silent wrong answer -- the statement stage without a step index,
    impossible shapes, null sections, a kimchi section whose statements do not derive exactly 40 public inputs"""
    import ctypes
    import mina_bridge_amd as m
    from kimchi_helpers import install_index, install_step_index, load_k15_fixture, make_step_index, statements_soa
    from wire_writers import synth_wrap_proof
    import random
    rng = random.Random(2)
    c = m.MinaContext(0)
    try:
        for f in (0, 1):
            c.poseidon_set_params(f, m.poseidon_params.default_params_bytes(f))
        c.srs_create(0, 1 << 15)
        w = synth_wrap_proof(rng, k=15); w["prev_optional"] = [None] * 19
        n_old, n_evals, sec = statements_soa([w], [5])
        st = c.make_pickles_statements(n_old, n_evals, sec)
        with pytest.raises(m.MinaError, match="index"):          # no step index / no wrap index yet
            c.pickles_public_inputs_batch(st, 1)
        ix, _, _ = load_k15_fixture()
        install_index(c, ix)
        with pytest.raises(m.MinaError, match="step index"):
            c.pickles_public_inputs_batch(st, 1)
        install_step_index(c, make_step_index(99))
        pub, ok = c.pickles_public_inputs_batch(st, 1)
        assert ok.tolist() == [1]
        for n_old_bad, n_evals_bad in ((5, n_evals), (n_old, 42), (n_old, 63)):
            with pytest.raises(m.MinaError):
                c.pickles_public_inputs_batch(c.make_pickles_statements(n_old_bad, n_evals_bad, sec), 1)
        missing = dict(sec); missing.pop("prev_evals")
        with pytest.raises(m.MinaError, match="null"):
            c.pickles_public_inputs_batch(c.make_pickles_statements(n_old, n_evals, missing), 1)
        with pytest.raises(m.MinaError):
            c.pickles_public_inputs_batch(st, 0)
        # a job whose kimchi section carries statements must ask for exactly 40 public inputs
        z = np.zeros(64 * 64, np.uint8)
        karr = {"prev_prechallenges": z, "prev_comms": z, "w_comm": z, "z_comm": z, "t_comm": z, "evals": z, "ft_eval1": z}
        kp = c.make_kimchi_proofs(1, 2, 39, karr, statements=st)
        ja = {"lr": z, "delta": z, "sg": z, "z1": z, "z2": z, "rand_base": oracle.int_to_le(7), "sg_rand_base": oracle.int_to_le(9)}
        with pytest.raises(m.MinaError):
            c.state_job_batch(c.make_state_jobs(1, ja, with_ipa=1, kimchi=kp, k=15, log2_domain=15, npub=39, n_evalpoints=2, n_comms=47))
        # a step index with more than 8 domains, or a malformed constant term, is refused
        with pytest.raises(m.MinaError):
            c.step_index_install(3, list(range(5, 14)), np.zeros(9 * 7 * 32, np.uint8), b"")
        with pytest.raises(m.MinaError):
            c.step_index_install(3, [10], np.zeros(7 * 32, np.uint8), bytes([250]))
        # and the context still works
        pub2, ok2 = c.pickles_public_inputs_batch(st, 1)
        assert (pub2 == pub).all() and ok2.tolist() == [1]
    finally:
        c.close()


def test_exchange_building_blocks_refuse_bad_shapes_and_null_pointers(ctx_srs):
    """the reduction operators of the multi-GPU exchange step (api_shard.hip): a shape outside the documented limits, a base range past the SRS or a null pointer
    is MINA_ERR_ARG before anything is queued, and the context computes afterwards"""
    c = ctx_srs
    lib, h = c._lib, c._h
    v, z, u32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32
    d = c.dev_malloc(4096)
    try:
        def sum_rows(ctx_h=h, field=0, rows=2, m=3, d_in=d, d_out=d + 2048):
            return lib.mina_field_sum_rows_dev(ctx_h, field, z(rows), z(m), v(d_in), v(d_out))
        for kw in ({"rows": 0}, {"rows": 4097}, {"m": 0}, {"m": (1 << 24) + 1}, {"field": 2}, {"ctx_h": None}, {"d_in": None}, {"d_out": None}):
            assert sum_rows(**kw) == MINA_ERR_ARG, kw

        def points_sum(ctx_h=h, curve=1, n=2, recs=d, out=d + 2048):
            return lib.mina_points_sum_dev(ctx_h, curve, z(n), v(recs), v(out))
        for kw in ({"n": 0}, {"n": 65537}, {"curve": 2}, {"ctx_h": None}, {"recs": None}, {"out": None}):
            assert points_sum(**kw) == MINA_ERR_ARG, kw

        def srs_range(ctx_h=h, curve=1, first=0, n=4, sc=d, out=d + 2048):
            return lib.mina_msm_srs_range_dev(ctx_h, curve, u32(first), z(n), v(sc), v(out))
        assert c.srs_depth(1) == 65536
        for kw in ({"first": 65536, "n": 1}, {"first": 65535, "n": 2}, {"first": 65533}, {"first": 1, "n": 65536}, {"first": 0xFFFFFFFF, "n": 2}, {"n": 65537}, {"n": 0},
                   {"n": 1 << 32}, {"curve": 2}, {"ctx_h": None}, {"sc": None}, {"out": None}):
            assert srs_range(**kw) == MINA_ERR_ARG, kw
        assert b"SRS" in lib.mina_last_error() or b"null" in lib.mina_last_error()

        def to_field(ctx_h=h, field=0, n=4, ch=d, out=d + 2048):
            return lib.mina_challenge_to_field_dev(ctx_h, field, z(n), v(ch), v(out))
        for kw in ({"field": 2}, {"ctx_h": None}, {"ch": None}, {"out": None}):
            assert to_field(**kw) == MINA_ERR_ARG, kw

        def equal(ctx_h=h, a=d, b=d + 1024, verdict=d + 2048):
            return lib.mina_point_records_equal_dev(ctx_h, v(a), v(b), v(verdict))
        for kw in ({"ctx_h": None}, {"a": None}, {"b": None}, {"verdict": None}):
            assert equal(**kw) == MINA_ERR_ARG, kw

        # and the context still computes: (p - 1) + 2 = 1 in Fp, one point summed is itself, it equals itself
        p = 0x40000000000000000000000000000000224698FC094CF91B992D30ED00000001
        c.dev_upload(d, np.frombuffer((p - 1).to_bytes(32, "little") + (2).to_bytes(32, "little"), np.uint8))
        assert sum_rows(rows=2, m=1) == 0
        assert c.dev_download(d + 2048, 32).tobytes() == (1).to_bytes(32, "little")
        rec = np.concatenate([c.srs_get_g(1, 7, 1)[0], np.zeros(4, np.uint8)])
        c.dev_upload(d, rec)
        assert points_sum(n=1) == 0
        assert c.dev_download(d + 2048, 68).tobytes() == rec.tobytes()
        c.dev_upload(d + 3072, np.full(4, 0xFF, np.uint8))
        assert equal(a=d, b=d + 2048, verdict=d + 3072) == 0
        assert c.dev_download(d + 3072, 4).tobytes() == (1).to_bytes(4, "little")
    finally:
        c.synchronize()
        c.dev_free(d)


def test_ipa_rows_selftest_refuses_bad_arguments(ctx_srs, oracle):
    """mina_selftest_ipa_rows: null pointers, a curve that is none, an empty batch, a foreign struct_size, a restore range past the batch, an expanded or overridden
    slot past the commitments, shared entries over more than 64 commitments or without their output buffers -- MINA_ERR_ARG each, before anything is queued"""
    import random
    import mina_bridge_amd as m
    import ipa_rows_model as M
    c = ctx_srs
    lib, L = c._lib, m.lib
    g = [oracle.bytes_to_point(b) for b in c.srs_get_g(0, 0, 8)]
    rng = random.Random(1)
    batch, k, ncomms = 2, 2, 3
    arr, keep = c.pack_ipa_openings([M.to_abi(M.random_proof(rng, 0, g, k, ncomms, 1)) for _ in range(batch)])
    big, keep2 = c.pack_ipa_openings([M.to_abi(M.random_proof(rng, 0, g, k, 65, 1)) for _ in range(batch)])
    rows = batch * (2 * k + ncomms + 4 + 7) + 3
    buf = {n: np.zeros(sz, np.uint8) for n, sz in (("points", rows * 64), ("scalars", rows * 32), ("chals", batch * k * 32), ("sigma", batch * 32), ("side", batch * 3 * 32))}
    off, flags, rb = np.zeros(3, np.uint32), np.zeros(3, np.uint32), np.ones(32, np.uint8)
    pts = np.zeros(batch * 7 * 64, np.uint8)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731

    def options(**kw):
        o = L.IpaRowsOptions(struct_size=ctypes.sizeof(L.IpaRowsOptions), override_slot=L.IPA_ROWS_NO_SLOT, expand_slot=L.IPA_ROWS_NO_SLOT)
        for name, v in kw.items():
            setattr(o, name, v)
        return o

    def call(h=c._h, curve=0, n=batch, ops=arr, rand=rb, sg_rand=rb, opt=None, **out):
        b = {name: P(a) for name, a in buf.items()}; b.update(offsets=P(off), flags=P(flags)); b.update(out)
        return lib.mina_selftest_ipa_rows(h, curve, ctypes.c_size_t(n), ops, None if rand is None else P(rand), None if sg_rand is None else P(sg_rand),
                                          None if opt is None else ctypes.byref(opt), b["points"], b["scalars"], b["chals"], b["sigma"], b["side"], b["offsets"], b["flags"])
    expand = dict(expand_point0=pts.ctypes.data, expand_points=pts.ctypes.data, expand_scalars=pts.ctypes.data)
    for kw in ({"h": None}, {"ops": None}, {"rand": None}, {"sg_rand": None}, {"points": None}, {"scalars": None}, {"chals": None}, {"sigma": None}, {"flags": None},
               {"curve": 2}, {"curve": -1}, {"n": 0}, {"n": (1 << 16) + 1},
               {"opt": options(struct_size=8)}, {"opt": options(struct_size=ctypes.sizeof(L.IpaRowsOptions) + 8)}, {"opt": options(pow_first=2)},
               {"opt": options(shared_h=1, restore_lo=batch, restore_cnt=1)}, {"opt": options(shared_h=1, restore_lo=0, restore_cnt=batch + 1)},
               {"opt": options(shared_h=1, restore_lo=0xFFFFFFFF, restore_cnt=2)},
               {"opt": options(expand_slot=ncomms, **expand)}, {"opt": options(expand_slot=ncomms + 5, **expand)}, {"opt": options(expand_slot=1)},
               {"opt": options(override_slot=ncomms, comm_override=pts.ctypes.data)}, {"opt": options(override_slot=1)},
               {"opt": options(shared_mask=1 << ncomms)}, {"opt": options(shared_mask=1, shared_h=1), "ops": big}, {"opt": options(shared_h=1), "side": None},
               {"opt": options(shared_mask=2), "offsets": None}):
        assert call(**kw) == MINA_ERR_ARG, {n: (v if not isinstance(v, ctypes.Structure) else {f: getattr(v, f) for f, _ in v._fields_}) for n, v in kw.items()}
    # and the entry point still computes, with and without options; the context's ordinary check as well
    assert call() == 0 and flags[0] == 0 and flags[1] in (16, 8, 3) and buf["sigma"][:32].tolist() == [1] + [0] * 31      # (rand bases 0x0101..: sigma_0 = 1)
    assert call(opt=options(shared_h=1, restore_lo=1, restore_cnt=1)) == 0 and off[0] == 0
    one = np.zeros(32, np.uint8); one[0] = 1
    assert (c.msm_srs(1, one) == c.srs_get_g(1, 0, 1)[0]).all()
