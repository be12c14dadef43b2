"""The single-lane state-hash form (api_state.hip pstate_hash1_kernel: one sponge per lane, diagonal-normalised rows) against the wave-packed 3-lane form
and the CPU oracle.  The form follows the jobs in flight (ctx.h hash_one_lane): with 2 or more pipeline lanes, a call of HASH1_MIN_STATES / lanes states or more
takes the single-lane form; a lone call (one lane) keeps the 3-lane form whatever its size.  Which form ran is read from the context's stage timing
(`pstate_hash1` records the single-lane launches)."""
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HASH1_MIN_STATES = 65536   # ctx.h
SLOTS = 64                 # MINA_PSTATE_SLOTS
PS_STATE_HASH1 = 15        # ctx.h ProfStage


def _context(lanes):
    import mina_bridge_amd as m
    c = m.MinaContext(0)
    for field in (0, 1):
        c.poseidon_set_params(field, m.poseidon_params.default_params_bytes(field))
    c.set_pipeline(lanes)
    return c


@pytest.fixture()
def ctx2():
    """a context with two pipeline lanes: the single-lane form from HASH1_MIN_STATES / 2 states per call"""
    c = _context(2)
    yield c
    c.close()


@pytest.fixture()
def ctx1():
    """a context with one lane: lone calls, the 3-lane form at every size"""
    c = _context(1)
    yield c
    c.close()


def _hash(c, recs, nf, want_body=False):
    """the hashes and whether the single-lane form ran"""
    c.prof_enable(1 << PS_STATE_HASH1)
    out = c.protocol_state_hash_batch(recs, nf, want_body=want_body)
    ran = c.prof_read().get("pstate_hash1", [0, 0.0])[0] > 0
    c.prof_enable(0)
    return out, ran


def _oracle_hashes(oracle, vals, counts):
    """(state hash, body hash) per record: H_"MinaProtoState"(field 0, H_"MinaProtoStateBody"(fields 1 .. 1 + count)) with the oracle's permutation"""
    import mina_bridge_amd.poseidon_params as PP
    from oracle import mina_state_ref as S, pasta_ref as R
    from state_job_helpers import pp_fp
    P = R.P
    pp = pp_fp(); params = PP.default_params_bytes(0)
    salts = [S.salt(S.PREFIX_PROTOCOL_STATE_BODY, pp), S.salt(S.PREFIX_PROTOCOL_STATE, pp)]
    perm = lambda st: [int.from_bytes(x.tobytes(), "little") for x in oracle.poseidon_permute(0, params, oracle.ints_to_le(st).reshape(1, 96)).reshape(3, 32)]
    want, want_body = [], []
    for r in range(len(counts)):
        st = list(salts[0]); nbody = min(counts[r], SLOTS - 1)
        for blk in range(0, nbody, 2):
            if blk: st = perm(st)
            for t in range(2):
                if blk + t < nbody:
                    st[t] = (st[t] + vals[r][1 + blk + t]) % P
        st = perm(st)
        want_body.append(st[0])
        st = perm([(salts[1][0] + vals[r][0]) % P, (salts[1][1] + st[0]) % P, salts[1][2]])
        want.append(st[0])
    return want, want_body


def test_one_lane_form_every_field_count_equals_three_lane_form_and_oracle(ctx2, ctx1, oracle):
    """ragged field counts 0 .. 63 (lanes of one wave absorb different numbers of blocks) and 256-bit words that are not canonical field elements: the
    single-lane form equals the oracle's sponge (state and body hashes) and, state for state, the 3-lane form on the same records"""
    from oracle import pasta_ref as R
    P = R.P
    rng = random.Random(777)
    counts = list(range(0, 64)) + [49, 49, 48, 1, 0]
    nrec = len(counts)
    vals = [[rng.randrange(P) for _ in range(SLOTS)] for _ in range(nrec)]
    vals[3][0] = (1 << 256) - 1; vals[6][5] = P; vals[40][40] = P + 99; vals[63][63] = (1 << 255) + 3; vals[62][1] = (1 << 256) - 1
    recs = np.zeros((nrec, SLOTS, 32), np.uint8)
    for r in range(nrec):
        for j in range(SLOTS):
            recs[r, j] = np.frombuffer(vals[r][j].to_bytes(32, "little"), np.uint8)
    nf = np.array(counts, np.uint32)
    want, want_body = _oracle_hashes(oracle, vals, counts)
    n = HASH1_MIN_STATES // 2 + 77                                # not a multiple of 64 nor of 256: a partial last wave
    idx = np.array([(i * 5 + i // 64) % nrec for i in range(n)])   # every wave mixes field counts
    (got, body), ran = _hash(ctx2, recs[idx].reshape(n, -1).copy(), nf[idx].copy(), want_body=True)
    assert ran, "the single-lane form did not run (normalised rows not installed, or the tier moved)"
    first = {}
    for i in range(n):
        first.setdefault(int(idx[i]), i)
    assert [oracle.le_to_int(got[first[r]]) for r in range(nrec)] == want
    assert [oracle.le_to_int(body[first[r]]) for r in range(nrec)] == want_body
    assert (got == got[[first[int(r)] for r in idx]]).all()
    m = 8200                                                      # the same records through the 3-lane form (one lane)
    (got3, body3), ran3 = _hash(ctx1, recs[idx[:m]].reshape(m, -1).copy(), nf[idx[:m]].copy(), want_body=True)
    assert not ran3
    assert (got3 == got[:m]).all() and (body3 == body[:m]).all()


def test_one_lane_form_both_sides_of_the_threshold(ctx2, ctx1, oracle):
    """at two lanes: HASH1_MIN_STATES / 2 - 1 distinct random states (3-lane form) and HASH1_MIN_STATES / 2 states (single-lane form) that share them give
    identical hashes; the extra state equals a call of its own, a sample equals the oracle; a lone call (one lane) of HASH1_MIN_STATES states stays 3-lane"""
    rng = np.random.Generator(np.random.PCG64(31337))
    n = HASH1_MIN_STATES // 2
    recs = rng.integers(0, 256, size=(n, SLOTS * 32), dtype=np.uint8)
    nf = rng.integers(0, SLOTS, size=n, dtype=np.uint32)
    nf[: 64 * 40] = 49                                            # whole waves of the real record length
    below, ran_below = _hash(ctx2, recs[: n - 1].copy(), nf[: n - 1].copy())
    at, ran_at = _hash(ctx2, recs, nf)
    assert not ran_below and ran_at
    assert (at[: n - 1] == below).all()
    assert (_hash(ctx2, recs[n - 1:].copy(), nf[n - 1:].copy())[0] == at[n - 1:]).all()
    sample = [0, 1, 63, 64, 4095, 20000, n - 2, n - 1]
    vals = [[int.from_bytes(recs[i, 32 * j: 32 * j + 32].tobytes(), "little") for j in range(SLOTS)] for i in sample]
    want, _ = _oracle_hashes(oracle, vals, [int(nf[i]) for i in sample])
    assert [oracle.le_to_int(at[i]) for i in sample] == want
    big = np.concatenate([recs, recs]); bnf = np.concatenate([nf, nf])
    lone, ran_lone = _hash(ctx1, big, bnf)
    assert not ran_lone
    assert (lone[:n] == at).all() and (lone[n:] == at).all()
