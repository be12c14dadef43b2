"""Pipelined device-resident Proof-of-State jobs under the role plan with a second state-hash carrier (ctx.h StreamPlan::carriers; mina_ctx_set_stream_budget 4
and 6) beside the plans without it (budgets 1 and 3): verdict and flag words equal across budgets and equal to what the CPU oracle says of the proofs.

The jobs are four oracle-minted proofs of the small shape (17 state hashes, 2^7 domain, k = 7 opening, 2^8 accumulator) tiled to 64 per call, on a context of their
own.  A call's words are its 64 per-proof verdicts and 4 flag words {opening ok, 0, accumulators ok, 0}.  The opening check and the accumulator check are FOLDED
over the call: a proof the oracle rejects for its opening fails every proof of its call (flag word 0 = 0), a proof it rejects for its chain fails alone."""
import copy
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPE = dict(k=7, log2_domain=7, npub=8, n_comms=6, slot=2, n_points=2, acc_k=8)
B, PER_LANE = 64, 3
BAD_STATE_AT, BAD_OPEN_AT = 21, 42          # positions of the tampered proofs in their calls
CLEAN, BAD_STATE, BAD_OPEN = 0, 1, 2


@pytest.fixture(scope="module")
def rig():
    """a context of its own with the three calls resident in HBM -- clean, one tampered state, one bad opening -- and the oracle's word on every distinct proof"""
    import mina_bridge_amd as m
    from oracle import oracle as O, state_job_ref as J
    from state_job_helpers import build_jobs, mint_job, oracle_job, pp_fp
    srs = {c: O.srs_create(c, 1 << 10, threads=4) for c in (0, 1)}
    minted = [mint_job(srs[0], srs[1], 2300 + 10 * i, **SHAPE) for i in range(4)]
    bad_state = copy.deepcopy(minted[BAD_STATE_AT % 4]); bad_state["expected"][5] ^= 2          # the chain no longer ends in the hashes the caller expects
    bad_open = copy.deepcopy(minted[BAD_OPEN_AT % 4]); bad_open["pubs"][0] ^= 1                  # the opening is of another public-input commitment
    verdict = lambda job: bool(J.verify_state_job(pp_fp(), srs[0], srs[1], oracle_job(job))["verdict"])
    assert all(verdict(j) for j in minted) and not verdict(bad_state) and not verdict(bad_open)
    tiles = {CLEAN: [minted[i % 4] for i in range(B)]}
    tiles[BAD_STATE] = [bad_state if i == BAD_STATE_AT else p for i, p in enumerate(tiles[CLEAN])]
    tiles[BAD_OPEN] = [bad_open if i == BAD_OPEN_AT else p for i, p in enumerate(tiles[CLEAN])]
    # the oracle's words of a call: chain verdicts per proof, the folded legs over the call
    want = {CLEAN: [1] * B + [1, 0, 1, 0],
            BAD_STATE: [int(i != BAD_STATE_AT) for i in range(B)] + [1, 0, 1, 0],
            BAD_OPEN: [0] * B + [0, 0, 1, 0]}
    c = m.MinaContext(0)
    try:
        for f in (0, 1):
            c.poseidon_set_params(f, m.poseidon_params.default_params_bytes(f))
        c.srs_create(0, 1 << 10); c.srs_create(1, 1 << 10)
        c.state_jobs_prepare(SHAPE["log2_domain"], SHAPE["npub"])
        dev, ptrs = {}, []
        for kind, tile in tiles.items():
            dev[kind], p = c.state_jobs_to_device(build_jobs(m, tile, SHAPE["k"], SHAPE["log2_domain"], SHAPE["slot"], SHAPE["acc_k"]))
            ptrs += p
        yield c, dev, want, tiles
        c.synchronize(); c.set_stream_budget(0); c.set_pipeline(1)
        for p in ptrs:
            c.dev_free(p)
    finally:
        c.close()


def run_calls(c, dev, kinds, lanes, budget):
    """the calls of `kinds` back to back over `lanes` lanes under `budget`, then mina_ctx_synchronize alone -> (their 68 words each, the plan statistic)"""
    c.set_pipeline(lanes); c.set_stream_budget(budget)
    outs = [c.dev_malloc(4 * B + 16) for _ in kinds]
    try:
        for o in outs:
            c.dev_upload(o, np.full(B + 4, 9, np.uint32).view(np.uint8))
        for kind, o in zip(kinds, outs):
            c.state_job_batch_dev(dev[kind], o, o + 4 * B)
        stats = c.stream_plan_stats()
        c.synchronize()
        return [c.dev_download(o, 4 * B + 16).view(np.uint32).tolist() for o in outs], stats
    finally:
        c.synchronize()
        for o in outs:
            c.dev_free(o)


def plan_of(lanes, budget):
    """what ctx.h stream_plan gives for the budgets of this file at 2 .. 5 lanes"""
    return {1: dict(roles=True, carriers=1, sets=1, streams=1), 3: dict(roles=True, carriers=1, sets=1, streams=3),
            4: dict(roles=True, carriers=2, sets=1, streams=4), 6: dict(roles=True, carriers=2, sets=2, streams=6)}[budget]


@pytest.mark.parametrize("lanes", [4, 5, 2])
@pytest.mark.parametrize("tampered", [False, True])
def test_words_equal_across_budgets_and_to_the_oracle(rig, lanes, tampered):
    """3 calls per lane in flight; budgets 1 and 3 (one carrier), 4 and 6 (two: 5 lanes load them 3 : 2, 2 lanes have one each).  Tampered: a bad state in a call
    of lane 1 (H1) and a bad opening in a call of lane 2 % lanes (H) -- exactly those calls show it, the same way under every budget"""
    c, dev, want, _ = rig
    kinds = [CLEAN] * (PER_LANE * lanes)
    if tampered:
        kinds[lanes + 1] = BAD_STATE          # call lanes + 1 runs on lane 1
        kinds[2 * lanes + 2 % lanes] = BAD_OPEN      # on lane 2 % lanes
    got = {}
    for budget in (1, 3, 4, 6):
        got[budget], stats = run_calls(c, dev, kinds, lanes, budget)
        assert stats == plan_of(lanes, budget), (budget, stats)
        for i, (kind, words) in enumerate(zip(kinds, got[budget])):
            assert words == want[kind], (lanes, budget, i, kind, [j for j, (a, e) in enumerate(zip(words, want[kind])) if a != e][:8])
    assert got[1] == got[3] == got[4] == got[6]


def test_a_leg_that_fails_at_queue_time_under_two_carriers(rig):
    """budget 4, 4 lanes: calls on both carriers in flight, then a call whose accumulator section names a 2^12 accumulator against the 2^10 SRS -- refused as its leg is
    queued, after its hashes went out.  The call returns the error; mina_ctx_synchronize alone then waits for both carriers (the words of the calls queued before
    are all there: the role streams' handles are the library's own, so the wait is read off what they wrote); the lane's next good call gives the oracle's words"""
    import mina_bridge_amd as m
    c, dev, want, _ = rig
    c.set_pipeline(4); c.set_stream_budget(4)
    outs = [c.dev_malloc(4 * B + 16) for _ in range(9)]
    try:
        for o in outs:
            c.dev_upload(o, np.full(B + 4, 9, np.uint32).view(np.uint8))
        for o in outs[:5]:                                   # lanes 0, 1, 2, 3, 0: both carriers busy
            c.state_job_batch_dev(dev[CLEAN], o, o + 4 * B)
        bad = type(dev[CLEAN])(); ctypes.memmove(ctypes.byref(bad), ctypes.byref(dev[CLEAN]), ctypes.sizeof(bad))
        bad.acc_k = 12
        with pytest.raises(m.MinaError):
            c.state_job_batch_dev(bad, outs[5], outs[5] + 4 * B)      # lane 1
        c.synchronize()
        for o in outs[:5]:
            assert c.dev_download(o, 4 * B + 16).view(np.uint32).tolist() == want[CLEAN]
        assert c.dev_download(outs[5], 4 * B + 16).view(np.uint32).tolist() == [9] * (B + 4), "a refused call writes no verdict"
        for o, kind in zip(outs[6:], (BAD_STATE, CLEAN, BAD_OPEN)):      # lanes 2, 3, 0 -- and then lane 1 again, below
            c.state_job_batch_dev(dev[kind], o, o + 4 * B)
        c.state_job_batch_dev(dev[BAD_STATE], outs[5], outs[5] + 4 * B)  # lane 1: the lane of the refused call
        assert c.stream_plan_stats() == plan_of(4, 4)
        c.synchronize()
        for o, kind in zip(outs[6:] + outs[5:6], (BAD_STATE, CLEAN, BAD_OPEN, BAD_STATE)):
            assert c.dev_download(o, 4 * B + 16).view(np.uint32).tolist() == want[kind], kind
    finally:
        c.synchronize()
        for o in outs:
            c.dev_free(o)


def test_a_pinned_lane_and_a_lone_lane_keep_plan_a(rig):
    c, dev, want, _ = rig
    zero = dict(roles=False, carriers=0, sets=0, streams=0)
    words, stats = run_calls(c, dev, [CLEAN, BAD_STATE], 1, 4)
    assert stats == zero and words == [want[CLEAN], want[BAD_STATE]]
    c.set_pipeline(4); c.set_stream_budget(4)
    o = c.dev_malloc(4 * B + 16)
    try:
        c.state_job_batch_dev(dev[CLEAN], o, o + 4 * B)
        assert c.stream_plan_stats() == plan_of(4, 4)
        c.synchronize()
        c.pin_lane(2)
        c.state_job_batch_dev(dev[BAD_OPEN], o, o + 4 * B)
        assert c.stream_plan_stats() == zero
        c.synchronize()
        assert c.dev_download(o, 4 * B + 16).view(np.uint32).tolist() == want[BAD_OPEN]
    finally:
        c.pin_lane(-1); c.synchronize(); c.dev_free(o)


def test_inputs_freed_and_allocated_again_between_calls(rig):
    """8 calls under budget 4 over 4 lanes; after each mina_ctx_synchronize the call's input buffers are freed and the next call's allocated (the allocator hands
    the same addresses out again, with other contents): a leg still reading the old ones, or a verdict kernel ahead of its legs, shows up as another call's words"""
    import mina_bridge_amd as m
    from state_job_helpers import build_jobs
    c, _, want, tiles = rig
    c.set_pipeline(4); c.set_stream_budget(4)
    o = c.dev_malloc(4 * B + 16)
    try:
        for call, kind in enumerate((CLEAN, BAD_OPEN, BAD_STATE, CLEAN, BAD_STATE, BAD_OPEN, CLEAN, BAD_STATE)):
            d, ptrs = c.state_jobs_to_device(build_jobs(m, tiles[kind], SHAPE["k"], SHAPE["log2_domain"], SHAPE["slot"], SHAPE["acc_k"]))
            c.state_job_batch_dev(d, o, o + 4 * B)
            c.synchronize()
            for p in ptrs:
                c.dev_free(p)
            assert c.dev_download(o, 4 * B + 16).view(np.uint32).tolist() == want[kind], (call, kind)
    finally:
        c.synchronize(); c.dev_free(o)
