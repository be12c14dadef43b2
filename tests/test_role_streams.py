"""Pipelined device-resident Proof-of-State jobs under every stream plan (ctx.h stream_plan; mina_ctx_set_stream_budget): the jobs of a 4-lane context forked per
lane (plan A, budget 23) and flowing through shared role streams (plan B: budget 3 = one state-hash stream and one W1 / W2 pair, budget 7 = three pairs) give,
job by job, the verdict words and flag words of the one-stream job (mina_verify_tuning.dev_fork = 0).

The jobs are the benchmark's own at 64 proofs per call (17 state hashes, statement -> 40 public inputs, kimchi, k = 15 opening, 2^16 accumulator).  13 go out
back to back without a wait, so every lane's workspaces are reused 3 times while 4 jobs are in flight; job k carries ONE tampered proof at position
(7 k + 3) % 64 (jobs 0, 5, 9: none), so a stale buffer or a missing wait shows up as a neighbour job's position or flags."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, NJOBS, CLEAN = 64, 13, (0, 5, 9)
LEGS = ("state", "z1", "sg")          # what the tamper of job k hits, in rotation over the tampered jobs
P_FP = 0x40000000000000000000000000000000224698FC094CF91B992D30ED00000001      # Vesta's scalar field = Pallas' base field: the accumulator leg's folded scalars


def tamper_of(k):
    """(position, leg) of job k's tampered proof, or None"""
    if k in CLEAN:
        return None
    order = [i for i in range(NJOBS) if i not in CLEAN]
    return (7 * k + 3) % B, LEGS[order.index(k) % 3]


@pytest.fixture(scope="module")
def jobs(ctx_srs):
    """the 13 jobs resident in HBM (built once, never written again) and the reference: verdict and flag words of each on ONE stream (dev_fork = 0)"""
    torch = pytest.importorskip("torch")
    import bench
    import mina_bridge_amd as m
    ctx, dev = ctx_srs, torch.device("cuda", 0)
    djobs = []
    for k in range(NJOBS):
        (hj, keep), kp, _, _ = bench.build_full_job(ctx, m, B, seed=5200)
        by_addr = {a.ctypes.data: a for a in keep if isinstance(a, np.ndarray)}
        t = tamper_of(k)
        if t:
            pos, leg = t
            if leg == "state": by_addr[hj.state_records].view(np.uint8).reshape(B, 17, 64, 32)[pos, 9, 20, 3] ^= 4
            if leg == "z1": by_addr[hj.z1].view(np.uint8).reshape(B, 32)[pos, 0] ^= 1
            if leg == "sg": by_addr[hj.acc_sg].view(np.uint8).reshape(B, 64)[pos, 1] ^= 2
        djobs.append(bench.device_jobs(m, hj, keep, kp, dev))
    ctx.state_jobs_prepare(bench.LOG2_DOMAIN, bench.NPUB)
    try:
        with m.lib.tuning(dev_fork=0):
            ref = run_jobs(ctx, torch, djobs, lanes=4, budget=0)
    finally:
        ctx.synchronize(); ctx.set_pipeline(1)
    # the reference itself: every tamper bites where it should, and nowhere else
    for k, w in enumerate(ref):
        t = tamper_of(k)
        if t is None:
            assert w == [1] * B + [1, 0, 1, 0], k
        elif t[1] == "state":
            assert w[:B] == [int(i != t[0]) for i in range(B)] and w[B:] == [1, 0, 1, 0], k
        elif t[1] == "z1":
            assert w[B] == 0 and w[B + 2] == 1 and not any(w[:B]), k
        else:
            assert w[B] == 1 and w[B + 2] == 0 and not any(w[:B]), k
    return djobs, ref


def run_jobs(ctx, torch, djobs, lanes, budget, order=None):
    """the jobs of `order` back to back on `lanes` lanes under stream budget `budget` (0: the environment's), then mina_ctx_synchronize ALONE -> their B + 4 words
    each.  The copies out run on torch's stream, which waits for nothing the library queued (its streams do not synchronise with the null stream)."""
    order = list(range(len(djobs))) if order is None else order
    ctx.set_pipeline(lanes)
    ctx.set_stream_budget(budget)
    outs = [torch.full((B + 4,), 9, dtype=torch.int32, device="cuda:0") for _ in order]
    torch.cuda.synchronize()
    for k, o in zip(order, outs):
        ctx.state_job_batch_dev(djobs[k][0], o.data_ptr(), o.data_ptr() + 4 * B)
    ctx.synchronize()
    return [o.cpu().numpy().tolist() for o in outs]


def restore(ctx):
    ctx.synchronize(); ctx.set_stream_budget(0); ctx.set_pipeline(1)


@pytest.mark.parametrize("budget", [3, 7, 23])
def test_parity_with_the_one_stream_job_under_every_plan(ctx_srs, jobs, budget):
    """13 jobs in flight over 4 lanes: budget 3 and 7 take the role plan (1 and 3 chain sets), 23 today's fork per lane"""
    torch = pytest.importorskip("torch")
    djobs, ref = jobs
    try:
        got = run_jobs(ctx_srs, torch, djobs, lanes=4, budget=budget)
        for k, (g, r) in enumerate(zip(got, ref)):
            assert g == r, (budget, k, tamper_of(k), [i for i, (a, e) in enumerate(zip(g, r)) if a != e][:8])
    finally:
        restore(ctx_srs)


def test_synchronize_waits_for_the_role_streams(ctx_srs, jobs):
    """under the role plan the lanes' own streams carry nothing: mina_ctx_synchronize must wait for the role streams.  Six jobs, then that call and nothing else
    (no device-wide wait), then the words are copied out: they are the expected ones, none still holds its fill value"""
    torch = pytest.importorskip("torch")
    djobs, ref = jobs
    order = [1, 2, 3, 4, 0, 6]
    try:
        got = run_jobs(ctx_srs, torch, djobs, lanes=4, budget=3, order=order)
        assert not any(9 in g[:B] for g in got)
        assert got == [ref[k] for k in order]
    finally:
        restore(ctx_srs)


def test_budget_changed_between_jobs(ctx_srs, jobs):
    """23 -> 3 -> 23 on one context, a synchronize between: the helper lanes' workspaces pass from the lanes' own streams to the role streams and back"""
    torch = pytest.importorskip("torch")
    djobs, ref = jobs
    order = [4, 0, 7, 8, 2, 5]
    try:
        for budget in (23, 3, 23, 3):
            got = run_jobs(ctx_srs, torch, djobs, lanes=4, budget=budget, order=order)
            assert got == [ref[k] for k in order], budget
    finally:
        restore(ctx_srs)


def test_pin_and_unpin_without_a_wait(ctx_srs, jobs):
    """a pinned context runs one job at a time and takes plan A whatever the budget; pinning and unpinning do not wait for the GPU: a lane's next job follows its
    last one across the change of plan (the lane's `done` event)"""
    torch = pytest.importorskip("torch")
    djobs, ref = jobs
    ctx = ctx_srs
    try:
        ctx.set_pipeline(4); ctx.set_stream_budget(3)
        order = [1, 2, 3, 4, 6, 7, 8, 0, 10, 11]
        outs = [torch.full((B + 4,), 9, dtype=torch.int32, device="cuda:0") for _ in order]
        torch.cuda.synchronize()
        for i, (k, o) in enumerate(zip(order, outs)):
            if i == 4: ctx.pin_lane(1)            # lane 1 ran job 2 on the role streams; jobs 6, 7, 8 now fork on lane 1
            if i == 7: ctx.pin_lane(-1)           # ... and the round-robin goes on over the role streams
            ctx.state_job_batch_dev(djobs[k][0], o.data_ptr(), o.data_ptr() + 4 * B)
        ctx.synchronize()
        for k, o in zip(order, outs):
            assert o.cpu().numpy().tolist() == ref[k], k
    finally:
        ctx.pin_lane(-1); restore(ctx)


def test_fold_variant_under_the_role_plan(ctx_srs, jobs):
    """mina_state_job_fold_dev on an unpinned 4-lane context, 6 calls in flight, budget 3 against plan A: verdict and flag words, the opening leg's folded scalars
    and partial point byte for byte.  The accumulator leg's exports carry ONE scalar each call draws from the operating system (api_ipa.hip
    mb_accumulator_check_dev), so two calls never agree byte for byte under any plan: there the folded scalars must be plan A's times one constant, and the
    partial point must be the commitment of the call's own scalars (the folded check, for every job whose accumulators are sound)."""
    torch = pytest.importorskip("torch")
    import mina_bridge_amd as m
    djobs, ref = jobs
    ctx = ctx_srs
    order = [0, 1, 2, 3, 5, 4]
    N_IPA, N_ACC = (1 << 15) * 32, (1 << 16) * 32

    def run(budget):
        ctx.set_pipeline(4); ctx.set_stream_budget(budget)
        bufs = [[torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda:0") for n in (4 * (B + 4), N_IPA, 68, N_ACC, 68)] for _ in order]
        torch.cuda.synchronize()
        for k, b in zip(order, bufs):
            p = [t.data_ptr() for t in b]
            ctx.state_job_fold_dev(djobs[k][0], p[0], p[0] + 4 * B, p[1], p[2], p[3], p[4])
        ctx.synchronize()
        return bufs

    try:
        a, b = run(23), run(3)
        rec, eq = torch.zeros(68, dtype=torch.uint8, device="cuda:0"), torch.zeros(1, dtype=torch.int32, device="cuda:0")
        for k, x, y in zip(order, a, b):
            for i in (0, 1, 2):
                assert torch.equal(x[i], y[i]), (k, i)
            ra, rb = (t[3].cpu().numpy().tobytes() for t in (x, y))
            ia, ib = ([int.from_bytes(r[i:i + 32], "little") for i in range(0, N_ACC, 32)] for r in (ra, rb))
            assert ia[0] and ib[0]
            assert all(u * ib[0] % P_FP == v * ia[0] % P_FP for u, v in zip(ia, ib)), k
            t = tamper_of(k)
            if t and t[1] == "sg":
                continue                      # (a malformed commitment: the partial point is no commitment of anything)
            for bufset in (x, y):
                ctx.msm_srs_range_dev(m.CURVE_VESTA, 0, 1 << 16, bufset[3].data_ptr(), rec.data_ptr()); ctx.synchronize()
                ctx.point_records_equal_dev(rec.data_ptr(), bufset[4].data_ptr(), eq.data_ptr()); ctx.synchronize()
                assert int(eq.cpu()[0]) == 1, (k, t)
    finally:
        restore(ctx)


def test_destroy_after_role_plan_jobs():
    """a context of its own: jobs under the role plan, then under plan A, then mina_ctx_destroy -- every stream is destroyed once (the helper lanes only alias the
    context's fork and role streams), and the device serves the next context"""
    import mina_bridge_amd as m
    from oracle import oracle as O
    from state_job_helpers import build_jobs, mint_job
    shape = dict(k=7, log2_domain=7, npub=8, n_comms=6, slot=2, n_points=2, acc_k=8)
    srs = {c: O.srs_create(c, 1 << 10, threads=4) for c in (0, 1)}
    minted = [mint_job(srs[0], srs[1], 1900 + 10 * i, **shape) for i in range(2)]
    nb = len(minted)
    for round_ in range(2):
        c = m.MinaContext(0)
        try:
            for f in (0, 1):
                c.poseidon_set_params(f, m.poseidon_params.default_params_bytes(f))
            c.srs_create(0, 1 << 10); c.srs_create(1, 1 << 10)
            c.state_jobs_prepare(shape["log2_domain"], shape["npub"])
            d, ptrs = c.state_jobs_to_device(build_jobs(m, minted, shape["k"], shape["log2_domain"], shape["slot"], shape["acc_k"]))
            c.set_pipeline(3)
            base = c.lane_streams()["live"]
            outs = [c.dev_malloc(4 * nb + 16) for _ in range(7)]
            for budget, n_streams in ((3, 3), (23, 3 + 9), (5, 3 + 9 + 2)):      # role plan (H, W1, W2); a fork per lane; two chain sets: two more role streams
                c.set_stream_budget(budget)
                for o in outs:
                    c.state_job_batch_dev(d, o, o + 4 * nb)
                c.synchronize()
                for o in outs:
                    w = c.dev_download(o, 4 * nb + 16).view(np.uint32)
                    assert w[:nb].tolist() == [1] * nb and w[nb:].tolist() == [1, 0, 1, 0], (budget, w.tolist())
                assert c.lane_streams()["live"] == base + n_streams, budget
            c.set_pipeline(1)
            for p in outs + ptrs:
                c.dev_free(p)
        finally:
            c.close()
