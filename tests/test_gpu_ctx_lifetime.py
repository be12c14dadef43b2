"""The end of a context on the real runtime: the buffers of a mina_ctx free themselves when mina_ctx_destroy deletes it (ctx.h DevBuf / PinnedBuf), behind the
synchronisation and destruction of the streams they were used on.  A context that kept its workspaces would lose their size in free device memory with every
create / close cycle; one that freed a block twice, or under a running kernel, would not come back from close()."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def surrogate_tables(m, c):
    for f in (0, 1):
        c.poseidon_set_params(f, m.poseidon_params.default_params_bytes(f))


def test_contexts_give_their_memory_back_and_every_close_returns():
    """Three cycles of MinaContext -> SRS of 2^6 points, an MSM over it, 4 sponges of 3 elements -> close(): free device memory after the third close() is not lower
    than after the first by more than HALF of what one context holds (`used`: the largest drop seen inside a cycle -- a context that kept its workspaces would lose
    about `used` per cycle, so the margin comes from the run itself).  Then a cycle whose context has helper lanes and role streams when it goes (4 lanes at
    stream budget 3, one device-resident job of 2 proofs), and the boundary's shutdown after one call of 2 proofs: the view context goes before its parent.  The
    test is about teardown: it asserts that every call succeeds and returns, not what the verdicts are."""
    torch = pytest.importorskip("torch")
    import mina_bridge_amd as m
    from oracle import oracle as O
    from state_job_helpers import build_jobs, mint_job
    curve = m.CURVE_VESTA
    rng = np.random.Generator(np.random.PCG64(41))
    scalars = rng.integers(0, 256, size=(64, 32), dtype=np.uint8); scalars[:, 31] &= 0x3F
    sponges = rng.integers(0, 256, size=(4 * 3, 32), dtype=np.uint8); sponges[:, 31] &= 0x3F
    free = lambda: torch.cuda.mem_get_info()[0]
    torch.cuda.synchronize()
    before, used, after = free(), 0, []
    for cycle in range(3):
        start = free()
        c = m.MinaContext(0)
        try:
            surrogate_tables(m, c)
            c.srs_create(curve, 1 << 6)
            assert c.msm_srs(curve, scalars).shape == (64,)
            assert c.poseidon_hash(m.FIELD_FP, sponges, 4, 3).shape == (4, 32)
            used = max(used, start - free())
        finally:
            c.close()
        after.append(free())
    print(f"free before {before}, after each close {after}, used by one context {used}")
    assert used > 0, "a context with an SRS and the workspaces of two calls holds no device memory: the reading says nothing"
    assert after[2] >= after[0] - used // 2, (before, after, used)

    # helper lanes and role streams exist when the destructors run
    shape = dict(k=7, log2_domain=7, npub=8, n_comms=6, slot=2, n_points=2, acc_k=8)
    srs = {cv: O.srs_create(cv, 1 << 10, threads=4) for cv in (0, 1)}
    minted = [mint_job(srs[0], srs[1], 2900 + 10 * i, **shape) for i in range(2)]
    c = m.MinaContext(0)
    try:
        surrogate_tables(m, c)
        c.srs_create(0, 1 << 10); c.srs_create(1, 1 << 10)
        c.state_jobs_prepare(shape["log2_domain"], shape["npub"])
        d, ptrs = c.state_jobs_to_device(build_jobs(m, minted, shape["k"], shape["log2_domain"], shape["slot"], shape["acc_k"]))
        out = c.dev_malloc(4 * 2 + 16)
        c.set_pipeline(4)
        c.set_stream_budget(3)
        c.state_job_batch_dev(d, out, out + 4 * 2)
        c.synchronize()
        for p in ptrs + [out]:
            c.dev_free(p)
    finally:
        c.close()

    # the boundary: the device's view context is destroyed before the context it borrows from
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "state_proofs_k15_bytes.json")))["proofs"][:2]
    m.lib.verify_shutdown()
    m.lib.verify_configure(m.lib.VERIFY_ALLOW_SURROGATE | m.lib.VERIFY_ALLOW_MISSING_KIMCHI)
    try:
        assert len(m.lib.verify_state_batch([bytes.fromhex(it["proof"]) for it in fx], [bytes.fromhex(it["pub"]) for it in fx])) == 2
    finally:
        m.lib.verify_configure(0)
        m.lib.verify_shutdown()
