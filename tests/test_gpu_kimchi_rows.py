"""The kernels behind mina_kimchi_to_batch (mina_bridge_amd/csrc/api_kimchi.hip: kimchi_fq_kernel in both roles, kimchi_pub_kernel<8> / <10>, kimchi_fr_kernel,
kimchi_scalar_kernel, kimchi_ftcomm_kernel, kimchi_rows_kernel, and the `_gcd` twins of pub, scalar and ftcomm) held to `oracle/kimchi_ref.py oracles_and_batch`
at shape and value edges.  Every comparison is equality of bytes and covers, for every proof of every call: the sponge state and position, the evaluation points
(zeta and zeta * omega: beta, gamma and alpha go into them through the transcript, and into ft_eval0), polyscale, evalscale, ft_eval0, the combined inner product
and all n_prev + 45 commitment rows.  The reference is never another GPU path.  The inputs are tests/kimchi_rows_cases.py's (proofs that need not verify;
tests/test_kimchi_rows_cases.py checks the tables on the CPU); a table's references are computed once and shared by the forms.

Every call runs under a forced lane form -- 16, 8 or 3 lanes per sponge in kimchi_fq_kernel and kimchi_fr_kernel (ctx.h transcript_lanes) -- and once more in
the 8-lane form with mina_ctx_set_chain_inverse on.  mina_kimchi_to_batch does not report the form it ran, so each call asserts the tuning read back, that the
context has one pipeline lane, and the form ctx.h's rule gives from those (lanes_rule restates it).  One proof alone cannot be put into the 3-lane form: the rule
counts proofs in flight and transcript_coop8_max = 0 means "the default"; that one call runs 8 lanes and says so.

Not claimed: the exceptional branches of the group law inside kimchi_ftcomm_body's shuffle tree (two partial sums equal or opposite).  They cannot be reached
from inputs: the scalars depend on zeta, which is squeezed after the t commitments are absorbed.  What is reached: infinity as a term (scalar_mul_affine's early
return), as all seven t terms, and -- in the rows kimchi_rows_kernel copies -- as any commitment.

Only a malformed proof's own rows are unspecified and skipped; its four neighbours are compared in full."""
from types import SimpleNamespace

import numpy as np
import pytest

import kimchi_rows_cases as C

pytestmark = pytest.mark.gpu

FORMS = {16: dict(coop16_max=1 << 30), 8: dict(coop16_max=0, kimchi_coop8_max=1 << 30, transcript_coop8_max=1 << 30), 3: dict(coop16_max=0, transcript_coop8_max=1),
         None: {}}
DEFAULTS = dict(coop16_max=64, transcript_coop8_max=0, kimchi_coop8_max=1024)
MODES = {"16-lane": (16, False), "8-lane": (8, False), "3-lane": (3, False), "8-lane-divstep": (8, True)}      # (lane form, mina_ctx_set_chain_inverse)


def lanes_rule(t, batch):
    """ctx.h transcript_lanes(c, batch, kimchi_coop8_max) on a context with one pipeline lane (proofs in flight = proofs per call)"""
    if batch <= t.coop16_max:
        return 16
    if t.transcript_coop8_max:
        return 8 if batch <= t.transcript_coop8_max else 3
    return 8 if (batch <= t.kimchi_coop8_max and batch <= 2048) or batch <= 2560 else 3


@pytest.fixture(scope="module")
def env(oracle):
    """a context of this module's own (the inversion mode and the installed index are context state), one pipeline lane, the 128-point Pallas SRS the proofs'
    points come from; every table with its references, built here once (pure-Python scalar multiplications: most of this module's time) and never written to"""
    import mina_bridge_amd as m
    world, h = C.shared_world()
    for name in C.all_tables():
        world.table(name)
    ctx = m.MinaContext(0)
    try:
        ctx.set_pipeline(1)
        for f in (0, 1):
            ctx.poseidon_set_params(f, m.poseidon_params.default_params_bytes(f))
        ctx.srs_create(C.CURVE, 128)
        assert (ctx.srs_get_h(C.CURVE) == h).all()
        yield SimpleNamespace(m=m, ctx=ctx, world=world, installed=None)
    finally:
        ctx.set_chain_inverse(False)
        ctx.close()


def run(env, table, arrays, batch, mode, lanes=None):
    """one mina_kimchi_to_batch call over `arrays` under the index of `table` and MODES[mode]; lanes: the form the call must run in where it is not the forced one"""
    from kimchi_helpers import install_index
    m, ctx = env.m, env.ctx
    form, chain = MODES.get(mode, (None, False))
    with m.lib.tuning(**FORMS[form]):
        with pytest.raises(m.lib.MinaError, match="outside the pipeline"):
            ctx.pin_lane(1)
        t, d = m.lib.verify_tuning_get(), m.lib.verify_tuning_default()
        for name, value in DEFAULTS.items():
            assert getattr(d, name) == value and getattr(t, name) == FORMS[form].get(name, value), name
        assert lanes_rule(t, batch) == (lanes or form), f"asked for the {lanes or form}-lane form, the rule gives {lanes_rule(t, batch)} at {batch} proofs"
        if env.installed is not table.index:
            install_index(ctx, table.index)
            env.installed = table.index
            assert int.from_bytes(ctx.verifier_index_digest().tobytes(), "little") == table.index.digest
        kp = m.MinaContext.make_kimchi_proofs(batch, table.n_prev, table.npub, arrays)
        before = ctx.chain_inverse_stats()
        ctx.set_chain_inverse(chain)
        try:
            got = ctx.kimchi_to_batch(kp, table.k)
        finally:
            ctx.set_chain_inverse(False)
        after = ctx.chain_inverse_stats()
        moved, still = ("gcd_launches", "fermat_launches") if chain else ("fermat_launches", "gcd_launches")
        assert after[moved] - before[moved] >= 3 and after[still] == before[still], (mode, before, after)       # kimchi_pub, kimchi_scalar, kimchi_ftcomm at the least
    return got


def same(got, table, order, skip=()):
    """every compared field of every proof but those in `skip` equals the reference of the distinct proof at that position"""
    batch = len(order)
    out = {f: np.asarray(got[f]).reshape(batch, -1) for f in C.FIELDS if f != "sponge"}
    out["sponge"] = np.concatenate([got["sponge_state"].reshape(batch, 96), got["sponge_pos"].view(np.uint8).reshape(batch, 8)], axis=1)
    keep = np.ones(batch, bool)
    keep[list(skip)] = False
    for f in C.FIELDS:
        want = table.want[f][order]
        assert out[f].shape == want.shape, (f, out[f].shape, want.shape)
        bad = np.nonzero((out[f] != want).any(axis=1) & keep)[0]
        if len(bad):
            b = int(bad[0])
            rows = np.nonzero((out[f][b].reshape(-1, 64) != want[b].reshape(-1, 64)).any(axis=1))[0].tolist() if f == "comms" else []
            raise AssertionError(f"{table.name}, {batch} proofs: {f} differs for {len(bad)} proofs, first at {bad[:8].tolist()} (distinct proof {int(order[b])})"
                                 + (f", commitment rows {rows[:8]} of {table.n_prev + 45}" if rows else "")
                                 + f"; got {out[f][b][:64].tobytes().hex()} want {want[b][:64].tobytes().hex()}")


def whole(env, name, mode):
    t = env.world.table(name)
    arrays, order = C.tile(t, len(t.cases))
    got = run(env, t, arrays, len(order), mode)
    assert not got["malformed"][0]
    same(got, t, order)
    return t


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("npub", C.NPUB_LIST)
def test_public_input_counts(env, npub, mode):
    """kimchi_pub_body from no work item to a fourth pass of the lanes, both chunk sizes, partial last chunks, the whole domain at 2^6 and at 2^7
    (tests/test_kimchi_rows_cases.py names the path each count takes); five distinct proofs"""
    t = whole(env, "npub/%d" % npub, mode)
    assert (t.npub, t.k, t.n_prev) == (npub, C.domain_of(npub), 2)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("n_prev", C.NPREV_LIST)
def test_recursion_accumulators(env, n_prev, mode):
    """0 to 8 accumulators: with none the challenge-digest sponge squeezes having absorbed nothing, no prev_* array is passed, and the combined inner product starts
    at the public evaluation"""
    t = whole(env, "nprev/%d" % n_prev, mode)
    assert t.n_prev == n_prev and ("prev_chals" in t.arrays) == (n_prev > 0)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", ["alpha/%d" % a for a in C.ALPHA_OFFSETS] + ["zk/%d" % z for z in C.ZK_ROWS])
def test_index_parameters(env, name, mode):
    """perm_alpha_offset and zk_rows at the limits mina_verifier_index_install admits and at the circuit's own; the index is installed afresh"""
    t = whole(env, name, mode)
    kind, _, arg = name.partition("/")
    assert getattr(t.index, "perm_alpha_offset" if kind == "alpha" else "zk_rows") == int(arg)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("batch", C.TILES)
def test_value_corners_at_batch_edges(env, batch, mode):
    """the corner table going round in calls of 1 to 129 proofs: the 4, 8 and 21 proofs per wave of the cooperative sponges (and the role split of kimchi_fq_kernel
    behind them), the 8 proofs per wave of kimchi_pub and kimchi_ftcomm, the 64-proof block of kimchi_scalar_kernel -- each short of, at and past its edge; the
    period is coprime to all of them, so every corner meets every position"""
    t = env.world.table("corners")
    arrays, order = C.tile(t, batch)
    got = run(env, t, arrays, batch, mode, lanes=8 if (MODES[mode][0], batch) == (3, 1) else None)
    assert not got["malformed"][0]
    same(got, t, order)


@pytest.mark.parametrize("batch,lanes", [(1024, 8), (1025, 8), (2560, 8), (2561, 3)])
def test_default_tuning_around_the_per_call_limit(env, batch, lanes):
    """the library's own choice: kimchi_coop8_max = 1024 proofs per call, and the 2560 proofs in flight up to which a call alone keeps the 8-lane form whatever the
    per-call limit says (ctx.h use_coop8_transcripts) -- so on one pipeline lane 1024 -> 1025 stays in 8 lanes and 2560 -> 2561 is where the form changes"""
    t = env.world.table("corners")
    arrays, order = C.tile(t, batch)
    got = run(env, t, arrays, batch, "default", lanes=lanes)
    assert not got["malformed"][0]
    same(got, t, order)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("slot,kind", C.malformed_variants())
def test_malformed_inputs(env, slot, kind, mode):
    """one bad value in one proof of five, the victim first, in the middle and last: the flag says 1 and the four clean proofs' outputs are still the oracle's"""
    t = env.world.table("nprev/%d" % C.BASE_NPREV)
    order = np.arange(C.BATCH)
    for victim in C.VICTIMS:
        got = run(env, t, C.malformed(env.world, slot, kind, victim), C.BATCH, mode)
        assert got["malformed"][0] == 1, (slot, kind, victim)
        same(got, t, order, skip=(victim,))
    got = run(env, t, dict(t.arrays), C.BATCH, mode)
    assert got["malformed"][0] == 0
    same(got, t, order)
