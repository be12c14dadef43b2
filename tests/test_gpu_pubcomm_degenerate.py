"""Public-input commitments  public_comm = h - sum_i pub_i L_i  on SRSs whose Lagrange points have KNOWN relations (tests/srs_helpers.py: L_i = c_i G, h = t G), loaded
through mina_srs_load.  On the honest SRS no two Lagrange points are related, so the fallbacks of every sum-of-points path for the group law's exceptional cases --
the 8 x 32 restart of pubcomm_direct29_kernel, the doubling / to-infinity branches of the 8 x 32 adds in a lane, in the shuffle tree and in the three finishes,
the butterflies of the group iFFT on equal and opposite points, table rows of a basis point at infinity, the bucket route over equal and opposite bases -- never run
there.  Here they do, and every result is compared bit for bit with the big-int reference (one dot product, one scalar multiplication), never with another route.
tests/test_pubcomm_cases.py checks on the CPU that the rows meet the cases they are named after."""
import random

import numpy as np
import pytest

import srs_helpers as S

pytestmark = pytest.mark.gpu

ROUTES = {"default": {}, "8x32": dict(msm_fp29=0), "buckets": dict(pubcomm_direct=0), "buckets_8x32": dict(pubcomm_direct=0, msm_fp29=0)}


def _new_ctx(m, oracle, curve, g, h):
    c = m.MinaContext(0)
    for field in (0, 1):
        c.poseidon_set_params(field, m.poseidon_params.default_params_bytes(field))
    c.srs_load(curve, S.srs_blob(oracle, curve, g, h))
    return c


@pytest.fixture(scope="module")
def crafted(oracle):
    """{(name, curve): the SRS (c, t, g, h, G), a context of its own holding it, and for S1 the rows of public inputs with their reference commitments}"""
    import mina_bridge_amd as m
    out = {}
    try:
        for curve in (0, 1):
            t = S.blinder(curve)
            for name, c in (("S1", S.s1_coefficients(curve)), ("S2", S.s2_coefficients())):
                g, h, G = S.structured_srs(oracle, curve, c, t)
                e = dict(c=c, t=t, g=g, h=h, G=G, ctx=_new_ctx(m, oracle, curve, g, h))
                out[name, curve] = e
                if name == "S1":
                    for key, cases in (("rows", S.s1_cases(curve, c, t)), ("rows_small", S.s1_cases_small(curve, c, t))):
                        e[key] = dict(names=list(cases), cases=cases, pub=S.rows_le(oracle, cases),
                                      want=np.stack([S.reference_commitment(oracle, curve, c, t, G, v["pubs"]) for v in cases.values()]))
        yield out
    finally:
        for e in out.values():
            e["ctx"].close()


def _wrong(names, got, want):
    return [n for n, a, b in zip(names, got, want) if not (a == b).all()]


def _check_batched(ctx, curve, names, pub, want):
    """the rows as one small batch (64 lanes per proof) and tiled past 1024 proofs (8 lanes per proof)"""
    rows = len(names)
    wrong = _wrong(names, ctx.public_input_commitment_batch(curve, S.LOG2_DOMAIN, pub, rows), want)
    assert not wrong, ("64-lane form", wrong)
    reps = 1100 // rows + 1
    got = ctx.public_input_commitment_batch(curve, S.LOG2_DOMAIN, np.tile(pub, (reps, 1, 1)), rows * reps).reshape(reps, rows, 64)
    wrong = [n for i, n in enumerate(names) if not (got[:, i] == want[i][None]).all()]
    assert not wrong, ("8-lane form", wrong)


@pytest.mark.parametrize("curve", [0, 1])
def test_lagrange_basis_of_crafted_srs(crafted, oracle, curve):
    """the group iFFT over points with relations: S1's basis is [c_i G] with infinity at 3 and 24 (butterflies that meet equal and opposite points on the way); on S2 every
    g_j is G -- each butterfly of the first stage adds G to G and G to -G -- and the basis is [G, 0, 0, ...], at the domains 2^6, 2^5 and 2^1"""
    e = crafted["S1", curve]
    assert (e["ctx"].srs_get_g(curve, 0, S.DEPTH) == e["g"]).all() and (e["ctx"].srs_get_h(curve) == e["h"]).all()
    got = e["ctx"].srs_lagrange_basis(curve, S.LOG2_DOMAIN)
    want = np.stack([S.point_mul(oracle, curve, e["G"], ci) for ci in e["c"]])
    assert not want[3].any() and not want[24].any() and (want[0] == want[8]).all()
    assert not _wrong(range(len(want)), got, want)
    e = crafted["S2", curve]
    for k in (S.LOG2_DOMAIN, 5, 1):
        got = e["ctx"].srs_lagrange_basis(curve, k)
        assert (got[0] == e["G"]).all() and not got[1:].any(), k


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("curve", [0, 1])
def test_commitments_on_related_lagrange_points(crafted, curve, route):
    """every row of srs_helpers.s1_cases (32 inputs) and s1_cases_small (5 inputs) through the batched entry point -- with the default tuning (29-bit limbs, restart on the
    8 x 32 law), the 8 x 32 law throughout, and the bucket MSM over the Lagrange window table in both -- in the 64-lane and the 8-lane form, against the big-int reference"""
    import mina_bridge_amd as m
    e = crafted["S1", curve]
    with m.lib.tuning(**ROUTES[route]):
        for key in ("rows", "rows_small"):
            r = e[key]
            _check_batched(e["ctx"], curve, r["names"], r["pub"], r["want"])
    rows = e["rows"]                                               # what the rows are for: h itself, infinity, and scalars above r acting as their residues
    want = dict(zip(rows["names"], rows["want"]))
    for name in ("opposite", "inf_basis"):
        assert (want[name] == e["h"]).all()
    for name in ("a_eq_h_one", "a_eq_h"):
        assert not want[name].any()
    assert (want["large"] == want["large_reduced"]).all()


@pytest.mark.parametrize("curve", [0, 1])
def test_single_proof_commitments_on_related_lagrange_points(crafted, curve):
    """the single-proof entry point: a variable-base MSM over a basis that holds duplicates, opposites and infinity, finished on the host (A = H: all zeros; A = -H: a doubling)"""
    e = crafted["S1", curve]
    for key in ("rows", "rows_small"):
        r = e[key]
        got = [e["ctx"].public_input_commitment(curve, S.LOG2_DOMAIN, p) for p in r["pub"]]
        assert not _wrong(r["names"], got, r["want"]), key


@pytest.mark.parametrize("curve", [0, 1])
def test_commitments_when_all_but_one_lagrange_point_are_infinity(crafted, oracle, curve):
    """S2: the commitment is h - pub_0 G whatever the other scalars are, through every route (table rows of a point at infinity are (0, 0) and skipped)"""
    import mina_bridge_amd as m
    e = crafted["S2", curve]
    r = S.scalar_modulus(curve)
    rng = random.Random(1010 + curve)
    vals = [[rng.randrange(r) for _ in range(S.NPUB)] for _ in range(4)] + [[0] + [rng.randrange(r) for _ in range(S.NPUB - 1)], [e["t"]] + [1] * (S.NPUB - 1),
                                                                             [r - e["t"]] + [r - 1] * (S.NPUB - 1), [r] + [(1 << 255) - 1] * (S.NPUB - 1)]
    names = ["random_%d" % i for i in range(4)] + ["zero_first", "a_eq_h", "a_eq_neg_h", "large"]
    pub = np.stack([oracle.ints_to_le(v) for v in vals])
    want = np.stack([S.reference_commitment(oracle, curve, e["c"], e["t"], e["G"], v) for v in vals])
    assert (want[4] == e["h"]).all() and not want[5].any() and (want[7] == e["h"]).all()
    for route, tune in ROUTES.items():
        with m.lib.tuning(**tune):
            _check_batched(e["ctx"], curve, names, pub, want)
    assert not _wrong(names, [e["ctx"].public_input_commitment(curve, S.LOG2_DOMAIN, p) for p in pub], want)


# ---------------------------------------------------------------- the job path's finish (api_state.hip pubcomm_finish16_kernel) and a reloaded SRS
@pytest.fixture(scope="module")
def kimchi_proof(srs_oracle):
    """the synthetic index of tests/test_kimchi.py and the first of its proofs (minted on the honest SRS)"""
    from ipa_helpers import poseidon_pp
    from oracle import kimchi_ref as K, oracle as O, pasta_ref as R
    from test_kimchi import K_LOG2, NPUB
    assert (K_LOG2, NPUB) == (S.LOG2_DOMAIN, S.NPUB_SMALL)
    g, h = srs_oracle[0]
    circuit = K.synthetic_circuit(0, g, O.bytes_to_point(h), poseidon_pp(0), poseidon_pp(1), K_LOG2, NPUB, seed=21)
    rng = random.Random(100)
    pubs = [rng.randrange(R.Q) for _ in range(NPUB)]
    return circuit, pubs, K.synthetic_proof(circuit, g, O.bytes_to_point(h), poseidon_pp(0), poseidon_pp(1), pubs, seed=200)


def test_kimchi_public_commitment_row_on_related_lagrange_points(crafted, kimchi_proof):
    """mina_kimchi_to_batch on a context holding S1 (Pallas): row n_prev of the commitment list is the public-input commitment, finished on the device by the job path's
    kernel -- the equal pair (a doubling in the tree), the opposite pair (A = infinity), A = H (the all-zero row) and A = -H (a doubling in the finish).  The call builds
    rows, it does not verify: the other rows belong to a proof that was minted for other public inputs and are not looked at."""
    import mina_bridge_amd as m
    from kimchi_helpers import install_index, kimchi_arrays
    e = crafted["S1", 0]
    circuit, _, proof = kimchi_proof
    r = e["rows_small"]
    B, n_prev = len(r["names"]), len(proof["prev"])
    install_index(e["ctx"], circuit.index)
    arrays, _ = kimchi_arrays([proof] * B, [v["pubs"] for v in r["cases"].values()])
    got = e["ctx"].kimchi_to_batch(m.MinaContext.make_kimchi_proofs(B, n_prev, S.NPUB_SMALL, arrays), S.LOG2_DOMAIN)
    assert not _wrong(r["names"], got["comms"][:, n_prev], r["want"])
    assert not got["comms"][r["names"].index("a_eq_h"), n_prev].any() and (got["comms"][r["names"].index("opposite"), n_prev] == e["h"]).all()


def test_reloading_the_srs_invalidates_the_lagrange_tables(oracle, crafted, kimchi_proof):
    """A context prepared for device jobs on the honest SRS, then given S1 by mina_srs_load: the Lagrange window / digit tables on the device belong to the old SRS.  A device
    job with a kimchi leg must be refused (MINA_ERR_STATE: prepare first) instead of committing with them; after mina_state_jobs_prepare it is taken.  The host entry points
    rebuild by themselves: the same rows before and after the reload, each against its own SRS' reference."""
    import mina_bridge_amd as m
    from conftest import rand_scalars
    from kimchi_helpers import install_index
    from oracle import pasta_ref as R
    from test_kimchi import _kimchi_job
    e = crafted["S1", 0]
    circuit, pubs, proof = kimchi_proof
    _, honest_h = oracle.srs_create(0, S.DEPTH, threads=4)
    c = m.MinaContext(0)
    ptrs = []
    try:
        for field in (0, 1):
            c.poseidon_set_params(field, m.poseidon_params.default_params_bytes(field))
        c.srs_create(0, S.DEPTH)
        install_index(c, circuit.index)
        c.state_jobs_prepare(S.LOG2_DOMAIN, S.NPUB_SMALL)
        # host entry points on the honest SRS, against the oracle's naive sum over the honest basis
        pub = rand_scalars(3 * S.NPUB, R.Q, seed=1111).reshape(3, S.NPUB, 32)
        basis = c.srs_lagrange_basis(0, S.LOG2_DOMAIN)
        mod = R.base_modulus(0)
        honest_want = np.stack([oracle.point_to_bytes(R.add(oracle.bytes_to_point(honest_h), R.neg(oracle.bytes_to_point(oracle.msm_naive(0, basis[:S.NPUB], p)), mod), mod)) for p in pub])
        assert (c.public_input_commitment_batch(0, S.LOG2_DOMAIN, pub, 3) == honest_want).all()
        assert (c.public_input_commitment(0, S.LOG2_DOMAIN, pub[0]) == honest_want[0]).all()
        dj, ptrs = c.state_jobs_to_device(_kimchi_job(m, [proof], [pubs]))
        out = c.dev_malloc(4 + 16); ptrs.append(out)
        c.state_job_batch_dev(dj, out, out + 4); c.synchronize()
        assert c.dev_download(out, 4).view(np.uint32).tolist() == [1]                     # the proof verifies on the SRS it was minted for
        c.srs_load(0, S.srs_blob(oracle, 0, e["g"], e["h"]))
        with pytest.raises(m.MinaError, match=r"\(-3\).*mina_state_jobs_prepare"):
            c.state_job_batch_dev(dj, out, out + 4)
        c.synchronize()
        c.state_jobs_prepare(S.LOG2_DOMAIN, S.NPUB_SMALL)
        c.state_job_batch_dev(dj, out, out + 4); c.synchronize()
        assert c.dev_download(out, 4).view(np.uint32).tolist() in ([0], [1])              # taken; what it answers on another SRS is not this test's subject
        r = e["rows"]
        assert not _wrong(r["names"], c.public_input_commitment_batch(0, S.LOG2_DOMAIN, r["pub"], len(r["names"])), r["want"])
        assert (c.public_input_commitment(0, S.LOG2_DOMAIN, r["pub"][0]) == r["want"][0]).all()
        assert (c.public_input_commitment_batch(0, S.LOG2_DOMAIN, pub, 3) != honest_want).any()
    finally:
        c.synchronize()
        for p in ptrs:
            c.dev_free(p)
        c.close()
