"""`ipa_prepare_kernel` (mina_bridge_amd/csrc/api_ipa.hip: phases 1 and 2 in its 16-, 8- and wave-packed 3-lane forms), `ipa_to_group_kernel` beside it,
`ipa_shared_tail_kernel` and `ipa_shared_restore_kernel`, held VALUE FOR VALUE to tests/ipa_rows_model.py through mina_selftest_ipa_rows: the (point, scalar) rows
that go to the combined MSM, the challenges, the fold weights, the side matrix of the batch-shared points, the malformed-input word.  Every comparison is equality
of bytes.  The inputs are no valid openings -- a valid proof cannot be steered to combined_inner_product = 2^255, a sponge position of one's choice or infinity as
L_0 -- and a verdict is not looked at anywhere: tests/test_ipa_rows_model.py ties the model to the restatement that decides verdicts.

Each call runs under a forced lane form (as FORCED_SHAPES of test_verify_fullsize.py forces them) and asserts the form and the side-stream word the library reports,
so a tuning change cannot move the cases onto one form unnoticed.  The model runs once per case table (the `env` fixture caches the tables) and is shared by the forms."""
import random

import numpy as np
import pytest

import ipa_rows_model as M
from ipa_helpers import poseidon_pp

pytestmark = pytest.mark.gpu

FORMS = {16: dict(coop16_max=1 << 30), 8: dict(coop16_max=0, ipa_coop8_max=1 << 30, transcript_coop8_max=1 << 30), 3: dict(coop16_max=0, transcript_coop8_max=1)}
SRS_POINTS = 64                       # the entry point needs h, not 2^k points of g: k = 20 runs on this


@pytest.fixture(scope="module")
def env(oracle):
    import mina_bridge_amd as m
    from oracle import pasta_ref as R
    c = m.MinaContext(0)
    e = {"m": m, "ctx": c, "g": {}, "h": {}, "pp": {}, "r": {}, "p": {}, "tables": {}}
    try:
        for f in (0, 1):
            c.poseidon_set_params(f, m.poseidon_params.default_params_bytes(f))
        for curve in (0, 1):
            c.srs_create(curve, SRS_POINTS)
            g, h = oracle.srs_create(curve, SRS_POINTS, threads=4)
            assert (c.srs_get_h(curve) == h).all()
            e["g"][curve], e["h"][curve] = [oracle.bytes_to_point(b) for b in g], oracle.bytes_to_point(h)
            e["pp"][curve], e["r"][curve], e["p"][curve] = poseidon_pp(curve), R.scalar_modulus(curve), R.base_modulus(curve)
        yield e
    finally:
        c.close()


def table(env, key, build):
    """the case table `key`, built once: build() -> (proofs, rand_base, sg_rand_base, model options) -> the packed openings, the model's rows and their bytes"""
    if key not in env["tables"]:
        curve = key[1]
        proofs, rb, sb, opts = build()
        rows = M.ipa_rows(curve, env["pp"][curve], env["h"][curve], proofs, rb, sb, **opts)
        env["tables"][key] = {"proofs": proofs, "packed": env["ctx"].pack_ipa_openings([M.to_abi(q) for q in proofs]), "rb": rb, "sb": sb, "opts": opts,
                              "rows": rows, "bytes": M.rows_bytes(rows)}
    return env["tables"][key]


def abi_opts(opts):
    """the model's keyword arguments -> those of MinaContext.selftest_ipa_rows"""
    o = {k: v for k, v in opts.items() if k in ("pow_first", "override_slot", "expand_slot", "shared_mask", "shared_h", "shared_expand0")}
    if "comm_override" in opts:
        o["comm_override"] = M.pts_bytes(opts["comm_override"])
    if "expand_slot" in opts:
        o["expand_point0"] = M.pt_bytes(opts["expand_point0"])
        o["expand_points"] = np.stack([M.pts_bytes(q) for q in opts["expand_points"]])
        o["expand_scalars"] = np.stack([M.ints_bytes(s) for s in opts["expand_scalars"]])
    return o


def run(env, curve, form, side, packed, rb, sb, **kw):
    with env["m"].lib.tuning(ipa_side_stream=side, **FORMS[form]):
        got = env["ctx"].selftest_ipa_rows(curve, packed, M.le32(rb), M.le32(sb), **kw)
    assert got["lanes"] == form, f"asked for the {form}-lane form, the library ran {got['lanes']}"
    assert got["side_stream"] == side, f"ipa_side_stream = {side}, the library reports {got['side_stream']}"
    return got


def first(env, packed, n):
    """the first n of a table's packed openings, as a batch of their own"""
    arr, keep = packed
    return (env["m"].lib.IpaOpening * n)(*arr[:n]), keep


def same(got, want, wb=None, skip=()):
    """every row, challenge, weight, side-matrix entry and offset equal, byte for byte; the proofs in `skip` (malformed ones: their rows are unspecified) left out"""
    wb = wb or M.rows_bytes(want)
    per, batch, ns = want["per"], len(want["sigma"]), want["nshared"]
    assert (got["per"], got["nshared"]) == (per, ns)
    keep = np.ones(batch * per + ns, bool)
    for b in skip:
        keep[b * per:(b + 1) * per] = False
    live = [b for b in range(batch) if b not in skip]
    for name in ("points", "scalars"):
        diff = np.nonzero(keep & (got[name] != wb[name]).any(axis=1))[0]
        where = [("tail", int(i - batch * per)) if i >= batch * per else (int(i // per), int(i % per)) for i in diff[:6]]
        assert not len(diff), f"{name}: {len(diff)} rows differ, first (proof, entry): {where}; got {got[name][diff[0]].tobytes().hex()} want {wb[name][diff[0]].tobytes().hex()}"
    assert (got["chals"][live] == wb["chals"][live]).all(), "challenges differ"
    assert (got["sigma"][live] == wb["sigma"][live]).all(), "fold weights differ"
    if not skip:
        assert (got["side"] == wb["side"]).all(), "side matrix differs"
    assert got["offsets"].tolist() == want["offsets"], "offsets of the shared entries differ"


# ------------------------------------------------------------------------------------------------ (a) the corner table
RUNS = [(rb, sb, pf) for pf in (0, 1) for (rb, sb) in (("rnd", "rnd"), (1, 0), (0, 1))]


def corner_proofs(env, curve):
    """45 proofs at k = 3 (full and partial waves in every form: 4, 8 and 21 proofs per wave), one corner each, then twelve that combine them"""
    r, g = env["r"][curve], env["g"][curve]
    rng = random.Random(100 + curve)
    ps = [M.random_proof(rng, curve, g, 3, 2, 2) for _ in range(45)]
    cips = [0, 1, (2 ** 255 - 1) % r, 2 ** 255 % r, (2 ** 255 + 1) % r, (2 ** 255 + 2) % r, r - 1]      # shift_scalar subtracts 2^255 (+ 1): zero, minus one, the low bit
    i = 0
    for v in cips:
        ps[i]["cip"] = v; i += 1
    for mode in (0, 1):
        for cnt in (0, 1, 2):
            ps[i]["sponge_mode"], ps[i]["sponge_count"] = mode, cnt; i += 1
    ps[i]["lr"][0] = (None, ps[i]["lr"][0][1]); i += 1
    ps[i]["lr"][2] = (ps[i]["lr"][2][0], None); i += 1
    ps[i]["delta"] = None; i += 1
    ps[i]["sg"] = None; i += 1
    ps[i]["comms"][1] = None; i += 1
    for key in ("evalscale", "polyscale", "z1", "z2"):
        for v in (0, 1, r - 1):
            ps[i][key] = v; i += 1
    for v in (0, 1, r - 1):
        ps[i]["evalpoints"] = [v, rng.randrange(r)]; i += 1
    assert i == 33
    for j in range(33, 45):
        ps[j]["cip"] = cips[j % 7]
        ps[j]["sponge_mode"], ps[j]["sponge_count"] = divmod(j % 6, 3)
        ps[j]["evalpoints"] = [(0, 1, r - 1)[j % 3], (r - 1, 0, 1)[j % 3]]
    return ps


def corner_table(env, curve, rb, sb, pf):
    def build():
        if ("corner-proofs", curve) not in env["tables"]:
            env["tables"][("corner-proofs", curve)] = corner_proofs(env, curve)
        base = env["tables"][("corner-proofs", curve)]
        rng = random.Random(7)
        val = lambda v: rng.randrange(env["r"][curve]) if v == "rnd" else v      # noqa: E731
        return base, val(rb), val(sb), {"pow_first": pf}
    return table(env, ("corner", curve, rb, sb, pf), build)


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("form", [16, 8, 3])
@pytest.mark.parametrize("curve", [0, 1])
def test_corner_table(env, curve, form, side):
    """cip around 2^255, every sponge start position, infinity in every point slot, 0 / 1 / r - 1 in every scalar slot; rand_base and sg_rand_base random, 1 and 0;
    pow_first 0 and 1; with and without the side stream"""
    for rb, sb, pf in RUNS:
        t = corner_table(env, curve, rb, sb, pf)
        got = run(env, curve, form, side, t["packed"], t["rb"], t["sb"], pow_first=pf)
        assert got["malformed"] == 0, (rb, sb, pf)
        try:
            same(got, t["rows"], t["bytes"])
        except AssertionError as e:
            raise AssertionError(f"rand_base {rb}, sg_rand_base {sb}, pow_first {pf}: {e}") from None


# ------------------------------------------------------------------------------------------------ (b) shapes
SHAPES = {   # name: (k, n_evalpoints, n_comms per proof)
    "k1": (1, 2, [2] * 3), "k2": (2, 2, [2] * 3), "k15": (15, 2, [2] * 3), "k20": (20, 2, [2] * 2),        # chal_m[20] and pre[20] exactly full at 20
    "evalpoints0": (2, 0, [2] * 3), "evalpoints1": (2, 1, [2] * 3), "evalpoints4": (2, 4, [2] * 3),
    "comms0": (2, 2, [0] * 3), "comms1": (2, 2, [1] * 3), "comms45": (2, 2, [45] * 3), "comms65": (2, 2, [65] * 3), "comms70": (2, 2, [70] * 3),
    "comms_mixed": (2, 2, [3, 0, 5, 1]),                                                                    # the short lists are padded with infinity
}


@pytest.mark.parametrize("form", [16, 8, 3])
@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("curve", [0, 1])
def test_shapes(env, curve, shape, form):
    k, npts, ncomms = SHAPES[shape]

    def build():
        rng = random.Random(200 + curve + 10 * sorted(SHAPES).index(shape))
        return [M.random_proof(rng, curve, env["g"][curve], k, nc, npts) for nc in ncomms], rng.randrange(env["r"][curve]), rng.randrange(env["r"][curve]), {}
    t = table(env, ("shape", curve, shape), build)
    got = run(env, curve, form, 1, t["packed"], t["rb"], t["sb"])
    assert got["malformed"] == 0 and got["per"] == 2 * k + max(ncomms) + 4
    same(got, t["rows"], t["bytes"])


# ------------------------------------------------------------------------------------------------ (c) batch sizes at the lane-group edges of each form
EDGES = [(16, 1), (16, 4), (16, 5), (8, 8), (8, 9), (3, 20), (3, 21), (3, 22), (3, 43), (3, 64)]      # 4, 8 and 21 proofs per wave (lane 63 of the 3-lane form shadows sponge 20)


@pytest.mark.parametrize("form,batch", EDGES)
@pytest.mark.parametrize("curve", [0, 1])
def test_batch_edges(env, curve, form, batch):
    def build():
        rng = random.Random(300 + curve)
        return [M.random_proof(rng, curve, env["g"][curve], 2, 2, 1) for _ in range(64)], rng.randrange(env["r"][curve]), rng.randrange(env["r"][curve]), {}
    t = table(env, ("edges", curve), build)
    want = M.prefix(t["rows"], batch, env["r"][curve])
    got = run(env, curve, form, 1, first(env, t["packed"], batch), t["rb"], t["sb"])
    assert got["malformed"] == 0
    same(got, want)


# ------------------------------------------------------------------------------------------------ (d) the options only the Proof-of-State job sets
def job_case(env, curve, name):
    r, g = env["r"][curve], env["g"][curve]
    rng = random.Random(400 + curve + 10 * sorted(JOB_CASES).index(name))
    pick = lambda: g[rng.randrange(len(g))]      # noqa: E731

    def proofs(batch, k, ncomms, mask=0):
        ps = [M.random_proof(rng, curve, g, k, ncomms, 2) for _ in range(batch)]
        for q in ps:                                            # the caller vouches that a shared entry is the same point in every proof
            q["comms"] = [ps[0]["comms"][i] if (mask >> i) & 1 else q["comms"][i] for i in range(ncomms)]
        return ps

    def expand(batch, scalars=None):
        return {"expand_point0": pick(), "expand_points": [[pick() for _ in range(7)] for _ in range(batch)],
                "expand_scalars": scalars or [[rng.randrange(r) for _ in range(8)] for _ in range(batch)]}
    if name == "kimchi":                                        # state_job.hip: n_prev = 2, 47 commitments, the ft commitment expanded, selectors + coefficients + sigma shared
        n_prev, mask = 2, 0
        for i in list(range(n_prev + 3, n_prev + 9)) + list(range(n_prev + 24, n_prev + 45)):
            mask |= 1 << i
        ps = proofs(5, 3, n_prev + 45, mask)
        opts = dict(expand_slot=n_prev + 1, shared_mask=mask, shared_h=1, shared_expand0=1, **expand(5))
    elif name == "mask_word_edges":                             # the mask is two 32-bit words behind an `i < 64` guard
        mask = 1 | 1 << 31 | 1 << 32 | 1 << 63
        ps, opts = proofs(4, 2, 64, mask), dict(shared_mask=mask)
    elif name == "override":
        ps, opts = proofs(5, 2, 3), dict(override_slot=1, comm_override=[pick(), None, pick(), pick(), pick()])
    elif name == "expand_plain":
        ps, opts = proofs(5, 2, 3), dict(expand_slot=2, **expand(5))
    else:                                                       # expand_corners: scalars 0, 1 and r - 1, infinity as an expanded point, term 0 shared alone
        sc = [[rng.randrange(r) for _ in range(8)] for _ in range(5)]
        sc[0][0], sc[0][7], sc[1][0], sc[1][3], sc[2][5], sc[3] = 0, r - 1, r - 1, 0, 1, [0] * 8
        ps, opts = proofs(5, 2, 3), dict(expand_slot=0, shared_expand0=1, **expand(5, sc))
        opts["expand_points"][1][2] = None; opts["expand_points"][4][6] = None
    return ps, rng.randrange(r), rng.randrange(r), opts


JOB_CASES = {"kimchi": 29, "mask_word_edges": 4, "override": 0, "expand_plain": 0, "expand_corners": 1}      # name: nshared


@pytest.mark.parametrize("form", [16, 8, 3])
@pytest.mark.parametrize("name", sorted(JOB_CASES))
@pytest.mark.parametrize("curve", [0, 1])
def test_job_options(env, curve, name, form):
    t = table(env, ("job", curve, name), lambda: job_case(env, curve, name))
    got = run(env, curve, form, 1, t["packed"], t["rb"], t["sb"], **abi_opts(t["opts"]))
    assert got["malformed"] == 0 and got["nshared"] == JOB_CASES[name]
    same(got, t["rows"], t["bytes"])


# ------------------------------------------------------------------------------------------------ (e) the shared tail and the restore
TAIL_OPTS = dict(shared_mask=0b101, shared_h=1)


def tail_table(env, curve):
    def build():
        rng = random.Random(500 + curve)
        g = env["g"][curve]
        ps = [M.random_proof(rng, curve, g, 1, 3, 1) for _ in range(600)]
        for q in ps:
            q["comms"][0], q["comms"][2] = g[3], g[11]
        return ps, rng.randrange(env["r"][curve]), rng.randrange(env["r"][curve]), dict(TAIL_OPTS)
    return table(env, ("tail", curve), build)


@pytest.mark.parametrize("batch", [1, 255, 256, 257, 600])
@pytest.mark.parametrize("curve", [0, 1])
def test_shared_tail_sums(env, curve, batch):
    """ipa_shared_tail_kernel sums with 256 threads striding over the batch: one short of, at, and one past a stride, and more than two"""
    t = tail_table(env, curve)
    want = M.prefix(t["rows"], batch, env["r"][curve])
    got = run(env, curve, 8 if batch == 1 else 3, 1, first(env, t["packed"], batch), t["rb"], t["sb"], **TAIL_OPTS)
    assert got["malformed"] == 0 and got["nshared"] == 3
    same(got, want)


@pytest.mark.parametrize("lo,cnt", [(0, 1), (255, 2), (599, 1), (0, 600)])
@pytest.mark.parametrize("curve", [0, 1])
def test_shared_restore(env, curve, lo, cnt):
    """ipa_shared_restore_kernel: exactly the proofs [lo, lo + cnt) carry their own scalars of the shared points again, everybody else's stay zero, the side matrix
    and the tail stay as they were"""
    t = tail_table(env, curve)
    got = run(env, curve, 8, 1, t["packed"], t["rb"], t["sb"], restore=(lo, cnt), **TAIL_OPTS)
    want = M.restore(t["rows"], lo, cnt)
    same(got, want)
    per = want["per"]
    sc = got["scalars"][: 600 * per].reshape(600, per, 32)
    inside = np.zeros(600, bool); inside[lo:lo + cnt] = True
    for q, o in enumerate(want["offsets"]):
        assert not sc[~inside, o].any(), "a proof outside the range got a scalar back"
        assert (sc[inside, o] == got["side"][inside, q]).all() and sc[inside, o].any()
    assert (got["side"] == t["bytes"]["side"]).all() and (got["scalars"][600 * per:] == t["bytes"]["scalars"][600 * per:]).all()


# ------------------------------------------------------------------------------------------------ (f) malformed inputs
VICTIM = 2
MALFORMED = ["L_off_curve", "R_off_curve", "delta_off_curve", "sg_off_curve", "comm_off_curve", "expanded_off_curve", "override_off_curve", "x_alias",
             "z1", "z2", "cip", "evalscale", "polyscale", "evalpoint", "sponge_state"]


def malformed_case(env, curve, kind):
    """a clean batch of 5 (k = 2, three commitments: one plain, one expanded, one overridden), then ONE malformed value in proof VICTIM"""
    r, p, g = env["r"][curve], env["p"][curve], env["g"][curve]
    rng = random.Random(600 + curve)
    pick = lambda: g[rng.randrange(len(g))]      # noqa: E731
    ps = [M.random_proof(rng, curve, g, 2, 3, 1) for _ in range(5)]
    opts = dict(expand_slot=1, override_slot=2, comm_override=[pick() for _ in range(5)], expand_point0=pick(),
                expand_points=[[pick() for _ in range(7)] for _ in range(5)], expand_scalars=[[rng.randrange(r) for _ in range(8)] for _ in range(5)])
    rb, sb = rng.randrange(r), rng.randrange(r)
    x, y = g[17]
    off = (x, (y + 1) % p)
    assert (off[1] ** 2 - off[0] ** 3 - 5) % p != 0
    v = ps[VICTIM]
    if kind == "L_off_curve": v["lr"][0] = (off, v["lr"][0][1])
    elif kind == "R_off_curve": v["lr"][1] = (v["lr"][1][0], off)
    elif kind == "delta_off_curve": v["delta"] = off
    elif kind == "sg_off_curve": v["sg"] = off
    elif kind == "comm_off_curve": v["comms"][0] = off
    elif kind == "expanded_off_curve": opts["expand_points"][VICTIM][4] = off
    elif kind == "override_off_curve": opts["comm_override"][VICTIM] = off
    elif kind == "x_alias": v["comms"][0] = (x + p, y)           # the same group element, an encoding upstream's deserialiser refuses
    elif kind in ("z1", "z2", "cip", "evalscale", "polyscale"): v[kind] += r
    elif kind == "evalpoint": v["evalpoints"][0] += r
    elif kind == "sponge_state": v["sponge_state"][1] += p
    else: assert kind == "clean"
    return ps, rb, sb, opts


@pytest.mark.parametrize("form", [16, 8, 3])
@pytest.mark.parametrize("kind", ["clean"] + MALFORMED)
@pytest.mark.parametrize("curve", [0, 1])
def test_malformed_inputs(env, curve, kind, form):
    """the flag says 1, and the rows of the four clean proofs are still the model's; with nothing malformed it says 0"""
    t = table(env, ("malformed", curve, kind), lambda: malformed_case(env, curve, kind))
    want = t["rows"]
    assert want["malformed_each"] == [kind != "clean" and b == VICTIM for b in range(5)]
    got = run(env, curve, form, 1, t["packed"], t["rb"], t["sb"], **abi_opts(t["opts"]))
    assert got["malformed"] == (0 if kind == "clean" else 1)
    same(got, want, t["bytes"], skip=() if kind == "clean" else (VICTIM,))
