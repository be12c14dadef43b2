"""The tables of tests/kimchi_rows_cases.py, checked on the CPU: they hold the corners they list, their periods meet every lane position, their distinct proofs
give pairwise different references (a tiled comparison cannot hide two proofs swapping lanes), the public-input counts reach every path of kimchi_pub_body's work
split, and the oracle is right where no test had used it: `pub_eval` at 0 public inputs, at the whole domain and in between, against the negated interpolant;
the evaluation list and the combined inner product at 0, 1, 3 and 8 recursion accumulators.  If the lane rule of kimchi_pub_body changes, pub_work_split changes
with it and the first test says which counts went dead."""
import math

import numpy as np
import pytest

import kimchi_rows_cases as C
from oracle import ipa_ref as I, kimchi_ref as K, pasta_ref as R


@pytest.fixture(scope="module")
def world(oracle):
    return C.shared_world()[0]


def test_public_input_counts_reach_every_path_of_the_work_split():
    s = {n: C.pub_work_split(n) for n in C.NPUB_LIST}
    assert [n for n in C.NPUB_LIST if s[n].ch == 10] == [33, 39, 40] and all(n <= 1 << C.domain_of(n) for n in C.NPUB_LIST)
    assert s[0].items == 0 and s[0].passes == [0] * 8 and s[0].last_chunk == 0                                       # no item at all
    assert s[1].passes == [1, 1, 0, 0, 0, 0, 0, 0] and s[1].last_chunk == 1                                         # one pass, partly filled
    assert s[7].passes == s[8].passes == s[1].passes and (s[7].last_chunk, s[8].last_chunk) == (7, 8)                # a chunk one short of full, and full
    assert s[9].passes == [1, 1, 1, 1, 0, 0, 0, 0] and s[9].last_chunk == 1
    assert (s[32].ch, s[32].passes, s[32].last_chunk) == (8, [1] * 8, 8)                                            # one pass exactly full, chunks of 8
    assert (s[40].ch, s[40].passes, s[40].last_chunk) == (10, [1] * 8, 10)                                          # ... and chunks of 10
    assert s[33].passes == s[39].passes == [1] * 8 and (s[33].last_chunk, s[39].last_chunk) == (3, 9)               # a partial last chunk at CH = 10
    assert s[41].passes == [2, 2, 2, 2, 1, 1, 1, 1] and s[41].last_chunk == 1                                       # a second pass on some lanes only
    assert s[63].passes == s[64].passes == [2] * 8 and (s[63].last_chunk, s[64].last_chunk) == (7, 8)               # two full passes; 64 is the whole 2^6 domain
    assert s[65].passes == [3, 3, 2, 2, 2, 2, 2, 2] and s[65].last_chunk == 1                                       # a third pass
    assert s[80].passes == [3, 3, 3, 3, 2, 2, 2, 2] and s[128].passes == [4] * 8                                    # 128 is the whole 2^7 domain
    for n in C.NPUB_LIST:                                                                                           # the split covers every input exactly once per side
        assert s[n].chunks * s[n].ch >= n > (s[n].chunks - 1) * s[n].ch or n == 0
        assert sum(s[n].passes) == s[n].items == 2 * s[n].chunks


def test_corner_table_holds_every_listed_corner(world):
    cases = C.corner_cases(world)
    seen = C.census(cases)
    assert len(cases) == C.PERIOD >= 45
    assert not C.required_corners() - seen, sorted(map(str, C.required_corners() - seen))
    evals = {x[1:] for x in seen if x[0] == "eval"}
    assert {col for col, _, _ in evals} == set(range(C.N_COLS))                                                     # every column meets a corner
    assert {(row, v) for _, row, v in evals} == {(row, v) for row in (0, 1) for v in C.CORNERS}                     # both rows, every corner
    all_t = {("inf", "t_comm", i) for i in range(7)} | {("inf", "t_comm", "all")}
    all_zero = {("pub", i, 0) for i in range(C.BASE_NPUB)} | {("pubs_all_zero",)}
    assert all(len(s) == 1 or s in (all_t, all_zero) for s in (C.census([c]) for c in cases[:81])), "a proof of the first 81 carries one corner"
    assert all(len(C.census([c])) >= 5 for c in cases[81:93]) and not C.census(cases[93:])
    # every point is an SRS point or infinity, every scalar canonical: the table is well-formed
    for c in cases:
        p = c.proof
        pts = [cm for _, cm in p["prev"]] + p["w_comm"] + [p["z_comm"]] + p["t_comm"]
        assert all(pt is None or pt in world.points for pt in pts)
        assert all(0 <= x < C.R_MOD for x in c.pubs + [p["ft_eval1"]] + [e for pair in p["evals"] for e in pair] + [x for ch, _ in p["prev"] for x in ch])


def test_periods_meet_every_lane_position():
    for period in (C.PERIOD, C.BATCH):
        assert all(math.gcd(period, n) == 1 for n in (3, 8, 21, 64)), period
    assert max(C.TILES) > C.PERIOD and {1, 3, 4, 5, 7, 8, 9, 21, 22, 43, 63, 64, 65, 129} == set(C.TILES)


@pytest.mark.parametrize("name", C.all_tables())
def test_distinct_proofs_give_pairwise_different_references(world, name):
    t = world.table(name)
    assert len(t.cases) == (C.PERIOD if name == "corners" else C.BATCH)
    for f in C.FIELDS:
        rows = {r.tobytes() for r in t.want[f]}
        assert len(rows) == len(t.cases), (name, f)
    ft_rows = {r.reshape(-1, 64)[t.n_prev + 1].tobytes() for r in t.want["comms"]}                                  # the row kimchi_ftcomm_body writes, on its own
    assert len(ft_rows) == len(t.cases) and bytes(64) not in ft_rows


def test_index_parameters_move_the_references(world):
    """the same five proofs under every perm_alpha_offset and every zk_rows: ft_eval0, the combined inner product and the ft row differ from variant to variant,
    so a kernel that read the wrong parameter could not pass; the parameters are the install call's limits and the circuit's own"""
    base = world.table("nprev/%d" % C.BASE_NPREV)
    assert (base.index.perm_alpha_offset, base.index.zk_rows) == (21, 3) and world.table("alpha/21") is base and world.table("zk/3") is base
    assert C.ALPHA_OFFSETS == (0, 1, 21, 1024) and C.ZK_ROWS == (1, 3, 8) and C.KC_MAX_ZK == 8
    for names in (["alpha/%d" % a for a in C.ALPHA_OFFSETS], ["zk/%d" % z for z in C.ZK_ROWS]):
        ts = [world.table(n) for n in names]
        for t, n in zip(ts, names):
            kind, _, arg = n.partition("/")
            assert getattr(t.index, "perm_alpha_offset" if kind == "alpha" else "zk_rows") == int(arg) and t.index.digest == K.index_digest(t.index, world.pp[0])
            assert t.cases is base.cases or t is base
        for b in range(C.BATCH):
            for f in ("ft_eval0", "cip"):
                assert len({t.want[f][b].tobytes() for t in ts}) == len(ts), (names, b, f)
            assert len({t.want["comms"][b].tobytes() for t in ts}) == len(ts)
            for f in ("sponge", "evalpoints", "polyscale", "evalscale"):                                            # the transcript does not see either parameter
                assert len({t.want[f][b].tobytes() for t in ts}) == 1, (names, b, f)


@pytest.mark.parametrize("npub", C.NPUB_LIST)
def test_oracle_public_evaluations_are_the_negated_interpolant(world, npub):
    t = world.table("npub/%d" % npub)
    r, n = C.R_MOD, 1 << t.k
    w = K.O_domain_generator(r, t.k)
    assert t.k == C.domain_of(npub) and npub <= n
    for c, o in zip(t.cases, t.oracles):
        assert len(c.pubs) == npub
        coeffs = K._ifft(list(c.pubs) + [0] * (n - npub), w, r)
        zeta = o["zeta"]
        want = tuple((-K._peval(coeffs, x, r)) % r for x in (zeta, zeta * w % r))
        assert o["public_evals"] == want
        assert (want == (0, 0)) == (npub == 0)


@pytest.mark.parametrize("n_prev", C.NPREV_LIST)
def test_oracle_evaluation_list_and_combined_inner_product(world, n_prev):
    t = world.table("nprev/%d" % n_prev)
    r = C.R_MOD
    w = K.O_domain_generator(r, t.k)
    for c, o in zip(t.cases, t.oracles):
        ev = o["evaluations"]
        assert len(c.proof["prev"]) == n_prev and len(ev) == len(o["comms"]) == n_prev + 45
        assert o["combined_inner_product"] == I.combined_inner_product([list(e) for e in ev], o["v"], o["u"], r)
        zeta = o["zeta"]
        for (chals, comm), e, cm in zip(c.proof["prev"], ev, o["comms"]):                                           # the list starts with the accumulators
            assert e == (R.b_poly(chals, zeta, r), R.b_poly(chals, zeta * w % r, r)) and cm == comm
        assert ev[n_prev] == o["public_evals"] and ev[n_prev + 1] == (o["ft_eval0"], c.proof["ft_eval1"]) and ev[n_prev + 2:] == list(c.proof["evals"])
        assert o["comms"][n_prev] == o["public_comm"] and o["comms"][n_prev + 1] == o["ft_comm"]


def test_ft_row_with_every_t_commitment_at_infinity(world, oracle):
    t = world.table("corners")
    hit = [i for i, c in enumerate(t.cases) if all(pt is None for pt in c.proof["t_comm"])]
    assert len(hit) >= 2
    for i in hit:
        o = t.oracles[i]
        want = R.scalar_mul(o["perm_scalar"], t.index.sigma_comm[K.PERMUTS - 1], C.P_MOD)
        assert want is not None and o["ft_comm"] == want
        assert t.want["comms"][i].reshape(-1, 64)[t.n_prev + 1].tobytes() == oracle.point_to_bytes(want).tobytes()
    inf_rows = [i for i, c in enumerate(t.cases) if c.proof["z_comm"] is None]                                      # infinity travels as (0, 0) through the rows
    assert inf_rows and all(not t.want["comms"][i].reshape(-1, 64)[t.n_prev + 2].any() for i in inf_rows)


def test_malformed_variants_change_one_value_of_one_proof(world):
    variants = C.malformed_variants()
    assert len(variants) == len(C.MALFORMED_SCALARS) + 2 * len(C.MALFORMED_POINTS) == 19
    for slot, kind in variants:
        for victim in C.VICTIMS:
            C.malformed(world, slot, kind, victim)                                                                  # asserts: one section, the victim's part alone


def test_tiles_go_round_the_distinct_proofs(world):
    t = world.table("nprev/0")
    assert "prev_chals" not in t.arrays and "prev_comms" not in t.arrays                                            # no recursion arrays are passed at all
    assert "public_inputs" not in world.table("npub/0").arrays
    arrays, order = C.tile(t, 13)
    assert order.tolist() == [i % 5 for i in range(13)]
    for key, a in arrays.items():
        per = t.arrays[key].size // C.BATCH
        assert a.size == 13 * per and (a.reshape(13, per) == t.arrays[key].reshape(C.BATCH, per)[order]).all()
