"""The inputs of tests/test_gpu_kimchi_rows.py and their references: proof dicts in the layout kimchi_helpers.kimchi_arrays takes, over kimchi_ref.synthetic_circuit's
verifier index at log2 domain 6 and 7, each with the batch entry `oracle/kimchi_ref.py oracles_and_batch` computes for it.  The proofs do not verify and need not:
`oracles_and_batch` and mina_kimchi_to_batch compute the same entry for any well-formed input.  Points are SRS points (or None, infinity), scalars are random
unless a case sets them.

Tables (World.table(name) builds one once, with its references, and keeps it):
  npub/<n>     5 proofs with n public inputs, n in NPUB_LIST, two recursion accumulators; domain 2^6 where n fits, 2^7 above
  nprev/<n>    5 proofs with n recursion accumulators, n in NPREV_LIST, 5 public inputs, domain 2^6
  alpha/<a>    the proofs of nprev/2 under the index with perm_alpha_offset = a, a in ALPHA_OFFSETS
  zk/<z>       the same under zk_rows = z, z in ZK_ROWS
  corners      PERIOD proofs of the nprev/2 shape: one corner each (census() names them), twelve that combine corners, two plain ones
malformed(world, slot, kind, victim) is nprev/2 with one bad value in proof `victim`.

tests/test_kimchi_rows_cases.py checks, without a GPU, that these tables are what they claim."""
import copy
import dataclasses
import random
from types import SimpleNamespace

import numpy as np

from oracle import kimchi_ref as K, oracle as O, pasta_ref as R

CURVE = 0                                      # Pallas: scalars in Fq, coordinates in Fp
R_MOD, P_MOD = R.scalar_modulus(CURVE), R.base_modulus(CURVE)
N_COLS = K.N_EVAL_COLS
NPUB_LIST = (0, 1, 7, 8, 9, 32, 33, 39, 40, 41, 63, 64, 65, 80, 128)
NPREV_LIST = (0, 1, 2, 3, 8)
ALPHA_OFFSETS = (0, 1, 21, 1024)
KC_MAX_ZK = 8                                  # csrc/kimchi_dev.cuh
ZK_ROWS = (1, 3, KC_MAX_ZK)                    # 3: synthetic_circuit's own
CORNERS = (0, 1, R_MOD - 1)
BASE_K, BASE_NPUB, BASE_NPREV = 6, 5, 2        # the shape of the corner and malformed tables
BATCH = 5
PERIOD = 95                                    # 5 x 19: coprime to 3, 8, 21 and 64
TILES = (1, 3, 4, 5, 7, 8, 9, 21, 22, 43, 63, 64, 65, 129)
# what a comparison covers; "sponge" is the state and the position after it (the position depends on the shape alone)
FIELDS = ("sponge", "evalpoints", "polyscale", "evalscale", "ft_eval0", "cip", "comms")
MALFORMED_SCALARS = ("eval_c0_r0", "eval_c42_r1", "ft_eval1", "pub_first", "pub_last", "chal_first", "chal_last")
MALFORMED_POINTS = ("prev_comm", "w_comm_0", "w_comm_14", "z_comm", "t_comm_0", "t_comm_6")
POINT_KINDS = ("off_curve", "x_alias")
VICTIMS = (0, 2, 4)


def pub_work_split(npub):
    """csrc/api_kimchi.hip kimchi_pub_body, restated: a proof's 8 lanes take the work items it = ln, ln + 8, ... of 2 * ceil(npub / CH) -- one per (chunk of CH
    public inputs, evaluation point) -- with CH = 10 for 33 to 40 inputs and 8 otherwise (mb_kimchi_to_batch_dev)"""
    ch = 10 if 32 < npub <= 40 else 8
    chunks = -(-npub // ch)
    items = 2 * chunks
    return SimpleNamespace(ch=ch, chunks=chunks, items=items, passes=[len(range(ln, items, 8)) for ln in range(8)], last_chunk=npub - (chunks - 1) * ch if chunks else 0)


def domain_of(npub):
    return 6 if npub <= 64 else 7


class World:
    """the SRS the proofs take their points from, the two circuits, and the tables built so far.  g, h: oracle.srs_create(0, n) with n >= 128"""
    def __init__(self, g, h):
        from ipa_helpers import poseidon_pp
        assert len(g) >= 128
        self.g, self.h = g, O.bytes_to_point(h)
        self.pp = (poseidon_pp(0), poseidon_pp(1))
        self.points = [O.bytes_to_point(b) for b in g[:128]]
        self._index, self._tables = {}, {}

    def index(self, k, **changes):
        """synthetic_circuit's verifier index at log2 domain k; with `changes` a copy with those fields replaced and the digest recomputed"""
        if k not in self._index:
            self._index[k] = K.synthetic_circuit(CURVE, self.g, self.h, self.pp[0], self.pp[1], k, BASE_NPUB, seed=15 + k).index
        ix = self._index[k]
        if changes:
            ix = dataclasses.replace(ix, **changes)
            ix.digest = K.index_digest(ix, self.pp[0])
        return ix

    def table(self, name):
        if name not in self._tables:
            self._tables[name] = _build(self, name)
        return self._tables[name]


_SHARED = []


def shared_world():
    """one World per process, on the first 128 points of the Pallas SRS: the CPU-tier test and the GPU tests of one session build each table once between them"""
    if not _SHARED:
        g, h = O.srs_create(CURVE, 128, threads=4)
        _SHARED.append((World(g, h), h))
    return _SHARED[0]


def all_tables():
    return (["npub/%d" % n for n in NPUB_LIST] + ["nprev/%d" % n for n in NPREV_LIST] + ["alpha/%d" % a for a in ALPHA_OFFSETS] + ["zk/%d" % z for z in ZK_ROWS]
            + ["corners"])


def random_case(rng, world, k, npub, n_prev):
    pick = lambda: world.points[rng.randrange(len(world.points))]      # noqa: E731
    sc = lambda: rng.randrange(R_MOD)      # noqa: E731
    proof = {"prev": [([sc() for _ in range(k)], pick()) for _ in range(n_prev)], "w_comm": [pick() for _ in range(K.COLUMNS)], "z_comm": pick(),
             "t_comm": [pick() for _ in range(K.PERMUTS)], "evals": [(sc(), sc()) for _ in range(N_COLS)], "ft_eval1": sc(), "opening": None}
    return SimpleNamespace(pubs=[sc() for _ in range(npub)], proof=proof)


def reference(world, index, case):
    """oracles_and_batch of one proof -> (its fields as the bytes mina_kimchi_to_batch returns them, the oracle's intermediates)"""
    o, entry = K.oracles_and_batch(index, case.proof, case.pubs, world.pp[0], world.pp[1], world.g, world.h)
    state, mode, count = o["sponge_after"].raw()
    le = O.int_to_le
    ref = {"sponge": np.concatenate([O.ints_to_le(state).reshape(-1), np.array([mode, count], np.uint32).view(np.uint8)]),
           "evalpoints": O.ints_to_le(entry["evalpoints"]).reshape(-1), "polyscale": le(o["v"]), "evalscale": le(o["u"]), "ft_eval0": le(o["ft_eval0"]),
           "cip": le(o["combined_inner_product"]), "comms": np.concatenate([O.point_to_bytes(c) for c in o["comms"]])}
    return ref, o


def make_table(world, name, index, k, npub, n_prev, cases):
    from kimchi_helpers import kimchi_arrays
    refs = [reference(world, index, c) for c in cases]
    want = {f: np.stack([r[f] for r, _ in refs]) for f in FIELDS}
    arrays, _ = kimchi_arrays([c.proof for c in cases], [c.pubs for c in cases])
    arrays = {key: a for key, a in arrays.items() if a is not None}
    for a in list(want.values()) + list(arrays.values()):
        a.setflags(write=False)
    assert want["comms"].shape == (len(cases), (n_prev + 45) * 64)
    return SimpleNamespace(name=name, index=index, k=k, npub=npub, n_prev=n_prev, cases=cases, oracles=[o for _, o in refs], want=want, arrays=arrays)


def _build(world, name):
    kind, _, arg = name.partition("/")
    if kind == "npub":
        npub = int(arg); k = domain_of(npub)
        rng = random.Random(1000 + npub)
        return make_table(world, name, world.index(k), k, npub, BASE_NPREV, [random_case(rng, world, k, npub, BASE_NPREV) for _ in range(BATCH)])
    if kind == "nprev":
        n_prev = int(arg)
        rng = random.Random(2000 + n_prev)
        return make_table(world, name, world.index(BASE_K), BASE_K, BASE_NPUB, n_prev, [random_case(rng, world, BASE_K, BASE_NPUB, n_prev) for _ in range(BATCH)])
    if kind in ("alpha", "zk"):
        field = "perm_alpha_offset" if kind == "alpha" else "zk_rows"
        base = world.table("nprev/%d" % BASE_NPREV)
        if int(arg) == getattr(base.index, field):
            return base
        return make_table(world, name, world.index(BASE_K, **{field: int(arg)}), BASE_K, BASE_NPUB, BASE_NPREV, base.cases)
    assert name == "corners"
    return make_table(world, name, world.index(BASE_K), BASE_K, BASE_NPUB, BASE_NPREV, corner_cases(world))


# ------------------------------------------------------------------------------------------------ value corners
def _set_eval(case, col, row, v):
    e = list(case.proof["evals"][col]); e[row] = v
    case.proof["evals"][col] = tuple(e)


def _set_chal(case, acc, pos, v):
    ch, cm = case.proof["prev"][acc]
    ch = list(ch); ch[pos] = v
    case.proof["prev"][acc] = (ch, cm)


def corner_cases(world):
    """PERIOD proofs.  One corner each: 0, 1, r - 1 going round the 43 evaluation columns and both rows; in ft_eval1; in each public input; in the first and last
    challenge of each accumulator; infinity as z_comm, w_comm[0], w_comm[14], t_comm[0], t_comm[6], all of t_comm, an accumulator's commitment; all-zero public
    inputs.  Then twelve proofs that combine corners, then plain ones up to PERIOD"""
    rng = random.Random(4100)
    cases = []

    def fresh():
        cases.append(random_case(rng, world, BASE_K, BASE_NPUB, BASE_NPREV))
        return cases[-1]
    for col in range(N_COLS):
        _set_eval(fresh(), col, col & 1, CORNERS[col % 3])               # col mod 6 goes through all six (row, corner) pairs
    for v in CORNERS:
        fresh().proof["ft_eval1"] = v
    for slot in range(BASE_NPUB):
        for v in CORNERS:
            fresh().pubs[slot] = v
    for acc in range(BASE_NPREV):
        for pos in (0, BASE_K - 1):
            for v in CORNERS:
                _set_chal(fresh(), acc, pos, v)
    fresh().proof["z_comm"] = None
    for i in (0, K.COLUMNS - 1):
        fresh().proof["w_comm"][i] = None
    for i in (0, K.PERMUTS - 1):
        fresh().proof["t_comm"][i] = None
    fresh().proof["t_comm"] = [None] * K.PERMUTS
    c = fresh(); c.proof["prev"][1] = (c.proof["prev"][1][0], None)
    fresh().pubs[:] = [0] * BASE_NPUB
    assert len(cases) == 81
    for j in range(12):
        c = fresh()
        for i in range(3):
            _set_eval(c, (7 * j + 13 * i) % N_COLS, (i + j) & 1, CORNERS[(i + j) % 3])
        c.proof["ft_eval1"] = CORNERS[j % 3]
        c.pubs[j % BASE_NPUB] = CORNERS[(j + 1) % 3]
        _set_chal(c, j & 1, (0, BASE_K - 1)[(j >> 1) & 1], CORNERS[(j + 2) % 3])
        if j % 4 == 0: c.proof["z_comm"] = None
        elif j % 4 == 1: c.proof["w_comm"][0] = c.proof["w_comm"][14] = None
        elif j % 4 == 2: c.proof["t_comm"] = [None] * K.PERMUTS
        else:
            c.proof["prev"][0] = (c.proof["prev"][0][0], None); c.proof["t_comm"][0] = None
    while len(cases) < PERIOD:
        fresh()
    return cases


def census(cases):
    """the (slot, corner) pairs the proofs really hold, found by looking at them"""
    seen = set()
    for c in cases:
        p = c.proof
        for col, pair in enumerate(p["evals"]):
            for row, e in enumerate(pair):
                if e in CORNERS: seen.add(("eval", col, row, e))
        if p["ft_eval1"] in CORNERS: seen.add(("ft_eval1", p["ft_eval1"]))
        for i, x in enumerate(c.pubs):
            if x in CORNERS: seen.add(("pub", i, x))
        if c.pubs and not any(c.pubs): seen.add(("pubs_all_zero",))
        for acc, (ch, cm) in enumerate(p["prev"]):
            for pos in (0, len(ch) - 1):
                if ch[pos] in CORNERS: seen.add(("chal", acc, pos, ch[pos]))
            if cm is None: seen.add(("inf", "prev_comm"))
        if p["z_comm"] is None: seen.add(("inf", "z_comm"))
        for key in ("w_comm", "t_comm"):
            for i, pt in enumerate(p[key]):
                if pt is None: seen.add(("inf", key, i))
            if all(pt is None for pt in p[key]): seen.add(("inf", key, "all"))
    return seen


def required_corners():
    """the issue's list for the corner table, as census() names them; the evaluation columns are asked for separately (every column some corner)"""
    need = {("ft_eval1", v) for v in CORNERS} | {("pub", i, v) for i in range(BASE_NPUB) for v in CORNERS}
    need |= {("chal", acc, pos, v) for acc in range(BASE_NPREV) for pos in (0, BASE_K - 1) for v in CORNERS}
    need |= {("inf", "z_comm"), ("inf", "w_comm", 0), ("inf", "w_comm", 14), ("inf", "t_comm", 0), ("inf", "t_comm", 6), ("inf", "t_comm", "all"), ("inf", "prev_comm"),
             ("pubs_all_zero",)}
    return need


# ------------------------------------------------------------------------------------------------ tiling
def tile(table, n):
    """n proofs going round the table's distinct ones -> (arrays for MinaContext.make_kimchi_proofs, the index of the distinct proof at each position)"""
    d = len(table.cases)
    order = np.arange(n) % d
    return {key: a.reshape(d, -1)[order].reshape(-1) for key, a in table.arrays.items()}, order


# ------------------------------------------------------------------------------------------------ malformed inputs
def malformed(world, slot, kind, victim):
    """the proofs of nprev/2 with ONE bad value in proof `victim` -> arrays.  A scalar slot gets the modulus (kind "modulus"); a point slot a point off the curve
    ("off_curve") or the alias x + p of its x coordinate ("x_alias")"""
    from kimchi_helpers import kimchi_arrays
    base = world.table("nprev/%d" % BASE_NPREV)
    cases = list(base.cases)
    c = cases[victim] = copy.deepcopy(cases[victim])
    p = c.proof

    def bad_point(pt):
        x, y = pt
        if kind == "x_alias":
            assert x + P_MOD < 1 << 256
            return (x + P_MOD, y)
        assert kind == "off_curve" and not R.is_on_curve((x, (y + 1) % P_MOD), P_MOD)
        return (x, (y + 1) % P_MOD)
    if slot in MALFORMED_SCALARS:
        assert kind == "modulus"
        if slot == "eval_c0_r0": _set_eval(c, 0, 0, R_MOD)
        elif slot == "eval_c42_r1": _set_eval(c, N_COLS - 1, 1, R_MOD)
        elif slot == "ft_eval1": p["ft_eval1"] = R_MOD
        elif slot == "pub_first": c.pubs[0] = R_MOD
        elif slot == "pub_last": c.pubs[-1] = R_MOD
        elif slot == "chal_first": _set_chal(c, 0, 0, R_MOD)
        else: _set_chal(c, BASE_NPREV - 1, BASE_K - 1, R_MOD)
    elif slot == "prev_comm": p["prev"][1] = (p["prev"][1][0], bad_point(p["prev"][1][1]))
    elif slot == "z_comm": p["z_comm"] = bad_point(p["z_comm"])
    else:
        key, i = {"w_comm_0": ("w_comm", 0), "w_comm_14": ("w_comm", 14), "t_comm_0": ("t_comm", 0), "t_comm_6": ("t_comm", 6)}[slot]
        p[key][i] = bad_point(p[key][i])
    arrays, _ = kimchi_arrays([x.proof for x in cases], [x.pubs for x in cases])
    changed = [key for key in arrays if not np.array_equal(arrays[key], base.arrays[key])]
    assert len(changed) == 1, (slot, kind, changed)              # one section differs from the clean batch, and (below) only inside the victim's part of it
    a, b = arrays[changed[0]].reshape(BATCH, -1), base.arrays[changed[0]].reshape(BATCH, -1)
    assert [bool((a[i] != b[i]).any()) for i in range(BATCH)] == [i == victim for i in range(BATCH)]
    return arrays


def malformed_variants():
    return [(slot, "modulus") for slot in MALFORMED_SCALARS] + [(slot, kind) for slot in MALFORMED_POINTS for kind in POINT_KINDS]
