"""A CPU model of the Merkle fold of Proof-of-Account (merkle_fold_coop_kernel in csrc/sponge.cuh, acct_fold_kernel in csrc/account_pack.cuh) with a depth per path,
level by level: every path still alive at height h goes through ONE call of the C oracle's batched permutation.  The state of a level is salt[h] with the node added
to element 0 or 1 by the direction and the sibling to the other; element 0 of the permuted state is the next node.  The salts are oracle/pasta_ref.py merkle_salt for
the installed constants.  tests/test_merkle_model.py holds it to the big-int pasta_ref.merkle_root; the GPU tests of the three lane forms take their references from
it (tests/test_gpu_merkle_forms.py, tests/test_gpu_account_forms.py), PERIOD distinct paths at a time."""
import random

import numpy as np

P = 0x40000000000000000000000000000000224698FC094CF91B992D30ED00000001
Q = 0x40000000000000000000000000000000224698FC0994A8DD8C46EB2100000001
MODS = {0: P, 1: Q}
PERIOD = 251                   # distinct paths per input set: coprime to 3, 21 and 64, so every distinct path meets every lane position of a tiled batch
MAX_DEPTH = 64


def le(x):
    return np.frombuffer(int(x).to_bytes(32, "little"), np.uint8)


def _raw(params_bytes):
    return bytes(params_bytes) if isinstance(params_bytes, (bytes, bytearray)) else np.ascontiguousarray(params_bytes, np.uint8).tobytes()


def pp_of(field, params_bytes):
    """parameter bytes (9 MDS entries by rows, then 55 x 3 round constants, 32-byte little-endian each) -> pasta_ref.PoseidonParams"""
    from oracle import pasta_ref as R
    b = _raw(params_bytes)
    assert len(b) == (9 + 165) * 32
    x = [int.from_bytes(b[32 * i:32 * i + 32], "little") for i in range(9 + 165)]
    return R.PoseidonParams(MODS[field], [x[3 * i:3 * i + 3] for i in range(3)], [x[9 + 3 * r:12 + 3 * r] for r in range(55)], "from bytes")


_SALTS = {}


def salts(field, params_bytes, depth):
    """[salt[0], .., salt[depth - 1]], three ints each (cached per table: a big-int permutation per height)"""
    from oracle import pasta_ref as R
    key = (field, _raw(params_bytes))
    have = _SALTS.setdefault(key, [])
    if len(have) < depth:
        pp = pp_of(field, key[1])
        have.extend(R.merkle_salt(h, pp) for h in range(len(have), depth))
    return have[:depth]


def roots(field, params_bytes, leaves, siblings, dirs, depths, salt_of=None):
    """leaves: n ints; siblings[i], dirs[i]: at least depths[i] ints each (what lies past a path's depth is not read) -> the n roots as ints.  Depth 0: the leaf.
    salt_of(h) -> three ints replaces the salt of height h (the sensitivity checks of tests/test_merkle_model.py swap two heights with it)."""
    from oracle import oracle as O
    m = MODS[field]
    n = len(leaves)
    assert len(siblings) == len(dirs) == len(depths) == n and all(0 <= d <= MAX_DEPTH and len(siblings[i]) >= d and len(dirs[i]) >= d for i, d in enumerate(depths))
    node = [int(x) for x in leaves]
    top = max(depths, default=0)
    table = salts(field, params_bytes, top)
    for h in range(top):
        alive = [i for i in range(n) if depths[i] > h]
        s = salt_of(h) if salt_of else table[h]
        flat = []
        for i in alive:
            sib, d = int(siblings[i][h]), int(dirs[i][h])
            assert d in (0, 1)
            l, r = (node[i], sib) if d == 0 else (sib, node[i])
            flat += [(s[0] + l) % m, (s[1] + r) % m, s[2]]
        out = O.poseidon_permute(field, params_bytes, O.ints_to_le(flat).reshape(len(alive), 96))
        for k, i in enumerate(alive):
            node[i] = int.from_bytes(out[k, :32].tobytes(), "little")
    return node


def edge_values(field):
    p = MODS[field]
    return [0, 1, p - 1, p - 2, 1 << 254, (p - 1) // 2]


def input_set(field, depth, seed=0, count=PERIOD):
    """-> (leaves, siblings, dirs): `count` paths of one depth.  Values are drawn below p with randrange(p) (reaching 2^254 and above), with 0, 1, p - 1, p - 2, 2^254
    and (p - 1) / 2 mixed in as leaf and as sibling; path 0 goes left all the way, path 1 right, path 2 alternates, the others are random.  Neighbouring paths differ in
    leaf and in path."""
    p = MODS[field]
    rng = random.Random(1000 * depth + 10 * seed + field)
    edges = edge_values(field)
    leaves = [rng.randrange(p) for _ in range(count)]
    sib = [[rng.randrange(p) for _ in range(depth)] for _ in range(count)]
    dirs = [[rng.randrange(2) for _ in range(depth)] for _ in range(count)]
    for k, v in enumerate(edges):
        if 3 + k < count: leaves[3 + k] = v                                       # an edge value as leaf, random siblings
        if depth and 9 + k < count: sib[9 + k][(k * 7) % depth] = v               # an edge value as sibling at some height
        if depth and 15 + k < count: leaves[15 + k] = edges[(k + 3) % 6]; sib[15 + k] = [edges[(k + h + 1) % 6] for h in range(depth)]      # edge values all the way
    for i, f in ((0, lambda h: 0), (1, lambda h: 1), (2, lambda h: h & 1)):
        if i < count: dirs[i] = [f(h) for h in range(depth)]
    return leaves, sib, dirs


def pack(leaves, siblings, dirs, depth, n=None):
    """paths of ONE depth tiled to n -> the byte arrays of mina_merkle_roots: leaves [n, 32], siblings [n * depth, 32], dirs [n * depth]"""
    k = len(leaves)
    n = k if n is None else n
    L = np.stack([le(x) for x in leaves])
    S = np.stack([le(x) for row in siblings for x in row[:depth]]).reshape(k, depth * 32) if depth else np.zeros((k, 0), np.uint8)
    D = np.array([row[:depth] for row in dirs], np.uint8).reshape(k, depth)
    idx = np.arange(n) % k
    return np.ascontiguousarray(L[idx]), np.ascontiguousarray(S[idx]).reshape(n * depth, 32), np.ascontiguousarray(D[idx]).reshape(n * depth)


def tile_roots(want, n):
    """the model's roots (ints) of the distinct paths -> [n, 32] bytes in tiled order"""
    W = np.stack([le(x) for x in want])
    return W[np.arange(n) % len(want)]
