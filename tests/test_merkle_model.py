"""tests/merkle_model.py (the level-by-level CPU model of the Merkle fold, over the C oracle's batched permutation) against the big-int oracle/pasta_ref.py merkle_root,
for depths 0, 1, 2, 35 and 64, a depth per path, both fields and the edge values the GPU tests mix in; and the model's sensitivity to the mistakes those GPU tests
(tests/test_gpu_merkle_forms.py, tests/test_gpu_account_forms.py) must catch on their own input sets: a flipped direction, the salts of two neighbouring heights
swapped, the siblings shifted by one path, a depth off by one.  No GPU."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import merkle_model as M  # noqa: E402

DEPTHS = (0, 1, 2, 35, 64)
SAMPLE = (0, 1, 2, 3, 5, 9, 12, 15, 17, 40)          # all-left, all-right, alternating; edge leaves; edge siblings; edge values all the way; a random path


def default_params(field):
    import mina_bridge_amd.poseidon_params as PP
    return PP.default_params_bytes(field)


def big_int_root(pp, leaf, sib, dirs, depth):
    from oracle import pasta_ref as R
    return R.merkle_root(leaf, [(dirs[h], sib[h]) for h in range(depth)], pp)


def test_params_bytes_round_trip():
    import mina_bridge_amd.poseidon_params as PP
    for field in (0, 1):
        pp = M.pp_of(field, default_params(field))
        mds, rc = PP.default_params_ints(field)
        assert pp.mds == [list(r) for r in mds] and pp.rc == [list(r) for r in rc] and pp.m == M.MODS[field]


@pytest.mark.parametrize("field", [0, 1])
def test_model_equals_big_int_merkle_root(oracle, field):
    params = default_params(field)
    pp = M.pp_of(field, params)
    p = M.MODS[field]
    seen = set()
    for depth in DEPTHS:                                            # one depth for all, as mina_merkle_roots takes them
        leaves, sib, dirs = M.input_set(field, depth)
        pick = [i for i in SAMPLE]
        got = M.roots(field, params, [leaves[i] for i in pick], [sib[i] for i in pick], [dirs[i] for i in pick], [depth] * len(pick))
        for k, i in enumerate(pick):
            assert got[k] == big_int_root(pp, leaves[i], sib[i], dirs[i], depth), (depth, i)
            seen |= {leaves[i], *sib[i]}
        if depth == 0: assert got == [leaves[i] for i in pick]
    assert set(M.edge_values(field)) <= seen and max(seen) >= 1 << 254 and all(0 <= x < p for x in seen)
    # a depth per path, as mina_account_job_dev takes them: the first 30 paths of the depth-64 set, depths going round
    leaves, sib, dirs = M.input_set(field, 64)
    depths = [DEPTHS[i % 5] for i in range(30)]
    got = M.roots(field, params, leaves[:30], sib[:30], dirs[:30], depths)
    for i in range(30):
        assert got[i] == big_int_root(pp, leaves[i], sib[i], dirs[i], depths[i]), i


def test_input_sets_tell_neighbours_apart():
    """what a wrong mapping from sponge to path would mix up differs between neighbours: leaf, siblings and (from depth 35 on) directions"""
    for field in (0, 1):
        for depth in (1, 2, 35, 64):
            leaves, sib, dirs = M.input_set(field, depth)
            assert len(leaves) == M.PERIOD and all(M.PERIOD % k for k in (3, 7, 8, 16, 21, 64))
            for i in range(M.PERIOD):
                j = (i + 1) % M.PERIOD
                assert leaves[i] != leaves[j] and all(sib[i][h] != sib[j][h] for h in range(depth)), (depth, i)
                if depth >= 35: assert dirs[i] != dirs[j]
            assert dirs[0] == [0] * depth and dirs[1] == [1] * depth and dirs[2] == [h & 1 for h in range(depth)]
            assert any(x >= 1 << 254 for x in leaves)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("depth", [1, 2, 35])
def test_model_is_sensitive_to_the_mistakes_the_gpu_tests_must_catch(oracle, field, depth):
    params = default_params(field)
    leaves, sib, dirs = M.input_set(field, depth)
    n = M.PERIOD
    depths = [depth] * n
    want = M.roots(field, params, leaves, sib, dirs, depths)
    differs = lambda got: [a != b for a, b in zip(got, want)]
    # a flipped direction, at height i mod depth of path i
    flipped = [[d ^ 1 if h == i % depth else d for h, d in enumerate(row)] for i, row in enumerate(dirs)]
    assert all(differs(M.roots(field, params, leaves, sib, flipped, depths)))
    # the siblings shifted by one path
    assert all(differs(M.roots(field, params, leaves, sib[1:] + sib[:1], dirs, depths)))
    # a depth off by one
    assert all(differs(M.roots(field, params, leaves, sib, dirs, [depth - 1] * n)))
    # the salts of heights h and h + 1 swapped
    if depth >= 2:
        table = M.salts(field, params, depth)
        for h in {0, depth - 2}:
            swap = {h: h + 1, h + 1: h}
            assert all(differs(M.roots(field, params, leaves, sib, dirs, depths, salt_of=lambda k: table[swap.get(k, k)])))


@pytest.mark.parametrize("field", [0, 1])
def test_mixed_depths_are_sensitive_too(oracle, field):
    """the account job's shape: a depth per path and a 64-sibling stride -- one more or one fewer level than a path has, or a neighbour's depth, changes the root"""
    params = default_params(field)
    leaves, sib, dirs = M.input_set(field, 64, count=42)
    depths = [(0, 1, 2, 3, 35, 64)[i % 6] for i in range(42)]
    want = M.roots(field, params, leaves, sib, dirs, depths)
    more = M.roots(field, params, leaves, sib, dirs, [min(d + 1, 64) for d in depths])
    fewer = M.roots(field, params, leaves, sib, dirs, [max(d - 1, 0) for d in depths])
    shifted = M.roots(field, params, leaves, sib, dirs, depths[1:] + depths[:1])
    for i, d in enumerate(depths):
        assert (more[i] != want[i]) == (d < 64) and (fewer[i] != want[i]) == (d > 0) and shifted[i] != want[i], i
