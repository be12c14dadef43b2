"""mina_merkle_roots and mina_merkle_verify_batch (merkle_fold_coop_kernel, csrc/sponge.cuh) in each of the three lane forms -- 16 lanes per path, 8 lanes per path
and wave-packed triples (21 paths per wave, lane 63 shadowing path 20) -- against tests/merkle_model.py, the level-by-level CPU model over the C oracle's
permutation.  Every root the GPU returns is compared: the reference is computed on PERIOD = 251 distinct paths per (field, depth) and tiled to n.

The form follows from ctx.h merkle_lanes: 16 lanes while paths x pipeline lanes <= coop16_max, 8 lanes up to 8192 paths, triples above.  Every test asserts the
preconditions of that rule -- the tuning read back and the context's single pipeline lane -- so that it cannot quietly run another form.  The sizes are the partial
waves and workgroups of each form: see SIZES."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import merkle_model as M  # noqa: E402

pytestmark = pytest.mark.gpu

FORCE16, FORCE8 = dict(coop16_max=1 << 30), dict(coop16_max=0)
# form -> (tuning, sizes).  16 lanes: 4 paths a wave, 16 a workgroup of 256 threads.  8 lanes: 8 a wave, 32 a workgroup.  Triples: 21 a wave, 84 a workgroup --
# 8193 = 390 x 21 + 3 (three live sponges in the last wave), 8210 (sponge 20 of the last wave and its shadow lane dead), 8211 (full waves), 8212 (one live sponge
# alone in a wave), 8232 = 98 x 84 (full workgroups), 8233 (a workgroup of one live sponge and three dead waves).  Default tuning: both sides of the 16 / 8 switch.
SIZES = {16: (FORCE16, (1, 3, 4, 5, 16, 17, 251, 8193)), 8: (FORCE8, (1, 7, 8, 9, 32, 33, 251, 8192)), 3: (FORCE8, (8193, 8210, 8211, 8212, 8232, 8233))}
DEEP_AT = {16: 251, 8: 251, 3: 8212}                 # depths 35 and 64
LEAF_AT = {16: 5, 8: 5, 3: 8193}                     # depth 0
CASES = [(form, n, depth) for form, (_, sizes) in SIZES.items() for n in sizes for depth in (1, 2)]
CASES += [(form, n, depth) for form, n in DEEP_AT.items() for depth in (35, 64)] + [(form, n, 0) for form, n in LEAF_AT.items()]
CASES += [("default", n, depth) for n in (64, 65) for depth in (1, 2)]


def install(c):
    import mina_bridge_amd as m
    for field in (0, 1): c.poseidon_set_params(field, m.poseidon_params.default_params_bytes(field))


@pytest.fixture(scope="module")
def mctx():
    """a context of this module's own, one pipeline lane"""
    import mina_bridge_amd as m
    c = m.MinaContext(0)
    c.set_pipeline(1)
    install(c)
    yield c
    c.close()


def lanes_of(c, n):
    """the lane form ctx.h merkle_lanes gives n paths on context c under the tuning in force; asserts that c has ONE pipeline lane (lane 1 is outside its pipeline)"""
    import mina_bridge_amd as m
    with pytest.raises(m.lib.MinaError, match="outside the pipeline"): c.pin_lane(1)
    t = m.lib.verify_tuning_get()
    return 16 if n <= t.coop16_max else (8 if n <= 8192 else 3)


class forced:
    """the tuning of a form for the block, with the preconditions asserted: coop16_max and coop8_max read back, and the form they give n paths"""
    def __init__(self, c, form, n):
        import mina_bridge_amd as m
        self.c, self.form, self.n = c, form, n
        self.tune = m.lib.tuning(**({} if form == "default" else SIZES[form][0]))
    def __enter__(self):
        import mina_bridge_amd as m
        self.tune.__enter__()
        try:
            t, d = m.lib.verify_tuning_get(), m.lib.verify_tuning_default()
            assert d.coop16_max == 64 and t.coop8_max == d.coop8_max == 8192
            assert t.coop16_max == {16: 1 << 30, 8: 0, 3: 0, "default": 64}[self.form]
            assert lanes_of(self.c, self.n) == (self.form if self.form != "default" else (16 if self.n <= 64 else 8)), (self.form, self.n)
        except BaseException:
            self.tune.__exit__(None, None, None)
            raise
        return self
    def __exit__(self, *exc):
        return self.tune.__exit__(*exc)


_REFS = {}


def reference(field, depth, params=None, name="compiled_in"):
    """(field, depth, table) -> (leaves, siblings, dirs of the PERIOD distinct paths, the model's roots as ints): computed once, never written to"""
    import mina_bridge_amd as m
    key = (field, depth, name)
    if key not in _REFS:
        params = m.poseidon_params.default_params_bytes(field) if params is None else params
        leaves, sib, dirs = M.input_set(field, depth)
        _REFS[key] = (leaves, sib, dirs, M.roots(field, params, leaves, sib, dirs, [depth] * len(leaves)))
    return _REFS[key]


def check_roots(c, field, n, depth, ref):
    leaves, sib, dirs, want = ref
    L, S, D = M.pack(leaves, sib, dirs, depth, n)
    got = c.merkle_roots(field, L, S, D, depth)
    bad = np.nonzero((got != M.tile_roots(want, n)).any(axis=1))[0]
    assert bad.size == 0, "%d of %d roots differ from the model, first at paths %s" % (bad.size, n, bad[:8].tolist())
    return got


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("form,n,depth", CASES)
def test_roots_equal_the_model_in_every_form(mctx, oracle, field, form, n, depth):
    ref = reference(field, depth)
    with forced(mctx, form, n):
        got = check_roots(mctx, field, n, depth, ref)
    if depth == 0: assert (got == M.pack(ref[0], ref[1], ref[2], 0, n)[0]).all()          # the root is the leaf


def flip_bit(x, b, p):
    """x with one bit changed, the first from bit b on (round 254) that leaves it below p"""
    for k in range(254):
        y = x ^ (1 << ((b + k) % 254))
        if y < p: return y
    raise AssertionError(x)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("form,n,depth", [(8, 251, 2), (8, 251, 35), (3, 8212, 2)])
def test_verify_batch_verdicts_equal_the_model(mctx, oracle, field, form, n, depth):
    """every fifth path tampered, in turn by a flipped direction at height i mod depth, the low bit of the last sibling, a leaf bit, and its neighbour's expected root:
    the verdict vector equals the model's, which holds both zeros and ones.  The model folds every tampered path itself (n / 5 of them: depth 35 only at n = 251)."""
    import mina_bridge_amd as m
    p = M.MODS[field]
    leaves, sib, dirs, want = reference(field, depth)
    k = len(leaves)
    L, S, D = M.pack(leaves, sib, dirs, depth, n)
    S = S.reshape(n, depth, 32).copy(); D = D.reshape(n, depth).copy()
    E = M.tile_roots(want, n).copy()
    bad, t_leaves, t_sib, t_dirs = list(range(0, n, 5)), [], [], []
    for i in bad:
        leaf, s, d = leaves[i % k], list(sib[i % k]), list(dirs[i % k])
        kind = (i // 5) % 4
        if kind == 0: d[i % depth] ^= 1
        if kind == 1: s[-1] = s[-1] ^ 1 if s[-1] ^ 1 < p else s[-1] - 1
        if kind == 2: leaf = flip_bit(leaf, i % 254, p)
        if kind == 3: E[i] = M.le(want[(i + 1) % n % k])
        L[i] = M.le(leaf); S[i] = np.stack([M.le(x) for x in s]); D[i] = d
        t_leaves.append(leaf); t_sib.append(s); t_dirs.append(d)
    model = M.roots(field, m.poseidon_params.default_params_bytes(field), t_leaves, t_sib, t_dirs, [depth] * len(bad))
    verdict = np.ones(n, np.uint8)
    for i, r in zip(bad, model): verdict[i] = 1 if (M.le(r) == E[i]).all() else 0
    assert verdict[bad].sum() == 0 and verdict.sum() == n - len(bad) and len(bad) >= 4          # each tampering changes the model's root: zeros and ones both occur
    with forced(mctx, form, n):
        got = mctx.merkle_verify_batch(field, L, S.reshape(n * depth, 32), D.reshape(-1), depth, E)
    wrong = np.nonzero(got != verdict)[0]
    assert wrong.size == 0, "verdicts differ from the model at paths %s" % wrong[:8].tolist()


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("form,n", [(3, 8212), (8, 251)])
def test_salt_table_grows_and_follows_the_poseidon_tables(oracle, field, form, n):
    """a fresh context runs depth 2, then 64, then 3: the salt table grows and is then used in part.  After mina_poseidon_set_params the roots follow the new table (the
    `random` one, then `zero_on_diagonal`, under which the triples run their plain rounds), and back on the first table the first roots come out again.  The model is
    given the same parameter bytes each time."""
    import mina_bridge_amd as m
    from test_gpu_tri_rows import param_sets
    sets = param_sets(field)
    c = m.MinaContext(0)
    try:
        c.set_pipeline(1)
        install(c)
        with forced(c, form, n):
            first = check_roots(c, field, n, 2, reference(field, 2))
            for depth in (64, 3):
                check_roots(c, field, n, depth, reference(field, depth))
            seen = [first]
            for name in ("random", "zero_on_diagonal", "compiled_in"):
                c.poseidon_set_params(field, sets[name])
                seen.append(check_roots(c, field, n, 2, reference(field, 2, sets[name], name)))
        assert (seen[3] == seen[0]).all() and all((seen[a] != seen[b]).any(axis=1).all() for a, b in ((0, 1), (0, 2), (1, 2)))
    finally:
        c.close()
