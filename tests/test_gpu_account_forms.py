"""The Poseidon stages of Proof-of-Account in every lane form, against the CPU: acct_hash_kernel and acct_fold_kernel (csrc/account_pack.cuh) through
mina_account_job_dev, salted_hash_kernel (csrc/api_account.hip) and merkle_fold_coop_kernel through the host path -- at more than 8192 pairs in one job, where the
default tuning takes the wave-packed triples (21 sponges per wave, lane 63 shadowing sponge 20), and at small sizes under forced forms.

The references rest on the CPU alone.  A distinct set D of 41 pairs -- the 24 account shapes of account_pack_helpers.accounts, depths 0, 1, 2, 3, 35, 64 going
round, the three failure kinds of with_failures -- gets its account hashes from the oracle (oracle/mina_account_ref.py), its roots and ledger hashes from
tests/merkle_model.py over those hashes, and its `passed` / `ran` masks by construction; the first test holds the host path on D to all three.  Every job is D in
some order, tiled: 41 is coprime to 3, 7, 8, 16, 21 and 64, so every pair of D meets every lane position.  Every pair's masks, hash and root are compared (hash and
root where FORMAT passed).  The lane form follows from ctx.h hash_lanes / merkle_lanes: each test asserts the tuning read back and the context's single lane."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import account_pack_helpers as H  # noqa: E402
import merkle_model as M  # noqa: E402
from test_account_job_gpu import OK, job_dev, with_failures  # noqa: E402

pytestmark = pytest.mark.gpu
DEPTHS = (0, 1, 2, 3, 35, 64)
N_D = 41
FORCED = {16: dict(coop16_max=1 << 30), 8: dict(coop16_max=0), 3: dict(coop16_max=0, coop8_max=0)}
SMALL = (1, 5, 22, 43, 65)


@pytest.fixture(scope="module")
def actx():
    """a context of this module's own, one pipeline lane"""
    import mina_bridge_amd as m
    c = m.MinaContext(0)
    c.set_pipeline(1)
    for field in (0, 1): c.poseidon_set_params(field, m.poseidon_params.default_params_bytes(field))
    yield c
    c.close()


@pytest.fixture(scope="module")
def D(oracle):
    """the distinct set and its CPU references: computed once, never written to"""
    import mina_bridge_amd as m
    from ipa_helpers import poseidon_pp
    from oracle import mina_account_ref as A
    pp, params = poseidon_pp(0), m.poseidon_params.default_params_bytes(0)
    hash_of = {}
    def oracle_hash(a):
        k = A.write_account(a, False)
        if k not in hash_of: hash_of[k] = A.account_hash(a, pp)
        return hash_of[k]
    def model_root(a, path):
        return M.roots(0, params, [oracle_hash(a)], [[s for _, s in path]], [[d for d, _ in path]], [len(path)])[0]
    cases = H.well_formed_pairs_at([DEPTHS[(i + i // 6) % 6] for i in range(26)], model_root)
    w = len(cases)
    pairs = with_failures(cases)[:N_D]
    assert len(pairs) == N_D and all(N_D % k for k in (3, 7, 8, 16, 21, 64))
    src, kind = list(range(w)), ["ok"] * w                   # the well-formed pair a failure was made from, and how (with_failures: three for every fifth)
    for i in range(0, w, 5):
        src += [i] * 3; kind += ["cut", "abi", "merkle"]
    src, kind = src[:N_D], kind[:N_D]
    assert {"ok", "cut", "abi", "merkle"} == set(kind)
    fmt = np.array([k != "cut" for k in kind])
    hashes = np.stack([M.le(oracle_hash(cases[s][3])) for s in src])
    roots = np.stack([M.le(model_root(cases[s][3], cases[s][4])) for s in src])
    passed = np.array([{"ok": OK, "cut": 0, "abi": OK & ~H.CHECK_ACCOUNT_ABI, "merkle": OK & ~H.CHECK_MERKLE}[k] for k in kind], np.uint32)
    ran = np.array([H.CHECK_FORMAT if k == "cut" else OK for k in kind], np.uint32)
    depths = np.array([len(cases[s][4]) for s in src])
    zk = np.array([cases[s][3]["zkapp"] is not None for s in src])
    assert set(depths[fmt].tolist()) == set(DEPTHS) and zk.any() and not zk.all()
    return SimpleNamespace(pairs=pairs, cases=cases, src=src, kind=kind, fmt=fmt, hashes=hashes, roots=roots, passed=passed, ran=ran, depths=depths, zk=zk,
                           accounts=[A.write_account(cases[s][3], False) for s in src])


class forced:
    """the tuning for the block with the preconditions of ctx.h hash_lanes / merkle_lanes asserted: coop16_max and coop8_max read back, ONE pipeline lane (lane 1 is
    outside the context's pipeline).  hash(pairs, sponges) / fold(paths) -> the lane form the rule then gives"""
    def __init__(self, c, **fields):
        import mina_bridge_amd as m
        self.c, self.fields, self.tune = c, fields, m.lib.tuning(**fields)
    def __enter__(self):
        import mina_bridge_amd as m
        self.tune.__enter__()
        try:
            with pytest.raises(m.lib.MinaError, match="outside the pipeline"): self.c.pin_lane(1)
            t, d = m.lib.verify_tuning_get(), m.lib.verify_tuning_default()
            assert (d.coop16_max, d.coop8_max, d.coop8_per_call) == (64, 8192, 0) and t.coop8_per_call == 0
            assert t.coop16_max == self.fields.get("coop16_max", 64) and t.coop8_max == self.fields.get("coop8_max", 8192)
            self.t = t
        except BaseException:
            self.tune.__exit__(None, None, None)
            raise
        return self
    def __exit__(self, *exc):
        return self.tune.__exit__(*exc)
    def hash(self, pairs, sponges): return 16 if pairs <= self.t.coop16_max else (8 if sponges <= self.t.coop8_max else 3)
    def fold(self, paths): return 16 if paths <= self.t.coop16_max else (8 if paths <= 8192 else 3)
    def job_forms(self, n):
        """mina_account_job_dev of n pairs: (URI + key stage, zkApp stage, account stage, fold)"""
        return (self.hash(n, 2 * n), self.hash(n, n), self.hash(n, n), self.fold(n))


def check_job(c, D, order):
    """one job over pairs `order` of D: every pair's masks, and where FORMAT passed its account hash and root, against D's references"""
    idx = np.asarray(order)
    passed, ran, hashes, roots = job_dev(c, [D.pairs[k] for k in order])
    bad = np.nonzero((passed != D.passed[idx]) | (ran != D.ran[idx]))[0]
    assert bad.size == 0, ("masks", bad.size, [(int(i), D.kind[idx[i]], hex(int(passed[i])), hex(int(ran[i]))) for i in bad[:5]])
    f = D.fmt[idx]
    for what, got, want in (("account hashes", hashes, D.hashes), ("roots", roots, D.roots)):
        bad = np.nonzero((got != want[idx]).any(axis=1) & f)[0]
        assert bad.size == 0, (what, bad.size, [(int(i), int(D.depths[idx[i]]), bool(D.zk[idx[i]])) for i in bad[:8]])


def tiled(n, members=None):
    members = list(range(N_D)) if members is None else list(members)
    return [members[i % len(members)] for i in range(n)]


def test_host_path_on_the_distinct_set_rests_on_the_cpu(actx, D):
    """the oracle's account hashes, the model's roots and the masks by construction: mina_account_hash_batch, mina_merkle_roots and mina_verify_account_ctx agree on D"""
    import mina_bridge_amd as m
    with forced(actx):
        ok = np.nonzero(D.fmt)[0]
        assert (actx.account_hash_batch([D.accounts[i] for i in ok], m.lib.ENC_BINCODE) == D.hashes[ok]).all()
        for depth in DEPTHS[1:]:
            grp = [i for i in ok if D.depths[i] == depth]
            paths = [D.cases[D.src[i]][4] for i in grp]
            L, S, Dr = M.pack([int.from_bytes(D.hashes[i].tobytes(), "little") for i in grp], [[s for _, s in p] for p in paths], [[d for d, _ in p] for p in paths], depth)
            assert (actx.merkle_roots(0, L, S, Dr, depth) == D.roots[grp]).all(), depth
        zero = [i for i in ok if D.depths[i] == 0]
        assert zero and (D.roots[zero] == D.hashes[zero]).all()
        hp, hr = actx.verify_account_checks([p for p, _ in D.pairs], [q for _, q in D.pairs])
        assert (hp == D.passed).all() and (hr == D.ran).all(), [(k, hex(int(a)), hex(int(b))) for k, a, b in zip(D.kind, hp, hr)]


@pytest.mark.parametrize("n", [8193, 8212])
def test_job_above_8192_pairs_runs_the_triples(actx, D, n):
    """8193 = 390 x 21 + 3 and 8212 = 391 x 21 + 1 pairs in one job under the default tuning: all three hash stages and the fold in the wave-packed form, every wave
    of the fold with mixed depths, 0 and 64 among them"""
    with forced(actx) as f:
        assert f.job_forms(n) == (3, 3, 3, 3)
        check_job(actx, D, tiled(n))


def test_depths_sorted_so_that_the_last_waves_are_all_depth_0(actx, D):
    n = 8212
    order = sorted(tiled(n), key=lambda k: -int(D.depths[k]))
    assert all(D.depths[k] == 0 for k in order[-21 * 40:]) and D.depths[order[0]] == 64
    with forced(actx) as f:
        assert f.job_forms(n) == (3, 3, 3, 3)
        check_job(actx, D, order)


def test_one_deep_path_in_a_wave_of_shallow_ones(actx, D):
    """a depth-64 path at wave position 20 (lanes 60 to 63) among paths of depth 0 and 1, then the same at wave position 0: every other lane group keeps its node for
    63 or 64 levels of the wave's loop"""
    n = 8212
    deep = [k for k in range(N_D) if D.fmt[k] and D.depths[k] == 64]
    shallow = [k for k in range(N_D) if D.depths[k] <= 1]
    assert deep and {int(D.depths[k]) for k in shallow} == {0, 1}
    order = []
    for i in range(n):
        wave, pos = divmod(i, 21)
        order.append(deep[wave % len(deep)] if pos == (20 if wave < 195 else 0) else shallow[i % len(shallow)])
    assert D.depths[order[20]] == 64 and D.depths[order[21 * 195]] == 64 and sum(D.depths[k] == 64 for k in order) == 392
    with forced(actx) as f:
        assert f.job_forms(n) == (3, 3, 3, 3)
        check_job(actx, D, order)


@pytest.mark.parametrize("zkapp", [False, True])
def test_no_pair_or_every_pair_carries_a_zkapp(actx, D, zkapp):
    """the compacted count in device memory is 0 or n: every wave of the zkApp stages leaves early, or none does"""
    n = 8193
    members = [k for k in range(N_D) if bool(D.zk[k]) == zkapp]
    while any(len(members) % k == 0 for k in (3, 7, 8)): members.pop()
    assert len(members) >= 10 and {D.kind[k] for k in members} >= {"ok", "cut"}
    with forced(actx) as f:
        assert f.job_forms(n) == (3, 3, 3, 3)
        check_job(actx, D, tiled(n, members))


@pytest.mark.parametrize("n", SMALL)
@pytest.mark.parametrize("form", [16, 8, 3])
def test_small_jobs_under_forced_forms(actx, D, form, n):
    """16 and 8: both stages in that form.  3: the hashes in triples, the fold in the 8-lane form (no knob forces a small fold into triples)."""
    with forced(actx, **FORCED[form]) as f:
        assert f.job_forms(n) == {16: (16, 16, 16, 16), 8: (8, 8, 8, 8), 3: (3, 3, 3, 8)}[form]
        check_job(actx, D, tiled(n))


@pytest.mark.parametrize("n", SMALL)
@pytest.mark.parametrize("form", [16, 8, 3])
def test_host_path_under_forced_forms(actx, D, form, n):
    """salted_hash_kernel in 16 lanes, 8 lanes and triples at sizes the default tuning gives another form: mina_account_hash_batch equals the oracle, the masks
    of mina_verify_account_ctx do not move"""
    import mina_bridge_amd as m
    order = tiled(n)
    ok = [k for k in order if D.fmt[k]]
    with forced(actx, **FORCED[form]) as f:
        assert ok and f.hash(2 * len(ok), 2 * len(ok)) == f.hash(len(ok), len(ok)) == form
        assert (actx.account_hash_batch([D.accounts[k] for k in ok], m.lib.ENC_BINCODE) == D.hashes[ok]).all()
        hp, hr = actx.verify_account_checks([D.pairs[k][0] for k in order], [D.pairs[k][1] for k in order])
        assert (hp == D.passed[order]).all() and (hr == D.ran[order]).all()
