"""The single-lane state-hash form (api_state.hip pstate_hash1_kernel, sponge.cuh poseidon_rounds_one), CPU tier.

1. The diagonal-normalised rows are an exact change of variables: with u_j = d_j s_j and d'_i = d_i^7 / M_ii every MDS row of rounds 0 .. 53 has a 1 on
   the diagonal, round 54 takes d' = 1, and the permutation maps the same unscaled state to the same unscaled state.  `rows1` is the Python big-int model of
   api_sponge.hip `poseidon_rows1` (same order of the two off-diagonal entries: next element, then previous); it must refuse a zero on the diagonal.
2. The code-object contract of the kernel: multiply-accumulates per sponge-round, no cross-lane moves, no scratch, no raised wave priority, waves per SIMD.
"""
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import mina_bridge_amd.poseidon_params as PP  # noqa: E402

P_FP = 0x40000000000000000000000000000000224698FC094CF91B992D30ED00000001
P_FQ = 0x40000000000000000000000000000000224698FC0994A8DD8C46EB2100000001


def permute_plain(s, mds, rc, p):
    for r in range(55):
        t = [pow(x, 7, p) for x in s]
        s = [(sum(mds[i][j] * t[j] for j in range(3)) + rc[r][i]) % p for i in range(3)]
    return s


def rows1(mds, rc, p):
    """(rows[r][i] = (a_next, a_prev, rc') for r < 54, last 3x3 matrix, last round constants); ValueError on a zero diagonal entry"""
    if any(mds[i][i] % p == 0 for i in range(3)):
        raise ValueError("zero on the MDS diagonal: no normalised rows")
    d = [1, 1, 1]
    rows, last, last_rc = [], None, None
    for r in range(55):
        d7inv = [pow(pow(x, 7, p), p - 2, p) for x in d]
        dn = [pow(d[i], 7, p) * pow(mds[i][i], p - 2, p) % p if r < 54 else 1 for i in range(3)]
        a = [[dn[i] * mds[i][j] * d7inv[j] % p for j in range(3)] for i in range(3)]
        rcs = [dn[i] * rc[r][i] % p for i in range(3)]
        if r < 54:
            assert all(a[i][i] == 1 for i in range(3))
            rows.append([(a[i][(i + 1) % 3], a[i][(i + 2) % 3], rcs[i]) for i in range(3)])
        else:
            last, last_rc = a, rcs
        d = dn
    return rows, last, last_rc


def permute_rows1(s, tables, p):
    rows, last, last_rc = tables
    for r in range(54):
        t = [pow(x, 7, p) for x in s]
        s = [(t[i] + rows[r][i][0] * t[(i + 1) % 3] + rows[r][i][1] * t[(i + 2) % 3] + rows[r][i][2]) % p for i in range(3)]
    t = [pow(x, 7, p) for x in s]
    return [(sum(last[i][j] * t[j] for j in range(3)) + last_rc[i]) % p for i in range(3)]


@pytest.mark.parametrize("field", [0, 1])
def test_normalised_rows_give_the_unscaled_permutation_surrogate_set(field):
    p = P_FP if field == 0 else P_FQ
    mds, rc = PP.default_params_ints(field)
    tables = rows1(mds, rc, p)
    rng = random.Random(7 + field)
    states = [[0, 0, 0], [1, 0, 0], [p - 1, p - 1, p - 1]] + [[rng.randrange(p) for _ in range(3)] for _ in range(6)]
    for s in states:
        assert permute_rows1(s, tables, p) == permute_plain(s, mds, rc, p)


def test_normalised_rows_give_the_unscaled_permutation_random_set():
    rng = random.Random(2026)
    for p in (P_FP, P_FQ):
        mds = [[rng.randrange(1, p) for _ in range(3)] for _ in range(3)]
        rc = [[rng.randrange(p) for _ in range(3)] for _ in range(55)]
        tables = rows1(mds, rc, p)
        for _ in range(4):
            s = [rng.randrange(p) for _ in range(3)]
            assert permute_rows1(s, tables, p) == permute_plain(s, mds, rc, p)


def test_zero_on_the_diagonal_is_refused():
    mds, rc = PP.default_params_ints(0)
    for i in range(3):
        bad = [row[:] for row in mds]
        bad[i][i] = 0
        with pytest.raises(ValueError):
            rows1(bad, rc, P_FP)


def test_library_refuses_zero_diagonal_in_the_derivation():
    """api_sponge.hip: the derivation returns false on a zero diagonal entry and the context keeps the 3-lane path (pparams_rows1 stays false; ctx.h hash_one_lane).
    That the single-lane form runs for the installed sets is the GPU tier's check (tests/test_gpu_state_hash_one_lane.py)."""
    src = open(os.path.join(ROOT, "mina_bridge_amd", "csrc", "api_sponge.hip")).read()
    assert "if (fe_is_zero(pp.mds[i][i])) return false;" in src
    assert "c->pparams_rows1[field] = both.q1.ok != 0;" in src
    ctx_h = open(os.path.join(ROOT, "mina_bridge_amd", "csrc", "ctx.h")).read()
    assert "return c->pparams_rows1[FIELD_FP] && jobs >= 2 && " in ctx_h


# ---- the code-object contract (needs the ROCm LLVM binutils and the built library, as tests/test_code_object.py)
import code_object as CO  # noqa: E402

_have_tools = os.path.exists(os.path.join(CO.LLVM_BIN, "llvm-objdump"))
KERNEL = "pstate_hash1_kernel<0>"


@pytest.fixture(scope="module")
def co():
    if not _have_tools:
        pytest.skip("LLVM binutils of the ROCm toolchain not present")
    c = CO.CodeObjects()
    yield c
    c.close()


def _round_loops(co, kernel, min_mac):
    loops = co.loops(kernel)
    out = []
    for (s, e) in loops:
        if any(s <= s2 and e2 <= e and (s2, e2) != (s, e) for (s2, e2) in loops):
            continue
        summ = CO.summarize(co.histogram(kernel, (s, e)))
        if summ["mac64"] >= min_mac:
            out.append(((s, e), summ))
    return out


def test_one_lane_registers_and_occupancy(co):
    """91 VGPRs at amdgpu_waves_per_eu(5, 5): five waves per SIMD, nothing in scratch (SGPR spills go to VGPR lanes, outside the round loops)"""
    m = co.kernels()[KERNEL]
    regs = -(-m["vgpr_count"] // 8) * 8
    assert min(8, 512 // regs) >= 5, m["vgpr_count"]
    assert m["vgpr_spill_count"] == 0
    assert m.get("private_segment_fixed_size", 0) == 0


def test_one_lane_round_loops(co):
    """per sponge-round (one lane, three elements): 3 x 156 S-box + 3 x 234 normalised-row multiply-accumulates = 2106 (the three first products of the
    columns start their accumulators), no ds_bpermute, no scratch, the row constants from scalar loads only"""
    loops = _round_loops(co, KERNEL, 1500)
    assert len(loops) == 3, [(s, x["mac64"]) for s, x in loops]
    for span, s in loops:
        assert 2100 <= s["mac64"] <= 2106, (span, s)
        assert s["valu"] <= 2560, (span, s)
        assert s["ds_bpermute"] == 0 and s["scratch"] == 0 and s["global_load"] == 0, (span, s)
        hist = co.histogram(KERNEL, span)
        assert not any("readlane" in mn or "writelane" in mn or "readfirstlane" in mn for mn in hist), (span, {k: v for k, v in hist.items() if "lane" in k})
        assert sum(v for mn, v in hist.items() if mn.startswith("s_load")) >= 1, (span, "the round's row constants come from scalar loads")
    whole = CO.summarize(co.histogram(KERNEL))
    assert whole["scratch"] == 0 and whole["ds_bpermute"] == 0, whole


def test_one_lane_wave_priority_not_raised(co):
    """like the other state-hash forms (tests/test_code_object.py test_wave_priorities): the chip-filling hashes leave the arbiter to the chain kernels"""
    assert not [mn for _, mn, _ in co.instructions(KERNEL) if mn == "s_setprio"]
