"""The rows tests/test_gpu_fe32.py runs the compiled 8 x 32 routines on (tests/fe32_model.py) are LEGAL and reach the corners of the arithmetic -- shown here without a
GPU -- and the PORTABLE forms of the same headers (tests/fuzz/fe32_twin.cpp, built for the host, once more under AddressSanitizer + UBSan) give the model's words on
every one of them.

  * every row satisfies its routine's contract (`in_contract`), and every row family the builders are specified by is present: removing one fails here;
  * every event of the chains (`chain_required`) and of the generated products (`required_events`: lo == 0 under a non-zero column, mid == 0xffffffff, a carry into hi
    inside every asm chunk, hi set when a later chunk begins, hi at the all-ones rows, the pre-reduction values up to the peak) is reached by a row or stands in the FIXED table
    fe32_model.UNREACHABLE with its argument -- and no row reaches an event that table calls unreachable;
  * the model agrees with what does not share its code: the textbook congruence, ark's inverse and square root and the oracle's point addition."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import fe32_model as M

ROOT = M.ROOT
CASES = [(F, op) for F in (0, 1) for op in M.OPS]


@pytest.fixture(scope="module")
def pts(oracle):
    return {F: M.srs_points(oracle, F) for F in (0, 1)}


@pytest.fixture(scope="module")
def expected(pts):
    """(F, op) -> (rows, [([four results], flag)]): the model's answer for every row, computed once"""
    out = {}
    for F, op in CASES:
        rows = M.rows_of(F, op, pts[F])
        out[F, op] = (rows, [M.expect(F, op, r.ops) for r in rows])
    return out


@pytest.mark.parametrize("F,op", CASES)
def test_every_row_is_inside_its_contract_and_every_family_is_there(pts, F, op):
    rows = M.rows_of(F, op, pts[F])
    assert 0 < len(rows) <= M.MAX_ROWS
    for r in rows:
        assert len(r.ops) <= M.SLOTS and M.in_contract(F, op, r.ops), (op, r)
    have = {r.family for r in rows}
    assert have == set(M.FAMILIES[op]), (op, "missing", set(M.FAMILIES[op]) - have, "unlisted", have - set(M.FAMILIES[op]))


@pytest.mark.parametrize("op", M.CHAINS)
@pytest.mark.parametrize("F", (0, 1))
def test_the_chains_rows_reach_every_named_value_and_run_through_the_immediate_zero_limbs_both_ways(F, op):
    seen = set()
    for r in M.chain_rows(F, op):
        seen |= M.chain_events(M.P[F], op, list(r.ops) + [0])
    missing = [e for e in M.chain_required(op) if e not in seen]
    assert not missing, (op, F, missing)


@pytest.mark.parametrize("routine", sorted(M.GENERATED))
@pytest.mark.parametrize("F", (0, 1))
def test_every_column_event_of_a_generated_product_is_reached_or_is_in_the_fixed_unreachable_table(F, routine):
    p, seen, peak = M.P[F], set(), 0
    for r in M.product_rows(F, routine):
        tr = M.product_trace(p, M.op_pairs(F, routine, r.ops))
        seen |= M.events_of(routine, F, tr)
        peak = max(peak, tr["prered"])
    required = M.required_events(routine)
    assert len(required) == len(set(required))
    missing = [e for e in required if e not in seen and (routine, e) not in M.UNREACHABLE]
    assert not missing, (routine, F, missing)
    contradicted = [e for e in required if e in seen and (routine, e) in M.UNREACHABLE]
    assert not contradicted, (routine, F, contradicted)
    assert all(e in required for rt, e in M.UNREACHABLE if rt == routine)
    # the largest pre-reduction value of the rows: a dot product reaches 2p - 1, the largest there is; a single product the exact optimum of the family
    # a = 2^256 - c (fe32_model.mul_family_peak, where the argument stands) -- above 2^255, within t + 2^101 of 2p
    assert peak == (M.mul_family_peak(F)[0] if routine == "MUL" else 2 * p - 1)
    assert 2 * p - 1 - peak < M.tee(p) + (1 << 101) and peak > 1 << 255


def _is_prime(n):
    """Miller-Rabin on the first 24 primes as bases: more than enough witnesses for the sizes here (deterministic below 3.3 10^24, 2^-48 beyond)"""
    bases = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67, 71, 73, 79, 83, 89)
    if n in bases: return True
    if n < 2 or any(n % b == 0 for b in bases): return False
    d, r = n - 1, 0
    while d % 2 == 0: d //= 2; r += 1
    for b in bases:
        x = pow(b, d, n)
        if x in (1, n - 1): continue
        for _ in range(r - 1):
            x = x * x % n
            if x == n - 1: break
        else:
            return False
    return True


def test_the_single_products_peak_row_is_the_optimum_its_argument_derives():
    """the factorisation of t the divisor enumeration rests on is a factorisation; the peak row is legal, has the quotient 2^256 - j the argument says, and no
    neighbour in (c, e) of the same family lies above it"""
    for F in (0, 1):
        p, t = M.P[F], M.tee(M.P[F])
        n = 1
        for q, e in M.T_FACTORS[F].items():
            assert _is_prime(q)
            n *= q ** e
        assert n == t
        v, a, b = M.mul_family_peak(F)
        tr = M.product_trace(p, [(a, b)])
        assert a * b < p * M.R and tr["prered"] == v and 1 <= M.R - tr["m"] < 1 << 80
        c, e = M.R - a, p - b
        for dc in range(-3, 4):
            for de in range(-3, 4):
                a2, b2 = M.R - (c + dc), p - (e + de)
                if a2 * b2 < p * M.R and a2 <= M.M256:
                    assert M.product_trace(p, [(a2, b2)])["prered"] <= v, (dc, de)
        for s in range(1, 200):                                   # and the family's small members by brute force: d = s - 1 + e for every e | 4 s t above t
            for c2 in range(1, 4 * s):
                if 4 * s * t % c2 == 0:
                    assert 2 * p - 1 - (s - 1 + 4 * s * t // c2) <= v
                    assert M.product_trace(p, [(M.R - c2, p - 4 * s * t // c2)])["prered"] == 2 * p - 1 - (s - 1 + 4 * s * t // c2)


def test_the_squares_rows_reach_the_pre_reduction_values_a_square_can():
    for F in (0, 1):
        p = M.P[F]
        seen = {M.product_trace(p, [(r.ops[0], r.ops[0])])["prered"] for r in M.product_rows(F, "SQR")}
        assert {p - 1, p, p + 1, p + (1 << 128)} <= seen          # -1 and 2^128 are squares mod p (p = 1 mod 4); p itself is a = p


def test_the_multi_chunk_columns_are_the_ones_the_generator_splits():
    """what `a carry inside every chunk` quantifies over: DOT2 and DOT3 have columns of more than MAX_TERMS_PER_ASM terms, MUL has none"""
    chunks = {rt: [-(-len(M.G.column_terms(k, n)) // M.G.MAX_TERMS_PER_ASM) for k in range(15)] for rt, n in M.GENERATED.items()}
    assert max(chunks["MUL"]) == 1 and max(chunks["DOT2"]) == 2 and max(chunks["DOT3"]) == 3
    src = M.G.emit(3)
    assert src.count('"+&v"(hi)') == sum(c - 1 for c in chunks["DOT3"])          # a later chunk READS hi: the statement the rows of `hi_set_at_chunk` exist for


def test_the_square_roots_rows_make_the_loop_take_every_first_order_and_every_gap():
    for F in (0, 1):
        K, first, gaps = M.field(F), set(), set()
        for r in M.sqrt_rows(F):
            x, ok, passes = K.sqrt(r.ops[0])
            if r.family.startswith("order 2^"):
                j = int(r.family[8:])
                assert ok and K.mm(x, x) == r.ops[0] and (passes[0][0] if passes else 0) == j, r
                first.add(j)
            if r.family == "non-residue":
                assert not ok
            gaps |= {g for _, g in passes}
        assert first == set(range(32)) and gaps == set(range(31)), (sorted(first), sorted(gaps))       # b == 1 at once (order 2^0: no pass at all) ... order 2: 30 squarings of z in one pass
    assert M.x_zero_point(0) is None and M.x_zero_point(1) is None                                    # 5 is a non-residue in both fields: a point with x = 0 would have order 3, and both groups have prime order


@pytest.mark.parametrize("F,op", [c for c in CASES if c[1] in M.PRODUCTS + M.LAW_OPS + ("INV", "SQRT")])
def test_the_model_agrees_with_the_textbook_congruence_and_the_oracle(oracle, expected, F, op):
    rows, want = expected[F, op]
    M.check_against_references(oracle, F, op, rows, want)


def test_the_op_codes_of_the_header_are_mirrored_in_python_and_in_the_kernel_table():
    import mina_bridge_amd.lib as lib
    hdr = open(os.path.join(ROOT, "include", "mina_verify.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define\s+MINA_FE32_(\w+)\s+(\d+)\b", hdr)}
    consts = {"IN_OPERANDS": lib.FE32_IN_OPERANDS, "OUT_RESULTS": lib.FE32_OUT_RESULTS, "FLAG_TRUE": lib.FE32_FLAG_TRUE, "FLAG_LANES_AGREE": lib.FE32_FLAG_LANES_AGREE}
    assert defs == dict(lib.FE32_OPS, **consts)
    assert len(set(lib.FE32_OPS.values())) == len(lib.FE32_OPS) and set(lib.FE32_OPS) == set(M.OPS)
    assert (lib.FE32_IN_OPERANDS, lib.FE32_OUT_RESULTS, lib.FE32_IN_WORDS, lib.FE32_OUT_WORDS) == (M.SLOTS, M.RESULTS, M.IN_WORDS, M.OUT_WORDS)
    assert (lib.FE32_FLAG_TRUE, lib.FE32_FLAG_LANES_AGREE) == (M.FLAG_TRUE, M.FLAG_LANES_AGREE)
    src = open(os.path.join(ROOT, "mina_bridge_amd", "csrc", "api_selftest.hip")).read()
    twin = open(os.path.join(ROOT, "tests", "fuzz", "fe32_twin.cpp")).read()
    assert all(f"X(MINA_FE32_{name})" in src and f"case MINA_FE32_{name}:" in twin for name in lib.FE32_OPS)
    assert "mina_selftest_fe32" in lib.EXPORTS


# ------------------------------------------------------------------------------------------------ the portable forms, compiled for the host
def _cxx():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import code_object as CO
    cxx = shutil.which("g++") or shutil.which("clang++") or os.path.join(CO.LLVM_BIN, "clang++")
    if not (cxx and os.path.exists(cxx)):
        pytest.skip("no C++ compiler")
    return cxx


def _build_twin(d, extra):
    fz = os.path.join(ROOT, "tests", "fuzz")
    exe = str(d / "fe32_twin")
    done = subprocess.run([_cxx(), "-std=c++17", "-O1", "-w", *extra, "-I", os.path.join(fz, "hip_stub"), os.path.join(fz, "fe32_twin.cpp"), "-o", exe], capture_output=True, text=True)
    return exe, done


def _run_twin(exe, d, expected):
    import mina_bridge_amd.lib as lib
    fin, fout = str(d / "in.bin"), str(d / "out.bin")
    with open(fin, "wb") as fh:
        for (F, op), (rows, _) in expected.items():
            fh.write(struct.pack("<3I", F, lib.FE32_OPS[op], len(rows)))
            fh.write(np.array([M.words(c) for c in M.field(F).consts], np.uint32).tobytes())
            fh.write(np.array(M.pack(rows), np.uint32).tobytes())
    done = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert done.returncode == 0, (done.returncode, done.stderr[-4000:])
    out = np.fromfile(fout, np.uint32)
    assert out.size == sum(len(rows) for rows, _ in expected.values()) * M.OUT_WORDS
    at, bad = 0, []
    for (F, op), (rows, want) in expected.items():
        got = M.unpack(out[at:at + len(rows) * M.OUT_WORDS].reshape(len(rows), M.OUT_WORDS).tolist())
        at += len(rows) * M.OUT_WORDS
        bad += [(F, op, i, rows[i].family) for i in range(len(rows)) if got[i] != (want[i][0], want[i][1])]      # every row: none skipped
    assert not bad, (len(bad), bad[:10])


def test_the_portable_forms_equal_the_model_word_for_word_on_every_row(tmp_path, expected):
    exe, done = _build_twin(tmp_path, [])
    assert done.returncode == 0, done.stderr[-4000:]
    _run_twin(exe, tmp_path, expected)


def test_the_portable_forms_run_clean_under_the_address_and_undefined_behaviour_sanitizers(tmp_path, expected):
    """a stand-alone program with its own main: nothing is loaded into the interpreter"""
    exe, done = _build_twin(tmp_path, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if done.returncode != 0:
        assert re.search(r"asan|ubsan|sanitize", done.stderr, re.I), done.stderr[-4000:]
        pytest.skip("the compiler has no AddressSanitizer / UBSan runtime")
    _run_twin(exe, tmp_path, expected)
