"""The COMPILED 8 x 32 routines -- the inline-assembly carry chains and generated products of fp.cuh, fe_inv / fe_sqrt of groupmap.cuh, the group laws of ec.cuh, the
lane-cooperative forms included -- on the rows of tests/fe32_model.py, through mina_selftest_fe32: one routine per kernel, raw words in, raw words out.

The device's words must EQUAL the model's on every row of every op, for both fields -- integer equality, no tolerance.  tests/test_fe32_rows.py shows without a GPU that
the rows are legal and reach the corners: the borrow of the subtraction of p and the carry of its add-back running through the limbs that are the literal 0 in the
assembly (and not running through them), a column with lo == 0 under a non-zero upper part, mid == 0xffffffff, a carry into hi in every asm chunk, every first order
the Tonelli-Shanks loop can meet, equal and opposite points in different XYZZ representations.  A carry-less instruction in one of those chains, a fold that takes its
carry from the wrong place, a chunk that forgets hi, a wrong lane selection in the cooperative add: each changes a word on some row.  On top, what does not share the
model's code: the textbook congruence for the products, ark's inverse and root, the oracle's point addition.

What this does NOT cover: each routine is compiled into a kernel of its own; a register-allocation-dependent defect of an asm constraint inside a composite kernel
is still seen only by the parity tests."""
import numpy as np
import pytest

import fe32_model as M

pytestmark = pytest.mark.gpu

CASES = [(F, op) for F in (0, 1) for op in M.OPS]


@pytest.fixture(scope="module")
def pts(oracle):
    return {F: M.srs_points(oracle, F) for F in (0, 1)}


def run(ctx, F, op, rows):
    import mina_bridge_amd.lib as lib
    table = np.array(M.pack(rows), np.uint32)
    assert table.shape == (len(rows), lib.FE32_IN_WORDS)
    return M.unpack(ctx.selftest_fe32(F, lib.FE32_OPS[op], table).tolist())


@pytest.mark.parametrize("F,op", CASES)
def test_the_device_equals_the_model_word_for_word_on_every_row(ctx, oracle, pts, F, op):
    rows = M.rows_of(F, op, pts[F])
    got = run(ctx, F, op, rows)
    bad = []
    for i, r in enumerate(rows):                                  # every row: none skipped
        want = M.expect(F, op, r.ops)
        if got[i] != (want[0], want[1]):
            bad.append(i)
    assert not bad, (f"{op} F={F}: {len(bad)} of {len(rows)} rows differ from the model; first: row {bad[0]} ({rows[bad[0]].family}) operands "
                     f"{[hex(x) for x in rows[bad[0]].ops]}: device {[hex(x) for x in got[bad[0]][0]]} flag {got[bad[0]][1]}, model {[hex(x) for x in M.expect(F, op, rows[bad[0]].ops)[0]]}")
    M.check_against_references(oracle, F, op, rows, got)          # the congruence / ark / the oracle's point addition, on the DEVICE's words
    if op.endswith("_QUAD"):                                      # the cooperative form returns the single-lane words bit for bit, all four lanes agreeing
        single = run(ctx, F, op.replace("_QUAD", ""), rows)
        assert [g[0] for g in got] == [s[0] for s in single] and all(g[1] == M.FLAG_LANES_AGREE for g in got)


def test_rows_that_do_not_fill_a_block_and_more_than_one_block(ctx):
    """1, 63, 64, 65 and 257 rows (four lanes per row in the cooperative forms: 65 rows end inside a wave): every row answered, nothing beyond the last written"""
    import mina_bridge_amd.lib as lib
    rows = M.rows_of(0, "MUL")
    for op, rs in (("MUL", rows), ("XYZZ_ADD_QUAD", [M.Row("words", list(r.ops) * 4) for r in rows if all(x < M.P[0] for x in r.ops)])):
        for n in (1, 63, 64, 65, 257):
            table = np.array(M.pack(rs[:n]), np.uint32)
            out = ctx.selftest_fe32(0, lib.FE32_OPS[op], table)
            assert out.shape == (n, lib.FE32_OUT_WORDS)
            assert M.unpack(out.tolist()) == [tuple(M.expect(0, op, r.ops)) for r in rs[:n]], (op, n)
    assert ctx.selftest_fe32(0, lib.FE32_OPS["MUL"], np.zeros((0, lib.FE32_IN_WORDS), np.uint32)).shape == (0, lib.FE32_OUT_WORDS)
