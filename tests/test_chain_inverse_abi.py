"""CPU tier of the chain inverse (mina_ctx_set_chain_inverse, mina_ctx_chain_inverse_stats): the two calls are declared, exported and bound in every layer, their
documentation says what the mode covers and what it leaves on the power, they refuse bad arguments without a GPU, and a view context takes the mode from its parent
where it takes the fast inverse."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mina_ctx_set_chain_inverse", "mina_ctx_chain_inverse_stats")
MINA_ERR_ARG = -1


def test_symbols_in_every_layer():
    import mina_bridge_amd as m
    hdr = open(os.path.join(ROOT, "include", "mina_verify.h")).read()
    rs = open(os.path.join(ROOT, "bindings", "rust", "src", "sys.rs")).read()
    go = open(os.path.join(ROOT, "bindings", "go", "minaverify.go")).read()
    lib = m.load_library()
    for s in SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % s, hdr), s
        assert s in m.EXPORTS and hasattr(lib, s), s
        assert "pub fn %s(" % s in rs, s
        assert "C.%s(" % s in go, s
    assert "int mina_ctx_set_chain_inverse(mina_ctx *ctx, int on);" in hdr
    assert "int mina_ctx_chain_inverse_stats(mina_ctx *ctx, uint64_t *gcd_launches, uint64_t *fermat_launches);" in hdr
    assert "pub fn mina_ctx_set_chain_inverse(ctx: *mut mina_ctx, on: c_int) -> c_int;" in rs
    assert "pub fn mina_ctx_chain_inverse_stats(ctx: *mut mina_ctx, gcd_launches: *mut u64, fermat_launches: *mut u64) -> c_int;" in rs
    for meth in ("set_chain_inverse", "chain_inverse_stats"):
        assert callable(getattr(m.MinaContext, meth)), meth
    for meth in ("SetChainInverse", "ChainInverseStats"):
        assert "func (c *Ctx) %s(" % meth in go, meth


def test_the_header_says_what_the_mode_covers_and_what_stays_on_the_power():
    hdr = open(os.path.join(ROOT, "include", "mina_verify.h")).read()
    at = hdr.index("int mina_ctx_set_chain_inverse")
    doc = hdr[hdr.rindex("/*", 0, at):at]
    for kernel in ("pickles_scalar_kernel", "kimchi_scalar_kernel", "kimchi_pub_kernel<8>, <10>", "kimchi_ftcomm_kernel", "pubcomm_finish16_kernel", "pubcomm_finish_kernel",
                   "lagrange_finish_kernel", "lagrange_digit_table_kernel", "points_sum_kernel"):
        assert kernel in doc, kernel
    for word in ("the default is 0", "the same bytes", "independent", "does not imply", "ipa_prepare_kernel", "group map", "square roots", "mina_field_inv", "HOST",
                 "view context", "queued after"):
        assert word in doc, word
    # the fast inverse keeps its documented meaning: the MSM finish alone
    fast = hdr[hdr.rindex("/*", 0, hdr.index("int mina_ctx_set_fast_inverse")):hdr.index("int mina_ctx_set_fast_inverse")]
    assert "The mode does not touch anything else" in fast and "chain" not in fast


def test_a_view_takes_the_mode_where_it_takes_the_fast_inverse():
    src = open(os.path.join(ROOT, "mina_bridge_amd", "csrc", "ctx.h")).read()
    body = src[src.index("static inline void mb_ctx_refresh_view"):]
    body = body[:body.index("}") + 1]
    assert "view->fast_inverse = parent->fast_inverse;" in body and "view->chain_inverse = parent->chain_inverse;" in body
    assert re.search(r"bool chain_inverse = false;", src)                                   # off by default


def test_bad_arguments_are_refused_without_a_gpu():
    import mina_bridge_amd as m
    lib = m.load_library()
    n = ctypes.c_uint64(0)
    stand_in = ctypes.c_void_p(ctypes.addressof((ctypes.c_uint8 * 64)()))       # never read: every refusal below comes before the context is touched
    assert lib.mina_ctx_set_chain_inverse(None, ctypes.c_int(1)) == MINA_ERR_ARG and lib.mina_last_error()
    assert lib.mina_ctx_chain_inverse_stats(None, ctypes.byref(n), ctypes.byref(n)) == MINA_ERR_ARG
    assert lib.mina_ctx_chain_inverse_stats(stand_in, None, ctypes.byref(n)) == MINA_ERR_ARG
    assert lib.mina_ctx_chain_inverse_stats(stand_in, ctypes.byref(n), None) == MINA_ERR_ARG
    assert lib.mina_ctx_set_chain_inverse(stand_in, ctypes.c_int(2)) == MINA_ERR_ARG and b"0 (off) or 1 (on)" in lib.mina_last_error()
    assert lib.mina_ctx_set_chain_inverse(stand_in, ctypes.c_int(-1)) == MINA_ERR_ARG
