"""CPU tier of the fast inverse (mina_bridge_amd/csrc/fe_modinv.cuh; mina_field_inv_gcd, mina_ctx_set_fast_inverse, mina_ctx_inverse_stats): the three calls are
declared, exported and bound in every layer and refuse bad arguments without a GPU; the three new kernels are in the gfx950 code object for both fields with nothing
in scratch, no spilled VGPR and -- the two MSM kernels -- the raised wave priority at their top; the kernels they mirror are still there."""
import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import code_object as CO  # noqa: E402

SYMBOLS = ("mina_field_inv_gcd", "mina_ctx_set_fast_inverse", "mina_ctx_inverse_stats")
MSM_KERNELS = tuple("%s<%d>" % (k, f) for k in ("msm_finish_gcd_kernel", "msm_tail_gcd_kernel") for f in (0, 1))
KERNELS = ("field_inv_gcd_kernel<0>", "field_inv_gcd_kernel<1>") + MSM_KERNELS
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
    assert "int mina_field_inv_gcd(mina_ctx *ctx, int field, size_t n, const uint8_t *a, uint8_t *out);" in hdr
    assert "int mina_ctx_set_fast_inverse(mina_ctx *ctx, int on);" in hdr
    assert "int mina_ctx_inverse_stats(mina_ctx *ctx, uint64_t *gcd_finishes, uint64_t *fermat_finishes);" in hdr
    assert "pub fn mina_field_inv_gcd(ctx: *mut mina_ctx, field: c_int, n: usize, a: *const u8, out: *mut u8) -> c_int;" in rs
    assert "pub fn mina_ctx_set_fast_inverse(ctx: *mut mina_ctx, on: c_int) -> c_int;" in rs
    assert "pub fn mina_ctx_inverse_stats(ctx: *mut mina_ctx, gcd_finishes: *mut u64, fermat_finishes: *mut u64) -> c_int;" in rs
    for meth in ("field_inv_gcd", "set_fast_inverse", "inverse_stats"):
        assert callable(getattr(m.MinaContext, meth)), meth
    for meth in ("FieldInvGcd", "SetFastInverse", "InverseStats"):
        assert "func (c *Ctx) %s(" % meth in go, meth
    # the header states the default, that results are the same bytes, the fixed bound and what the mode leaves alone
    at = hdr.index("int mina_ctx_set_fast_inverse")
    doc = hdr[at - 2600:at]
    for word in ("the default is 0", "the same bytes", "at most 25 batches", "FIXED bound", "does not touch", "mina_field_inv", "view context"):
        assert word in doc, word
    from mina_bridge_amd import build as B
    assert "fe_modinv.cuh" in B.HEADERS


def test_the_tuning_struct_and_the_boundary_flags_are_untouched():
    hdr = open(os.path.join(ROOT, "include", "mina_verify.h")).read()
    tuning = hdr[hdr.index("typedef struct mina_verify_tuning"):hdr.index("} mina_verify_tuning;")]
    assert "inverse" not in tuning and "gcd" not in tuning
    assert not re.search(r"#define MINA_VERIFY_\w*(INVERSE|GCD)", hdr)
    src = open(os.path.join(ROOT, "mina_bridge_amd", "csrc", "groupmap.cuh")).read()
    fieldk = src[src.index("struct FieldK {"):src.index("};", src.index("struct FieldK {"))]
    members = re.findall(r"\b\w+(?=[,;])", re.sub(r"//.*", "", fieldk))
    assert len(members) == 16 and "r2" in members, members       # FieldK is a by-value argument of pinned kernels: it has not grown


def test_bad_arguments_are_refused_without_a_gpu():
    import mina_bridge_amd as m
    lib = m.load_library()
    n = ctypes.c_uint64(0)
    buf = (ctypes.c_uint8 * 32)()
    stand_in = ctypes.c_void_p(ctypes.addressof((ctypes.c_uint8 * 64)()))       # never read: every refusal below comes before the context is touched
    assert lib.mina_ctx_set_fast_inverse(None, ctypes.c_int(1)) == MINA_ERR_ARG and lib.mina_last_error()
    assert lib.mina_ctx_inverse_stats(None, ctypes.byref(n), ctypes.byref(n)) == MINA_ERR_ARG
    assert lib.mina_field_inv_gcd(None, 0, ctypes.c_size_t(1), buf, buf) == MINA_ERR_ARG
    assert lib.mina_field_inv_gcd(stand_in, 0, ctypes.c_size_t(1), None, buf) == MINA_ERR_ARG
    assert lib.mina_field_inv_gcd(stand_in, 0, ctypes.c_size_t(1), buf, None) == MINA_ERR_ARG
    assert lib.mina_field_inv_gcd(stand_in, 2, ctypes.c_size_t(1), buf, buf) == MINA_ERR_ARG
    assert lib.mina_ctx_inverse_stats(stand_in, None, ctypes.byref(n)) == MINA_ERR_ARG
    assert lib.mina_ctx_inverse_stats(stand_in, ctypes.byref(n), None) == MINA_ERR_ARG
    assert lib.mina_ctx_set_fast_inverse(stand_in, ctypes.c_int(2)) == MINA_ERR_ARG and b"0 (off) or 1 (on)" in lib.mina_last_error()
    assert lib.mina_ctx_set_fast_inverse(stand_in, ctypes.c_int(-1)) == MINA_ERR_ARG


needs_llvm = pytest.mark.skipif(not os.path.exists(os.path.join(CO.LLVM_BIN, "llvm-objdump")), reason="LLVM binutils of the ROCm toolchain not present")


@pytest.fixture(scope="module")
def co():
    c = CO.CodeObjects()
    yield c
    c.close()


@needs_llvm
@pytest.mark.parametrize("kernel", KERNELS)
def test_the_kernel_uses_no_scratch(co, kernel):
    ks = co.kernels()
    assert kernel in ks, sorted(k for k in ks if "gcd" in k)
    meta = ks[kernel]
    assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0 and not meta.get("uses_dynamic_stack", False), meta
    ins = co.instructions(kernel)
    assert not any(mn.startswith("scratch_") for _, mn, _ in ins)
    assert any(mn == "v_mad_i64_i32" for _, mn, _ in ins), "the limb products are signed 32 x 32 -> 64 multiply-adds"


@needs_llvm
@pytest.mark.parametrize("kernel", MSM_KERNELS)
def test_the_msm_kernels_raise_their_priority(co, kernel):
    ins = co.instructions(kernel)
    prios = [op.strip() for _, mn, op in ins if mn == "s_setprio"]
    assert prios and set(prios) <= {"2", "0x2"}, prios
    assert "s_setprio" in [mn for _, mn, _ in ins][:40], "the priority is raised at the top of the kernel"


@needs_llvm
def test_the_batch_loop_is_there_once(co):
    """25 batches are 25 trips of ONE loop body (two matrix updates over nine limbs: some 80 signed products, of which the compiler keeps a part as v_mad_i64_i32),
    not 25 copies of it"""
    for k in KERNELS:
        assert 1 <= sum(mn == "v_mad_i64_i32" for _, mn, _ in co.instructions(k)) <= 100, k


@needs_llvm
def test_the_kernels_they_mirror_are_still_there(co):
    ks = co.kernels()
    for f in (0, 1):
        for k in ("msm_finish_kernel<%d>", "msm_tail_kernel<%d>", "field_inv_kernel<%d>"):
            assert k % f in ks, k % f
            assert not any(mn == "v_mad_i64_i32" for _, mn, _ in co.instructions(k % f)), "no kernel holds both inversions"
