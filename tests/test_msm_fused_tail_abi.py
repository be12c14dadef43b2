"""CPU tier of the fused MSM tail (mina_bridge_amd/csrc/msm.cuh msm_tail_kernel): the two context calls are declared, exported and bound in every layer and refuse a
null context without a GPU; the kernel is in the gfx950 code object for both fields with nothing in scratch, no spilled VGPR and the raised wave priority at its top."""
import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import code_object as CO  # noqa: E402

SYMBOLS = ("mina_ctx_set_msm_fused_tail", "mina_ctx_msm_tail_stats")
KERNELS = ("msm_tail_kernel<0>", "msm_tail_kernel<1>")
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
    assert re.search(r"int mina_ctx_set_msm_fused_tail\(mina_ctx \*ctx, int on\);", hdr)
    assert re.search(r"int mina_ctx_msm_tail_stats\(mina_ctx \*ctx, uint64_t \*fused_runs, uint64_t \*staged_runs\);", hdr)
    assert "pub fn mina_ctx_set_msm_fused_tail(ctx: *mut mina_ctx, on: c_int) -> c_int;" in rs
    assert "pub fn mina_ctx_msm_tail_stats(ctx: *mut mina_ctx, fused_runs: *mut u64, staged_runs: *mut u64) -> c_int;" in rs
    for meth in ("set_msm_fused_tail", "msm_tail_stats"):
        assert callable(getattr(m.MinaContext, meth)), meth
    for meth in ("SetMsmFusedTail", "MsmTailStats"):
        assert "func (c *Ctx) %s(" % meth in go, meth
    # the header states the default, what keeps the staged tail and that results are the same bytes
    at = hdr.index("int mina_ctx_set_msm_fused_tail")
    doc = hdr[at - 2000:at]
    for word in ("the default is 0", "keep the staged tail", "the same bytes", "No workgroup waits", "view context"):
        assert word in doc, word


def test_the_tuning_struct_and_the_boundary_flags_are_untouched():
    hdr = open(os.path.join(ROOT, "include", "mina_verify.h")).read()
    assert "fused_tail" not in hdr[hdr.index("typedef struct mina_verify_tuning"):hdr.index("} mina_verify_tuning;")]
    assert not re.search(r"#define MINA_VERIFY_\w*TAIL", hdr)


def test_null_arguments_are_refused_without_a_gpu():
    import mina_bridge_amd as m
    lib = m.load_library()
    n = ctypes.c_uint64(0)
    assert lib.mina_ctx_set_msm_fused_tail(None, ctypes.c_int(1)) == MINA_ERR_ARG and lib.mina_last_error()
    assert lib.mina_ctx_msm_tail_stats(None, ctypes.byref(n), ctypes.byref(n)) == MINA_ERR_ARG


needs_llvm = pytest.mark.skipif(not os.path.exists(os.path.join(CO.LLVM_BIN, "llvm-objdump")), reason="LLVM binutils of the ROCm toolchain not present")


@pytest.fixture(scope="module")
def co():
    c = CO.CodeObjects()
    yield c
    c.close()


@needs_llvm
@pytest.mark.parametrize("kernel", KERNELS)
def test_the_kernel_uses_no_scratch_and_raises_its_priority(co, kernel):
    ks = co.kernels()
    assert kernel in ks, sorted(k for k in ks if "msm_" in k)
    meta = ks[kernel]
    assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0 and not meta.get("uses_dynamic_stack", False), meta
    ins = co.instructions(kernel)
    assert not any(mn.startswith("scratch_") for _, mn, _ in ins)
    prios = [op.strip() for _, mn, op in ins if mn == "s_setprio"]
    assert prios and set(prios) <= {"2", "0x2"}, prios
    assert "s_setprio" in [mn for _, mn, _ in ins][:40], "the priority is raised at the top of the kernel"


@needs_llvm
def test_the_staged_tail_kernels_are_still_there(co):
    ks = co.kernels()
    for f in (0, 1):
        for k in ("msm_bucket_sum_kernel<%d>", "msm_bucket_sum_lane_kernel<%d>", "msm_bucket_sum_heavy_kernel<%d>", "msm_segsum_kernel<%d, true>", "msm_segsum_kernel<%d, false>",
                  "msm_wsum16_kernel<%d>", "msm_reduce2d_kernel<%d>", "msm_finish_kernel<%d>"):
            assert k % f in ks, k % f
