"""CPU tier of the segmented matrix-core b_poly fold (mina_bridge_amd/csrc/bpoly_mfma_seg.cuh): the two context calls are declared, exported and bound in every
layer and refuse a null context without a GPU; the two new kernels are in the gfx950 code object with nothing in scratch, the raised wave priority at their top and,
in the GEMM, only the int8 MFMA of the single fold, sixteen of them in the K loop."""
import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import code_object as CO  # noqa: E402

SYMBOLS = ("mina_ctx_set_seg_fold_mfma_min", "mina_ctx_seg_fold_stats")
GEMM = "bpoly_field_gemm_seg_kernel"
KERNELS = (GEMM, "bpoly_colsum_reduce_seg_kernel<0>", "bpoly_colsum_reduce_seg_kernel<1>")
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
    for meth in ("set_seg_fold_mfma_min", "seg_fold_stats"):
        assert callable(getattr(m.MinaContext, meth)), meth
    from mina_bridge_amd import build as B
    assert "bpoly_mfma_seg.cuh" in B.HEADERS
    # the header states the rule, the default, the accumulator bound and the colsum budget
    at = hdr.index("int mina_ctx_set_seg_fold_mfma_min")
    doc = hdr[at - 2500:at]
    for word in ("min_len <= length < 2^17", "default is 256", "256 MiB", "not carried over"):
        assert word in doc, word


def test_null_context_is_refused_without_a_gpu():
    import mina_bridge_amd as m
    lib = m.load_library()
    n = ctypes.c_uint64(0)
    assert lib.mina_ctx_set_seg_fold_mfma_min(None, ctypes.c_uint32(256)) == MINA_ERR_ARG and lib.mina_last_error()
    assert lib.mina_ctx_seg_fold_stats(None, ctypes.byref(n), ctypes.byref(n), ctypes.byref(n)) == MINA_ERR_ARG


needs_llvm = pytest.mark.skipif(not os.path.exists(os.path.join(CO.LLVM_BIN, "llvm-objdump")), reason="LLVM binutils of the ROCm toolchain not present")


@pytest.fixture(scope="module")
def co():
    c = CO.CodeObjects()
    yield c
    c.close()


@needs_llvm
@pytest.mark.parametrize("kernel", KERNELS)
def test_new_kernels_use_no_scratch_and_raise_their_priority(co, kernel):
    ks = co.kernels()
    assert kernel in ks, sorted(k for k in ks if "bpoly" in k)
    meta = ks[kernel]
    assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0 and meta.get("sgpr_spill_count", 0) == 0 and not meta.get("uses_dynamic_stack", False), meta
    ins = co.instructions(kernel)
    assert not any(mn.startswith("scratch_") for _, mn, _ in ins)
    prios = [op.strip() for _, mn, op in ins if mn == "s_setprio"]
    assert prios and set(prios) <= {"2", "0x2"}, prios
    assert "s_setprio" in [mn for _, mn, _ in ins][:40], "the priority is raised at the top of the kernel"


@needs_llvm
def test_segmented_gemm_runs_on_the_matrix_cores(co):
    ins = co.instructions(GEMM)
    mfma = [mn for _, mn, _ in ins if mn.startswith("v_mfma")]
    assert mfma and all(mn == "v_mfma_i32_32x32x32_i8" for mn in mfma), sorted(set(mfma))
    hot = max((CO.summarize(co.histogram(GEMM, sp)) for sp in co.loops(GEMM)), key=lambda s: s["mfma"])
    assert hot["mfma"] >= 16 and hot["scratch"] == 0
    assert co.kernels()[GEMM]["group_segment_fixed_size"] == co.kernels()["bpoly_field_gemm_kernel"]["group_segment_fixed_size"], "the same LDS staging as the single fold"


@needs_llvm
def test_the_single_fold_and_the_valu_segment_kernels_are_still_there(co):
    ks = co.kernels()
    for k in ("bpoly_field_gemm_kernel", "bpoly_colsum_reduce_kernel<0>", "bpoly_colsum_reduce_kernel<1>", "bpoly_fold_seg_kernel<0>", "bpoly_fold_seg_kernel<1>",
              "bpoly_finish_seg_kernel<0>", "bpoly_finish_seg_kernel<1>"):
        assert k in ks, k
