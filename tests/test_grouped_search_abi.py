"""CPU tier of the segmented building blocks, the grouped culprit search and the per-proof verdicts of a device-resident job: the new symbols are declared,
exported and bound in every layer and refuse a null context without a GPU; the new kernels are in the gfx950 code object with nothing in scratch and the raised wave
priority at their top, like their neighbours; and the stubbed-device builds of tests/fuzz -- which compile api_verify.hip against stand-in contexts that link no
kernel -- still build from an unmodified tests/fuzz."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import code_object as CO  # noqa: E402

# the five entry points; the boundary flag MINA_VERIFY_GROUPED_SEARCH = 64u is checked beside them
SYMBOLS = ("mina_msm_segments_dev", "mina_b_poly_fold_segments_dev", "mina_ctx_set_search_groups", "mina_ctx_search_stats", "mina_state_job_each_dev")
KERNELS = ("msm_part_seg_kernel<false>", "msm_part_seg_kernel<true>", "msm_digits_seg_kernel", "bpoly_fold_seg_kernel<0>", "bpoly_fold_seg_kernel<1>",
           "bpoly_finish_seg_kernel<0>", "bpoly_finish_seg_kernel<1>", "xyzz_compare_parts_kernel<0>", "xyzz_compare_parts_kernel<1>",
           "points_to_mont_checked_each_kernel<1>")
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
    assert re.search(r"#define\s+MINA_VERIFY_GROUPED_SEARCH\s+64u", hdr)
    assert m.lib.VERIFY_GROUPED_SEARCH == 64 and "MINA_VERIFY_GROUPED_SEARCH" in go
    assert m.lib.VERIFY_GROUPED_SEARCH & (m.lib.VERIFY_ALLOW_MISSING_KIMCHI | m.lib.VERIFY_ALLOW_UNBOUND_STATEMENT | m.lib.VERIFY_ALLOW_SURROGATE | m.lib.VERIFY_DEDUP_STATES
                                          | m.lib.VERIFY_PACK_ON_DEVICE | m.lib.VERIFY_ACCOUNT_ON_DEVICE) == 0
    for meth in ("msm_segments_dev", "b_poly_fold_segments_dev", "set_search_groups", "search_stats", "state_job_each_dev"):
        assert callable(getattr(m.MinaContext, meth)), meth
    from mina_bridge_amd import build as B
    assert {"msm_seg.cuh", "bpoly_seg.cuh", "segments.cuh"} <= set(B.HEADERS)
    # the header states the pipeline's limits and that the per-proof call waits for its lane
    at = hdr.index("int mina_msm_segments_dev")
    assert "2^26" in hdr[at - 3000:at + 3000] and "2^28" in hdr[at - 3000:at + 3000]
    at = hdr.index("int mina_state_job_each_dev")
    assert "SYNCHRONISES ITS LANE" in hdr[at - 1500:at]


def test_null_context_is_refused_without_a_gpu():
    import mina_bridge_amd as m
    lib = m.load_library()
    buf = (ctypes.c_uint8 * 256)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    z = ctypes.c_size_t
    n = ctypes.c_uint64(0)
    assert lib.mina_msm_segments_dev(None, 1, z(4), z(1), p, p, p, p, p) == MINA_ERR_ARG and lib.mina_last_error()
    assert lib.mina_b_poly_fold_segments_dev(None, 0, ctypes.c_uint32(3), z(4), z(1), p, p, p, p, p) == MINA_ERR_ARG
    assert lib.mina_ctx_set_search_groups(None, ctypes.c_uint32(8)) == MINA_ERR_ARG
    assert lib.mina_ctx_search_stats(None, ctypes.byref(n), ctypes.byref(n), ctypes.byref(n)) == MINA_ERR_ARG
    assert lib.mina_state_job_each_dev(None, p, p, None) == MINA_ERR_ARG
    live = ctypes.c_uint32(0)
    assert lib.mina_ctx_lane_streams(None, ctypes.byref(live), ctypes.byref(n)) == MINA_ERR_ARG and "mina_ctx_lane_streams" in m.EXPORTS


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
    assert kernel in ks, sorted(k for k in ks if "seg" in k or "parts" in k)
    meta = ks[kernel]
    assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0 and not meta.get("uses_dynamic_stack", False), meta
    ins = co.instructions(kernel)
    assert not any(mn.startswith("scratch_") for _, mn, _ in ins)
    prios = [op.strip() for _, mn, op in ins if mn == "s_setprio"]
    assert prios and set(prios) <= {"2", "0x2"}, prios
    assert "s_setprio" in [mn for _, mn, _ in ins][:40], "the priority is raised at the top of the kernel"


@needs_llvm
def test_existing_sort_kernels_are_still_there(co):
    """the segmented digit passes are kernels of their own: the unsegmented ones stay as separate instantiations"""
    ks = co.kernels()
    for k in ("msm_part_kernel<false>", "msm_part_kernel<true>", "msm_digits_kernel", "bpoly_fold_kernel<0>", "bpoly_finish_kernel<0>"):
        assert k in ks, k


@pytest.mark.skipif(not (shutil.which("make") and (shutil.which("g++") or shutil.which("clang++"))), reason="no make / C++ compiler")
def test_stubbed_device_builds_still_compile(tmp_path):
    """`make -C tests/fuzz tsan trace_boundary` from a copy of the tree's csrc, include and tests/fuzz: api_verify.hip and ctx.h compile against the HIP stub"""
    for d in ("mina_bridge_amd/csrc", "include", "tests/fuzz"):
        shutil.copytree(os.path.join(ROOT, d), tmp_path / d, ignore=shutil.ignore_patterns("*.o", "build", "out", "corpus*"))
    r = subprocess.run(["make", "-C", str(tmp_path / "tests" / "fuzz"), "tsan", "trace_boundary"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
