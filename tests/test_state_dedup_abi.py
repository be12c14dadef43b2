"""CPU tier of the deduplicated protocol-state leg (mina_ctx_set_state_dedup): the new symbols are declared, exported and bound in every layer, refuse a
NULL context without a GPU, and the new kernels keep the register contract of their plain siblings (read from the gfx950 code objects, as
tests/test_code_object.py does for the rest of the hot path)."""
import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import code_object as CO  # noqa: E402

SYMBOLS = ("mina_protocol_state_dedup_dev", "mina_protocol_state_hash_batch_dedup", "mina_ctx_set_state_dedup", "mina_ctx_state_dedup_stats")
MINA_ERR_ARG = -1


def test_symbols_and_flag_in_every_layer():
    import mina_bridge_amd as m
    hdr = open(os.path.join(ROOT, "include", "mina_verify.h")).read()
    rs = open(os.path.join(ROOT, "bindings", "rust", "src", "sys.rs")).read()
    go = open(os.path.join(ROOT, "bindings", "go", "minaverify.go")).read()
    lib = m.load_library()
    for s in SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % s, hdr), s
        assert s in m.EXPORTS and hasattr(lib, s), s
        assert "pub fn %s(" % s in rs, s
    assert re.search(r"#define\s+MINA_VERIFY_DEDUP_STATES\s+8u", hdr)
    assert m.lib.VERIFY_DEDUP_STATES == 8 and m.lib.VERIFY_DEDUP_STATES & (m.lib.VERIFY_ALLOW_MISSING_KIMCHI | m.lib.VERIFY_ALLOW_UNBOUND_STATEMENT | m.lib.VERIFY_ALLOW_SURROGATE) == 0
    assert "mina_ctx_set_state_dedup" in go and "MINA_VERIFY_DEDUP_STATES" in go
    assert "changes NO result" in hdr                       # the header states the exactness claim
    for meth in ("protocol_state_dedup_dev", "protocol_state_hash_batch_dedup", "set_state_dedup", "state_dedup_stats"):
        assert callable(getattr(m.MinaContext, meth)), meth


def test_null_context_is_refused_without_a_gpu():
    import mina_bridge_amd as m
    lib = m.load_library()
    err = lib.mina_last_error
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    n_out = ctypes.c_size_t(7)
    a, b, c = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    assert lib.mina_protocol_state_dedup_dev(None, ctypes.c_size_t(1), p, p, p, p, ctypes.c_uint32(0)) == MINA_ERR_ARG and err()
    assert lib.mina_protocol_state_hash_batch_dedup(None, ctypes.c_size_t(1), p, p, p, None, ctypes.byref(n_out)) == MINA_ERR_ARG
    assert lib.mina_ctx_set_state_dedup(None, 1) == MINA_ERR_ARG
    assert lib.mina_ctx_state_dedup_stats(None, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == MINA_ERR_ARG


needs_llvm = pytest.mark.skipif(not os.path.exists(os.path.join(CO.LLVM_BIN, "llvm-objdump")), reason="LLVM binutils of the ROCm toolchain not present")


@pytest.fixture(scope="module")
def co():
    c = CO.CodeObjects()
    yield c
    c.close()


@needs_llvm
@pytest.mark.parametrize("uniq,plain", [("pstate_hash_uniq_kernel<0, 3>", "pstate_hash_kernel<0, 3>"), ("pstate_hash_uniq_kernel<0, 8>", "pstate_hash_kernel<0, 8>"),
                                        ("pstate_hash_uniq_kernel<0, 16>", "pstate_hash_kernel<0, 16>")])
def test_uniq_hash_kernels_keep_their_siblings_contract(co, uniq, plain):
    """no more VGPRs, spills and scratch than the plain sibling's entry in tests/test_code_object.py's CONTRACT, the same waves per SIMD, no LDS, no raised priority"""
    from test_code_object import CONTRACT, waves_per_simd
    ks = co.kernels()
    assert uniq in ks, sorted(k for k in ks if "pstate" in k)
    m = ks[uniq]
    vmax, spill_max, scratch_max, lds, waves_min = CONTRACT[plain]
    assert m["vgpr_count"] <= vmax and m["vgpr_spill_count"] <= spill_max and m["private_segment_fixed_size"] <= scratch_max, m
    assert m["group_segment_fixed_size"] == lds and not m.get("uses_dynamic_stack", False)
    assert waves_per_simd(m) >= waves_min and waves_per_simd(m) == waves_per_simd(ks[plain]), (waves_per_simd(m), waves_per_simd(ks[plain]))
    assert [op for _, mn, op in co.instructions(uniq) if mn == "s_setprio"] == []


@needs_llvm
def test_single_lane_uniq_kernel_matches_its_sibling(co):
    """pstate_hash1_kernel has no CONTRACT entry: its sibling is measured against the kernel itself -- five waves per SIMD, nothing spilled, no raised priority"""
    from test_code_object import waves_per_simd
    ks = co.kernels()
    u, p = ks["pstate_hash1_uniq_kernel<0>"], ks["pstate_hash1_kernel<0>"]
    assert u["vgpr_count"] <= p["vgpr_count"] <= 96 and u["vgpr_spill_count"] == 0 and u["private_segment_fixed_size"] == 0
    assert waves_per_simd(u) == waves_per_simd(p) == 5
    assert [op for _, mn, op in co.instructions("pstate_hash1_uniq_kernel<0>") if mn == "s_setprio"] == []


@needs_llvm
@pytest.mark.parametrize("kernel", ["pstate_dedup_group_kernel", "pstate_dedup_rep_kernel", "pstate_dedup_scan_kernel", "pstate_dedup_compact_kernel", "pstate_dedup_scatter_kernel"])
def test_dedup_kernels_spill_nothing(co, kernel):
    m = co.kernels()[kernel]
    assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0 and not m.get("uses_dynamic_stack", False), m


@needs_llvm
def test_group_kernel_reads_16_bytes_per_lane_and_reduces_across_lanes_without_lds(co):
    """the fingerprint / grouping kernel: 16-byte loads, 64-bit compare-and-swap and a min on the table, cross-lane moves in registers (no LDS allocation)"""
    ins = [mn for _, mn, _ in co.instructions("pstate_dedup_group_kernel")]
    assert any(mn.startswith("global_load_dwordx4") for mn in ins)
    assert any("cmpswap_x2" in mn for mn in ins) and any("atomic_umin" in mn for mn in ins), sorted(set(mn for mn in ins if "atomic" in mn))
    assert co.kernels()["pstate_dedup_group_kernel"]["group_segment_fixed_size"] == 0
    assert not any(mn.startswith(("ds_read", "ds_write", "ds_load", "ds_store")) for mn in ins)
