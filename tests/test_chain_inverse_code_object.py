"""CPU tier of the chain inverse's kernels (tools/code_object.py over the gfx950 code object inside libminaverify.so): every `_gcd` twin is there beside the kernel it
mirrors, none keeps anything in scratch (tests/test_code_object.py exempts names that begin with kimchi_scalar / pickles_scalar, and so does this file), each raises
its wave priority at its top where its original does, and the LDS columns of kimchi_pub_gcd_kernel<10> leave the CU room."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import code_object as CO  # noqa: E402

# twin -> (the kernel it mirrors, whether that kernel opens with mb_wave_prio())
TWINS = {
    "pickles_scalar_gcd_kernel": ("pickles_scalar_kernel", True),
    "kimchi_scalar_gcd_kernel": ("kimchi_scalar_kernel", True),
    "kimchi_pub_gcd_kernel<8>": ("kimchi_pub_kernel<8>", True),
    "kimchi_pub_gcd_kernel<10>": ("kimchi_pub_kernel<10>", True),
    "kimchi_ftcomm_gcd_kernel": ("kimchi_ftcomm_kernel", True),
    "pubcomm_finish16_gcd_kernel<0>": ("pubcomm_finish16_kernel<0>", True),
    "pubcomm_finish_gcd_kernel<0>": ("pubcomm_finish_kernel<0>", True),
    "pubcomm_finish_gcd_kernel<1>": ("pubcomm_finish_kernel<1>", True),
    "lagrange_finish_gcd_kernel<0>": ("lagrange_finish_kernel<0>", False),
    "lagrange_finish_gcd_kernel<1>": ("lagrange_finish_kernel<1>", False),
    "lagrange_digit_table_gcd_kernel<0>": ("lagrange_digit_table_kernel<0>", False),
    "lagrange_digit_table_gcd_kernel<1>": ("lagrange_digit_table_kernel<1>", False),
    "points_sum_gcd_kernel<0>": ("points_sum_kernel<0>", False),
    "points_sum_gcd_kernel<1>": ("points_sum_kernel<1>", False),
}
# Deliberately without a twin (include/mina_verify.h says so too):
#   group_law_selftest_kernel   api_core.hip's one device inversion: a self-test hook of the parity tests, on no job's path
#   ipa_prepare_kernel          its latency form keeps its challenge arrays in scratch, which tests/test_code_object.py allows under that kernel's name only
LEFT_ON_THE_POWER = ("group_law_selftest_gcd_kernel", "ipa_prepare_gcd_kernel")
SCRATCH_EXEMPT = ("kimchi_scalar", "pickles_scalar")
LDS_PER_CU = 160 * 1024                                          # gfx950: 160 KiB of LDS per compute unit

needs_llvm = pytest.mark.skipif(not os.path.exists(os.path.join(CO.LLVM_BIN, "llvm-objdump")), reason="LLVM binutils of the ROCm toolchain not present")


@pytest.fixture(scope="module")
def co():
    c = CO.CodeObjects()
    yield c
    c.close()


@needs_llvm
@pytest.mark.parametrize("twin", sorted(TWINS))
def test_the_twin_is_there_beside_its_original_with_nothing_in_scratch(co, twin):
    ks = co.kernels()
    original, _ = TWINS[twin]
    assert twin in ks and original in ks, sorted(k for k in ks if "_gcd_kernel" in k)
    meta = ks[twin]
    assert not meta.get("uses_dynamic_stack", False), meta
    assert meta["max_flat_workgroup_size"] <= ks[original]["max_flat_workgroup_size"]
    if not twin.startswith(SCRATCH_EXEMPT):
        assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0, meta
    assert meta["group_segment_fixed_size"] >= ks[original]["group_segment_fixed_size"]


@needs_llvm
@pytest.mark.parametrize("twin", sorted(t for t, (_, prio) in TWINS.items() if prio))
def test_the_twin_raises_its_priority_where_its_original_does(co, twin):
    for k in (twin, TWINS[twin][0]):
        ins = co.instructions(k)
        prios = [op.strip() for _, mn, op in ins if mn == "s_setprio"]
        assert prios and set(prios) <= {"2", "0x2"}, (k, prios)
        assert "s_setprio" in [mn for _, mn, _ in ins][:40], (k, "the priority is raised at the top of the kernel")


@needs_llvm
def test_the_originals_without_a_raised_priority_have_twins_without_one(co):
    for twin, (original, prio) in TWINS.items():
        if not prio:
            for k in (twin, original):
                assert not [1 for _, mn, _ in co.instructions(k) if mn == "s_setprio"], k


@needs_llvm
def test_the_lds_columns_of_the_public_polynomial_leave_the_cu_room(co):
    """kimchi_pub_gcd_kernel<CH>: 2 CH columns (denominators, prefix products) x 8 words x 64 lanes x 4 B -- 40 960 B at CH = 10, 32 768 B at CH = 8: a quarter and
    a fifth of the 160 KiB a CU has, so three workgroups fit beside each other where one is asked for; kimchi_pub_kernel keeps them out of LDS"""
    ks = co.kernels()
    assert ks["kimchi_pub_gcd_kernel<10>"]["group_segment_fixed_size"] == 2 * 10 * 8 * 64 * 4 == 40960
    assert ks["kimchi_pub_gcd_kernel<8>"]["group_segment_fixed_size"] == 2 * 8 * 8 * 64 * 4 == 32768
    assert 3 * ks["kimchi_pub_gcd_kernel<10>"]["group_segment_fixed_size"] <= LDS_PER_CU
    assert ks["kimchi_pub_kernel<10>"]["group_segment_fixed_size"] == 0 and ks["kimchi_pub_kernel<8>"]["group_segment_fixed_size"] == 0


@needs_llvm
def test_what_is_left_on_the_power_has_no_twin(co):
    ks = co.kernels()
    for name in LEFT_ON_THE_POWER:
        assert not [k for k in ks if k.startswith(name)], name
    gcd = sorted(k.split("<")[0] for k in ks if "_gcd_kernel" in k)
    assert set(gcd) == {t.split("<")[0] for t in TWINS} | {"field_inv_gcd_kernel", "msm_finish_gcd_kernel", "msm_tail_gcd_kernel"}, gcd
