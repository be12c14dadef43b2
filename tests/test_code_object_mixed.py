"""The `_net` twins of the index-reading kernels (mixed jobs: include/mina_verify.h "MIXED jobs"), read from the gfx950 code objects inside libminaverify.so
(CPU tier, as tests/test_code_object.py): every twin is there in every form its launch site can pick, none keeps anything in scratch but the two PolishToken
interpreters (allowed under their names, as their kernels are), the public polynomial's twin holds its columns in LDS, and each opens with the raised wave
priority of the wrap-proof chain."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import code_object as CO  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists(os.path.join(CO.LLVM_BIN, "llvm-objdump")), reason="LLVM binutils of the ROCm toolchain not present")

TWINS = ["kimchi_fq_net_kernel<16>", "kimchi_fq_net_kernel<8>", "kimchi_fq_net_kernel<3>", "kimchi_rows_net_kernel", "kimchi_pub_net_kernel<8>", "kimchi_pub_net_kernel<10>",
         "kimchi_scalar_net_kernel", "kimchi_ftcomm_net_kernel", "pickles_digest_net_kernel<16>", "pickles_digest_net_kernel<8>", "pickles_digest_net_kernel<3>",
         "pickles_scalar_net_kernel"]


@pytest.fixture(scope="module")
def co():
    c = CO.CodeObjects()
    yield c
    c.close()


def test_every_twin_is_built_and_nothing_else_carries_the_name(co):
    have = sorted(k.split("#")[0] for k in co.kernels() if "_net_kernel" in k)
    assert have == sorted(TWINS), have
    assert not [k for k in have if "gcd" in k], "a mixed job inverts by the power: no `_gcd` twins of the `_net` kernels"


@pytest.mark.parametrize("kernel", TWINS)
def test_scratch_lds_and_priority(co, kernel):
    m = co.kernels()[kernel]
    assert not m.get("uses_dynamic_stack", False) and m.get("wavefront_size", 64) == 64
    if "_scalar_net" not in kernel:
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (kernel, m["private_segment_fixed_size"], m["vgpr_spill_count"])
    if kernel.startswith("kimchi_pub_net_kernel"):              # PubLds: 2 CH columns of 8 words for 64 lanes
        ch = 10 if "<10>" in kernel else 8
        assert m["group_segment_fixed_size"] == 2 * ch * 8 * 64 * 4, m["group_segment_fixed_size"]
    ins = co.instructions(kernel)
    prios = [op.strip() for _, mn, op in ins if mn == "s_setprio"]
    assert prios and set(prios) <= {"2", "0x2"}, (kernel, prios)
    assert "s_setprio" in [mn for _, mn, _ in ins][:40], (kernel, "the priority is raised at the top of the kernel")


def test_the_three_lane_transcript_twins_keep_their_waves(co):
    """kimchi_fq_net_kernel<3> trades the fourth wave per SIMD of kimchi_fq_kernel<3> for an empty scratch segment (amdgpu_waves_per_eu(2, 8)): three at the least;
    pickles_digest_net_kernel<3> keeps the four of its kernel"""
    waves = lambda m: min(8, 512 // (-(-m["vgpr_count"] // 8) * 8))
    ks = co.kernels()
    assert waves(ks["kimchi_fq_net_kernel<3>"]) >= 3, ks["kimchi_fq_net_kernel<3>"]["vgpr_count"]
    assert waves(ks["pickles_digest_net_kernel<3>"]) >= 4, ks["pickles_digest_net_kernel<3>"]["vgpr_count"]
