"""The stream plan of pipelined device-resident jobs (ctx.h stream_plan, env_stream_budget): pure host functions, compiled into a stand-alone program against
the HIP stand-in header of the ThreadSanitizer tier -- no GPU, no HIP runtime."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "ctx.h"
int main(int argc, char **argv) {
    if (argc > 1) { printf("%d\n", env_stream_budget()); return 0; }
    for (int lanes = 1; lanes <= MB_DEV_FORK_MAX; ++lanes)
        for (int budget = -1; budget <= 32; ++budget) {
            const StreamPlan p = stream_plan(lanes, budget);
            printf("%d %d %d %d %d", lanes, budget, p.roles ? 1 : 0, p.sets, p.streams);
            for (int l = 0; l < lanes; ++l) printf(" %d:%d", p.roles ? p.w1(l) : -1, p.roles ? p.w2(l) : -1);
            printf("\n");
        }
    printf("max %d\n", MB_ROLE_STREAMS);
    return 0;
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    if not (cxx and os.path.exists(cxx)):
        pytest.skip("no C++ compiler")
    d = tmp_path_factory.mktemp("stream_plan")
    src, out = str(d / "stream_plan.cpp"), str(d / "stream_plan")
    open(src, "w").write(PROGRAM)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-w", "-I", os.path.join(ROOT, "tests", "fuzz", "hip_stub"), "-I", os.path.join(ROOT, "mina_bridge_amd", "csrc"), src, "-o", out])
    return out


@pytest.fixture(scope="module")
def table(exe):
    """{(lanes, budget): (roles, sets, streams, [(w1, w2) per lane])} for lanes 1 .. 8 and budgets -1 .. 32, and the size of the context's role-stream array"""
    t, cap = {}, None
    for line in subprocess.check_output([exe], text=True).splitlines():
        f = line.split()
        if f[0] == "max":
            cap = int(f[1])
            continue
        t[(int(f[0]), int(f[1]))] = (f[2] == "1", int(f[3]), int(f[4]), [tuple(int(x) for x in w.split(":")) for w in f[5:]])
    return t, cap


def test_the_table_of_the_issue(table):
    t, _ = table
    for budget in range(-1, 33):
        assert not t[(1, budget)][0], "a lone job always forks on its own lane's streams (plan A)"
    assert not t[(4, 23)][0] and not t[(4, 16)][0]
    assert t[(4, 15)][0], "16 streams do not fit 15"
    assert t[(4, 3)][:2] == (True, 1)
    assert t[(4, 7)][:2] == (True, 3)
    for lanes in range(2, 9):
        for budget in (-1, 0, 1, 2):
            assert t[(lanes, budget)][:2] == (True, 1)


def test_plan_a_exactly_when_four_streams_per_lane_fit(table):
    t, _ = table
    for (lanes, budget), (roles, sets, streams, _) in t.items():
        assert roles == (lanes >= 2 and 4 * lanes > budget)
        if not roles:
            assert sets == 0 and streams == 0
        else:
            assert sets == min(max((budget - 1) // 2, 1), lanes)


def test_plan_b_stays_within_the_budget_and_the_array(table):
    t, cap = table
    for (lanes, budget), (roles, sets, streams, w) in t.items():
        if not roles:
            continue
        assert 1 <= streams <= max(budget, 1) and streams <= cap, "a process with one hardware queue (budget 0) still gets the one stream"
        assert streams == min(1 + 2 * sets, max(budget, 1))
        used = {0} | {x for pair in w for x in pair}
        assert max(used) < streams
        for lane, (w1, w2) in enumerate(w):
            if streams >= 3:      # three roles apart: H = 0, and the lane's set has a W1 / W2 pair of its own
                assert (w1, w2) == (1 + 2 * (lane % sets), 2 + 2 * (lane % sets))
            else:                 # two streams: the two stages of the chain share one beside H; one stream: everything on it
                assert w1 == w2 == streams - 1
        if streams >= 3:
            assert used == set(range(streams)), "every stream of the plan serves some lane"


def test_budget_from_the_environment(exe):
    def budget(value):
        env = dict(os.environ)
        env.pop("GPU_MAX_HW_QUEUES", None)
        if value is not None:
            env["GPU_MAX_HW_QUEUES"] = value
        return int(subprocess.check_output([exe, "env"], text=True, env=env))
    assert budget("4") == 3 and budget("24") == 23 and budget("16") == 15
    assert budget("1") == 0 and budget("0") == 0 and budget("-3") == 0, "clamped to 1 .. 32 queues, less the null stream's"
    assert budget("32") == 31 and budget("1000") == 31
    assert budget(None) == 3, "HIP's own default is 4 queues"
