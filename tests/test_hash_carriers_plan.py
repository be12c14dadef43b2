"""The second state-hash carrier of the role plan (ctx.h StreamPlan::carriers, stream_plan, stream_plan_env, role_piece_waves): pure host functions, compiled into
a stand-alone program against the HIP stand-in header of the ThreadSanitizer tier -- no GPU, no HIP runtime.  tests/test_stream_plan.py holds sets, streams, w1
and w2 for every budget as they were before the second carrier; here: the carrier count, h(lane), where the opening check goes, the streams kept busy, the plan of
a context that forces no budget, and the pieces of a leg under two carriers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "ctx.h"
static void show(const char *tag, int lanes, int budget, const StreamPlan &p) {
    printf("%s %d %d %d %d %d %d %d", tag, lanes, budget, p.roles ? 1 : 0, p.sets, p.streams, p.carriers, p.busy());
    for (int l = 0; l < lanes; ++l) printf(" %d:%d:%d:%d", p.roles ? p.h(l) : -1, p.roles ? p.w1(l) : -1, p.roles ? p.w2(l) : -1, p.roles && p.check_on_w1(l) ? 1 : 0);
    printf("\n");
}
int main() {
    for (int lanes = 1; lanes <= MB_DEV_FORK_MAX; ++lanes) {
        for (int budget = 0; budget <= 33; ++budget) show("plan", lanes, budget, stream_plan(lanes, budget));
        for (int env = 0; env <= 31; ++env) show("env", lanes, env, stream_plan_env(lanes, env));
    }
    for (int lanes = 1; lanes <= MB_DEV_FORK_MAX; ++lanes)
        for (int one = 0; one <= 1; ++one)
            for (size_t waves : {1u, 52u, 767u, 768u, 769u, 1536u, 1537u, 3072u, 3073u, 4352u, 6144u, 13264u, 65536u})
                printf("piece %d %d %zu %u\n", lanes, one, waves, role_piece_waves(waves, lanes, one != 0));
    printf("h1 %d %d\n", MB_ROLE_H1, MB_ROLE_STREAMS);
    return 0;
}
"""

# stream_plan(lanes, budget) for budget <= 3 as it was BEFORE the second carrier (taken from the parent of the change): (roles, sets, streams, w1, w2) -- the same
# for every lane of the plan -- for 2 .. 8 lanes; one lane is plan A at every budget
BEFORE = {0: (True, 1, 1, 0, 0), 1: (True, 1, 1, 0, 0), 2: (True, 1, 2, 1, 1), 3: (True, 1, 3, 1, 2)}


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    if not (cxx and os.path.exists(cxx)):
        pytest.skip("no C++ compiler")
    d = tmp_path_factory.mktemp("hash_carriers")
    src, out = str(d / "plan.cpp"), str(d / "plan")
    open(src, "w").write(PROGRAM)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-w", "-I", os.path.join(ROOT, "tests", "fuzz", "hip_stub"), "-I", os.path.join(ROOT, "mina_bridge_amd", "csrc"), src, "-o", out])
    plan, env, piece, h1 = {}, {}, {}, None
    for line in subprocess.check_output([out], text=True).splitlines():
        f = line.split()
        if f[0] == "piece":
            piece[(int(f[1]), f[2] == "1", int(f[3]))] = int(f[4])
        elif f[0] == "h1":
            h1 = (int(f[1]), int(f[2]))
        else:
            per_lane = [tuple(int(x) for x in w.split(":")) for w in f[8:]]
            (plan if f[0] == "plan" else env)[(int(f[1]), int(f[2]))] = dict(roles=f[3] == "1", sets=int(f[4]), streams=int(f[5]), carriers=int(f[6]), busy=int(f[7]), lanes=per_lane)
    return plan, env, piece, h1


def test_budgets_up_to_three_are_the_plan_as_it_was(tables):
    plan, _, _, _ = tables
    for budget in range(0, 4):
        p = plan[(1, budget)]
        assert not p["roles"] and (p["sets"], p["streams"], p["carriers"], p["busy"]) == (0, 0, 0, 0)
        for lanes in range(2, 9):
            p = plan[(lanes, budget)]
            roles, sets, streams, w1, w2 = BEFORE[budget]
            assert (p["roles"], p["sets"], p["streams"]) == (roles, sets, streams), (lanes, budget)
            assert p["carriers"] == 1 and p["busy"] == streams
            assert p["lanes"] == [(0, w1, w2, 0)] * lanes, "one carrier: every lane hashes on H, every opening check on W2"


def test_plan_a_is_chosen_where_it_was(tables):
    plan, env, _, _ = tables
    for (lanes, budget), p in plan.items():
        assert p["roles"] == (lanes >= 2 and 4 * lanes > budget), (lanes, budget)
        if not p["roles"]:
            assert (p["sets"], p["streams"], p["carriers"], p["busy"]) == (0, 0, 0, 0)
    for (lanes, e), p in env.items():
        assert p["roles"] == plan[(lanes, e)]["roles"], "the environment's plan A is decided on queues - 1"


def test_the_plan_stays_within_its_budget(tables):
    plan, _, _, (h1, cap) = tables
    for (lanes, budget), p in plan.items():
        if not p["roles"]:
            continue
        assert 1 <= p["busy"] <= max(budget, 1), (lanes, budget)
        used = {x for h, w1, w2, _ in p["lanes"] for x in (h, w1, w2)}
        assert len(used) <= p["busy"] and max(used) < cap
        # sets, streams, w1, w2: untouched by the second carrier (the rule of tests/test_stream_plan.py)
        assert p["sets"] == min(max((budget - 1) // 2, 1), lanes) and p["streams"] == min(1 + 2 * p["sets"], max(budget, 1))


def test_a_second_carrier_exactly_where_the_budget_has_a_stream_to_spare(tables):
    plan, _, _, (h1, cap) = tables
    for (lanes, budget), p in plan.items():
        if not p["roles"]:
            continue
        two = p["streams"] >= 3 and budget > p["streams"]
        assert p["carriers"] == (2 if two else 1), (lanes, budget)
        assert p["busy"] == p["streams"] + (1 if two else 0)
        hs = [h for h, _, _, _ in p["lanes"]]
        if two:
            assert hs == [h1 if l % 2 else 0 for l in range(lanes)], "consecutive lanes alternate between H and H1"
            assert h1 == cap - 1 and h1 >= p["streams"], "H1 stands behind every chain pair: no budget makes it another role's stream"
            for l, (_, _, _, on_w1) in enumerate(p["lanes"]):
                assert on_w1 == (1 if (l // p["sets"]) % 2 == 0 else 0), "every other lane of a set keeps its opening check on W1"
        else:
            assert hs == [0] * lanes and not any(c for _, _, _, c in p["lanes"])
    for lanes in range(2, 9):
        p = plan[(lanes, 4)]
        assert (p["sets"], p["streams"], p["carriers"], p["busy"]) == (1, 3, 2, 4), "budget 4: H, H1, W1, W2"
        assert plan[(lanes, 5)]["carriers"] == 1 and plan[(lanes, 6)]["carriers"] == 2, "5: two chain pairs fill the budget; 6: a stream to spare"


def test_the_environments_plan_takes_the_last_queue_for_the_second_carrier(tables):
    plan, env, _, _ = tables
    for (lanes, e), p in env.items():
        base, more = plan[(lanes, e)], plan.get((lanes, e + 1))
        if lanes >= 4 and base["roles"] and base["carriers"] == 1 and more and more["roles"] and more["carriers"] == 2 and more["sets"] == base["sets"]:
            assert p == more, (lanes, e)
        else:
            assert p == base, (lanes, e)
    for lanes in range(2, 9):
        assert env[(lanes, 3)] == plan[(lanes, 4 if lanes >= 4 else 3)], "4 queues: two carriers and one chain pair, where that was timed (4 lanes or more)"
        assert env[(lanes, 2)] == plan[(lanes, 2)] and env[(lanes, 1)] == plan[(lanes, 1)] and env[(lanes, 0)] == plan[(lanes, 0)]
    assert env[(4, 23)] == plan[(4, 23)] and not env[(4, 23)]["roles"]


def test_pieces_under_two_carriers_are_equal(tables):
    _, _, piece, _ = tables
    assert piece[(4, True, 4352)] == 1451, "the headline's leg: three pieces of 1451 / 1451 / 1450 waves"
    assert piece[(2, True, 4352)] == 2176 and piece[(4, True, 1536)] == 0 and piece[(4, False, 52)] == 0
    for (lanes, one, waves), pw in piece.items():
        target = (6144 if one else 3072) // lanes
        if waves <= target:
            assert pw == 0, "a leg of one piece is one launch"
            continue
        n = -(-waves // pw)
        assert pw <= target and n == -(-waves // target), (lanes, one, waves, pw)
        assert waves - (n - 1) * pw > pw - n, "the last piece is short by less than a wave per piece: no thin remainder"
