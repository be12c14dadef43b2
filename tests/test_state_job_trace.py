"""The ORDER of the runtime calls behind ONE Proof-of-State job (mina_bridge_amd/csrc/state_job.hip: the fork of a job's legs onto helper streams, the role streams,
the event records and waits that tie the legs together, where the verdict kernel goes), held against a recorded log -- the layer test_boundary_trace.py stubs
out.  Verdict parity on a GPU (test_role_streams.py) passes with a wait dropped as long as the race does not bite that day; here the dropped wait is a diff."""
import difflib
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUZZ = os.path.join(ROOT, "tests", "fuzz")
GOLDEN = os.path.join(ROOT, "tests", "golden", "state_job_call_trace.txt")
TAIL = "# FAILURE PATHS"


def unordered_waits(lines):
    """The rule the comment above state_job.hip's JobRoute states: every `hipStreamWaitEvent sX waits for eN` stands below a `hipEventRecord eN` of that event
    (a record does not outlive its event: a wait on a destroyed event is as wrong), and no line names the null event e0.  Returns the offending lines."""
    recorded, bad = set(), []
    for n, line in enumerate(lines, 1):
        if re.search(r"\be0\b", line):
            bad.append((n, line))
            continue
        m = re.match(r"hipEventRecord (e\d+) ", line)
        if m:
            recorded.add(m.group(1))
        m = re.match(r"hipEventDestroy (e\d+)", line)
        if m:
            recorded.discard(m.group(1))
        m = re.match(r"hipStreamWaitEvent s\d+ waits for (e\d+)", line)
        if m and m.group(1) not in recorded:
            bad.append((n, line))
    return bad


def test_a_state_job_queues_the_same_runtime_calls_in_the_same_order():
    """tests/fuzz/trace_state_job.cpp (`make -C tests/fuzz trace_job`: the product's state_job.hip and host_core.hip against the stand-in runtime, the device layer
    beneath them stubbed) runs a fixed script from ONE thread: the inline job with each section off in turn and every form of the wrap-proof leg, the three-lane
    plan of state_job_each, the boundary's two phases for every lane triple setup_legs can produce with 0 / part / all of the states hashed early, and
    mina_state_job_batch_dev / _fold_dev through dev_fork_lanes -- one lane, a pinned lane, 4 lanes at stream budgets 23 / 7 / 3 / 2 / 1, 9 lanes, every dev_fork
    mode, dev_acc_lane, the piece and LDS knobs, the piece arithmetic on either side of HASH1_MIN_STATES, 13 jobs back to back, budgets 23 -> 3 -> 23 -> 3 on one
    context, deduplicated states.  Done = the log equals tests/golden/state_job_call_trace.txt line for line, and no wait stands above the record of its event.

    The golden file was recorded at the commit that only MOVED this code out of api_state.hip, before anything in it was rewritten (`tests/fuzz/trace_state_job
    moved` built against that commit's state_job.hip), except the section from `# FAILURE PATHS` on: a leg that fails after the job has forked, recorded after
    the one body that owns fork and join joined such a job too.  A change that moves the queueing on purpose records the file again (`tests/fuzz/trace_state_job`,
    behind the first line); its diff then shows what moved."""
    subprocess.check_call(["make", "-C", FUZZ, "-s", "trace_job"])
    r = subprocess.run([os.path.join(FUZZ, "trace_state_job")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])                    # a job that failed where it should pass, or passed where it should fail
    want = open(GOLDEN).read().splitlines()[1:]                                 # (the first line says where the file comes from)
    got = r.stdout.splitlines()
    assert len(got) > 3000 and sum(l.startswith(TAIL) for l in got) == 1, (len(got), r.stderr[-500:])
    assert got == want, "\n".join(list(difflib.unified_diff(want, got, "recorded", "now", lineterm="", n=6))[:80])
    bad = unordered_waits(got)
    assert not bad, bad[:10]


def test_the_wait_rule_sees_a_wait_above_its_record():
    """the rule itself, on three lines: a wait below its record passes, above it or on the null event does not"""
    ok = ["hipEventCreate -> e1", "hipEventRecord e1 on s1", "hipStreamWaitEvent s2 waits for e1"]
    assert unordered_waits(ok) == []
    assert [n for n, _ in unordered_waits([ok[0], ok[2], ok[1]])] == [2]
    assert [n for n, _ in unordered_waits(ok + ["hipStreamWaitEvent s2 waits for e0"])] == [4]
    assert [n for n, _ in unordered_waits(ok + ["hipEventDestroy e1", ok[2]])] == [5]
