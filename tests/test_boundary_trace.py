"""The ORDER of the runtime calls behind mina_verify_state_batch (api_verify.hip ShapePass: copies, event records and waits per stream, job phases, slot set-up
and teardown), held against a recorded log.  The ThreadSanitizer tier (test_fuzz_parsers.py) proves the locking of that code, not what it queues where; a change
that moves a copy behind a wait, drops an event or queues a phase on another stream passes every verdict test on a stand-in device and shows here."""
import difflib
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUZZ = os.path.join(ROOT, "tests", "fuzz")
GOLDEN = os.path.join(ROOT, "tests", "golden", "boundary_call_trace.txt")


def test_boundary_queues_the_same_runtime_calls_in_the_same_order():
    """tests/fuzz/tsan_boundary.cpp built with -DMB_STUB_TRACE (`make -C tests/fuzz trace`: the product's api_verify.hip against the stand-in runtime, no sanitizer)
    runs a fixed script from ONE thread on one logical device -- the 37 proofs of test_boundary_pipeline_chunks_and_device_shards_give_the_same_verdicts (folded
    failures at 0, 12, 13, 36, states cut short at 5 and 25, garbage at 30) as one chunk, chunks of 5 and 2, streamed in runs of 3 / 2 / 1, streaming off, windows
    (1, 0), (3, 2), (16, 4) over 16 slots, no upload stream, the culprit search on the device's one context, MINA_VERIFY_DEDUP_STATES, chunks in which nothing
    parses, a step index (shape vote, tables prepared again), shutdown -- and checks every verdict; the stand-in runtime and the stub device layer print each call
    with streams, events and allocations named by creation order.  All runtime calls of a pass come from the calling thread (the pool only parses), so the log is
    the same run after run (five runs compared when it was recorded).  Done = the log equals tests/golden/boundary_call_trace.txt line for line.

    The golden file was recorded from the commit BEFORE run_device_shape became ShapePass, except the tail behind `# mina_verify_shutdown`, recorded after it: the
    teardown moved into Slot::destroy, which also frees pk_host / pk_dev (the stand-in context never allocates them, so the tail came out the same).  The tail was
    recorded once more when the contexts' buffers began to free themselves: their hipFree lines moved behind the stream destruction, and `hipFree m65+0` (the
    context's dedup_totals, which the stand-in mina_ctx_destroy had forgotten) is new -- with the free lines taken out, the old and the new file are the same.  A change
    that moves the queueing on purpose records the file again (`tests/fuzz/trace_boundary <the two fixtures> trace`, behind the first line); its diff then shows
    what moved."""
    subprocess.check_call(["make", "-C", FUZZ, "-s", "trace"])
    r = subprocess.run([os.path.join(FUZZ, "trace_boundary"), os.path.join(ROOT, "tests", "golden", "state_proofs_k15_bytes.json"),
                        os.path.join(ROOT, "tests", "golden", "account_proofs_bytes.json"), "trace"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])                    # a wrong verdict, a failed call, no culprit search
    want = open(GOLDEN).read().splitlines()[1:]                                 # (the first line says where the file comes from)
    got = r.stdout.splitlines()
    assert len(got) > 2000 and sum(l.startswith("# ") for l in got) == 19, (len(got), r.stderr[-500:])
    assert got == want, "\n".join(list(difflib.unified_diff(want, got, "recorded", "now", lineterm="", n=6))[:80])
    print(r.stderr.strip())
