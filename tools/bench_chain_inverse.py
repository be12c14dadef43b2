#!/usr/bin/env python3
"""What the chain inverse (mina_ctx_set_chain_inverse: the `_gcd` twins of pickles_scalar, kimchi_scalar, kimchi_pub, kimchi_ftcomm, pubcomm_finish16 / pubcomm_finish,
lagrange_finish, lagrange_digit_table, points_sum) costs and saves, mode off against mode on of ONE build, interleaved, on a caller-owned context:

  (i)   ONE full-size proof per call (bench.py's job at one proof: 17 state hashes, statement -> 40 public inputs, kimchi, the k = 15 opening, the 2^16 accumulator)
        through `mina_state_job_batch_dev` alone on the chip: wall us per call (host clock around call + synchronise), with the chain inverse off, on, and on together
        with the fast inverse (mina_ctx_set_fast_inverse: the MSM finishes);
  (ii)  the same calls with HIP-event stage timing (mina_prof_*): the `pickles_statement` and `kimchi_to_batch` stages -- the two that hold the covered kernels of a
        job -- and the sum of all stages;
  (iii) `mina_state_jobs_prepare(15, 40)` from scratch (Lagrange basis of 2^15 points, window table, the 128 digit multiples of 40 x 32 windows): wall ms.

Every figure is the median of `--reps` (>= 3) runs per mode; inside every repetition the order is off, on, both, off again: the second off run gives the run-to-run
spread "off against off" that a difference has to exceed.  The boundary (mina_verify_*) has no flag for the mode, so `mina_verify_state` is not measured here.
`--parent-lib <libminaverify.so of the parent commit>` adds bench.py's headline on this build against the parent's, mode off, alternating, one fresh process each.

The driver never opens the GPU: every step that does is a child process under its own `timeout`, and the first one that fails ends the run.

    python tools/bench_chain_inverse.py [--reps 5] [--calls 48] [--parent-lib PATH] [--out profiles/chain_inverse.json]
"""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIB = os.path.join(ROOT, "mina_bridge_amd", "libminaverify.so")
ALL_STAGES = 0xffff                                 # ctx.h ProfStage: every stage
MODES = ("off", "on", "both", "off_again")          # both: chain inverse + fast inverse


def med(xs):
    return statistics.median(xs)


def child_measure(args):
    import numpy as np
    import torch                                                   # first: its bundled HIP runtime initialises before the library's
    torch.cuda.is_available()
    import mina_bridge_amd as m
    import bench

    ctx = m.MinaContext(0)
    for f in (0, 1):
        ctx.poseidon_set_params(f, m.poseidon_params.default_params_bytes(f))
    ctx.srs_create(bench.CURVE_VESTA, 1 << 16)
    ctx.srs_create(bench.CURVE_PALLAS, 1 << 16)
    B = 1
    (hj, keep), kp, _, _ = bench.build_full_job(ctx, m, B, 0x6D696E61)
    dev = torch.device("cuda", 0)
    dj, dk, dtensors = bench.device_jobs(m, hj, keep, kp, dev)
    ctx.state_jobs_prepare(bench.LOG2_DOMAIN, bench.NPUB)
    out = torch.zeros(B + 4, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def set_mode(mode):
        ctx.set_chain_inverse(mode in ("on", "both"))
        ctx.set_fast_inverse(mode == "both")

    def call():
        ctx.state_job_batch_dev(dj, out.data_ptr(), out.data_ptr() + 4 * B); ctx.synchronize()

    def lone():
        t0 = time.perf_counter()
        for _ in range(args.calls):
            call()
        wall = (time.perf_counter() - t0) / args.calls * 1e6
        ctx.prof_enable(ALL_STAGES)
        for _ in range(args.calls):
            call()
        p = ctx.prof_read(); ctx.prof_enable(0)
        st = {k: v[1] / args.calls * 1e3 for k, v in p.items() if v[0]}
        return wall, st

    def prepare_ms():
        ctx.state_jobs_prepare(bench.LOG2_DOMAIN - 1, bench.NPUB)          # another domain: the next prepare builds everything again
        ctx.synchronize()
        t0 = time.perf_counter()
        ctx.state_jobs_prepare(bench.LOG2_DOMAIN, bench.NPUB)
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3

    verdicts = set()
    for mode in MODES:                                             # the same verdicts and flags before anything is timed
        set_mode(mode)
        for _ in range(3):
            call()
        verdicts.add(tuple(out.cpu().numpy().tolist()))
    assert verdicts == {(1, 1, 0, 1, 0)}, verdicts

    legs = ("job_wall_us", "pickles_statement_stage_us", "kimchi_to_batch_stage_us", "all_stages_us", "prepare_wall_ms")
    runs = {leg: {mode: [] for mode in MODES} for leg in legs}
    stages = {}
    sampler = bench.PowerSampler(None, interval=0.05).start()
    for rep in range(args.warmup + args.reps):
        for mode in MODES:
            set_mode(mode)
            wall, st = lone()
            prep = prepare_ms()
            if rep >= args.warmup:
                for leg, v in zip(legs, (wall, st.get("pickles_statement", 0.0), st.get("kimchi_to_batch", 0.0), sum(st.values()), prep)):
                    runs[leg][mode].append(v)
                stages[mode] = st
    set_mode("off")
    call()
    assert tuple(out.cpu().numpy().tolist()) == (1, 1, 0, 1, 0)
    power = sampler.stop()
    stats = {"chain": ctx.chain_inverse_stats(), "msm_finish": ctx.inverse_stats()}
    ctx.close()
    medians = {}
    for leg, by_mode in runs.items():
        off, again = by_mode["off"], by_mode["off_again"]
        row = {mode: med(v) for mode, v in by_mode.items()}
        row["off_against_off"] = abs(row["off_again"] - row["off"]) / row["off"] if row["off"] else 0.0
        row["off_spread"] = (max(off + again) - min(off + again)) / row["off"] if row["off"] else 0.0
        row["on_over_off"] = row["on"] / row["off"] if row["off"] else None
        row["both_over_off"] = row["both"] / row["off"] if row["off"] else None
        medians[leg] = row
        print(leg, json.dumps(row), flush=True)
    json.dump({"device": torch.cuda.get_device_name(0), "clock": power, "stats": stats, "stages_us_last_run": stages, "runs": runs, "medians": medians},
              open(args.child_out, "w"), indent=1)


def step(cmd, seconds, **kw):
    """one GPU step: a fresh child under its own time limit; a failure ends the run"""
    r = subprocess.run(["timeout", "-k", "10", str(seconds)] + cmd, cwd=ROOT, **kw)
    if r.returncode != 0:
        sys.exit("step failed (exit %d): %s" % (r.returncode, " ".join(cmd)))
    return r


def bench_headline(lib, steps, warmup):
    """bench.py's headline (proofs/s) with `lib` in the library's place, in a fresh process; the build's own library is put back whatever happens"""
    keep = LIB + ".keep"
    shutil.copy(LIB, keep)
    try:
        if lib:
            shutil.copy(lib, LIB)
        r = step([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--no-cpu-baseline", "--no-boundary", "--no-probes"], 420,
                 capture_output=True, text=True)
    finally:
        shutil.move(keep, LIB)
    line = [l for l in r.stdout.splitlines() if l.startswith('{"metric"')][-1]
    return json.loads(line)["value"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=48, help="lone calls per timed run")
    ap.add_argument("--parent-lib", default="", help="libminaverify.so built from the parent commit: adds the bench.py headline of both builds, mode off")
    ap.add_argument("--bench-rounds", type=int, default=2)
    ap.add_argument("--bench-steps", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chain_inverse.json"))
    ap.add_argument("--child-out", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.reps < 3:
        sys.exit("medians of at least 3 runs: --reps >= 3")
    if args.child_out:
        return child_measure(args)
    tmp = args.out + ".part"
    step([sys.executable, os.path.abspath(__file__), "--warmup", str(args.warmup), "--reps", str(args.reps), "--calls", str(args.calls), "--child-out", tmp], 900)
    result = {"commit": subprocess.run(["git", "-C", ROOT, "describe", "--always", "--dirty"], capture_output=True, text=True).stdout.strip() or "unknown",
              "warmup": args.warmup, "reps": args.reps, "calls_per_run": args.calls,
              "method": "a caller-owned context, one full-size proof per mina_state_job_batch_dev call, host clock around call + synchronise, then the same calls with "
                        "HIP-event stage timing; mina_state_jobs_prepare(15, 40) after a prepare of another domain; per repetition: off, on, both (chain + fast "
                        "inverse), off again; medians over reps, every run listed; off_against_off = |median(off again) - median(off)| / median(off)",
              "mina_verify_state": "not measured: the boundary has no flag for the mode in this build"}
    result.update(json.load(open(tmp)))
    os.remove(tmp)
    if args.parent_lib:
        rounds = {"this_build": [], "parent": []}
        for _ in range(args.bench_rounds):
            rounds["this_build"].append(bench_headline("", args.bench_steps, 3))
            rounds["parent"].append(bench_headline(args.parent_lib, args.bench_steps, 3))
        a, b = med(rounds["this_build"]), med(rounds["parent"])
        spread = max((max(v) - min(v)) / med(v) for v in rounds.values())
        result["bench_headline_proofs_per_s"] = dict(rounds, this_over_parent=a / b, run_to_run_spread=spread, level=abs(a / b - 1) <= max(spread, result["medians"]["job_wall_us"]["off_spread"]))
        print("bench.py headline", json.dumps(result["bench_headline_proofs_per_s"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
