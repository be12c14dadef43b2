#!/usr/bin/env python3
"""What the fused MSM tail (mina_ctx_set_msm_fused_tail; msm.cuh msm_tail_kernel) costs and saves, mode off against mode on of ONE build, interleaved in ONE process:

  (i)   one 2^16 Vesta `mina_msm_srs_dev` alone on the chip: wall us per call (host clock around call + synchronise) and the sum of its kernels' stage times
        (HIP events on the lane's stream: mina_prof_enable), per stage;
  (ii)  one `mina_accumulator_check_dev` (batch 1, k = 16: BASELINE C2 as written) alone, the same two figures;
  (iii) the pipelined C2 rate over `--lanes` lanes (16: bench.py's `c2_accumulator_only`): `multi8` is bench.py's shape, 8 un-folded checks per call -- a
        bucket-lane plan, which keeps the staged tail in both modes and is here to show that the mode leaves it alone -- and `single` is one check per call, the
        task form the mode changes.

Every figure is the median of `--reps` (>= 3) runs per mode, the modes alternating inside every repetition; every run is listed, with the spread of the off runs
and the shader clock sampled during the timed regions.  `--mode off` uses only entry points older than the mode: with `--lib` it measures another build of the
library (the parent commit's), and `--baseline FILE` copies such a result into the output as `parent` -- mode off against the parent is the bar, measured the same
day by alternating the two processes.

`--one-call off|on` is the run for `rocprofv3 --kernel-trace --stats -- python tools/bench_msm_tail.py --one-call on`: the set-up, then `--trace-calls` lone MSMs in
that mode and nothing else; the launches per MSM are the msm_* kernels' call counts in the trace divided by `--trace-calls`, read from the trace and not from the
code.  `--trace-stats OFF.csv ON.csv` reads the two kernel_stats.csv files and writes the counts per kernel into the output.

    python tools/bench_msm_tail.py [--mode all|off] [--lib other/libminaverify.so] [--baseline parent.json] [--reps 5] [--out profiles/msm_fused_tail.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CURVE_VESTA, K = 1, 16
MSM_STAGES, ALL_STAGES = 0xff, 0x7ff               # ctx.h ProfStage: the MSM's eight stages | with the b_poly stages of the accumulator check


def med(xs):
    return statistics.median(xs)


def launches_from_traces(off_csv, on_csv, calls):
    """kernel_stats.csv of the two --one-call runs -> launches per lone MSM, per kernel and in total.  The set-up (SRS generation, window tables) is the same in both
    runs and launches no MSM pipeline kernel; the buffer fill behind hipMemsetAsync is a launch too and is counted by its difference between the two runs."""
    import csv
    setup = ("msm_build_table_kernel", "msm_table29_kernel", "msm_table29s_kernel")
    out, fills = {}, {}
    for mode, path in (("off", off_csv), ("on", on_csv)):
        per = {}
        fills[mode] = 0
        for r in csv.DictReader(open(path)):
            name, n = r["Name"].replace("void ", "").split("(")[0].replace("mb::", ""), int(r["Calls"])
            if name.startswith("msm_") and not name.startswith(setup):
                per[name] = {"per_msm": n / calls, "avg_us": float(r["AverageNs"]) / 1e3}
            elif "fill" in name.lower():
                fills[mode] += n
        out[mode] = per
        out["launches_" + mode] = sum(v["per_msm"] for v in per.values())
        out["kernel_us_" + mode] = sum(v["per_msm"] * v["avg_us"] for v in per.values())
    out["fill_launches_on_minus_off_per_msm"] = (fills["on"] - fills["off"]) / calls
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("all", "off"), default="all")
    ap.add_argument("--lib", default=None, help="load this build of libminaverify.so instead of the tree's (the parent commit's, with --mode off)")
    ap.add_argument("--baseline", default=None, help="a --mode off result of the parent commit's build, copied into the output as `parent`")
    ap.add_argument("--one-call", choices=("off", "on"), default=None, help="set-up, then --trace-calls lone MSMs in this mode and nothing else (for a kernel trace)")
    ap.add_argument("--trace-calls", type=int, default=10)
    ap.add_argument("--trace-stats", nargs=2, metavar=("OFF.csv", "ON.csv"), default=None, help="rocprofv3's kernel_stats.csv of the --one-call off / on runs: launches per lone MSM go into the output")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=64, help="lone calls per timed run")
    ap.add_argument("--lanes", type=int, default=16)
    ap.add_argument("--pipe-calls", type=int, default=400, help="pipelined calls per timed run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "msm_fused_tail.json"))
    args = ap.parse_args()
    if args.reps < 3:
        sys.exit("medians of at least 3 runs: --reps >= 3")
    import torch                                                   # first: its bundled HIP runtime initialises before the library's
    torch.cuda.is_available()
    import mina_bridge_amd as m
    if args.lib:
        m.lib.LIB_PATH = os.path.abspath(args.lib)
    import bench
    lib = m.load_library()
    have_mode = hasattr(lib, "mina_ctx_set_msm_fused_tail")
    if (args.mode == "all" or args.one_call == "on") and not have_mode:
        sys.exit("this build has no fused MSM tail: run with --mode off")
    modes = ["off", "on"] if args.mode == "all" else ["off"]

    ctx = m.MinaContext(0)
    for f in (0, 1):
        ctx.poseidon_set_params(f, m.poseidon_params.default_params_bytes(f))
    ctx.srs_create(CURVE_VESTA, 1 << K)
    rng = np.random.Generator(np.random.PCG64(0x6D696E61))
    sc = rng.integers(0, 256, size=(1 << K, 32), dtype=np.uint8); sc[:, 31] &= 0x3F
    d_sc = ctx.dev_upload(ctx.dev_malloc(sc.size), sc.reshape(-1))
    d_rec = ctx.dev_malloc(2 * 68 + 16)
    msm = lambda: ctx.msm_srs_dev(CURVE_VESTA, 1 << K, d_sc, d_rec)

    def set_mode(mode):
        if have_mode:
            ctx.set_msm_fused_tail(mode == "on")

    if args.one_call:
        set_mode(args.one_call)
        for _ in range(args.trace_calls):
            msm(); ctx.synchronize()
        print(json.dumps({"one_call_mode": args.one_call, "msm_calls": args.trace_calls, "tail_stats": ctx.msm_tail_stats() if have_mode else None}))
        ctx.close()
        return

    pre8, sg8 = bench.make_accumulators(ctx, 8, 4242)
    d_pre8 = ctx.dev_upload(ctx.dev_malloc(pre8.size), pre8.reshape(-1)); d_sg8 = ctx.dev_upload(ctx.dev_malloc(sg8.size), sg8.reshape(-1))
    d_v8 = ctx.dev_upload(ctx.dev_malloc(32), np.zeros(32, np.uint8))
    verdicts = lambda: ctx.dev_download(d_v8, 32).view(np.uint32).tolist()

    check1 = lambda: ctx.accumulator_check_dev(CURVE_VESTA, K, 1, d_pre8, d_sg8, 0, d_v8)
    check8 = lambda: ctx.accumulator_check_multi_dev(CURVE_VESTA, K, 8, d_pre8, d_sg8, d_v8)

    def lone(call, stages):
        """-> (wall us per call, kernel us per call, {stage: us per call}): the wall run without the stage events, then a run with them"""
        t0 = time.perf_counter()
        for _ in range(args.calls):
            call(); ctx.synchronize()
        wall = (time.perf_counter() - t0) / args.calls * 1e6
        ctx.prof_enable(stages)
        for _ in range(args.calls):
            call(); ctx.synchronize()
        p = ctx.prof_read(); ctx.prof_enable(0)
        per_stage = {k: v[1] / args.calls * 1e3 for k, v in p.items() if v[0]}
        return wall, sum(per_stage.values()), per_stage

    def piped(call, per_call):
        for _ in range(32):
            call()
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.pipe_calls):
            call()
        ctx.synchronize()
        return per_call * args.pipe_calls / (time.perf_counter() - t0)

    # the two modes give the same record before anything is timed
    records = {}
    for mode in modes:
        set_mode(mode)
        for _ in range(4):
            msm(); check1()
        ctx.synchronize()
        records[mode] = ctx.dev_download(d_rec, 68).tobytes()
        assert verdicts()[0] == 1, mode
    assert len(set(records.values())) == 1, "the modes disagree on the MSM's record"

    sampler = bench.PowerSampler(None, interval=0.05).start()
    runs = {leg: {mode: [] for mode in modes} for leg in ("msm_wall_us", "msm_kernel_us", "check_wall_us", "check_kernel_us", "c2_multi8_per_s", "c2_single_per_s")}
    stages = {"msm": {}, "check": {}}
    for rep in range(args.warmup + args.reps):
        for mode in modes:
            set_mode(mode)
            w, k, st = lone(msm, MSM_STAGES)
            w2, k2, st2 = lone(check1, ALL_STAGES)
            if rep >= args.warmup:
                runs["msm_wall_us"][mode].append(w); runs["msm_kernel_us"][mode].append(k); runs["check_wall_us"][mode].append(w2); runs["check_kernel_us"][mode].append(k2)
                stages["msm"][mode], stages["check"][mode] = st, st2
    ctx.set_pipeline(args.lanes)
    for rep in range(args.warmup + args.reps):
        for mode in modes:
            set_mode(mode)
            r8, r1 = piped(check8, 8), piped(check1, 1)
            if rep >= args.warmup:
                runs["c2_multi8_per_s"][mode].append(r8); runs["c2_single_per_s"][mode].append(r1)
    assert verdicts()[0] == 1
    ctx.set_pipeline(1)
    set_mode("off")
    power = sampler.stop()
    tail_stats = ctx.msm_tail_stats() if have_mode else None
    ctx.close()

    result = {"commit": subprocess.run(["git", "-C", ROOT, "describe", "--always", "--dirty"], capture_output=True, text=True).stdout.strip() or "unknown",
              "library": args.lib or "the tree's build", "device": torch.cuda.get_device_name(0) if torch.cuda.is_available() else "unknown",
              "warmup": args.warmup, "reps": args.reps, "calls_per_run": args.calls, "lanes": args.lanes, "pipelined_calls_per_run": args.pipe_calls,
              "method": "one process, the modes alternate inside every repetition; lone calls: host clock around call + synchronise, then the same calls with HIP-event stage "
                        "timing for the kernel sums; pipelined: calls queued back to back over the lanes, one wait; medians over reps, every run listed",
              "clock": power, "tail_stats": tail_stats, "stages_us_last_run": stages, "runs": runs, "medians": {}}
    for leg, by_mode in runs.items():
        off = by_mode["off"]
        row = {"off": med(off), "off_min": min(off), "off_max": max(off), "off_spread": (max(off) - min(off)) / med(off)}
        if "on" in by_mode:
            row["on"] = med(by_mode["on"]); row["on_over_off"] = row["on"] / row["off"]
        result["medians"][leg] = row
        print(leg, json.dumps(row), flush=True)
    if args.trace_stats:
        result["launches_per_lone_msm_from_trace"] = launches_from_traces(args.trace_stats[0], args.trace_stats[1], args.trace_calls)
        print("launches", json.dumps({k: v for k, v in result["launches_per_lone_msm_from_trace"].items() if k.startswith("launches")}), flush=True)
    if args.baseline:
        result["parent"] = json.load(open(args.baseline))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
