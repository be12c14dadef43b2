#!/usr/bin/env python3
"""What the grouped culprit search (mina_ctx_set_search_groups) costs and saves: the time of ONE `mina_state_job_batch` call on a failing batch at the real
sizes -- bench.py's input builder: k = 15 wrap openings, 2^16 accumulators, 17 state hashes per proof -- with 1024 and 8192 proofs per call and three culprit
sets (one in the middle; 8 spread evenly; one per 64 proofs), each as bad openings and as bad accumulators.

A host clock around the call (it ends in a synchronisation).  On a build with the mode: the fan search (off) and groups of 16, 64 and 128 alternate in ONE
process, `--warmup` untimed and `--reps` timed searches each; medians, every run and the spread of the off runs are written, with mina_ctx_search_stats (rounds,
parts) per search.  `--fold-mfma-min 0,64,128,256` sweeps the shortest segment the segmented fold sends to the matrix cores (mina_ctx_set_seg_fold_mfma_min; 0 = the
VALU kernels at every size) in the same alternation -- every group count at every value, labelled `G@MIN` -- and records mina_ctx_seg_fold_stats per search; the
comparison for the segmented matrix-core fold is the parent commit's library through `--lib ... --mode off` and this build at `@0`.  A clean call is timed before and after 20 searches: searches must not leave later calls slower (the effect of searches that created streams,
api_state.hip).  `--mode off` uses only entry points older than the mode -- with `--lib` it measures another build of the library (the parent commit's): that
run is the baseline, and `--baseline FILE` copies its figures into the output.

    python tools/bench_search.py [--mode all|off] [--lib other/libminaverify.so] [--baseline parent.json] [--sizes 1024,8192] [--fold-mfma-min 0,64,128,256] [--out profiles/grouped_search.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def view(ptr, nbytes):
    """the numpy array behind a pointer field of a host-side mina_state_jobs (kept alive by the job's keep list)"""
    return np.ctypeslib.as_array((ctypes.c_uint8 * nbytes).from_address(ptr))


def culprit_sets(B):
    return {"one_middle": [B // 2], "eight_spread": [B * (2 * i + 1) // 16 for i in range(8)], "one_per_64": list(range(32, B, 64))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("all", "off"), default="all")
    ap.add_argument("--lib", default=None, help="load this build of libminaverify.so instead of the tree's (the parent commit's, with --mode off)")
    ap.add_argument("--baseline", default=None, help="a --mode off result of the parent commit's build, copied into the output as `parent`")
    ap.add_argument("--sizes", default="1024,8192")
    ap.add_argument("--groups", default="16,64,128")
    ap.add_argument("--fold-mfma-min", default="256", help="shortest segment of the segmented fold on the matrix cores, swept with the group counts (0 = never; one value: labels stay the group count)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grouped_search.json"))
    args = ap.parse_args()
    import torch                                                   # first: its bundled HIP runtime initialises before the library's
    torch.cuda.is_available()
    import mina_bridge_amd as m
    if args.lib:
        m.lib.LIB_PATH = os.path.abspath(args.lib)
    import bench
    lib = m.load_library()
    grouped = args.mode == "all"
    if grouped and not hasattr(lib, "mina_ctx_set_search_groups"):
        sys.exit("this build has no grouped search: run with --mode off")
    fold_mins = [int(x) for x in args.fold_mfma_min.split(",")]
    seg_fold = grouped and hasattr(lib, "mina_ctx_set_seg_fold_mfma_min")
    if len(fold_mins) > 1 and not seg_fold:
        sys.exit("this build has no mina_ctx_set_seg_fold_mfma_min: nothing to sweep")
    # a mode: (label, groups, shortest matrix-core segment or None); "0" = the fan search
    modes = [("0", 0, None)]
    if grouped:
        for g in args.groups.split(","):
            modes += [(g if len(fold_mins) == 1 else f"{g}@{fm}", int(g), fm if seg_fold else None) for fm in fold_mins]
    ctx = m.MinaContext(0)
    for f in (0, 1):
        ctx.poseidon_set_params(f, m.poseidon_params.default_params_bytes(f))
    for curve in (0, 1):
        ctx.srs_create(curve, 65536)
    result = {"commit": subprocess.run(["git", "-C", ROOT, "describe", "--always", "--dirty"], capture_output=True, text=True).stdout.strip() or "unknown",
              "library": args.lib or "the tree's build", "device": torch.cuda.get_device_name(0) if torch.cuda.is_available() else "unknown", "warmup": args.warmup, "reps": args.reps,
              "method": "host clock around one mina_state_job_batch call (host buffers in, verdict bytes out; the call synchronises); modes alternate in one process; "
                        "medians over reps, every run listed; mode 0 = the fan search; G@MIN = groups of G with the segmented fold on the matrix cores from MIN proofs per segment (0 = never)",
              "fold_mfma_min": fold_mins, "configs": {}}

    def set_mode(g, fold_min):
        if grouped:
            ctx.set_search_groups(g)
        if fold_min is not None:
            ctx.set_seg_fold_mfma_min(fold_min)

    def counters():
        s = ctx.search_stats()
        if seg_fold:
            s.update(ctx.seg_fold_stats())
        return s

    def call(job, B):
        t0 = time.perf_counter()
        v = ctx.state_job_batch(job)
        return (time.perf_counter() - t0) * 1e3, v

    for B in [int(x) for x in args.sizes.split(",")]:
        job, kp, _, _ = bench.build_full_job(ctx, m, B, 0x6D696E61, distinct_chains=min(B, 64))
        sj = job[0]
        z1, acc_sg = view(sj.z1, B * 32), view(sj.acc_sg, B * 64)
        z1_0, sg_0 = z1.copy(), acc_sg.copy()
        for _ in range(3):
            ms, v = call(job, B)
        assert v.tolist() == [1] * B, "the untampered batch must be accepted"
        clean_before = [call(job, B)[0] for _ in range(10)]
        searches_run = 0
        for leg in ("opening", "accumulator"):
            for name, bad in culprit_sets(B).items():
                z1[:] = z1_0; acc_sg[:] = sg_0
                for b in bad:
                    if leg == "opening":
                        z1[b * 32] ^= 1                             # another opening scalar: the folded opening check fails
                    else:
                        o = (b + 1) % B                             # the neighbour's commitment (another wrap proof of the fixtures): a valid point, the wrong one
                        acc_sg[b * 64:(b + 1) * 64] = sg_0[o * 64:(o + 1) * 64]
                want = [0 if b in set(bad) else 1 for b in range(B)]
                runs = {label: [] for label, _, _ in modes}
                stats = {}
                for rep in range(args.warmup + args.reps):
                    for label, g, fold_min in modes:
                        set_mode(g, fold_min)
                        s0 = counters() if grouped else None
                        ms, v = call(job, B)
                        searches_run += 1
                        assert v.tolist() == want, (B, leg, name, label)
                        if rep >= args.warmup:
                            runs[label].append(ms)
                        if grouped:
                            s1 = counters(); stats[label] = {k: s1[k] - s0[k] for k in s1}
                set_mode(0, 256 if seg_fold else None)
                off = runs["0"]
                cfg = {"proofs": B, "leg": leg, "culprits": len(bad), "ms_off": statistics.median(off), "ms_off_min": min(off), "ms_off_max": max(off),
                       "ms_off_spread": (max(off) - min(off)) / statistics.median(off), "runs_ms": runs}
                for label, _, _ in modes[1:]:
                    cfg[f"ms_groups_{label}"] = statistics.median(runs[label]); cfg[f"groups_{label}_over_off"] = statistics.median(runs[label]) / statistics.median(off)
                    cfg[f"stats_groups_{label}"] = stats[label]
                key = f"{leg}_{name}_{B}"
                result["configs"][key] = cfg
                print(key, json.dumps({k: v for k, v in cfg.items() if k != "runs_ms"}), flush=True)
        z1[:] = z1_0; acc_sg[:] = sg_0
        clean_after = [call(job, B)[0] for _ in range(10)]
        result[f"clean_call_{B}"] = {"ms_before": statistics.median(clean_before), "ms_after": statistics.median(clean_after), "searches_between": searches_run,
                                     "after_over_before": statistics.median(clean_after) / statistics.median(clean_before), "before_runs": clean_before, "after_runs": clean_after}
        print(f"clean_call_{B}", json.dumps({k: v for k, v in result[f"clean_call_{B}"].items() if not k.endswith("_runs")}), flush=True)
        del sj, job, kp
    ctx.close()
    if args.baseline:
        result["parent"] = json.load(open(args.baseline))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
