#!/usr/bin/env python3
"""What the fast inverse (mina_ctx_set_fast_inverse; fe_modinv.cuh, msm_finish_gcd_kernel / msm_tail_gcd_kernel) costs and saves, mode off against mode on of ONE
build, interleaved in ONE process:

  (i)   one 2^16 Vesta `mina_msm_srs_dev` alone on the chip: wall us per call (host clock around call + synchronise) and its `msm_finish` stage time (HIP events
        on the lane's stream: mina_prof_enable) -- the stage the mode changes;
  (ii)  one `mina_accumulator_check_dev` (batch 1, k = 16: BASELINE C2 as written) alone, the same two figures;
  (iii) (i) and (ii) once more with the fused MSM tail on (mina_ctx_set_msm_fused_tail): msm_tail_kernel against msm_tail_gcd_kernel;
  (iv)  `mina_field_inv` against `mina_field_inv_gcd` at n = 1 and n = 2^16: wall us per call, uploads and downloads included (the same in both).

Every figure is the median of `--reps` (>= 3) runs per mode, the modes alternating inside every repetition; every run is listed, with the spread of the off runs and
the shader clock sampled during the timed regions.  The bar is the mode off of the same run; 193 us of the lone MSM's finish stage was the inversion when the mode
was proposed (profiles/msm_fused_tail.json).

    python tools/bench_inverse.py [--reps 5] [--calls 64] [--out profiles/fast_inverse.json]
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

CURVE_VESTA, FIELD_FQ, K = 1, 1, 16
ALL_STAGES = 0x7ff                                  # ctx.h ProfStage: the MSM's eight stages and the b_poly stages of the accumulator check


def med(xs):
    return statistics.median(xs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=64, help="lone calls per timed run")
    ap.add_argument("--inv-calls", type=int, default=16, help="batch inversions per timed run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fast_inverse.json"))
    args = ap.parse_args()
    if args.reps < 3:
        sys.exit("medians of at least 3 runs: --reps >= 3")
    import torch                                                   # first: its bundled HIP runtime initialises before the library's
    torch.cuda.is_available()
    import mina_bridge_amd as m
    import bench

    ctx = m.MinaContext(0)
    for f in (0, 1):
        ctx.poseidon_set_params(f, m.poseidon_params.default_params_bytes(f))
    ctx.srs_create(CURVE_VESTA, 1 << K)
    rng = np.random.Generator(np.random.PCG64(0x6D696E61))
    sc = rng.integers(0, 256, size=(1 << K, 32), dtype=np.uint8); sc[:, 31] &= 0x3F
    d_sc = ctx.dev_upload(ctx.dev_malloc(sc.size), sc.reshape(-1))
    d_rec = ctx.dev_malloc(2 * 68 + 16)
    msm = lambda: ctx.msm_srs_dev(CURVE_VESTA, 1 << K, d_sc, d_rec)
    pre8, sg8 = bench.make_accumulators(ctx, 8, 4242)
    d_pre8 = ctx.dev_upload(ctx.dev_malloc(pre8.size), pre8.reshape(-1)); d_sg8 = ctx.dev_upload(ctx.dev_malloc(sg8.size), sg8.reshape(-1))
    d_v8 = ctx.dev_upload(ctx.dev_malloc(32), np.zeros(32, np.uint8))
    verdicts = lambda: ctx.dev_download(d_v8, 32).view(np.uint32).tolist()
    check1 = lambda: ctx.accumulator_check_dev(CURVE_VESTA, K, 1, d_pre8, d_sg8, 0, d_v8)
    elems = {1: sc[:1].copy(), 1 << 16: sc.copy()}                 # below 2^254: canonical in both fields
    MODES = ("off", "on")

    def set_mode(mode, fused_tail=False):
        ctx.set_fast_inverse(mode == "on")
        ctx.set_msm_fused_tail(fused_tail)

    def lone(call):
        """-> (wall us per call, finish-stage us per call, kernel us per call): the wall run without the stage events, then a run with them"""
        t0 = time.perf_counter()
        for _ in range(args.calls):
            call(); ctx.synchronize()
        wall = (time.perf_counter() - t0) / args.calls * 1e6
        ctx.prof_enable(ALL_STAGES)
        for _ in range(args.calls):
            call(); ctx.synchronize()
        p = ctx.prof_read(); ctx.prof_enable(0)
        per_stage = {k: v[1] / args.calls * 1e3 for k, v in p.items() if v[0]}
        return wall, per_stage.get("msm_finish", 0.0), sum(per_stage.values()), per_stage

    def inv_wall(fn, a):
        t0 = time.perf_counter()
        for _ in range(args.inv_calls):
            fn(FIELD_FQ, a)
        return (time.perf_counter() - t0) / args.inv_calls * 1e6

    # the same bytes before anything is timed
    records = set()
    for fused in (False, True):
        for mode in MODES:
            set_mode(mode, fused)
            for _ in range(4):
                msm(); check1()
            ctx.synchronize()
            records.add(ctx.dev_download(d_rec, 68).tobytes())
            assert verdicts()[0] == 1, (mode, fused)
    assert len(records) == 1, "the modes disagree on the MSM's record"
    for a in elems.values():
        assert (ctx.field_inv(FIELD_FQ, a) == ctx.field_inv_gcd(FIELD_FQ, a)).all()

    legs = ("msm_wall_us", "msm_finish_stage_us", "msm_kernel_us", "check_wall_us", "check_finish_stage_us", "check_kernel_us",
            "fused_tail_msm_wall_us", "fused_tail_msm_kernel_us", "fused_tail_check_wall_us", "field_inv_n1_wall_us", "field_inv_n65536_wall_us")
    runs = {leg: {mode: [] for mode in MODES} for leg in legs}
    stages = {}
    sampler = bench.PowerSampler(None, interval=0.05).start()
    for rep in range(args.warmup + args.reps):
        for mode in MODES:
            set_mode(mode)
            w, fin, k, st = lone(msm)
            w2, fin2, k2, st2 = lone(check1)
            set_mode(mode, fused_tail=True)
            w3, _, k3, st3 = lone(msm)
            w4, _, _, _ = lone(check1)
            set_mode(mode)
            fn = ctx.field_inv_gcd if mode == "on" else ctx.field_inv
            i1, i64k = inv_wall(fn, elems[1]), inv_wall(fn, elems[1 << 16])
            if rep >= args.warmup:
                for leg, v in zip(legs, (w, fin, k, w2, fin2, k2, w3, k3, w4, i1, i64k)):
                    runs[leg][mode].append(v)
                stages[mode] = {"msm": st, "check": st2, "fused_tail_msm": st3}
    assert verdicts()[0] == 1
    set_mode("off")
    power = sampler.stop()
    inverse_stats = ctx.inverse_stats()
    ctx.close()

    result = {"commit": subprocess.run(["git", "-C", ROOT, "describe", "--always", "--dirty"], capture_output=True, text=True).stdout.strip() or "unknown",
              "device": torch.cuda.get_device_name(0) if torch.cuda.is_available() else "unknown",
              "warmup": args.warmup, "reps": args.reps, "calls_per_run": args.calls, "inversions_per_run": args.inv_calls,
              "method": "one process, the modes alternate inside every repetition; lone calls: host clock around call + synchronise, then the same calls with HIP-event "
                        "stage timing (msm_finish: the stage the mode changes); field_inv legs: off = mina_field_inv, on = mina_field_inv_gcd, host clock around the "
                        "call, transfers included; medians over reps, every run listed",
              "clock": power, "inverse_stats": inverse_stats, "stages_us_last_run": stages, "runs": runs, "medians": {}}
    for leg, by_mode in runs.items():
        off, on = by_mode["off"], by_mode["on"]
        row = {"off": med(off), "off_min": min(off), "off_max": max(off), "off_spread": (max(off) - min(off)) / med(off) if med(off) else 0.0,
               "on": med(on), "on_min": min(on), "on_max": max(on)}
        row["on_over_off"] = row["on"] / row["off"] if row["off"] else None
        result["medians"][leg] = row
        print(leg, json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
