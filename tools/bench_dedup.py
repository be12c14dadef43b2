#!/usr/bin/env python3
"""What the deduplicated protocol-state leg (mina_ctx_set_state_dedup) costs and what it saves, measured the way bench.py measures the headline: the same input
builder, `mina_state_job_batch_dev`, warm-up, then `--steps` steps between one pair of synchronisations, the sampled shader clock beside each figure.  Mode off and
mode on run in the SAME process, interleaved (off, on, off, on, ...), on

  * all-distinct chains   -- bench.py's headline input: the price of looking (mode off is the code path without this feature);
  * sliding-window chains -- proof t carries states [t, t + 16) of one long chain and every proof the same bridge tip: the traffic the mode exists for;

each at 16 384 proofs per call over 4 lanes and at 4096 proofs per lone call (the 3-lane hash form), plus `mina_protocol_state_dedup_dev` alone at 17 x 16 384
records (HIP events).  Writes profiles/dedup_state_job.json; README.md / DESIGN.md / INTEGRATION.md quote from that file.

    python tools/bench_dedup.py [--steps 20] [--warmup 8] [--reps 3] [--out profiles/dedup_state_job.json]
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

HBM_SPEC_TBS, HBM_COPY_TBS = 8.0, 6.3          # MI355X: specified bandwidth, measured device-to-device copy rate


def sliding_chains(ctx, bench, B, seed):
    """records[B,17,2048], nfields[B,17], hashes[B,17,32]: proof t = states [t, t + 16) of ONE chain of B + 15 linked states + one bridge tip state for all"""
    rng = np.random.Generator(np.random.PCG64(seed))
    L, S, F = B + 15, bench.PSTATE_SLOTS, bench.PSTATE_BODY_FIELDS
    recs = np.zeros((L + 1, S, 32), np.uint8)
    body = rng.integers(0, 256, size=(L + 1, F, 32), dtype=np.uint8); body[..., 31] &= 0x3F
    recs[:, 1:1 + F] = body
    nf1 = np.array([F], np.uint32)
    hashes = np.zeros((L + 1, 32), np.uint8)
    prev = rng.integers(0, 256, size=32, dtype=np.uint8); prev[31] &= 0x3F
    for s in range(L + 1):
        if s == L:                                             # the bridge tip: not linked
            prev = rng.integers(0, 256, size=32, dtype=np.uint8); prev[31] &= 0x3F
        recs[s, 0] = prev
        hashes[s] = ctx.protocol_state_hash_batch(recs[s].reshape(1, -1), nf1)[0]
        prev = hashes[s].copy()
    idx = np.concatenate([np.arange(B)[:, None] + np.arange(16)[None, :], np.full((B, 1), L)], axis=1)
    return recs.reshape(L + 1, S * 32)[idx], np.full((B, 17), F, np.uint32), hashes[idx]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3, help="off / on pairs per configuration (the median is reported, every run is listed)")
    ap.add_argument("--jobs", type=int, default=16384)
    ap.add_argument("--lone-jobs", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dedup_state_job.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_dedup.py needs a GPU")
    import bench
    import mina_bridge_amd as m
    dev = torch.device("cuda", 0)
    ctx = m.MinaContext(0)
    for f in (0, 1):
        ctx.poseidon_set_params(f, m.poseidon_params.default_params_bytes(f))
    ctx.srs_create(bench.CURVE_VESTA, 1 << 16); ctx.srs_create(bench.CURVE_PALLAS, 1 << 16)
    try:
        pr_ = torch.cuda.get_device_properties(0)
        bdf = "%04x:%02x:%02x.0" % (getattr(pr_, "pci_domain_id", 0), pr_.pci_bus_id, pr_.pci_device_id)
    except Exception:
        bdf = None

    def inputs(B, seed):
        """{name: (device job, keep-alive, distinct / states)} for the two inputs at B proofs per call"""
        out = {}
        (hj, keep), kp, _, distinct = bench.build_full_job(ctx, m, B, seed)
        assert distinct["chains"] == B
        ctx.state_jobs_prepare(bench.LOG2_DOMAIN, bench.NPUB)
        out["all_distinct"] = bench.device_jobs(m, hj, keep, kp, dev) + (None,)
        r, f, h = sliding_chains(ctx, bench, B, seed + 7)
        arrs = [np.ascontiguousarray(r.reshape(-1)), np.ascontiguousarray(f.reshape(-1)), np.ascontiguousarray(h.reshape(-1))]
        for name, a in zip(("state_records", "state_nfields", "expected_hashes"), arrs):
            setattr(hj, name, a.ctypes.data)
        out["sliding_window"] = bench.device_jobs(m, hj, list(keep) + arrs, kp, dev) + (None,)
        return out

    def timed(dj, B, lanes, on):
        ctx.set_pipeline(lanes)
        ctx.set_state_dedup(on)
        outs = [torch.zeros(B + 4, dtype=torch.int32, device=dev) for _ in range(max(lanes, 8))]
        it = [0]

        def step():
            o = outs[it[0] % len(outs)]; it[0] += 1
            ctx.state_job_batch_dev(dj, o.data_ptr(), o.data_ptr() + 4 * B)
        for _ in range(max(args.warmup, lanes, 1)):
            step()
        ctx.synchronize()
        assert all(o.cpu().numpy().tolist() == [1] * B + [1, 0, 1, 0] for o in outs[:min(len(outs), it[0])]), "warm-up verdicts must be ACCEPT"
        sampler = bench.PowerSampler(bdf, interval=0.05)
        torch.cuda.synchronize()
        sampler.start()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        ctx.synchronize(); torch.cuda.synchronize()
        el = time.perf_counter() - t0
        pw = sampler.stop()
        st = ctx.state_dedup_stats() if on else None
        ctx.set_state_dedup(False)
        return {"ms_per_step": el / args.steps * 1e3, "proofs_per_s": B * args.steps / el, "sclk_mhz_avg": pw and pw["sclk_mhz_avg"],
                "distinct_over_states": (st.distinct / st.states) if st and st.states else None, "collisions": st.collisions if st else None}

    result = {"commit": subprocess.run(["git", "-C", ROOT, "describe", "--always", "--dirty"], capture_output=True, text=True).stdout.strip() or "unknown",
              "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup, "reps": args.reps,
              "method": "mina_state_job_batch_dev as bench.py times it; mode off / on interleaved in one process; medians over reps, every run listed", "configs": {}}
    for B, lanes in ((args.jobs, 4), (args.lone_jobs, 1)):
        jobs = inputs(B, 0x6D696E61)
        for name, (dj, dk, tensors, _) in jobs.items():
            runs = {"off": [], "on": []}
            for _ in range(args.reps):
                for mode in ("off", "on"):
                    runs[mode].append(timed(dj, B, lanes, mode == "on"))
            med = {mode: statistics.median(r["ms_per_step"] for r in runs[mode]) for mode in runs}
            key = f"{name}_{B}x{lanes}"
            result["configs"][key] = {"proofs_per_call": B, "lanes": lanes, "input": name, "ms_per_step_off": med["off"], "ms_per_step_on": med["on"], "on_over_off": med["on"] / med["off"],
                                      "proofs_per_s_off": B / med["off"] * 1e3, "proofs_per_s_on": B / med["on"] * 1e3, "distinct_over_states": runs["on"][-1]["distinct_over_states"],
                                      "sclk_mhz_off": statistics.median(r["sclk_mhz_avg"] for r in runs["off"]) if runs["off"][0]["sclk_mhz_avg"] else None,
                                      "sclk_mhz_on": statistics.median(r["sclk_mhz_avg"] for r in runs["on"]) if runs["on"][0]["sclk_mhz_avg"] else None, "runs": runs}
            print(key, json.dumps({k: v for k, v in result["configs"][key].items() if k != "runs"}), flush=True)
        # the grouping alone on the records of the headline-size job (HIP events on the context's own stream)
        if B == args.jobs:
            ctx.set_pipeline(1); ctx.pin_lane(0)
            ext = torch.cuda.ExternalStream(ctx.stream)
            n = 17 * B
            group = {}
            for name, (dj, dk, tensors, _) in jobs.items():
                d_rep = torch.zeros(n, dtype=torch.int32, device=dev); d_cnt = torch.zeros(2, dtype=torch.int32, device=dev)
                torch.cuda.synchronize()
                times = []
                for i in range(8):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    with torch.cuda.stream(ext):
                        e0.record()
                        ctx.protocol_state_dedup_dev(n, dj.state_records, dj.state_nfields, d_rep.data_ptr(), d_cnt.data_ptr(), 0)
                        e1.record()
                    ctx.synchronize(); torch.cuda.synchronize()
                    times.append(e0.elapsed_time(e1))
                ms = statistics.median(times[2:])
                used = n * (1 + bench.PSTATE_BODY_FIELDS) * 32
                cnt = d_cnt.cpu().numpy().tolist()
                group[name] = {"records": n, "ms": ms, "record_bytes_used": used, "own_record_tb_per_s": used / ms / 1e9, "hbm_spec_tb_per_s": HBM_SPEC_TBS, "hbm_copy_tb_per_s": HBM_COPY_TBS,
                               "n_distinct": cnt[0], "n_collisions": cnt[1], "runs_ms": times,
                               "note": "every record is read once for its fingerprint (the figure above counts these bytes only); a record that meets its class's owner reads the owner's record too"}
                print("dedup_dev", name, json.dumps(group[name]), flush=True)
            result["dedup_dev_alone"] = group
            ctx.pin_lane(-1)
        del jobs
        torch.cuda.empty_cache()
    ctx.set_pipeline(1)
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
