#!/usr/bin/env python3
"""What MINA_VERIFY_MIXED_NETWORK_JOB buys at the boundary, on one GPU in one process.  Writes profiles/mixed_network_job.json.

The forms of tools/bench_networks.py that hold proofs of both networks, with the flag off (one pass per network, one after the other) and on (one pass, one job per
chunk, the index set chosen per proof on the GPU), beside the same run's reference points:
  b_one_mixed_call         1024 proofs, half per network, in ONE call               off | on      reference: b_two_single_pair_calls (two calls of 512 on the single-pair library)
  c_different_networks     two concurrent single-proof callers, one network each    off | on      reference: c_same_network (two callers of one network)
  a_lone_network_call      a lone 1024-proof call of ONE network                    off | on      expected equal: no mixed job is formed
Every repetition sets up the single-pair library and network mode afresh and times each form once, off and on alternating; medians of `--reps` repetitions with
their spread (min, max).  A difference inside the spread of the flag-off runs is reported as none.  The shader clock is sampled around every repetition
(the amdgpu hwmon freq1_input of the first card that has one; null where there is none).  The device context's mina_ctx_mixed_job_stats are recorded with the figures.
Proofs: the fixtures' (tests/network_helpers.py: pair A four proofs, pair B two), tiled.  Run:  python tools/bench_mixed_networks.py [--reps 5] [--proofs 1024]"""
import argparse
import glob
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
MAINNET, DEVNET = 0, 1


def sclk_mhz():
    for path in sorted(glob.glob("/sys/class/drm/card*/device/hwmon/hwmon*/freq1_input")):
        try:
            return int(open(path).read()) / 1e6
        except (OSError, ValueError):
            pass
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--proofs", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixed_network_job.json"))
    args = ap.parse_args()
    try:
        import torch  # noqa: F401  (the wheel's HIP runtime initialises first where torch is present: tests/conftest.py)
        torch.cuda.is_available()
    except ImportError:
        pass
    import mina_bridge_amd as m
    from network_helpers import load_pairs
    L = m.lib
    A, B = load_pairs()
    N, H = args.proofs, args.proofs // 2
    tile = lambda calls, n: [calls[i % len(calls)] for i in range(n)]
    dev_n, dev_h, main_h = tile(A.good(DEVNET), N), tile(A.good(DEVNET), H), tile(B.good(MAINNET), H)
    mixed = [x for pair in zip(dev_h, main_h) for x in pair]
    OFF, ON = L.VERIFY_ALLOW_SURROGATE, L.VERIFY_ALLOW_SURROGATE | L.VERIFY_MIXED_NETWORK_JOB

    def call(calls, want=1):
        p, q = [c[0] for c in calls], [c[1] for c in calls]
        t0 = time.perf_counter()
        v = L.verify_state_batch(p, q)
        dt = (time.perf_counter() - t0) * 1e3
        assert v.tolist() == [want] * len(calls), "the benchmark's proofs must all be accepted"
        return dt

    def two_callers(x, y, inner=5):
        out = []
        for _ in range(inner):
            gate = threading.Barrier(3); got = [None, None]
            def worker(i, c):
                gate.wait(); got[i] = L.verify_state(*c)
            th = [threading.Thread(target=worker, args=(i, c)) for i, c in enumerate((x, y))]
            for t in th: t.start()
            gate.wait(); t0 = time.perf_counter()
            for t in th: t.join()
            out.append((time.perf_counter() - t0) * 1e3)
            assert got == [True, True]
        return statistics.median(out)

    names = ("b_two_single_pair_calls", "b_one_mixed_call_off", "b_one_mixed_call_on", "c_same_network", "c_different_networks_off", "c_different_networks_on",
             "a_lone_network_call_off", "a_lone_network_call_on")
    rows = {k: [] for k in names}
    clocks, stats = [], None
    for rep in range(args.reps):
        clk = [sclk_mhz()]
        # ---- the single-pair library: pair A declared devnet, then pair B declared mainnet
        L.verify_configure(OFF)
        L.verify_drop_network_indexes(); L.verify_set_network(-1); L.verify_shutdown()
        A.install(L.verify_all_devices()); L.verify_set_network(DEVNET)
        call(dev_h); t_a = call(dev_h)
        L.verify_set_network(-1); B.install(L.verify_all_devices()); L.verify_set_network(MAINNET)
        call(main_h); t_b = call(main_h)
        rows["b_two_single_pair_calls"].append(t_a + t_b)
        # ---- network mode: A for devnet, B for mainnet; every form warmed under either setting, then timed off / on in turn
        L.verify_set_network(-1); L.verify_shutdown()
        A.install(L.verify_network_devices(DEVNET)); B.install(L.verify_network_devices(MAINNET))
        for flags in (OFF, ON):
            L.verify_configure(flags); call(mixed); call(dev_n); two_callers(dev_n[0], main_h[0], inner=2)
        L.verify_configure(OFF)
        rows["c_same_network"].append(two_callers(dev_n[0], dev_n[1]))
        for flags, tag in ((OFF, "off"), (ON, "on")):
            L.verify_configure(flags)
            rows["b_one_mixed_call_" + tag].append(call(mixed))
            rows["c_different_networks_" + tag].append(two_callers(dev_n[0], main_h[0]))
            rows["a_lone_network_call_" + tag].append(call(dev_n))
        stats = L.verify_device_ctx(0).mixed_job_stats()
        clk.append(sclk_mhz()); clocks.append(clk)
        print("rep", rep, {k: round(v[-1], 2) for k, v in rows.items()}, "sclk MHz", clk, flush=True)
    L.verify_configure(OFF)
    L.verify_drop_network_indexes(); L.verify_shutdown(); L.verify_configure(0)

    stat = lambda v: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3), "runs_ms": [round(x, 3) for x in v]}
    res = {k: stat(v) for k, v in rows.items()}

    def compare(form, reference=None):
        off, on = res[form + "_off"], res[form + "_on"]
        d, spread = on["median_ms"] - off["median_ms"], off["max_ms"] - off["min_ms"]
        out = {"form": form, "off_ms": off["median_ms"], "on_ms": on["median_ms"], "difference_ms": round(d, 3), "off_spread_ms": round(spread, 3),
               "reading": "none (inside the spread of the flag-off runs)" if abs(d) <= spread else ("slower" if d > 0 else "faster")}
        if reference:
            out["reference"] = reference; out["reference_ms"] = res[reference]["median_ms"]
        return out
    out = {"what": "MINA_VERIFY_MIXED_NETWORK_JOB at the boundary, flag off against on (tools/bench_mixed_networks.py)", "proofs_per_call": N, "reps": args.reps,
           "poseidon_constants": L.poseidon_params_name(), "sclk_mhz_before_after_each_rep": clocks, "mixed_job_stats_last_rep": stats, "forms_ms": res,
           "comparisons": {"b_one_mixed_call": compare("b_one_mixed_call", "b_two_single_pair_calls"),
                           "c_two_concurrent_single_proof_callers": compare("c_different_networks", "c_same_network"),
                           "a_lone_call_of_one_network": compare("a_lone_network_call")}}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps(out["comparisons"], indent=1))


if __name__ == "__main__":
    main()
