#!/usr/bin/env python3
"""What network mode (an index pair per network: mina_verify_install_*_net) costs at the boundary, on one GPU in one process.  Writes profiles/network_indexes.json.

  (a) a lone 1024-proof call of ONE network: the single-pair library with that network declared, against network mode with both pairs installed
  (b) the same 1024 proofs split half and half between the networks in ONE call (two passes, one after the other), against two single-pair calls of 512
  (c) two concurrent single-proof callers of DIFFERENT networks (the second pass waits for the first), against two callers of the same network

The forms are interleaved -- every repetition sets up the single-pair library and network mode afresh and times each form once -- and the medians of
`--reps` repetitions are reported with their spread (min, max).  A difference inside the spread of the single-pair runs is reported as none.
Proofs: the fixtures' (tests/network_helpers.py: pair A four proofs, pair B two), tiled.  Run:  python tools/bench_networks.py [--reps 5] [--proofs 1024]"""
import argparse
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
MAINNET, DEVNET = 0, 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--proofs", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "network_indexes.json"))
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

    L.verify_configure(L.VERIFY_ALLOW_SURROGATE)
    rows = {k: [] for k in ("a_single_pair", "a_network_mode", "b_two_single_pair_calls", "b_one_mixed_call", "c_same_network", "c_different_networks")}
    for rep in range(args.reps):
        # ---- the single-pair library: pair A declared devnet, then pair B declared mainnet
        L.verify_drop_network_indexes(); L.verify_set_network(-1); L.verify_shutdown()
        A.install(L.verify_all_devices()); L.verify_set_network(DEVNET)
        call(dev_n)                                              # warm: contexts, tables, buffers
        rows["a_single_pair"].append(call(dev_n))
        call(dev_h); t_a = call(dev_h)
        L.verify_set_network(-1); B.install(L.verify_all_devices()); L.verify_set_network(MAINNET)
        call(main_h); t_b = call(main_h)
        rows["b_two_single_pair_calls"].append(t_a + t_b)
        # ---- network mode: A for devnet, B for mainnet
        L.verify_set_network(-1); L.verify_shutdown()
        A.install(L.verify_network_devices(DEVNET)); B.install(L.verify_network_devices(MAINNET))
        call(mixed); call(dev_n)
        rows["a_network_mode"].append(call(dev_n))
        rows["b_one_mixed_call"].append(call(mixed))
        two_callers(dev_n[0], main_h[0], inner=2)
        rows["c_same_network"].append(two_callers(dev_n[0], dev_n[1]))
        rows["c_different_networks"].append(two_callers(dev_n[0], main_h[0]))
        print("rep", rep, {k: round(v[-1], 2) for k, v in rows.items()}, flush=True)
    L.verify_drop_network_indexes(); L.verify_shutdown(); L.verify_configure(0)

    stat = lambda v: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3), "runs_ms": [round(x, 3) for x in v]}
    res = {k: stat(v) for k, v in rows.items()}

    def compare(base, form):
        d = res[form]["median_ms"] - res[base]["median_ms"]
        spread = res[base]["max_ms"] - res[base]["min_ms"]
        return {"baseline": base, "form": form, "difference_ms": round(d, 3), "baseline_spread_ms": round(spread, 3),
                "reading": "none (inside the spread of the baseline runs)" if abs(d) <= spread else ("slower" if d > 0 else "faster")}
    out = {"what": "cost of network mode at the boundary (tools/bench_networks.py)", "proofs_per_call": N, "reps": args.reps, "poseidon_constants": L.poseidon_params_name(),
           "forms_ms": res,
           "comparisons": {"a_lone_call_of_one_network": compare("a_single_pair", "a_network_mode"),
                           "b_mixed_call_against_two_calls": compare("b_two_single_pair_calls", "b_one_mixed_call"),
                           "c_two_concurrent_single_proof_callers": compare("c_same_network", "c_different_networks")}}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps(out["comparisons"], indent=1))


if __name__ == "__main__":
    main()
