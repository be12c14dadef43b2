#!/usr/bin/env python3
"""What the batch form of the Proof-of-State check masks (mina_verify_state_checks_batch) costs and saves: one call on n full-size pairs (the committed k = 15
statements of tests/golden/statement_k15.json with their 17 protocol states, as tests/test_state_checks_gpu.py builds them), clean and with two bad openings,
against
  * a loop of mina_verify_state_checks over the same pairs (three synchronous jobs per proof: what an operator has without the batch form), timed on
    min(n, --loop-pairs) pairs and scaled to n -- the loop's cost per pair does not depend on n;
  * mina_verify_state_batch of the same build on the same pairs (one verdict byte per proof): the price of the masks over plain verdicts.

A host clock around each call (every one of them ends in a synchronisation); the three forms alternate in ONE process, `--warmup` untimed and `--reps` timed
rounds; medians, every run, and the socket power / shader clock sampled during the timed rounds (bench.py's PowerSampler) are written.

    python tools/bench_checks.py [--sizes 64,1024] [--reps 5] [--out profiles/state_checks.json]
"""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def make_pairs():
    """the three committed statements as (good proof, proof with a bad opening, pub)"""
    import state_pack_helpers as H
    from ipa_helpers import poseidon_pp
    from kimchi_helpers import load_statement_fixture, make_chain
    from oracle import mina_state_ref as S
    from wire_writers import state_pub_bytes, wrap_proof_bytes
    items, _ = load_statement_fixture()
    proof_bytes = lambda wrap, states: wrap_proof_bytes(wrap, binprot=False) + b"".join(H.bincode_state(s) for s in states)
    out = []
    for it in items[:3]:
        states, hashes = make_chain(random.Random(it["chain_seed"]), poseidon_pp(0))
        p, ev = it["proof"], it["proof"]["evals"]
        wrap = dict(it["wrap"])
        wrap.update(w_comm=p["w_comm"], z_comm=p["z_comm"], t_comm=p["t_comm"], z_eval=ev[0], selector_eval=ev[1:7], w_eval=ev[7:22], coefficients_eval=ev[22:37],
                    s_eval=ev[37:43], ft_eval1=p["ft_eval1"], lr=p["opening"]["lr"], z1=p["opening"]["z1"], z2=p["opening"]["z2"], delta=p["opening"]["delta"], sg=p["opening"]["sg"])
        bad = dict(wrap); bad["z2"] = (wrap["z2"] + 1) % (1 << 254)
        out.append((proof_bytes(wrap, states), proof_bytes(bad, states), state_pub_bytes(True, hashes[16], hashes[:16], [S.snarked_ledger_hash(s) for s in states[:16]])))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,1024")
    ap.add_argument("--loop-pairs", type=int, default=64, help="pairs the single-proof loop is timed on (scaled to n)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "state_checks.json"))
    args = ap.parse_args()
    import torch                                                   # first: its bundled HIP runtime initialises before the library's
    torch.cuda.is_available()
    import mina_bridge_amd as m
    import bench
    from kimchi_helpers import install_index, install_step_index, load_k15_fixture, make_step_index
    L = m.lib
    base = make_pairs()
    L.verify_configure(L.VERIFY_ALLOW_SURROGATE)
    gctx = L.verify_global_ctx()
    install_index(gctx, load_k15_fixture()[0])
    install_step_index(gctx, make_step_index(99))
    result = {"commit": subprocess.run(["git", "-C", ROOT, "describe", "--always", "--dirty"], capture_output=True, text=True).stdout.strip() or "unknown",
              "device": torch.cuda.get_device_name(0) if torch.cuda.is_available() else "unknown", "warmup": args.warmup, "reps": args.reps,
              "method": "host clock around each call; checks_batch / single-proof loop / verify_state_batch alternate in one process; medians over reps, every run listed; "
                        "the loop is timed on loop_pairs pairs and scaled to n", "configs": {}}
    ALL = 63
    sampler = bench.PowerSampler().start()
    try:
        for n in [int(x) for x in args.sizes.split(",")]:
            for name, culprits in (("clean", set()), ("two_bad_openings", {n // 3, 2 * n // 3})):
                proofs = [base[i % 3][1 if i in culprits else 0] for i in range(n)]
                pubs = [base[i % 3][2] for i in range(n)]
                want = [(ALL & ~32 if i in culprits else ALL, ALL) for i in range(n)]
                nl = min(n, args.loop_pairs)
                runs = {"checks_batch": [], "checks_loop": [], "verify_batch": []}
                for rep in range(args.warmup + args.reps):
                    s0 = gctx.checks_stats()
                    t0 = time.perf_counter(); passed, ran = L.verify_state_checks_batch(proofs, pubs); t_batch = (time.perf_counter() - t0) * 1e3
                    s1 = gctx.checks_stats()
                    assert list(zip(passed.tolist(), ran.tolist())) == want and s1["jobs"] - s0["jobs"] == 1, (n, name)
                    t0 = time.perf_counter(); single = [tuple(L.verify_state_checks(p, q)) for p, q in zip(proofs[:nl], pubs[:nl])]; t_loop = (time.perf_counter() - t0) * 1e3 * n / nl
                    assert single == want[:nl], (n, name)
                    with L.tuning(merge=0):
                        t0 = time.perf_counter(); v = L.verify_state_batch(proofs, pubs); t_verdicts = (time.perf_counter() - t0) * 1e3
                    assert v.tolist() == [int(p == r) for p, r in want], (n, name)
                    if rep >= args.warmup:
                        runs["checks_batch"].append(t_batch); runs["checks_loop"].append(t_loop); runs["verify_batch"].append(t_verdicts)
                med = {k: statistics.median(v) for k, v in runs.items()}
                cfg = {"pairs": n, "culprits": len(culprits), "loop_pairs_timed": nl, "ms_checks_batch": med["checks_batch"], "ms_checks_loop_scaled": med["checks_loop"],
                       "ms_verify_batch": med["verify_batch"], "loop_over_batch": med["checks_loop"] / med["checks_batch"], "masks_over_verdicts": med["checks_batch"] / med["verify_batch"],
                       "ms_per_pair_loop": med["checks_loop"] / n, "runs_ms": runs}
                result["configs"][f"{name}_{n}"] = cfg
                print(f"{name}_{n}", json.dumps({k: v for k, v in cfg.items() if k != "runs_ms"}), flush=True)
    finally:
        result["clock"] = sampler.stop()
        L.verify_configure(0)
        L.verify_shutdown()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
