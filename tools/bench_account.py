#!/usr/bin/env python3
"""What MINA_VERIFY_ACCOUNT_ON_DEVICE (a Proof-of-Account call parsed, cross-checked, hashed, folded and compared on the GPU, mina_account_job_dev) costs and saves.
Measured, not gated: the mode is opt-in whatever comes out, and the numbers go into README.md / DESIGN.md / INTEGRATION.md as they are.

  (a) mina_account_job_dev alone on resident bytes (HIP events on the context's pinned lane): 256 and 16 384 pairs of the fixture mix, 256 all-plain, 256 all-zkApp;
  (b) the boundary (mina_verify_account_batch) with the flag off and on: the same process, the same pairs, calls interleaved off / on, medians of `--reps` with every
      run listed and the sampled shader clock beside them -- a lone 256-pair call (BASELINE C4's shape) with all-plain and with all-zkApp accounts, a lone
      16 384-pair call, 16 caller threads of 256 pairs.  "Off" on the same build is the yardstick and its own spread the margin: a gain inside it is reported as none;
  (c) one call per mode for a kernel trace, in a run of its own and without counters:
          rocprofv3 --kernel-trace --stats -d OUT -- python tools/bench_account.py --one-call off|on [--size 256]

    python tools/bench_account.py [--reps 3] [--out profiles/account_on_device.json]

The pairs are the committed byte fixture (tests/golden/account_proofs_bytes.json: 256 distinct depth-35 pairs, every other one with a zkApp) repeated; a process gets
16 CPUs on the measuring box ($MINA_HOST_THREADS sizes the pool)."""
import argparse
import base64
import ctypes
import json
import os
import statistics
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
os.environ.setdefault("MINA_HOST_THREADS", "16")

import numpy as np  # noqa: E402


def fixture():
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "account_proofs_bytes.json")))
    pairs = [(base64.b64decode(p["proof"]), base64.b64decode(p["pub"])) for p in fx["proofs"]]
    zk = [pairs[i] for i in range(len(pairs)) if i % 4 in (1, 2)]; plain = [pairs[i] for i in range(len(pairs)) if i % 4 in (0, 3)]      # tests/golden/gen_account_fixture.py SHAPES
    return pairs, plain, zk


def take(pairs, n):
    return [pairs[i % len(pairs)] for i in range(n)]


class Caller:
    """one caller's arguments of mina_verify_account_batch, built once"""
    def __init__(self, L, pairs):
        self.n = len(pairs); self.keep = (L._ptr_arrays([p for p, _ in pairs]), L._ptr_arrays([q for _, q in pairs])); self.out = np.zeros(self.n, np.uint8)
        self.lib = L.load_library(); self.L = L
    def __call__(self):
        (_, PP, PL), (_, QQ, QL) = self.keep
        rc = self.lib.mina_verify_account_batch(ctypes.c_size_t(self.n), PP, PL, QQ, QL, self.L._p(self.out))
        assert rc == 0 and self.out.all(), "every fixture pair must verify"


def run(callers, calls_each):
    """-> pairs per second and milliseconds per call of `callers` threads making `calls_each` calls each"""
    th = [threading.Thread(target=lambda c=c: [c() for _ in range(calls_each)]) for c in callers]
    t0 = time.perf_counter()
    for t in th: t.start()
    for t in th: t.join()
    dt = time.perf_counter() - t0
    return sum(c.n for c in callers) * calls_each / dt, 1e3 * dt / calls_each


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20, help="calls per caller thread and run")
    ap.add_argument("--size", type=int, default=256, help="--one-call: pairs in the call")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "account_on_device.json"))
    ap.add_argument("--one-call", choices=("off", "on"), help="(c): warm up, then ONE call in this mode, for a profiler")
    args = ap.parse_args()
    import torch                       # PyTorch-ROCm bundles its HIP runtime: it initialises first when it shares the process
    torch.cuda.is_available()
    import mina_bridge_amd as m
    from mina_bridge_amd import lib as L
    pairs, plain, zk = fixture()
    base = m.lib.VERIFY_ALLOW_SURROGATE
    on = base | m.lib.VERIFY_ACCOUNT_ON_DEVICE
    if args.one_call:
        m.lib.verify_configure(on if args.one_call == "on" else base)
        c = Caller(L, take(pairs, args.size))
        for _ in range(3): c()
        c()
        return
    import bench
    try:
        pr_ = torch.cuda.get_device_properties(0)
        bdf = "%04x:%02x:%02x.0" % (getattr(pr_, "pci_domain_id", 0), pr_.pci_bus_id, pr_.pci_device_id)
    except Exception:
        bdf = None
    result = {"commit": subprocess.run(["git", "-C", ROOT, "describe", "--always", "--dirty"], capture_output=True, text=True).stdout.strip() or "unknown",
              "device": torch.cuda.get_device_name(0), "reps": args.reps, "calls_per_run": args.calls, "host_threads": os.environ["MINA_HOST_THREADS"],
              "method": "flag off / on interleaved in one process on the same pairs; medians over reps, every run listed; a gain inside the spread of `off` is reported as none"}

    # ---- (a) the job alone on resident bytes
    ctx = m.MinaContext(0)
    for f in (0, 1): ctx.poseidon_set_params(f, m.poseidon_params.default_params_bytes(f))
    ctx.pin_lane(0)
    ext = torch.cuda.ExternalStream(ctx.stream)
    dev = torch.device("cuda", 0)
    result["job_dev"] = {}
    for name, ps in (("256_fixture_mix", take(pairs, 256)), ("256_all_plain", take(plain, 256)), ("256_all_zkapp", take(zk, 256)), ("16384_fixture_mix", take(pairs, 16384))):
        blob = bytearray(); cols = [[], [], [], []]
        for p, q in ps:
            for j, b in enumerate((p, q)): cols[2 * j].append(len(blob)); cols[2 * j + 1].append(len(b)); blob.extend(b)
        n = len(ps)
        d_blob = torch.frombuffer(blob, dtype=torch.uint8).to(dev)
        d_cols = [torch.tensor(c, dtype=torch.int64, device=dev) for c in cols]
        d_p = torch.zeros(n, dtype=torch.int32, device=dev); d_r = torch.zeros(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        times = []
        for _ in range(12):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(ext):
                e0.record()
                ctx.account_job_dev(n, d_blob.data_ptr(), len(blob), *[c.data_ptr() for c in d_cols], d_p.data_ptr(), d_r.data_ptr())
                e1.record()
            ctx.synchronize(); torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        assert (d_p.cpu().numpy() == 193).all() and (d_r.cpu().numpy() == 193).all(), "every fixture pair passes FORMAT, ACCOUNT_ABI and MERKLE"
        med = statistics.median(times[2:])
        result["job_dev"][name] = {"pairs": n, "bytes": len(blob), "ms_median": med, "ms_runs": times, "pairs_per_s": n / med * 1e3}
        print("job_dev", name, json.dumps({k: v for k, v in result["job_dev"][name].items() if k != "ms_runs"}), flush=True)
    ctx.pin_lane(-1); ctx.close()

    # ---- (b) the boundary, flag off against flag on
    m.lib.verify_configure(base)
    result["boundary"] = {}
    for name, make, calls in (("lone_256_all_plain", lambda: [Caller(L, take(plain, 256))], args.calls), ("lone_256_all_zkapp", lambda: [Caller(L, take(zk, 256))], args.calls),
                              ("lone_16384_fixture_mix", lambda: [Caller(L, take(pairs, 16384))], max(2, args.calls // 5)),
                              ("16_callers_256_fixture_mix", lambda: [Caller(L, take(pairs[16 * t:] + pairs[:16 * t], 256)) for t in range(16)], args.calls)):
        callers = make()
        for flags in (base, on):                               # warm both paths (lane, pinned staging, workspaces, salts)
            m.lib.verify_configure(flags); run(callers, 2)
        runs = {"off": [], "on": []}
        for _ in range(args.reps):
            for mode, flags in (("off", base), ("on", on)):
                m.lib.verify_configure(flags)
                sampler = bench.PowerSampler(bdf, interval=0.05); sampler.start()
                r, ms = run(callers, calls)
                pw = sampler.stop()
                runs[mode].append({"pairs_per_s": r, "ms_per_call": ms, "sclk_mhz_avg": pw and pw.get("sclk_mhz_avg")})
        med = {k: statistics.median(x["pairs_per_s"] for x in v) for k, v in runs.items()}
        med_ms = {k: statistics.median(x["ms_per_call"] for x in v) for k, v in runs.items()}
        spread = (max(x["pairs_per_s"] for x in runs["off"]) - min(x["pairs_per_s"] for x in runs["off"])) / med["off"]
        gain = med["on"] / med["off"] - 1
        result["boundary"][name] = {"pairs_per_s_off": med["off"], "pairs_per_s_on": med["on"], "ms_per_call_off": med_ms["off"], "ms_per_call_on": med_ms["on"],
                                    "on_over_off": med["on"] / med["off"], "off_spread": spread,
                                    "verdict": "none" if abs(gain) <= max(spread, 0.03) else ("gain" if gain > 0 else "loss"), "runs": runs}
        print(name, json.dumps({k: v for k, v in result["boundary"][name].items() if k != "runs"}), flush=True)
    m.lib.verify_configure(0); m.lib.verify_shutdown()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
