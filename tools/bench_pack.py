#!/usr/bin/env python3
"""What MINA_VERIFY_PACK_ON_DEVICE (the protocol states of a chunk flattened and pre-checked on the GPU, mina_state_frontend_dev) costs and saves.  Measured,
not gated: the mode is opt-in whatever comes out, and the numbers go into README.md / DESIGN.md / INTEGRATION.md as they are.

  (a) the front-end kernels alone on 8192 x 17 serialized states in HBM (HIP events on the context's pinned lane), beside the time the boundary's host pool takes
      for the same states in a flag-off call (its own MINA_VERIFY_TIMING trace: "states parsed" minus "wrap proofs parsed", read from a child process);
  (b) the boundary's rate with the flag off and on: the same process, the same proofs, calls interleaved off / on, medians of `--reps` with every run listed and
      the sampled shader clock beside them; a lone 8192-proof call, then 2 and 4 caller threads.  "Off" on the same build is the yardstick and its own spread the
      margin: a gain inside it is reported as none;
  (c) one call per mode for a kernel trace, in a run of its own and without counters:
          rocprofv3 --kernel-trace --stats -d OUT -- python tools/bench_pack.py --one-call off|on

    python tools/bench_pack.py [--size 8192] [--reps 3] [--out profiles/pack_on_device.json]

The proofs are the committed byte fixtures (tests/golden/state_proofs_k15_bytes.json) repeated; a process gets 16 CPUs on the measuring box ($MINA_HOST_THREADS
sizes the pool)."""
import argparse
import ctypes
import json
import os
import re
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


def setup(size):
    import mina_bridge_amd as m
    from mina_bridge_amd import lib as L
    from kimchi_helpers import install_index, install_step_index, load_k15_fixture, make_step_index
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "state_proofs_k15_bytes.json")))
    ix, _, _ = load_k15_fixture()
    base = m.lib.VERIFY_ALLOW_SURROGATE
    m.lib.verify_configure(base)
    gctx = m.lib.verify_global_ctx()
    install_index(gctx, ix); install_step_index(gctx, make_step_index(99))
    proofs = [bytes.fromhex(p["proof"]) for p in fx["proofs"]]; pubs = [bytes.fromhex(p["pub"]) for p in fx["proofs"]]
    P = [proofs[i % len(proofs)] for i in range(size)]; Q = [pubs[i % len(pubs)] for i in range(size)]
    return m, L, base, P, Q


class Caller:
    """one caller's arguments of mina_verify_state_batch, built once"""
    def __init__(self, L, P, Q):
        self.n = len(P); self.keep = (L._ptr_arrays(P), L._ptr_arrays(Q)); self.out = np.zeros(self.n, np.uint8); self.lib = L.load_library(); self.L = L
    def __call__(self):
        (_, PP, PL), (_, QQ, QL) = self.keep
        rc = self.lib.mina_verify_state_batch(ctypes.c_size_t(self.n), PP, PL, QQ, QL, self.L._p(self.out))
        assert rc == 0 and self.out.all(), "every fixture proof must verify"


def rate(callers, calls_each):
    """proofs per second of `callers` threads making `calls_each` calls each"""
    th = [threading.Thread(target=lambda c=c: [c() for _ in range(calls_each)]) for c in callers]
    t0 = time.perf_counter()
    for t in th: t.start()
    for t in th: t.join()
    dt = time.perf_counter() - t0
    return sum(c.n for c in callers) * calls_each / dt, dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--calls", type=int, default=4, help="calls per caller thread and run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pack_on_device.json"))
    ap.add_argument("--one-call", choices=("off", "on"), help="(c): warm up, then ONE call in this mode, for a profiler")
    ap.add_argument("--timing-probe", action="store_true", help="(a), child process: one warm flag-off call under MINA_VERIFY_TIMING")
    args = ap.parse_args()
    m, L, base, P, Q = setup(args.size)
    on = base | m.lib.VERIFY_PACK_ON_DEVICE
    lone = Caller(L, P, Q)
    if args.timing_probe:
        for _ in range(3): lone()
        sys.stderr.write("PROBE-BEGIN\n"); lone(); sys.stderr.write("PROBE-END\n")
        return
    if args.one_call:
        flags = on if args.one_call == "on" else base
        m.lib.verify_configure(flags)
        for _ in range(2): lone()
        lone()
        return
    import torch
    import bench
    try:
        pr_ = torch.cuda.get_device_properties(0)
        bdf = "%04x:%02x:%02x.0" % (getattr(pr_, "pci_domain_id", 0), pr_.pci_bus_id, pr_.pci_device_id)
    except Exception:
        bdf = None
    result = {"commit": subprocess.run(["git", "-C", ROOT, "describe", "--always", "--dirty"], capture_output=True, text=True).stdout.strip() or "unknown",
              "device": torch.cuda.get_device_name(0), "proofs_per_call": args.size, "reps": args.reps, "calls_per_run": args.calls, "host_threads": os.environ["MINA_HOST_THREADS"],
              "method": "flag off / on interleaved in one process on the same proofs; medians over reps, every run listed; a gain inside the spread of `off` is reported as none"}

    # ---- (a) the front-end kernels alone
    ctx = m.MinaContext(0)
    uniq = list(dict.fromkeys(P))
    st_at = {p: L.state_proof_split(p)[1][0] for p in uniq}
    blob = bytearray(); begin, end = [], []
    for p in P:
        begin.append(len(blob)); blob.extend(p[st_at[p]:]); end.append(len(blob))
    B = args.size
    exp = b"".join(q[33:545] + q[1:33] for q in Q); led = b"".join(q[545:1057] for q in Q)
    dev = torch.device("cuda", 0)
    t8 = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    d_blob, d_exp, d_led = t8(blob), t8(exp), t8(led)
    d_b = torch.tensor(begin, dtype=torch.int64, device=dev); d_e = torch.tensor(end, dtype=torch.int64, device=dev)
    d_rec = torch.zeros(B * 17 * 2048, dtype=torch.uint8, device=dev); d_nf = torch.zeros(B * 17, dtype=torch.int32, device=dev)
    d_pre = torch.zeros(B, dtype=torch.uint8, device=dev); d_m = torch.zeros(B, dtype=torch.int32, device=dev)
    ctx.pin_lane(0)
    ext = torch.cuda.ExternalStream(ctx.stream)
    torch.cuda.synchronize()
    times = []
    for _ in range(10):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(ext):
            e0.record()
            ctx.state_frontend_dev(B, d_blob.data_ptr(), len(blob), d_b.data_ptr(), d_e.data_ptr(), d_exp.data_ptr(), d_led.data_ptr(), 0, d_rec.data_ptr(), d_nf.data_ptr(), d_pre.data_ptr(), d_m.data_ptr())
            e1.record()
        ctx.synchronize(); torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    assert d_pre.cpu().numpy().all() and (d_m.cpu().numpy() == 11).all(), "every fixture proof passes FORMAT, LEDGER and CONSENSUS"
    ctx.pin_lane(-1); ctx.close()
    kern_ms = statistics.median(times[2:])
    probe = subprocess.run([sys.executable, os.path.abspath(__file__), "--timing-probe", "--size", str(args.size)], capture_output=True, text=True, env=dict(os.environ, MINA_VERIFY_TIMING="1"))
    seg = probe.stderr.split("PROBE-BEGIN")[-1].split("PROBE-END")[0]
    mt = re.search(r"wrap proofs parsed at ([\d.]+) ms, legs queued at ([\d.]+), states parsed at ([\d.]+)", seg)
    host_ms = (float(mt.group(3)) - float(mt.group(1))) if mt else None
    result["frontend"] = {"states": B * 17, "state_bytes": len(blob), "kernels_ms_median": kern_ms, "kernels_ms_runs": times, "read_gb_per_s": len(blob) / kern_ms / 1e6,
                          "host_pool_ms": host_ms, "host_pool_trace": seg.strip().splitlines()[:4],
                          "note": "host_pool_ms = `states parsed` - `wrap proofs parsed` of one warm flag-off call (the pool's job B beside the chunk's uploads); kernels: split + pack + precheck + clear"}
    print("frontend", json.dumps({k: v for k, v in result["frontend"].items() if k not in ("kernels_ms_runs", "host_pool_trace")}), flush=True)

    # ---- (b) the boundary's rate, flag off against flag on
    result["boundary"] = {}
    for ncallers in (1, 2, 4):
        callers = [Caller(L, P, Q) for _ in range(ncallers)]
        for flags in (base, on):                               # warm both paths (slots, pinned staging, workspaces)
            m.lib.verify_configure(flags); rate(callers, 2)
        runs = {"off": [], "on": []}
        for _ in range(args.reps):
            for mode, flags in (("off", base), ("on", on)):
                m.lib.verify_configure(flags)
                sampler = bench.PowerSampler(bdf, interval=0.05); sampler.start()
                r, dt = rate(callers, args.calls)
                pw = sampler.stop()
                runs[mode].append({"proofs_per_s": r, "seconds": dt, "sclk_mhz_avg": pw and pw.get("sclk_mhz_avg")})
        med = {k: statistics.median(x["proofs_per_s"] for x in v) for k, v in runs.items()}
        spread = (max(x["proofs_per_s"] for x in runs["off"]) - min(x["proofs_per_s"] for x in runs["off"])) / med["off"]
        gain = med["on"] / med["off"] - 1
        result["boundary"][f"{ncallers}_callers"] = {"proofs_per_s_off": med["off"], "proofs_per_s_on": med["on"], "on_over_off": med["on"] / med["off"], "off_spread": spread,
                                                     "verdict": "none" if abs(gain) <= max(spread, 0.03) else ("gain" if gain > 0 else "loss"), "runs": runs}
        print(f"{ncallers} caller(s)", json.dumps({k: v for k, v in result["boundary"][f"{ncallers}_callers"].items() if k != "runs"}), flush=True)
    m.lib.verify_configure(0); m.lib.verify_shutdown()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
