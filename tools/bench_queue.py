#!/usr/bin/env python3
"""The completion queue (`mina_verify_queue_*`) against the two call shapes it sits between, on the full-size proofs of bench.py's `one_proof_per_call` leg, in ONE
process of its own (a process that has once held many streams stays slower: DESIGN.md), the forms alternating, medians of `--reps`:

  (a) N synchronous caller threads, one `mina_verify_state` call each  -- the reference's call shape, one blocked OS thread per proof in flight
  (b) ONE submitting thread and ONE waiting thread on a queue of capacity N, for workers in {1, 2} x mina_verify_tuning.max_jobs in {1, 2}
  (c) one `mina_verify_state_batch` call of N                           -- the ceiling
  (b, burst) as (b) with workers = max_jobs = 1 and MINA_SUBMIT_MORE on every submission but the last: a caller that knows its burst

for N = 64, 1024 and 8192 proofs in flight, and the same three forms for Proof-of-Account at N = 256.  Per form: proofs/s, mean and p99 time from a proof's hand-over
(the start of the call / `submit`) to its verdict, and for (b) the queue's `jobs` / `max_job`.  Callers are pthreads of a small C helper: no interpreter lock between
a verdict and the next call.  Writes the table as JSON (default profiles/verify_queue.json).

    python tools/bench_queue.py [--out PATH] [--reps 5] [--device 0]
"""
import argparse
import base64
import ctypes
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HELPER_C = r"""
#include <pthread.h>
#include <stdlib.h>
#include <time.h>
#include "mina_verify.h"
static double now(void) { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec + 1e-9 * t.tv_nsec; }
struct cases { int kind, ncases; const uint8_t *const *proofs; const size_t *pl; const uint8_t *const *pubs; const size_t *ql; };
/* (a) n threads, one call each, released together; lat[i] = the call's length; returns the wall time from the release to the last verdict */
struct sync_job { const struct cases *c; int i; pthread_barrier_t *bar; double t0, t1; int ok; };
static void *sync_worker(void *a) { struct sync_job *j = a; const struct cases *c = j->c; const int k = j->i % c->ncases;
  pthread_barrier_wait(j->bar); j->t0 = now();
  j->ok = c->kind ? mina_verify_account(c->proofs[k], c->pl[k], c->pubs[k], c->ql[k]) : mina_verify_state(c->proofs[k], c->pl[k], c->pubs[k], c->ql[k]);
  j->t1 = now(); return 0; }
double run_sync(const struct cases *c, int n, double *lat, long *bad) {
  pthread_t *th = malloc(sizeof *th * n); struct sync_job *jobs = malloc(sizeof *jobs * n); pthread_barrier_t bar; pthread_attr_t at;
  pthread_barrier_init(&bar, 0, n + 1); pthread_attr_init(&at); pthread_attr_setstacksize(&at, 512 * 1024);
  for (int i = 0; i < n; ++i) { jobs[i] = (struct sync_job){c, i, &bar, 0, 0, 0}; if (pthread_create(&th[i], &at, sync_worker, &jobs[i])) return -1; }
  pthread_barrier_wait(&bar); const double t0 = now(); double t1 = t0;
  for (int i = 0; i < n; ++i) { pthread_join(th[i], 0); lat[i] = jobs[i].t1 - jobs[i].t0; if (jobs[i].t1 > t1) t1 = jobs[i].t1; if (!jobs[i].ok) ++*bad; }
  pthread_barrier_destroy(&bar); pthread_attr_destroy(&at); free(th); free(jobs); return t1 - t0; }
/* (b) one submitting thread, the calling thread waits; lat[i] = submit .. the wait that handed the verdict out */
struct sub_job { mina_verify_queue *q; const struct cases *c; int n; double *t_sub; long full; int burst; };
static void *submitter(void *a) { struct sub_job *j = a; const struct cases *c = j->c;
  for (int i = 0; i < j->n; ++i) { const int k = i % c->ncases; j->t_sub[i] = now();
    while (mina_verify_queue_submit(j->q, (uint32_t)c->kind, c->proofs[k], c->pl[k], c->pubs[k], c->ql[k], (uint64_t)i, j->burst && i + 1 < j->n ? MINA_SUBMIT_MORE : 0) == MINA_ERR_FULL) { ++j->full; sched_yield(); } }
  return 0; }
double run_queue(mina_verify_queue *q, const struct cases *c, int n, int burst, double *lat, long *bad) {
  double *t_sub = malloc(sizeof *t_sub * n); struct sub_job sj = {q, c, n, t_sub, 0, burst}; pthread_t th; mina_verify_completion out[256]; size_t k; int got = 0;
  const double t0 = now(); double t1 = t0;
  if (pthread_create(&th, 0, submitter, &sj)) return -1;
  while (got < n) { if (mina_verify_queue_wait(q, out, 256, &k, -1) != MINA_OK) return -1; t1 = now();
    for (size_t i = 0; i < k; ++i, ++got) { lat[out[i].tag] = t1 - t_sub[out[i].tag]; if (out[i].verdict != 1 || out[i].rc != MINA_OK) ++*bad; } }
  pthread_join(th, 0); free(t_sub); return t1 - t0; }
"""


class Cases(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int), ("ncases", ctypes.c_int), ("proofs", ctypes.c_void_p), ("pl", ctypes.c_void_p), ("pubs", ctypes.c_void_p), ("ql", ctypes.c_void_p)]


def make_cases(kind, items):
    nc = len(items)
    keep = [(ctypes.c_char_p * nc)(*[c[0] for c in items]), (ctypes.c_size_t * nc)(*[len(c[0]) for c in items]),
            (ctypes.c_char_p * nc)(*[c[1] for c in items]), (ctypes.c_size_t * nc)(*[len(c[1]) for c in items])]
    return Cases(kind, nc, *[ctypes.cast(k, ctypes.c_void_p) for k in keep]), keep


def row(n, wall, lat):
    lat = sorted(lat)
    return {"proofs_per_s": n / wall, "wall_ms": wall * 1e3, "mean_ms": 1e3 * sum(lat) / n, "p99_ms": 1e3 * lat[min(n - 1, int(0.99 * n))]}


def median_rows(rows):
    out = {k: statistics.median(r[k] for r in rows) for k in ("proofs_per_s", "wall_ms", "mean_ms", "p99_ms")}
    for k in ("jobs", "max_job"):
        if k in rows[0]:
            out[k] = statistics.median(r[k] for r in rows)
    out["runs"] = len(rows)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_queue.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", default="0")
    ap.add_argument("--sizes", default="64,1024,8192")
    args = ap.parse_args()
    import torch; torch.cuda.is_available()                      # noqa: E702 -- the wheel's runtime initialises first (mina_bridge_amd/lib.py)
    import bench
    import mina_bridge_amd as m
    L = m.lib
    setup = bench._boundary_setup(m, args.device)
    if isinstance(setup, dict):
        print(json.dumps(setup)); return 1
    lib, items, _ = setup
    fxa = json.load(open(os.path.join(ROOT, "tests", "golden", "account_proofs_bytes.json")))
    acct = [(base64.b64decode(p["proof"]), base64.b64decode(p["pub"])) for p in fxa["proofs"][:256]]
    tmp = tempfile.mkdtemp()
    with open(os.path.join(tmp, "queue_helper.c"), "w") as f:
        f.write(HELPER_C)
    libdir = os.path.dirname(m.LIB_PATH)
    subprocess.check_call(["gcc", "-O2", "-D_GNU_SOURCE", "-shared", "-fPIC", "-pthread", "-I", os.path.join(ROOT, "include"), os.path.join(tmp, "queue_helper.c"), "-o",
                           os.path.join(tmp, "libqueue_helper.so"), "-L", libdir, "-lminaverify", "-Wl,-rpath," + libdir])
    H = ctypes.CDLL(os.path.join(tmp, "libqueue_helper.so"))
    H.run_sync.restype = H.run_queue.restype = ctypes.c_double
    H.run_sync.argtypes = [ctypes.POINTER(Cases), ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_long)]
    H.run_queue.argtypes = [ctypes.c_void_p, ctypes.POINTER(Cases), ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_long)]

    def sync_form(cases, n):
        lat = (ctypes.c_double * n)(); bad = ctypes.c_long(0)
        wall = H.run_sync(ctypes.byref(cases), n, lat, ctypes.byref(bad))
        assert wall > 0 and bad.value == 0, (wall, bad.value)
        return row(n, wall, list(lat))

    def queue_form(cases, n, workers, max_jobs, burst=0):
        with L.tuning(max_jobs=max_jobs), L.VerifyQueue(capacity=n, workers=workers) as q:
            lat = (ctypes.c_double * n)(); bad = ctypes.c_long(0)
            wall = H.run_queue(q._h, ctypes.byref(cases), n, burst, lat, ctypes.byref(bad))
            assert wall > 0 and bad.value == 0, (wall, bad.value)
            st = q.stats()
        r = row(n, wall, list(lat)); r["jobs"] = st["jobs"]; r["max_job"] = st["max_job"]
        return r

    def batch_form(kind, its, n):
        P = [its[i % len(its)][0] for i in range(n)]; Q = [its[i % len(its)][1] for i in range(n)]
        t0 = time.perf_counter()
        v = (L.verify_account_batch if kind else L.verify_state_batch)(P, Q)
        wall = time.perf_counter() - t0
        assert int(v.sum()) == n
        return row(n, wall, [wall] * n)

    table = {}
    for kind, name, its, sizes in ((0, "state", items, [int(s) for s in args.sizes.split(",")]), (1, "account", acct, [256])):
        cases, keep = make_cases(kind, its)
        for n in sizes:
            forms = {"a_sync_threads": lambda: sync_form(cases, n), "c_one_batch_call": lambda: batch_form(kind, its, n)}
            for w in (1, 2):
                for mj in (1, 2):
                    forms[f"b_queue_workers{w}_max_jobs{mj}"] = (lambda w=w, mj=mj: queue_form(cases, n, w, mj))
            forms["b_queue_burst_workers1_max_jobs1"] = lambda: queue_form(cases, n, 1, 1, burst=1)
            runs = {k: [] for k in forms}
            for rep in range(args.reps + 1):                         # the first pass warms every form and is dropped
                for k, fn in forms.items():
                    r = fn()
                    if rep:
                        runs[k].append(r)
            table[f"{name}_{n}"] = {k: median_rows(v) for k, v in runs.items()}
            print(name, n, json.dumps(table[f"{name}_{n}"]), flush=True)
    L.verify_shutdown()
    out = {"tool": "tools/bench_queue.py", "reps": args.reps, "proofs": "tests/golden/state_proofs_k15_bytes.json (full size), account_proofs_bytes.json",
           "forms": {"a": "N synchronous caller threads, one proof per call", "b": "one submitting + one waiting thread on a queue of capacity N", "b_burst": "b with MINA_SUBMIT_MORE on all but the last submission", "c": "one batch call of N"},
           "latency": "a: length of the call; b: submit to the wait that hands the verdict out; c: the call", "table": table}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
