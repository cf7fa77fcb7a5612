#!/usr/bin/env python3
"""Time egs_dense_iterate_batch (sparse::{GaussSeidel,SOR}Iteration on explicit matrices, many systems per call) against
its two yardsticks: a loop of egs_dense_iterate single calls over the same systems, and the CPU restatement
(oracle/dense_iter.c built with the reference's flags, one thread).

usage: gpu_time_dense_iterate_batch.py [--part batch,loop,oracle] [--lib PATH] [--runs 20] [--oracle-runs 5]
                                       [--cases NAME,...] [--out DIR]

  --part   which of the three legs to run (default: all three)
  --lib    the library the LOOP leg (and only it) loads.  The single entry is older than the batch, so the honest
           loop is that of the commit before the batch existed: build that commit's libeggshell_amd.so somewhere and
           run `--part loop --lib that/libeggshell_amd.so` as a process of its own; without --lib the loop runs on
           this build's single entry
  --out    directory for <leg>.json (default profiles/dense_iter_batch)

Systems: the recipe of tests/test_gpu_dense_iter_batch.py (A = m' m + (0.5 sqrt(n) + 1) I, mixed rows, box
[-0.05, 0.08]), tol 1e-9, at most 500 sweeps, Gauss-Seidel and SOR.  Medians over `runs` repetitions after 2 warm-up
calls; batch_ms is the packed call end to end, batch_kernel_ms is egs_kernel_time (events round the launches).
Prints one JSON line per case and method."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from eggshell_amd import capi  # noqa: E402

CASES = [("2048x24", 2048, 24), ("256x96", 256, 96), ("16x24", 16, 24), ("8x512", 8, 512), ("1x24", 1, 24), ("1x96", 1, 96)]
METHODS = (("gs", capi.GAUSS_SEIDEL), ("sor", capi.SOR))


def system(seed, n):
    rng = np.random.default_rng(seed)
    m = rng.uniform(-1, 1, (n, n))
    A = m.T @ m + (0.5 * n ** 0.5 + 1.0) * np.eye(n)
    return A, rng.uniform(-1, 1, n), rng.integers(0, 2, n).astype(np.uint8), np.full(n, -0.05), np.full(n, 0.08)


def median_seconds(fn, runs, warm=2):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="batch,loop,oracle")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--oracle-runs", type=int, default=5)
    ap.add_argument("--cases", default=",".join(c[0] for c in CASES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_iter_batch"))
    args = ap.parse_args()
    parts = args.part.split(",")
    if args.lib:
        if parts != ["loop"]:
            sys.exit("--lib goes with --part loop alone")
        capi.LIB_PATH = os.path.abspath(args.lib)
    ctx = capi.Context(0) if ("batch" in parts or "loop" in parts) else None
    rows = {p: [] for p in parts}
    for name, count, n in CASES:
        if name not in args.cases.split(","):
            continue
        probs = [system(9000 + k, n) for k in range(count)]
        for mname, method in METHODS:
            prm = capi.params(method=method, max_iters=500, tol=1e-9)
            base = {"case": name, "count": count, "n": n, "method": mname}
            if "batch" in parts:
                ns = np.full(count, n, np.int32)
                A, b, C, lo, hi = (np.concatenate([p[i].reshape(-1) for p in probs]) for i in range(5))
                x, it, res = ctx.dense_iterate_batch_packed(ns, A, b, prm, C, lo, hi)
                t = median_seconds(lambda: ctx.dense_iterate_batch_packed(ns, A, b, prm, C, lo, hi), args.runs)
                ctx.kernel_time(reset=True)
                k = []
                for _ in range(args.runs):
                    ctx.dense_iterate_batch_packed(ns, A, b, prm, C, lo, hi)
                    k.append(ctx.kernel_time(reset=True)[0])
                row = dict(base, runs=args.runs, batch_ms=t * 1e3, batch_kernel_ms=float(np.median(k)), systems_per_s=count / t,
                           sweeps_min=int(it.min()), sweeps_max=int(it.max()), residual_max=float(res.max()))
                print(json.dumps(row), flush=True)
                rows["batch"].append(row)
            if "loop" in parts:
                t = median_seconds(lambda: [ctx.dense_iterate(p[0], p[1], prm, p[2], p[3], p[4]) for p in probs], args.runs)
                row = dict(base, runs=args.runs, single_loop_ms=t * 1e3, systems_per_s=count / t, library=capi.LIB_PATH if args.lib else "this build")
                print(json.dumps(row), flush=True)
                rows["loop"].append(row)
            if "oracle" in parts:
                from oracle import oracle as orc
                with orc.timing_build() as flags:
                    t = median_seconds(lambda: [orc.dense_iterate(p[0], p[1], method, p[2], p[3], p[4], max_iters=500) for p in probs],
                                       args.oracle_runs, warm=1)
                row = dict(base, runs=args.oracle_runs, cpu_ms=t * 1e3, systems_per_s=count / t, cpu_flags=flags)
                print(json.dumps(row), flush=True)
                rows["oracle"].append(row)
    if ctx:
        ctx.close()
    os.makedirs(args.out, exist_ok=True)
    for p in parts:
        with open(os.path.join(args.out, p + ".json"), "w") as f:
            json.dump({"tool": "gpu_time_dense_iterate_batch", "leg": p, "rows": rows[p]}, f, indent=1)


if __name__ == "__main__":
    main()
