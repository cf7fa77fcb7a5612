#!/usr/bin/env python3
"""Time egs_mixed_constraints_solve_batch (Lcp::MixedConstraintsSolver on many explicit problems per call) against its
two yardsticks: a loop of egs_mixed_constraints_solve single calls over the same problems, and the CPU restatement
(oracle/lcp_dense.c built with the reference's flags, one thread).

usage: gpu_time_mixed_batch.py [--part batch,loop,oracle] [--lib PATH] [--runs 20] [--oracle-runs 20]
                               [--cases NAME,...] [--out DIR]

  --part   which of the three legs to run (default: all three)
  --lib    the library the LOOP leg (and only it) loads.  The batch leaves the single entry's path as it was, so the
           loop of this build is the loop of the commit before it; to time that commit's own library all the same, build
           it somewhere and run `--part loop --lib that/libeggshell_amd.so` as a process of its own
  --out    directory for <leg>.json (default profiles/mixed_batch)

Problems: A = GenerateSPDMatrix (utils.cc:203-215: M' M, cond < 1e7; the `_spd` of tests/test_oracle_lcp.py), b in
U(-1, 1), C ~ Bernoulli(1/2), use_bounds = 0, from default_rng(4000 + case).  Medians over `runs` repetitions after 2
warm-up calls; batch_ms is the packed call end to end, batch_kernel_ms is egs_kernel_time (events round the launches).
Prints one JSON line per case and leg."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from eggshell_amd import capi  # noqa: E402

CASES = [("2048x24", 2048, 24), ("256x96", 256, 96), ("100x50", 100, 50), ("16x24", 16, 24), ("1x24", 1, 24), ("1x96", 1, 96)]


def spd(rng, dim):
    while True:
        M = rng.uniform(-1, 1, (dim, dim))
        A = M.T @ M
        if np.linalg.cond(A) < 1e7:
            return A


def problem(rng, n):
    A = spd(rng, n)
    return A, rng.uniform(-1, 1, n), rng.integers(0, 2, n).astype(np.uint8), np.zeros(n), np.full(n, np.inf)


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
    ap.add_argument("--oracle-runs", type=int, default=20)
    ap.add_argument("--cases", default=",".join(c[0] for c in CASES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixed_batch"))
    args = ap.parse_args()
    parts = args.part.split(",")
    if args.lib:
        if parts != ["loop"]:
            sys.exit("--lib goes with --part loop alone")
        capi.LIB_PATH = os.path.abspath(args.lib)
    ctx = capi.Context(0) if ("batch" in parts or "loop" in parts) else None
    rows = {p: [] for p in parts}
    for ci, (name, count, n) in enumerate(CASES):
        if name not in args.cases.split(","):
            continue
        rng = np.random.default_rng(4000 + ci)
        probs = [problem(rng, n) for _ in range(count)]
        base = {"case": name, "count": count, "n": n}
        if "batch" in parts:
            ns = np.full(count, n, np.int32)
            A, b, C, lo, hi = (np.concatenate([p[i].reshape(-1) for p in probs]) for i in range(5))
            ok, x, w, piv = ctx.mixed_constraints_solve_batch_packed(ns, A, b, C, lo, hi)
            t = median_seconds(lambda: ctx.mixed_constraints_solve_batch_packed(ns, A, b, C, lo, hi), args.runs)
            ctx.kernel_time(reset=True)
            k = []
            for _ in range(args.runs):
                ctx.mixed_constraints_solve_batch_packed(ns, A, b, C, lo, hi)
                k.append(ctx.kernel_time(reset=True)[0])
            row = dict(base, runs=args.runs, batch_ms=t * 1e3, batch_kernel_ms=float(np.median(k)), problems_per_s=count / t,
                       ok=int(ok.sum()), pivots_min=int(piv.min()), pivots_max=int(piv.max()))
            print(json.dumps(row), flush=True)
            rows["batch"].append(row)
        if "loop" in parts:
            t = median_seconds(lambda: [ctx.mixed_constraints_solve(*p) for p in probs], args.runs)
            row = dict(base, runs=args.runs, single_loop_ms=t * 1e3, problems_per_s=count / t, library=capi.LIB_PATH if args.lib else "this build")
            print(json.dumps(row), flush=True)
            rows["loop"].append(row)
        if "oracle" in parts:
            from oracle import oracle as orc
            with orc.timing_build() as flags:
                t = median_seconds(lambda: [orc.mixed_constraints(*p) for p in probs], args.oracle_runs, warm=1)
            row = dict(base, runs=args.oracle_runs, cpu_ms=t * 1e3, problems_per_s=count / t, cpu_flags=flags)
            print(json.dumps(row), flush=True)
            rows["oracle"].append(row)
    if ctx:
        ctx.close()
    os.makedirs(args.out, exist_ok=True)
    for p in parts:
        with open(os.path.join(args.out, p + ".json"), "w") as f:
            json.dump({"tool": "gpu_time_mixed_batch", "leg": p, "rows": rows[p]}, f, indent=1)


if __name__ == "__main__":
    main()
