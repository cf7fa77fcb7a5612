#!/usr/bin/env python3
"""Time egs_box_lcp_schur_batch (lcp::SolveLCP's default path on many problems, fused for n <= 96) against its two
yardsticks, measured in the same run: a loop of egs_box_lcp_schur single calls over the same problems, and the CPU
port (oracle/lcp_toolkit.c::otk_box_schur built with the reference's flags, one thread).
usage: gpu_time_lcp_schur_batch.py [reps=20] [out.json]; prints one JSON line per workload and a final summary line.
Medians over `reps` repetitions after 3 warm-up calls; kernel-only time is egs_kernel_time (events round the launch)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from eggshell_amd import capi  # noqa: E402
from oracle import oracle as orc  # noqa: E402

BIG = np.finfo(np.float64).max
WORKLOADS = [("2048x24", 2048, 24), ("64x96", 64, 96), ("16x24", 16, 24), ("1x20", 1, 20), ("1x96", 1, 96)]


def problem(rng, n, frac=0.5):
    A0 = rng.uniform(-1, 1, (n, n))
    A = np.tril(A0 @ A0.T + 0.05 * np.eye(n))
    b = rng.uniform(-1, 1, n)
    lo = np.full(n, -BIG); hi = np.full(n, BIG)
    pick = rng.uniform(size=n) < frac
    lo[pick] = -rng.uniform(0.01, 0.3, pick.sum()); hi[pick] = rng.uniform(0.01, 0.3, pick.sum())
    return A, b, lo, hi


def median_seconds(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t))


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    ctx = capi.Context(0)
    rows = []
    for name, count, n in WORKLOADS:
        rng = np.random.default_rng(8)
        probs = [problem(rng, n) for _ in range(count)]
        ns, A, b, lo, hi = capi.pack_lcp_batch(*[[p[i] for p in probs] for i in range(4)])
        res = ctx.box_lcp_schur_batch_packed(ns, A, b, lo, hi)
        row = {"workload": name, "count": count, "n": n, "reps": reps, "all_ok": bool(res[0].all()), "inner_steps_max": int(res[6].max())}
        # the batch: end to end (packed arrays in, packed arrays out) and the launch alone
        t_batch = median_seconds(lambda: ctx.box_lcp_schur_batch_packed(ns, A, b, lo, hi), reps)
        ctx.kernel_time(reset=True)
        k = []
        for _ in range(reps):
            ctx.box_lcp_schur_batch_packed(ns, A, b, lo, hi)
            k.append(ctx.kernel_time(reset=True)[0])
        row["batch_ms"] = t_batch * 1e3
        row["batch_kernel_ms"] = float(np.median(k))
        row["batch_problems_per_s"] = count / t_batch
        row["batch_kernel_problems_per_s"] = count / (row["batch_kernel_ms"] * 1e-3)
        # yardstick 1: the single entry, one call per problem
        t_loop = median_seconds(lambda: [ctx.box_lcp_schur(*p) for p in probs], reps)
        row["single_loop_ms"] = t_loop * 1e3
        row["single_loop_problems_per_s"] = count / t_loop
        row["batch_over_single_loop"] = t_loop / t_batch
        # yardstick 2: the CPU port, the reference's flags, one thread
        with orc.timing_build() as flags:
            t_cpu = median_seconds(lambda: [orc.tk_box_schur(*p) for p in probs], reps)
            row["cpu_flags"] = flags
        row["cpu_ms"] = t_cpu * 1e3
        row["cpu_problems_per_s"] = count / t_cpu
        row["batch_over_cpu"] = t_cpu / t_batch
        row["winner"] = "batch" if t_batch < t_cpu else "cpu"
        # the answers of the three agree
        single = [ctx.box_lcp_schur(*p) for p in probs[:4]]
        vo, _ = capi.lcp_batch_offsets(ns)
        row["max_diff_vs_single"] = float(max(np.abs(s[1] - res[1][vo[i]:vo[i + 1]]).max() for i, s in enumerate(single)))
        cpu = [orc.tk_box_schur(*p) for p in probs[:64]]
        row["max_diff_vs_cpu"] = float(max(np.abs(c[1] - res[1][vo[i]:vo[i + 1]]).max() for i, c in enumerate(cpu)))
        print(json.dumps(row), flush=True)
        rows.append(row)
    ctx.close()
    if len(sys.argv) > 2:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
        with open(sys.argv[2], "w") as f:
            json.dump({"tool": "gpu_time_lcp_schur_batch", "reps": reps, "rows": rows}, f, indent=1)
    print(json.dumps({"summary": {r["workload"]: {"x_single_loop": round(r["batch_over_single_loop"], 2), "x_cpu": round(r["batch_over_cpu"], 2)}
                                  for r in rows}}), flush=True)


if __name__ == "__main__":
    main()
