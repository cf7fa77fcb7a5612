#!/usr/bin/env python3
"""The fixed cost of one solve launch at the headline configuration (24 C3 piles, GS, fp64): the bench problem runs
through Problem.step at 1, 50 and 100 sweeps, the solve launch's time per step comes from ctx.kernel_time (the event
pair around the solve launch; with the fused assembly that launch assembles as well), and a least-squares line
t = fixed + slope * sweeps splits it into what every launch pays once (prologue, epilogue) and what each sweep costs.
The assemble and velocity kernels are outside the event pair: rocprofv3 --kernel-trace --stats of the bench has them.
usage: gpu_time_solve_fixed.py [steps=20] [warmup=5] [piles=24]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from eggshell_amd import capi, scenes  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 5
npiles = int(sys.argv[3]) if len(sys.argv) > 3 else 24
nx, ny, nz, _, _, dt = bench.WORKLOADS["c3"]
ctx = capi.Context(0)
sc = scenes.concat([scenes.box_stack(nx, ny, nz, jitter=1e-3, seed=k + 1, origin=(0.0, 100.0 * k)) for k in range(npiles)])
m = int(sc["kind"].shape[0])
rows = []
for sweeps in (1, 50, 100):
    pr, _ = bench.build_problem(ctx, sc, capi.F64)
    prm = capi.params(method=capi.GAUSS_SEIDEL, max_iters=sweeps, tol=0.0, cfm=0.01)
    elapsed, kernel_ms, launches = bench.time_region(ctx, lambda: pr.step(dt, 0.2, prm), steps, warmup)
    st = pr.stats()
    rows.append({"sweeps": sweeps, "solve_ms": kernel_ms, "launches": launches, "step_ms": elapsed * 1e3 / steps,
                 "schedule": st.schedule, "status": st.status})
    pr.close()
s = np.array([r["sweeps"] for r in rows], dtype=float)
t = np.array([r["solve_ms"] for r in rows])
slope, fixed = np.polyfit(s, t, 1)
print(json.dumps({"env": {k: v for k, v in os.environ.items() if k.startswith("EGS_")}, "piles": npiles, "constraints": m,
                  "steps": steps, "warmup": warmup, "runs": rows, "fixed_us": fixed * 1e3, "us_per_sweep": slope * 1e3,
                  "fit_max_abs_err_us": float(np.abs(fixed + slope * s - t).max() * 1e3)}))
ctx.close()
