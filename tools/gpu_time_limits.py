#!/usr/bin/env python3
"""What the hinge angle limits (egs_world_set_joint_limits) cost in a world's step, and that a build with them costs
nothing while no table is set.

  python tools/gpu_time_limits.py [--parent-tree DIR] [--samples 5] [--steps 20] [--sweeps 20] [--links 64]
                                  [--worlds 1 16 256] [--bench-runs 3] [--out profiles/limits/limits.json]

One batched world of E chains of --links boxes (tools/gpu_time_joints.py's: 0.6 m apart, nothing touches, ball joints
link to link and the first link to the world), every second link-to-link joint a hinge about y beside its ball joint,
every fourth of them with a motor; egs_world_step with --sweeps SOR sweeps, fp64, cfm 0.01: ms per step (device events,
egs_timer_*), the median and the range of --samples samples, each a process of its own that loads ONE library, the legs
in turn so that a drift of the clocks hits all alike:
  off      no limit table, this build
  parent   the same world on the parent build (--parent-tree: a built checkout of the parent commit)
  on       every hinge limited to +-0.02 rad: the chains sag under gravity, so stops become active while it runs
Then bench.py --gpus 1 --steps 20 --warmup 5, --bench-runs runs for this build and for the parent in turn, each from its
own tree.  The off leg and this build's bench must sit inside the parent's own run-to-run range.

One JSON document with every sample goes to --out; the tables are printed."""
import argparse
import json
import math
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

DT, ERP, CFM = 0.005, 0.2, 0.01
RANGE = 0.02


def leg_world(a):
    from eggshell_amd import capi
    from gpu_time_joints import chain
    if a.lib:
        capi.LIB_PATH = os.path.abspath(a.lib)
    ctx = capi.Context(0)
    n, E = a.links, a.ensembles
    w, off = capi.World.batch(ctx, [n] * E) if E > 1 else (capi.World(ctx, n), [0, n])
    P, B0, B1, D, K, M, L = [], [], [], [], [], [], []
    stop = [1.0, 0.0, 0.0, 0.0, math.sin(-RANGE), math.cos(-RANGE), math.sin(RANGE), math.cos(RANGE)]      # R = I everywhere: q = 1
    for e in range(E):
        p, b0, b1, data = chain(n, 2.0 * e)
        o = int(off[e])
        P.append(p)
        kinds, motor, lim = [0] * n, [[0.0, -1.0]] * n, [[0.0] * 8] * n
        b0, b1, data = list(b0), list(b1), list(data)
        for k, i in enumerate(range(0, n - 1, 2)):      # a hinge about y beside every second link-to-link ball joint
            b0.append(i); b1.append(i + 1)
            data.append(np.array([0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0]))
            kinds.append(capi.JOINT_HINGE_AXIS)
            motor.append([0.5, 2.0] if k % 4 == 0 else [0.0, -1.0])
            lim.append(stop)
        B0.append(np.where(np.array(b0) >= 0, np.array(b0) + o, -1)); B1.append(np.where(np.array(b1) >= 0, np.array(b1) + o, -1))
        D.append(np.array(data)); K.append(np.array(kinds)); M.append(np.array(motor)); L.append(np.array(lim))
    N = n * E
    Minv = np.tile(np.diag([1.0] * 3 + [10.0] * 3).reshape(36), (N, 1))
    f = np.zeros((N, 6)); f[:, 2] = -9.8
    w.set_bodies(np.concatenate(P), np.tile(np.eye(3).reshape(9), (N, 1)), np.zeros((N, 3)), np.zeros((N, 3)), Minv, f)
    b0, b1, data = np.concatenate(B0), np.concatenate(B1), np.concatenate(D)
    w.set_joints_kinds(np.concatenate(K), b0, b1, data)
    w.set_joint_motors(np.concatenate(M))
    if a.limits:
        w.set_joint_limits(np.concatenate(L))
    prm = capi.params(method=capi.SOR, max_iters=a.sweeps, tol=0.0, cfm=CFM)
    for _ in range(5):
        w.step(DT, ERP, prm, detect_contacts=False)
    ctx.synchronize()
    ctx.timer_start()
    for _ in range(a.steps - 1):
        w.step(DT, ERP, prm, detect_contacts=False)
    st = w.step(DT, ERP, prm, detect_contacts=False, want_stats=True)
    ms = ctx.timer_stop() / a.steps
    lo, hi = w.blocks()[3:5]
    hinge_rows = np.repeat(np.concatenate(K) == capi.JOINT_HINGE_AXIS, 3)      # the joints come first in the world's list
    lo, hi = lo[:hinge_rows.size], hi[:hinge_rows.size]
    active = int(np.sum(hinge_rows & (np.isinf(lo) | np.isinf(hi)) & (lo != -hi)))      # one-sided rows (a motor's are symmetric)
    print(json.dumps(dict(ms=ms, schedule=st.schedule, residual=st.residual, m=int(b0.shape[0]), active_stops=active)))
    w.close()
    ctx.close()


def child(a, **kw):
    """The leg as a process of its own (one library per process); its JSON line."""
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", "world", "--steps", str(a.steps), "--sweeps", str(a.sweeps),
           "--links", str(a.links)]
    for k, v in kw.items():
        if v is True:
            cmd.append("--" + k)
        elif v not in (None, False):
            cmd += ["--" + k, str(v)]
    out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600).stdout
    return json.loads(out.strip().splitlines()[-1])


def bench(tree):
    """bench.py --gpus 1 --steps 20 --warmup 5 from the tree given: its JSON result line."""
    out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"], cwd=tree, check=True,
                         capture_output=True, text=True, timeout=900).stdout
    return json.loads([l for l in out.strip().splitlines() if l.startswith("{")][-1])


def summary(name, rows):
    ms = np.array([r["ms"] for r in rows])
    print("  %-8s %9.4f ms  (%.4f .. %.4f)   m = %d   schedule %#x   residual %.3g   active stops %d" %
          (name, np.median(ms), ms.min(), ms.max(), rows[-1]["m"], rows[-1]["schedule"], rows[-1]["residual"], rows[-1]["active_stops"]),
          flush=True)
    return dict(name=name, ms=ms.tolist(), median=float(np.median(ms)), m=rows[-1]["m"], schedule=rows[-1]["schedule"],
                residual=rows[-1]["residual"], active_stops=rows[-1]["active_stops"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree")
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--sweeps", type=int, default=20)
    ap.add_argument("--links", type=int, default=64)
    ap.add_argument("--worlds", type=int, nargs="*", default=[1, 16, 256])
    ap.add_argument("--bench-runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "limits", "limits.json"))
    ap.add_argument("--leg", choices=["world"])      # internal: one sample
    ap.add_argument("--lib")
    ap.add_argument("--limits", action="store_true")
    ap.add_argument("--ensembles", type=int, default=16)
    a = ap.parse_args()
    if a.leg == "world":
        return leg_world(a)
    parent_lib = os.path.join(a.parent_tree, "eggshell_amd", "libeggshell_amd.so") if a.parent_tree else None
    doc = dict(sweeps=a.sweeps, steps=a.steps, samples=a.samples, links=a.links, dt=DT, erp=ERP, cfm=CFM, range=RANGE, results=[])
    for E in a.worlds:
        legs = [("off", dict(ensembles=E)), ("on", dict(ensembles=E, limits=True))]
        if parent_lib:
            legs.insert(1, ("parent", dict(ensembles=E, lib=parent_lib)))
        rows = {name: [] for name, _ in legs}
        for _ in range(a.samples):
            for name, kw in legs:      # in turn
                rows[name].append(child(a, **kw))
        print("egs_world_step, E = %d chains of %d links, every second joint a hinge, %d SOR sweeps:" % (E, a.links, a.sweeps))
        doc["results"].append(dict(workload="world", ensembles=E, legs=[summary(name, rows[name]) for name, _ in legs]))
    trees = [("this", ROOT)] + ([("parent", os.path.abspath(a.parent_tree))] if a.parent_tree else [])
    runs = {name: [] for name, _ in trees}
    for _ in range(a.bench_runs):
        for name, tree in trees:      # in turn
            runs[name].append(bench(tree))
    if a.bench_runs:
        print("bench.py --gpus 1 --steps 20 --warmup 5:")
        for name, _ in trees:
            vals = [r.get("value") for r in runs[name]]
            print("  %-8s %s %s   median %.6g  (%.6g .. %.6g)" % (name, runs[name][-1].get("metric", "value"), runs[name][-1].get("unit", ""),
                                                                 np.median(vals), min(vals), max(vals)), flush=True)
        doc["bench"] = runs
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
