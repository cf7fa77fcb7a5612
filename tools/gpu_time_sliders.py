#!/usr/bin/env python3
"""What slider joints (EGS_JOINT_LOCK + EGS_JOINT_SLIDER_AXIS) cost in a world's step, and that a build with them costs
nothing on lists without them.  Modelled on tools/gpu_time_joints.py.

  python tools/gpu_time_sliders.py [--parent-lib PATH/libeggshell_amd.so] [--samples 5] [--steps 20] [--sweeps 20]
                                   [--links 64] [--worlds 1 16 256] [--out profiles/sliders/sliders.json]

One batched world of E chains of --links boxes, 0.6 m apart so that nothing touches (no contact detection), ball joints
link to link and the first link to the world; egs_world_step with --sweeps SOR sweeps, fp64, cfm 0.01: ms per step
(device events, egs_timer_*), the median and the range of --samples samples, each a process of its own that loads ONE
library, the legs in turn so that a drift of the clocks hits all alike:
  ball          ball joints only, this build
  parent        ball joints only, the parent build (--parent-lib, if given)
  hinge         every second link-to-link joint a hinge (a HINGE_AXIS block about y beside its ball joint, every fourth
                with a motor), this build: a list with angular blocks and no slider
  parent-hinge  the same on the parent build
  slider        every second link-to-link joint a slider: its ball joint replaced by a LOCK and a SLIDER_AXIS block along
                the chain (so the list is half as long again), every fourth with a motor, every one with travel stops at
                +-0.05 m
The ball and hinge legs (no slider: no changed kernel runs) must sit inside the parent's own run-to-run range.

One JSON document with every sample goes to --out; the table is printed."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DT, ERP, CFM = 0.005, 0.2, 0.01


def chain(n, y):
    """n unit boxes along x at height 2, 0.6 apart; ball joints link to link, link 0 to the world: (bodies, joints)."""
    p = np.array([[0.6 * i, y, 2.0] for i in range(n)])
    b0 = np.arange(n, dtype=np.int32)
    b1 = np.append(np.arange(1, n, dtype=np.int32), -1).astype(np.int32)
    data = np.zeros((n, 7))
    data[:n - 1, 0:3] = [0.3, 0.0, 0.0]
    data[:n - 1, 3:6] = [-0.3, 0.0, 0.0]
    b0[n - 1] = 0
    data[n - 1, 0:3] = [-0.3, 0.0, 0.0]
    data[n - 1, 3:6] = [-0.3, y, 2.0]
    return p, b0, b1, data


def leg_world(a):
    from eggshell_amd import capi
    if a.lib:
        capi.LIB_PATH = os.path.abspath(a.lib)
    ctx = capi.Context(0)
    n, E = a.links, a.ensembles
    w, off = capi.World.batch(ctx, [n] * E) if E > 1 else (capi.World(ctx, n), [0, n])
    P, B0, B1, D, K, M, T = [], [], [], [], [], [], []
    for e in range(E):
        p, b0, b1, data = chain(n, 2.0 * e)
        o = int(off[e])
        P.append(p)
        kinds, motor, travel = [0] * n, [[0.0, -1.0]] * n, [[-np.inf, np.inf]] * n
        b0, b1, data = list(b0), list(b1), list(data)
        if a.sliders:
            for k, i in enumerate(range(0, n - 1, 2)):      # every second link-to-link ball joint becomes lock + slider along x
                kinds[i] = capi.JOINT_LOCK
                data[i] = np.array([1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0])
                b0.append(i); b1.append(i + 1)
                data.append(np.array([1.0, 0.0, 0.0, 0.6, 0.0, 0.0, 0.0]))      # the rail through both centres: x = 0 now
                kinds.append(capi.JOINT_SLIDER_AXIS)
                motor.append([0.5, 2.0] if k % 4 == 0 else [0.0, -1.0])
                travel.append([-0.05, 0.05])
        if a.hinges:
            for k, i in enumerate(range(0, n - 1, 2)):      # a hinge about y beside every second link-to-link ball joint
                b0.append(i); b1.append(i + 1)
                data.append(np.array([0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0]))
                kinds.append(capi.JOINT_HINGE_AXIS)
                motor.append([0.5, 2.0] if k % 4 == 0 else [0.0, -1.0])
                travel.append([-np.inf, np.inf])
        B0.append(np.where(np.array(b0) >= 0, np.array(b0) + o, -1)); B1.append(np.where(np.array(b1) >= 0, np.array(b1) + o, -1))
        D.append(np.array(data)); K.append(np.array(kinds)); M.append(np.array(motor)); T.append(np.array(travel))
    N = n * E
    Minv = np.tile(np.diag([1.0] * 3 + [10.0] * 3).reshape(36), (N, 1))
    f = np.zeros((N, 6)); f[:, 2] = -9.8
    w.set_bodies(np.concatenate(P), np.tile(np.eye(3).reshape(9), (N, 1)), np.zeros((N, 3)), np.zeros((N, 3)), Minv, f)
    b0, b1, data = np.concatenate(B0), np.concatenate(B1), np.concatenate(D)
    if a.hinges or a.sliders:
        w.set_joints_kinds(np.concatenate(K), b0, b1, data)
        w.set_joint_motors(np.concatenate(M))
        if a.sliders:
            w.set_slider_limits(np.concatenate(T))
    else:
        w.set_joints(b0, b1, data)
    prm = capi.params(method=capi.SOR, max_iters=a.sweeps, tol=0.0, cfm=CFM)
    for _ in range(5):
        w.step(DT, ERP, prm, detect_contacts=False)
    ctx.synchronize()
    ctx.timer_start()
    for _ in range(a.steps - 1):
        w.step(DT, ERP, prm, detect_contacts=False)
    st = w.step(DT, ERP, prm, detect_contacts=False, want_stats=True)
    ms = ctx.timer_stop() / a.steps
    print(json.dumps(dict(ms=ms, schedule=st.schedule, residual=st.residual, m=int(b0.shape[0]))))
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


def summary(name, rows):
    ms = np.array([r["ms"] for r in rows])
    print("  %-13s %9.4f ms  (%.4f .. %.4f)   m = %d   schedule %#x   residual %.3g" %
          (name, np.median(ms), ms.min(), ms.max(), rows[-1]["m"], rows[-1]["schedule"], rows[-1]["residual"]), flush=True)
    return dict(name=name, ms=ms.tolist(), median=float(np.median(ms)), m=rows[-1]["m"], schedule=rows[-1]["schedule"],
                residual=rows[-1]["residual"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--sweeps", type=int, default=20)
    ap.add_argument("--links", type=int, default=64)
    ap.add_argument("--worlds", type=int, nargs="*", default=[1, 16, 256])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sliders", "sliders.json"))
    ap.add_argument("--leg", choices=["world"])      # internal: one sample
    ap.add_argument("--lib")
    ap.add_argument("--hinges", action="store_true")
    ap.add_argument("--sliders", action="store_true")
    ap.add_argument("--ensembles", type=int, default=16)
    a = ap.parse_args()
    if a.leg == "world":
        return leg_world(a)
    doc = dict(sweeps=a.sweeps, steps=a.steps, samples=a.samples, links=a.links, dt=DT, erp=ERP, cfm=CFM, results=[])
    for E in a.worlds:
        legs = [("ball", dict(ensembles=E)), ("hinge", dict(ensembles=E, hinges=True)), ("slider", dict(ensembles=E, sliders=True))]
        if a.parent_lib:
            legs.insert(1, ("parent", dict(ensembles=E, lib=a.parent_lib)))
            legs.insert(3, ("parent-hinge", dict(ensembles=E, hinges=True, lib=a.parent_lib)))
        rows = {name: [] for name, _ in legs}
        for _ in range(a.samples):
            for name, kw in legs:      # in turn
                rows[name].append(child(a, **kw))
        print("egs_world_step, E = %d chains of %d links, %d SOR sweeps:" % (E, a.links, a.sweeps))
        doc["results"].append(dict(workload="world", ensembles=E, legs=[summary(name, rows[name]) for name, _ in legs]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
