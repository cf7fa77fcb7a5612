#!/usr/bin/env python3
"""What restitution (egs_problem_set_restitution / egs_world_set_restitution) costs, and that a build with it costs
nothing while it is off.

  python tools/gpu_time_restitution.py [--parent-lib PATH/libeggshell_amd.so] [--samples 7] [--steps 20] [--sweeps 100]
                                       [--piles 24] [--rest 0.5] [--worlds 16 256]
                                       [--out profiles/restitution/restitution.json]

step     egs_problem_step (assembly + --sweeps GS sweeps + velocity update, fp64, cfm 0.01) on --piles 16 x 16 x 16 piles
         in one problem, and on one pile: ms per step (device events, egs_timer_*), the median and the range of --samples
         samples, each a process of its own that loads ONE library, the legs in turn so that a drift of the clocks hits
         all alike: this build with restitution off, the parent build (--parent-lib, if given; it has no restitution
         entry), this build with the coefficient on every contact (threshold 0; the step stays on the fused launch:
         the schedule column shows it).  Off must sit inside the parent's own run-to-run range.
world    one batched world of E 4 x 4 x 4 piles (--worlds), SOR, the same sweeps: ms per frame with restitution off and on.

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


def leg_step(a):
    """One sample: a fresh problem of a.piles piles, three warm-up steps, a.steps timed ones."""
    import bench
    from eggshell_amd import capi, scenes
    if a.lib:
        capi.LIB_PATH = os.path.abspath(a.lib)
    ctx = capi.Context(0)
    piles = [scenes.box_stack(16, 16, 16, origin=(0.0, 100.0 * b)) for b in range(a.piles)]
    sc = scenes.concat(piles) if a.piles > 1 else piles[0]
    Minv, f_ext = bench.host_mass_and_force(sc)
    pr = capi.Problem(ctx, sc["p"].shape[0], sc["body0"], sc["body1"])
    pr.set_state(sc["p"], sc["R"], sc["v"], sc["w"], Minv, f_ext)
    pr.set_constraints(sc["kind"], sc["data"])
    if a.restitution:
        pr.set_restitution(np.full(pr.m, a.rest), 0.0)
    prm = capi.params(method=capi.GAUSS_SEIDEL, max_iters=a.sweeps, tol=0.0, cfm=CFM)
    for _ in range(3):
        pr.step(DT, ERP, prm)
    ctx.synchronize()
    ctx.timer_start()
    for _ in range(a.steps):
        pr.step(DT, ERP, prm)
    ms = ctx.timer_stop() / a.steps
    st = pr.stats()
    print(json.dumps(dict(ms=ms, schedule=st.schedule, residual=st.residual, m=pr.m)))
    pr.close()
    ctx.close()


def leg_world(a):
    import bench
    from eggshell_amd import capi, scenes
    ctx = capi.Context(0)
    pitch = 0.31 * 4 + 2.0
    ens = []
    for e in range(a.ensembles):
        sc = scenes.box_stack(4, 4, 4, jitter=1e-3, seed=e + 1, origin=(pitch * (e % 16), pitch * (e // 16)))
        Minv, f_ext = bench.host_mass_and_force(sc)
        ens.append((sc, np.asarray(Minv).reshape(-1, 36), np.asarray(f_ext).reshape(-1, 6)))
    w, _ = capi.World.batch(ctx, [sc["p"].shape[0] for sc, _, _ in ens])
    cat = lambda k: np.concatenate([sc[k] for sc, _, _ in ens])
    w.set_bodies(cat("p"), cat("R"), cat("v"), cat("w"), np.concatenate([m for _, m, _ in ens]),
                 np.concatenate([f for _, _, f in ens]))
    if a.restitution:
        w.set_restitution(np.full(a.ensembles, a.rest), 0.0)
    prm = capi.params(method=capi.SOR, max_iters=a.sweeps, tol=0.0, cfm=CFM)
    for _ in range(5):
        w.step(DT, ERP, prm)
    ctx.synchronize()
    ctx.timer_start()
    for _ in range(a.steps - 1):
        w.step(DT, ERP, prm)
    st = w.step(DT, ERP, prm, want_stats=True)
    ms = ctx.timer_stop() / a.steps
    print(json.dumps(dict(ms=ms, schedule=st.schedule, residual=st.residual)))
    w.close()
    ctx.close()


def child(a, leg, **kw):
    """The leg as a process of its own (one library per process); its JSON line."""
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--steps", str(a.steps), "--sweeps", str(a.sweeps),
           "--rest", str(a.rest)]
    for k, v in kw.items():
        if v is True:
            cmd.append("--" + k)
        elif v not in (None, False):
            cmd += ["--" + k, str(v)]
    out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600).stdout
    return json.loads(out.strip().splitlines()[-1])


def summary(name, rows):
    ms = np.array([r["ms"] for r in rows])
    print("  %-22s %9.4f ms  (%.4f .. %.4f)   schedule %#x   residual %.3g" %
          (name, np.median(ms), ms.min(), ms.max(), rows[-1]["schedule"], rows[-1]["residual"]), flush=True)
    return dict(name=name, ms=ms.tolist(), median=float(np.median(ms)), schedule=rows[-1]["schedule"], residual=rows[-1]["residual"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--sweeps", type=int, default=100)
    ap.add_argument("--piles", type=int, default=24)
    ap.add_argument("--rest", type=float, default=0.5)
    ap.add_argument("--worlds", type=int, nargs="*", default=[16, 256])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "restitution", "restitution.json"))
    ap.add_argument("--leg", choices=["step", "world"])      # internal: one sample
    ap.add_argument("--lib")
    ap.add_argument("--restitution", action="store_true")
    ap.add_argument("--ensembles", type=int, default=16)
    a = ap.parse_args()
    if a.leg == "step":
        return leg_step(a)
    if a.leg == "world":
        return leg_world(a)
    doc = dict(sweeps=a.sweeps, steps=a.steps, samples=a.samples, rest=a.rest, dt=DT, erp=ERP, cfm=CFM, results=[])
    for piles in sorted({a.piles, 1}, reverse=True):
        legs = [("off", dict(piles=piles)), ("on", dict(piles=piles, restitution=True))]
        if a.parent_lib:
            legs.insert(1, ("parent", dict(piles=piles, lib=a.parent_lib)))
        rows = {name: [] for name, _ in legs}
        for _ in range(a.samples):
            for name, kw in legs:      # in turn
                rows[name].append(child(a, "step", **kw))
        print("egs_problem_step, %d x 16x16x16, %d GS sweeps, m = %d:" % (piles, a.sweeps, rows["off"][0]["m"]))
        doc["results"].append(dict(workload="step", piles=piles, legs=[summary(name, rows[name]) for name, _ in legs]))
    for E in a.worlds:
        rows = {"off": [], "on": []}
        for _ in range(a.samples):
            rows["off"].append(child(a, "world", ensembles=E))
            rows["on"].append(child(a, "world", ensembles=E, restitution=True))
        print("egs_world_step, E = %d x 4x4x4, %d SOR sweeps:" % (E, a.sweeps))
        doc["results"].append(dict(workload="world", ensembles=E, legs=[summary(k, rows[k]) for k in ("off", "on")]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
