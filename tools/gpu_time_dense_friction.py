#!/usr/bin/env python3
"""What the friction pyramid costs on the dense world step (egs_world_set_dense_friction), that a build with it costs
nothing while it is off, and the same world through the friction sweeps.

  python tools/gpu_time_dense_friction.py [--parent-lib PATH/libeggshell_amd.so] [--samples 5] [--steps 20] [--mu 0.5]
                                          [--worlds 1 16 256] [--out profiles/dense_friction/dense_friction.json]

The workload: E copies of the 2 x 2 x 2 pile (96 rows each, the fused kernel's 112-row class), every body pushed by
v += (0.3, 0.1, 0), dt 5e-3, erp 0.2, cfm 0.01, contact detection on.  ms per step (device events, egs_timer_*), the
median and the range of --samples samples; each sample is a process of its own that loads ONE library, the legs in turn
so that a drift of the clocks hits all alike:

  off      egs_world_step_dense, use_bounds 1, friction off, this build
  parent   the same on the parent build (--parent-lib, if given; it has no dense friction entry)
  on       egs_world_step_dense, use_bounds 1, egs_world_set_friction(mu) + egs_world_set_dense_friction(32, 1e-10)
  sweeps   egs_world_step with the same friction: SOR(1.5), tol 1e-9, at most 500 sweeps

`off` must sit inside the parent's own run-to-run range.  `on` and `sweeps` are recorded, not thresholded.
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
PUSH = (0.3, 0.1, 0.0)


def leg(a):
    """One sample: a fresh world of a.ensembles pushed piles, three warm-up steps, a.steps timed ones."""
    import bench
    from eggshell_amd import capi, scenes
    if a.lib:
        capi.LIB_PATH = os.path.abspath(a.lib)
    ctx = capi.Context(0)
    pitch = 0.31 * 2 + 2.0
    ens = []
    for e in range(a.ensembles):
        sc = scenes.box_stack(2, 2, 2, origin=(pitch * (e % 16), pitch * (e // 16)))
        sc["v"] = sc["v"] + np.asarray(PUSH)
        Minv, f_ext = bench.host_mass_and_force(sc)
        ens.append((sc, np.asarray(Minv).reshape(-1, 36), np.asarray(f_ext).reshape(-1, 6)))
    w, _ = capi.World.batch(ctx, [sc["p"].shape[0] for sc, _, _ in ens])
    cat = lambda k: np.concatenate([sc[k] for sc, _, _ in ens])
    w.set_bodies(cat("p"), cat("R"), cat("v"), cat("w"), np.concatenate([m for _, m, _ in ens]),
                 np.concatenate([f for _, _, f in ens]))
    if a.friction:
        w.set_friction(np.full(a.ensembles, a.mu))
        if a.leg == "dense":
            w.set_dense_friction(32, 1e-10)
    prm = capi.params(method=capi.SOR, max_iters=500, tol=1e-9, cfm=CFM, omega=1.5)

    piv, outer = [], []      # per timed step, the largest over the ensembles (host tables of the step: no device work)

    def step():
        if a.leg == "dense":
            assert w.step_dense(DT, ERP, CFM, use_bounds=1) == 0
            piv.append(int(w.dense_info()["pivots"].max()))
            if a.friction:
                outer.append(int(w.dense_friction_info()[0].max()))
        else:
            w.step(DT, ERP, prm)

    for _ in range(3):
        step()
    del piv[:], outer[:]
    ctx.synchronize()
    ctx.timer_start()
    for _ in range(a.steps):
        step()
    ms = ctx.timer_stop() / a.steps
    out = dict(ms=ms, rows=3 * w.info()["n_constraints"] // a.ensembles)
    if a.leg == "dense" and a.friction:
        out.update(outer_mean=float(np.mean(outer)), outer_max=int(max(outer)), converged_last=int(w.dense_friction_info()[1].sum()))
    if a.leg == "dense":
        out.update(pivots_mean=float(np.mean(piv)), pivots_max=int(max(piv)))
    else:
        out.update(sweeps_max=int(w.batch_info()["iterations"].max()) if a.ensembles > 1 else None)
    print(json.dumps(out))
    w.close()
    ctx.close()


def child(a, which, **kw):
    """The leg as a process of its own (one library per process); its JSON line."""
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", which, "--steps", str(a.steps), "--mu", str(a.mu)]
    for k, v in kw.items():
        if v is True:
            cmd.append("--" + k)
        elif v not in (None, False):
            cmd += ["--" + k, str(v)]
    out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600).stdout
    return json.loads(out.strip().splitlines()[-1])


def summary(name, rows):
    ms = np.array([r["ms"] for r in rows])
    extra = {k: v for k, v in rows[-1].items() if k != "ms"}
    print("  %-8s %9.4f ms  (%.4f .. %.4f)   %s" % (name, np.median(ms), ms.min(), ms.max(), extra), flush=True)
    return dict(name=name, ms=ms.tolist(), median=float(np.median(ms)), **extra)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--mu", type=float, default=0.5)
    ap.add_argument("--worlds", type=int, nargs="*", default=[1, 16, 256])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_friction", "dense_friction.json"))
    ap.add_argument("--leg", choices=["dense", "sweeps"])      # internal: one sample
    ap.add_argument("--lib")
    ap.add_argument("--friction", action="store_true")
    ap.add_argument("--ensembles", type=int, default=16)
    a = ap.parse_args()
    if a.leg:
        return leg(a)
    doc = dict(steps=a.steps, samples=a.samples, mu=a.mu, dt=DT, erp=ERP, cfm=CFM, results=[])
    for E in a.worlds:
        legs = [("off", "dense", dict(ensembles=E)), ("on", "dense", dict(ensembles=E, friction=True)),
                ("sweeps", "sweeps", dict(ensembles=E, friction=True))]
        if a.parent_lib:
            legs.insert(1, ("parent", "dense", dict(ensembles=E, lib=a.parent_lib)))
        rows = {name: [] for name, _, _ in legs}
        for _ in range(a.samples):
            for name, which, kw in legs:      # in turn
                rows[name].append(child(a, which, **kw))
        print("E = %d x 2x2x2 pushed piles, %d rows each:" % (E, rows["off"][0]["rows"]))
        res = dict(ensembles=E, legs=[summary(name, rows[name]) for name, _, _ in legs])
        if a.parent_lib:
            p = np.array([r["ms"] for r in rows["parent"]])
            off = float(np.median([r["ms"] for r in rows["off"]]))
            res["off_within_parent_range"] = bool(p.min() <= off <= p.max())
            res["off_over_parent_median"] = off / float(np.median(p))
            print("  off's median inside the parent's range: %s (off / parent = %.4f)" %
                  (res["off_within_parent_range"], res["off_over_parent_median"]))
        doc["results"].append(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
