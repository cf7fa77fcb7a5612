#!/usr/bin/env python3
"""What live inertia (egs_world_set_live_inertia) costs per frame, against the route a caller had to take before it, and
that a build with it costs nothing while it is off.

  python tools/gpu_time_live_inertia.py [--parent-lib PATH/libeggshell_amd.so] [--samples 5] [--steps 50] [--sweeps 20]
                                        [--worlds 1 16 256] [--free] [--out profiles/live_inertia/live_inertia.json]

The workload: one batched world of E ensembles (--worlds) of 64 bricks (sides 0.1 x 0.3 x 0.6, mass 1) -- each ensemble a
chain of 64 links with small seeded spins, or with --free 64 free bricks -- stepped by egs_world_step (SOR, --sweeps
sweeps, cfm 0.01, dt 1e-3, contact detection off: the links are joined corner to corner).  A cube pile would measure
nothing: its bodies are skipped.  ms per frame (wall clock around --steps steps, synchronised at both ends), the median
and the range of --samples samples, each a process of its own that loads ONE library, the legs in turn:
  live     (a) live inertia on
  off      (b) live inertia off
  host     (c) the host-refresh route: egs_world_get_bodies, the oracle's values, egs_world_set_bodies(Minv, f_ext), step
  parent   (d) the parent build (--parent-lib, if given; it has no live-inertia entry), off
and the refresh kernel's own time, from egs_kernel_time on a world of free bricks (no solve launch: the refresh is the
only launch it counts).  One JSON document with every sample goes to --out; the table is printed."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DT, ERP, CFM = 1e-3, 0.2, 0.01
BRICK = np.diag([(0.3 ** 2 + 0.6 ** 2) / 12.0, (0.1 ** 2 + 0.6 ** 2) / 12.0, (0.1 ** 2 + 0.3 ** 2) / 12.0])


def build_world(a, capi, scenes, orc, ctx):
    n = 64
    ens = []
    for e in range(a.ensembles):
        rng = np.random.default_rng(e + 1)
        sc = scenes.chain(n, anchor=(0.0, 5.0 * e, 2.0))
        sc["I_body"] = np.tile(BRICK.reshape(9), (n, 1))
        sc["w"] = rng.uniform(-0.3, 0.3, (n, 3))
        sc["Minv"] = orc.minv_blocks(sc["R"], sc["mass"], sc["I_body"])
        sc["f_ext"] = orc.external_force(sc["R"], sc["w"], sc["mass"], sc["I_body"])
        ens.append(sc)
    w, off = capi.World.batch(ctx, [n] * a.ensembles)
    cat = lambda k: np.concatenate([sc[k] for sc in ens])
    w.set_bodies(cat("p"), cat("R"), cat("v"), cat("w"), cat("Minv"), cat("f_ext"))
    if not a.free:
        glob = lambda sc, o, k: np.where(sc[k] >= 0, sc[k] + o, -1)
        w.set_joints(np.concatenate([glob(sc, o, "body0") for sc, o in zip(ens, off)]),
                     np.concatenate([glob(sc, o, "body1") for sc, o in zip(ens, off)]), cat("data"))
    return w, cat("mass"), cat("I_body"), cat("Minv"), cat("f_ext")


def leg(a):
    """One sample: a fresh world, five warm-up frames, a.steps timed ones."""
    from eggshell_amd import capi, scenes
    from oracle import oracle as orc
    if a.lib:
        capi.LIB_PATH = os.path.abspath(a.lib)
    ctx = capi.Context(0)
    w, mass, I_body, Minv, f_ext = build_world(a, capi, scenes, orc, ctx)
    if a.route == "live":
        w.set_live_inertia(I_body)
    prm = capi.params(method=capi.SOR, max_iters=a.sweeps, tol=0.0, cfm=CFM)

    def frame():
        if a.route == "host":
            _, R, _, wv = w.bodies()
            M = orc.minv_blocks(R, mass, I_body)
            f = orc.external_force(R, wv, mass, I_body)
            w.set_bodies(None, None, None, None, M, f)
        w.step(DT, ERP, prm, detect_contacts=False)

    for _ in range(5):
        frame()
    ctx.synchronize()
    ctx.kernel_time(reset=True)
    t0 = time.perf_counter()
    for _ in range(a.steps):
        frame()
    ctx.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / a.steps
    ksum, klaunches = ctx.kernel_time(reset=True)
    print(json.dumps(dict(ms=ms, kernel_ms=ksum, kernel_launches=klaunches, bodies=int(mass.shape[0]))))
    w.close()
    ctx.close()


def child(a, **kw):
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", "--steps", str(a.steps), "--sweeps", str(a.sweeps)]
    for k, v in kw.items():
        if v is True:
            cmd.append("--" + k)
        elif v not in (None, False):
            cmd += ["--" + k, str(v)]
    out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600).stdout
    return json.loads(out.strip().splitlines()[-1])


def summary(name, rows):
    ms = np.array([r["ms"] for r in rows])
    print("  %-8s %9.4f ms/frame  (%.4f .. %.4f)" % (name, np.median(ms), ms.min(), ms.max()), flush=True)
    return dict(name=name, ms=ms.tolist(), median=float(np.median(ms)), min=float(ms.min()), max=float(ms.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--sweeps", type=int, default=20)
    ap.add_argument("--worlds", type=int, nargs="*", default=[1, 16, 256])
    ap.add_argument("--free", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "live_inertia", "live_inertia.json"))
    ap.add_argument("--leg", action="store_true")      # internal: one sample
    ap.add_argument("--lib")
    ap.add_argument("--route", choices=["live", "off", "host"], default="off")
    ap.add_argument("--ensembles", type=int, default=16)
    a = ap.parse_args()
    if a.leg:
        return leg(a)
    doc = dict(sweeps=a.sweeps, steps=a.steps, samples=a.samples, free=a.free, dt=DT, erp=ERP, cfm=CFM, results=[])
    for E in a.worlds:
        legs = [("live", dict(route="live")), ("off", dict(route="off")), ("host", dict(route="host"))]
        if a.parent_lib:
            legs.append(("parent", dict(route="off", lib=a.parent_lib)))
        rows = {name: [] for name, _ in legs}
        for _ in range(a.samples):
            for name, kw in legs:      # in turn
                rows[name].append(child(a, ensembles=E, free=a.free, **kw))
        print("egs_world_step, E = %d x 64 bricks (%s), %d SOR sweeps:" % (E, "free" if a.free else "chains", a.sweeps))
        res = dict(ensembles=E, bodies=rows["off"][0]["bodies"], legs=[summary(name, rows[name]) for name, _ in legs])
        # the refresh kernel alone: free bricks, so that no solve launch is counted with it
        k = child(a, ensembles=E, free=True, route="live")
        res["refresh_kernel_us"] = 1e3 * k["kernel_ms"] / max(1, k["kernel_launches"])
        print("  live_mass_kernel: %.2f us per launch (%d launches)" % (res["refresh_kernel_us"], k["kernel_launches"]))
        doc["results"].append(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
